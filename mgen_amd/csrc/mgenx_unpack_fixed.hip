// mgenx_unpack_fixed.hip -- unpack + receive CRC for fixed-length records: the pipelined
// kernel (any length in [65, 1024], columns or rows) and the ring kernel (512- / 1024-byte
// records with row output).
#include "mgenx_unpack.hpp"

namespace mgenx {

// Fixed-length records (fixed stride, one length L in [65, 1024]; BASELINE config 2 and
// the recvmmsg fixed-slot layout), software-pipelined across groups.  With one L every
// group has the same row geometry (V = ceil(L/64) rows, padded to the template's NR), so
// while a wave consumes row j of group g it reloads the register with row j of its next
// group g' = g + n_waves: the wave keeps ~NR x 1 KiB of loads in flight through its own
// LDS-bound CRC work and tail, at no register cost.  The header of g' is issued at the top
// of g (before g's reloads), so with in-order completion the CRC decision for g' waits for
// that header only, and row j of g' waits only for row j.
// Semantics are those of unpack_kernel<true> (same helpers, same column stores).
// MODE (diagnostic ablations, never the product path) is a bit mask:
//   1 = loads + XOR only (no LDS lookups)       2 = no tail (no decode, no stores)
//   4 = decode but no stores (kept alive)       8 = every store to the sink
//   16 = the other store flavour (rows: temporal; columns: non-temporal)
//   128 = non-temporal row loads
template <int NR, int MODE = 0, bool kRows = false, bool kAligned = false>
__global__ void __launch_bounds__(kUnpackThreads)
unpack_fixed_kernel(UnpackParams p, uint32_t expect) {
  constexpr bool kAblXor = (MODE & 1) != 0, kAblNoTail = (MODE & 2) != 0;
  constexpr bool kAblNoStore = (MODE & 4) != 0, kAblSink = (MODE & 8) != 0;
  constexpr bool kAblAltStore = (MODE & 16) != 0;
  constexpr bool kAblNtLoad = (MODE & 128) != 0;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* rep = lds;
  uint32_t* fold = lds + kRepDwords;  // [A4 | A8 | A12 | A16 | A32 | A48]
  const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(rep);
  const TableRegs<> tab_regs = table_loads(p.tabs);  // staged below, after the first rows
  asm volatile("" ::: "memory");  // these loads issue before the rows (in-order vmcnt)

  const int lane = threadIdx.x & 63;
  const int q = lane & 3;
  const uint32_t s1 = a64_s1((uint32_t)lane);
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(
      blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t n_groups = (p.n + 15u) >> 4;
  const bool force = (p.opts & MGENX_OPT_CHECKSUM_FORCE) != 0;
  const bool tcp = (p.opts & MGENX_OPT_TCP) != 0;
  const uint32_t L = p.fixed_len;          // host guarantees 65 <= L <= 1024
  constexpr int V = NR;                    // rows: ceil(L / 64), 2..16 (host-checked)

  // Groups are dealt round-robin (wave w takes w, w + n_waves, ...): measured faster than
  // contiguous runs per wave (254 vs 241 us on config 2), whose 4096 concurrent 256-KiB
  // streams spread worse over the HBM channels.
  uint32_t g = wave_id;
  const uint32_t g_end = n_groups;

  // Geometry.  Every load is slab (uniform SGPR base) + 32-bit per-lane offset + constant:
  // the saddr form, one VGPR per address (host guarantees slab_bytes < 4 GiB).  A dead
  // lane (past the batch or outside the slab) reads at base offset 64 instead, inside the
  // slab (host guarantees slab_bytes >= 64 (NR + 1) + 16).
  auto rec_idx = [&](uint32_t gg) { return (gg << 4) + (uint32_t)(lane >> 2); };
  auto rec_ptr = [&](uint32_t i) { return p.slab + (uint64_t)i * p.stride; };
  auto is_live = [&](uint32_t i) {
    const uint64_t off = (uint64_t)i * p.stride;
    return i < p.n && off <= p.slab_bytes && L <= p.slab_bytes - off;
  };
  auto base_off = [&](bool lv, uint32_t i) { return lv ? i * (uint32_t)p.stride : 64u; };
  // lane's byte offset of row 0 (> -64; < 0 when row 0 starts before the record)
  const int pos0 = (int)L - 64 * V + 16 * q;
  auto ld = [&](uint32_t off, int imm) {
    if (kAblNtLoad) return ldnt128(p.slab + (uint64_t)off + imm);
    return ldu128(p.slab + (uint64_t)off + imm);
  };
  // row j of the record at boff (row 0 clamped to the record start).  Rows j >= 1 start at
  // boff + pos0 + 64 j with pos0 + 64 > 0: the 32-bit part must stay non-negative (it is
  // zero-extended), so the constant part is 64 (j - 1).
  auto ld_row = [&](uint32_t boff, int j) {
    return j == 0 ? ld(boff + (uint32_t)(pos0 > 0 ? pos0 : 0), 0)
                  : ld(boff + (uint32_t)(pos0 + 64), 64 * (j - 1));
  };
  auto ld_hdr = [&](uint32_t boff) { return ld(boff + 16u * (uint32_t)q, 0); };

  u32x4_t d[NR];
  // The tail is split in two so the aligned loop can decode a group's header as soon as its
  // row 0 arrives (then reload row 0 at once): decode() turns the quad's header into the
  // lane's store values, emit() applies the checksum verdict and stores.
  struct Out {
    uint32_t o[5];
  };
  auto decode = [&](const u32x4_t& pf, uint32_t idx, bool live) {
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = prefix_word(pf, j);
    const uint32_t w10 = prefix_word(pf, 10);
    const uint32_t D = w[5] >> 24;
    const uint32_t hw = (D == 4u) ? w[7] : w10;
    const uint32_t gi = (28u + D + (hw >> 24)) >> 2;  // GPS block word (fast layouts)
    const uint32_t g3 = (prefix_word(pf, 11) & (0u - (uint32_t)(gi == 8u))) |
                        (prefix_word(pf, 12) & (0u - (uint32_t)(gi == 9u))) |
                        (prefix_word(pf, 14) & (0u - (uint32_t)(gi == 11u))) |
                        (prefix_word(pf, 15) & (0u - (uint32_t)(gi == 12u)));
    // fast layout (mgenMsg.cpp:323-497 with every field word-aligned)
    uint32_t flow = bswap32(w[1]), seq = bswap32(w[2]), sec = bswap32(w[3]);
    uint32_t usec = bswap32(w[4]), dst4 = w[6];
    uint32_t msg_len = bswap16((uint16_t)(w[0] & 0xffffu));
    uint32_t dport = bswap16((uint16_t)(w[5] & 0xffffu));
    const uint32_t hlen = 44u + D + (hw >> 24);
    uint32_t plen = bswap16((uint16_t)(g3 >> 16));
    if (!(plen != 0 && hlen + plen <= L)) plen = 0;  // mgenMsg.cpp:488-497
    uint32_t flags = w[0] >> 24, err = 0, dtype = (w[5] >> 16) & 0xffu, dlen = D;
    uint32_t ptype = (g3 >> 8) & 0xffu, gps = g3 & 0xffu;
    // general layouts: quad lane 0 parses (with loads), then broadcasts to its quad
    const bool slow = live && !fast_layout(w[0], w[5], hw);
    if (__any(slow)) {
      Hdr h;
      if (slow && q == 0) parse_header(rec_ptr(idx), L, false, w, h);
      auto bc = [&](uint32_t& dst, uint32_t v) {
        v = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, false);
        if (slow) dst = v;
      };
      bc(flow, h.flow); bc(seq, h.seq); bc(sec, h.sec); bc(usec, h.usec); bc(dst4, h.dst4);
      bc(msg_len, h.msg_len); bc(dport, h.dst_port); bc(plen, h.plen); bc(flags, h.flags);
      bc(err, h.err); bc(dtype, h.dst_type); bc(dlen, h.dst_len); bc(ptype, h.ptype);
      bc(gps, h.gps);
    }
    if (!live) {  // descriptor outside the slab (or past the batch end)
      flow = seq = sec = usec = dst4 = msg_len = dport = plen = flags = dtype = dlen = 0;
      ptype = gps = 0;
      err = MGENX_ERROR_OOB;
    }
    Out r;
    if (kRows) {  // mgenx_rec: lane q holds bytes 8q..8q+7 of its record
      r.o[0] = q == 0 ? flow : q == 1 ? sec : q == 2 ? dst4 : (plen | flags << 16 | err << 24);
      r.o[1] = q == 0 ? seq : q == 1 ? usec : q == 2 ? (msg_len | dport << 16)
                                                    : (dtype | dlen << 8 | ptype << 16 | gps << 24);
      r.o[2] = r.o[3] = r.o[4] = 0;
    } else {  // the lane's column values: u32 (column q), dst_addr4, u16, u8a, u8b
      r.o[0] = q == 0 ? flow : q == 1 ? seq : q == 2 ? sec : usec;
      r.o[1] = dst4;
      r.o[2] = q == 0 ? msg_len : q == 1 ? dport : plen;
      r.o[3] = q == 0 ? flags : q == 1 ? err : q == 2 ? dtype : dlen;
      r.o[4] = (q & 1) == 0 ? ptype : gps;
    }
    return r;
  };
  // Store one record per quad.  Every lane runs the same instructions: the four lanes of a
  // quad store four different columns (or the four 8-byte parts of a row), with no branch
  // around the stores.  (gfx950 counts stores in vmcnt: a store that might be skipped makes
  // LLVM's wait counts assume it was, so the next row wait would also wait for the store's
  // acknowledgement.)  Lanes past the batch end write to the sink.
  auto emit = [&](Out r, uint32_t idx, bool crc_bad) {
    if (crc_bad) {  // the caller's receive check (mgenTransport.cpp:971): err, TCP flag
      const uint32_t fl = tcp ? (uint32_t)MGENX_FLAG_CHECKSUM_ERROR : 0u;
      if (kRows) {
        if (q == 3) r.o[0] = (r.o[0] & 0x00ffffffu) | fl << 16 | (uint32_t)MGENX_ERROR_CHECKSUM << 24;
      } else {
        if (q == 0) r.o[3] |= fl;
        if (q == 1) r.o[3] = MGENX_ERROR_CHECKSUM;
      }
    }
    const bool in = idx < p.n && !kAblSink;
    const uint64_t sink = (uint64_t)p.sink + 4u * (uint32_t)lane;
    auto at = [&](uint64_t base, uint32_t size) { return in ? base + (uint64_t)idx * size : sink; };
    const mgenx_cols& c = p.cols;
    if (kAblNoStore) {  // the tail's work without its stores (kept alive)
      const uint32_t all = r.o[0] ^ r.o[1] ^ r.o[2] ^ r.o[3] ^ r.o[4];
      if (all == 0x9E3779B9u) st_g32(sink, all);
      return;
    }
    if (kRows) {  // 16 records = 512 contiguous bytes per store instruction
      const uint64_t v = (uint64_t)r.o[1] << 32 | r.o[0];
      const uint64_t ra = in ? (uint64_t)p.cols.rows + (uint64_t)idx * 32 + 8 * q
                             : (uint64_t)p.sink + 8u * lane;
      // non-temporal: the streamed output must not compete with the read stream in L2
      if (kAblAltStore) st_g64(ra, v);  // ablation: ordinary (temporal) row stores
      else st_g64_nt(ra, v);
      return;
    }
    const uint64_t u32 = pick4(q, (uint64_t)c.flow_id, (uint64_t)c.seq_num, (uint64_t)c.tx_sec,
                               (uint64_t)c.tx_usec);
    const uint64_t u16 = pick4(q, (uint64_t)c.msg_len, (uint64_t)c.dst_port,
                               (uint64_t)c.payload_len, (uint64_t)c.payload_len);
    const uint64_t u8a = pick4(q, (uint64_t)c.flags, (uint64_t)c.err, (uint64_t)c.dst_type,
                               (uint64_t)c.dst_len);
    const uint64_t u8b = pick4(q, (uint64_t)c.payload_type, (uint64_t)c.gps_status,
                               (uint64_t)c.payload_type, (uint64_t)c.gps_status);
    if (kAblAltStore) {  // ablation: non-temporal column stores
      st_g32_nt(at(u32, 4), r.o[0]);
      st_g32_nt(at((uint64_t)c.dst_addr4, 4), r.o[1]);
      st_g16_nt(at(u16, 2), r.o[2]);
      st_g8_nt(at(u8a, 1), r.o[3]);
      st_g8_nt(at(u8b, 1), r.o[4]);
      return;
    }
    // u32: flow, seq, tx_sec, tx_usec (lane q -> column q); then dst_addr4 (all lanes);
    // u16: msg_len, dst_port, payload_len (lane 3 repeats lane 2's store);
    // u8: flags, err, dst_type, dst_len; then payload_type, gps_status (lanes 2,3 repeat)
    st_g32(at(u32, 4), r.o[0]);
    st_g32(at((uint64_t)c.dst_addr4, 4), r.o[1]);
    st_g16(at(u16, 2), r.o[2]);
    st_g8(at(u8a, 1), r.o[3]);
    st_g8(at(u8b, 1), r.o[4]);
  };
  // the receive-side CRC decision from words 0 and 5 (mgenTransport.cpp:960-963)
  auto decide = [&](const u32x4_t& pf, bool live) {
    const uint32_t w0 = prefix_word(pf, 0);
    const uint32_t w5 = prefix_word(pf, 5);
    const bool v2 = ((w0 >> 16) & 0xffu) == 2u;
    const bool flagged = force || ((((w0 >> 24) & MGENX_FLAG_CHECKSUM) != 0) && v2);
    const uint32_t t = (w5 >> 16) & 0xffu;
    return live && flagged && (tcp || (v2 && (t == 1u || t == 2u)));
  };

  u32x4_t pf;
  // The first group's rows go in flight before the tables are written to LDS (the staging's
  // load latency and LDS writes then overlap the first HBM round trip); a wave without a
  // group still loads (dummy rows) and joins the barrier.
  auto load_group = [&](uint32_t gg) {
    const uint32_t i = rec_idx(gg);
    const uint32_t boff = base_off(is_live(i), i);
    if (!kAligned) pf = ld_hdr(boff);
    // in row order (the loop's first wait is for row 0 alone)
#pragma unroll
    for (int j = 0; j < NR; j++) {
      d[j] = ld_row(boff, j);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  load_group(g);  // unconditional (a wave past the end reads the dummy rows at offset 64)
  table_writes(lds, tab_regs);
  // barrier without __syncthreads()'s fence: its vmcnt(0) would wait for the rows above
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (g >= g_end) return;
  bool first = true;
  while (g < g_end) {
    // ---- pipelined mode: rows of every group speculatively in flight one group ahead.
    // No load in this loop is conditional (a conditional reload makes LLVM copy the row
    // registers at the join, and a copy of an in-flight load drains the whole queue).
    uint32_t idx = rec_idx(g);
    bool live = is_live(idx);
    if (!first) {
      const uint32_t boff = base_off(live, idx);
      if (!kAligned) pf = ld_hdr(boff);
#pragma unroll
      for (int j = 0; j < NR; j++) {
        d[j] = ld_row(boff, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    first = false;
    // one pipelined group; the header registers alternate between two variables (the loop
    // is unrolled twice) so the next header never needs a register copy
    auto step = [&](const u32x4_t& pf_cur, u32x4_t& pf_nxt) {
      const uint32_t gn = g + n_waves;
      const bool has_next = gn < g_end;
      const uint32_t idx_n = rec_idx(has_next ? gn : g);
      const bool live_n = has_next && is_live(idx_n);
      // next group's header first (completes before any of its rows)
      const uint32_t boff_n = base_off(live_n, idx_n);
      if (!kAligned) pf_nxt = ld_hdr(boff_n);
      asm volatile("" ::: "memory");
      const u32x4_t hdr = kAligned ? d[0] : pf_cur;  // aligned: row 0 is the header
      const bool needs_crc = decide(hdr, live);
      const bool any = __any(needs_crc);
      // aligned: decode now, so row 0's registers are free for its reload
      Out early;
      if (kAligned && !kAblNoTail) early = decode(hdr, idx, live);

      // braid state word b = ha[b] ^ hb[b] (split so the next row folds in one XOR3)
      uint32_t ha[4] = {0u, 0u, 0u, 0u}, hb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < NR - 1; j++) {
        u32x4_t x = d[j];
        if (j == 0) {
          const int s0 = -pos0;
          if (s0 > 0) {
            const u32x4_t zero = {0u, 0u, 0u, 0u};
            x = s0 < 16 ? shl_bytes(x, s0) : zero;
          }
        }
        const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
        uint32_t c4[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
          if (kAblXor)
            c4[b] = (ha[b] << 1) ^ xw[b];
          else
            c4[b] = xor3(ha[b], hb[b], xw[b]);
        }
        // row j of g is dead now: reload its register for g' (same physical register, so
        // no loop-carried copy -- a copy of an in-flight load would drain the queue)
        __builtin_amdgcn_sched_barrier(0);
        d[j] = ld_row(boff_n, j);
        __builtin_amdgcn_sched_barrier(0);
        if (kAblXor) {
#pragma unroll
          for (int b = 0; b < 4; b++) ha[b] = c4[b];
          continue;
        }
#pragma unroll
        for (int b = 0; b < 4; b++) a64_parts(ldsb, c4[b], s1, ha[b], hb[b]);
      }
      // final row (V >= 2, so never row 0): the big-endian trailer goes to stream order
      const u32x4_t xf = d[NR - 1];
      uint32_t f0 = xor3(ha[0], hb[0], xf.x), f1 = xor3(ha[1], hb[1], xf.y);
      uint32_t f2 = xor3(ha[2], hb[2], xf.z);
      uint32_t f3 = xor3(ha[3], hb[3], q == 3 ? bswap32(xf.w) : xf.w);
      // opaque: later index math must not reach back to the row registers (which would keep
      // them live across their reload and cost a loop-carried copy of the in-flight load)
      asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
      __builtin_amdgcn_sched_barrier(0);
      d[NR - 1] = ld_row(boff_n, NR - 1);
      __builtin_amdgcn_sched_barrier(0);
      const uint32_t v = shift_tab(fold + 3 * 1024, f0) ^ shift_tab(fold + 2 * 1024, f1) ^
                         shift_tab(fold + 1 * 1024, f2) ^ shift_tab(fold, f3);
      const uint32_t* lt = fold + (q == 0 ? 5 : (q == 1 ? 4 : 3)) * 1024;  // A48/A32/A16
      uint32_t s = (q == 3) ? v : shift_tab(lt, v);
      s ^= __shfl_xor(s, 1);
      s ^= __shfl_xor(s, 2);
      if (kAblNoTail) {
        if (s == 0x9E3779B9u && lane == 0) p.cols.err[idx] = (uint8_t)needs_crc;  // keep alive
      } else {
        const Out r = kAligned ? early : decode(hdr, idx, live);
        emit(r, idx, needs_crc && s != expect);
      }
      // keep the row base of g' alive past its last reload: otherwise the register allocator
      // gives that load the dying address register as destination, and the loop needs a copy
      // of the in-flight row at its back edge (a full drain)
      asm volatile("" ::"v"(boff_n + (uint32_t)(pos0 + 64)));
      g = gn;
      idx = idx_n;
      live = live_n;
      // a group without any checksummed record: stop streaming bodies (the rows of g' in
      // flight are simply overwritten later)
      return has_next && any;
    };
    u32x4_t pf2;
    if (kAligned) {
      while (step(pf, pf2)) {
      }
    } else {
      for (;;) {
        if (!step(pf, pf2)) break;
        if (!step(pf2, pf)) break;
      }
    }
    // ---- header-only mode: header first, bodies only for groups that need the CRC
    for (; g < g_end; g += n_waves) {
      const uint32_t i = rec_idx(g);
      const bool lv = is_live(i);
      const u32x4_t ph = ld_hdr(base_off(lv, i));
      const bool nc = decide(ph, lv);
      if (__any(nc)) break;  // back to pipelined mode at this group
      emit(decode(ph, i, lv), i, false);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Aligned fixed-length records of NR = 8 or 16 rows (512 / 1024 B) with row output -- the
// headline layout -- reading and writing in separate phases.  On the MI355X boxes where
// mixing the 32-B row stores into the 1 GiB read stream costs most (config 2): the read
// pattern alone takes 168 us, with the row stores interleaved 201 us.  So each wave keeps
// the rows of its last K = 16 groups in registers (2 dwords per group and lane, written by a
// wave-uniform indexed move) and stores them in one burst every K groups and at its end: for
// config 2 (16 groups per wave) one burst, after the wave's reads (measured 0.194 ms against
// 0.215 ms for the interleaved kernel on the same box; K = 12 with two bursts: 0.204 ms).
// The load ring is NB blocks of BR rows per wave, each reloaded as a BLOCK: when the last of a
// block's rows is consumed, the rows RS = NB * BR further on in the wave's row stream are
// requested by BR back-to-back loads.  Rows 2j and 2j + 1 are the halves of a record's 128-byte
// line; requesting whole lines together measured 4% faster than one reload per consumed row.
// The product shape is ONE block of 4 rows (two lines per record, 4 KiB per wave, 0 .. 64 KiB
// in flight per CU) at 16 waves per workgroup, K = 16: the wave computes with nothing of its
// own in flight and the CU's other waves cover it.  Every shape that keeps more in flight --
// a second block (16 or 8 waves per workgroup, K = 32 at 8), or one block of 8 rows at 16
// waves -- measured 6-7% SLOWER on config 2 (0.199 against 0.186 ms, DESIGN 4.1 "r08"; of
// those the diagnostics build keeps the two-block shape, launch_unpack variant 18).  What did pay there
// is the kind of load: the loads that open a group in the ring are non-temporal (kNt), the
// reloads inside the group plain: 0.1744 against 0.1873 ms.
// A ring of two records' rows (512-byte records with RS = 16, diagnostics only) runs two
// groups per loop trip so that every ring index stays static.
// Semantics are those of unpack_fixed_kernel<NR, 0, true, true>.
template <int NR, int BR = 4, int NB = 1, int K = 16, int NW = 16, bool kNt = false>
__global__ void __launch_bounds__(NW * 64)
unpack_fixed_ring_kernel(UnpackParams p, uint32_t expect) {
  // BR: rows per load block; NB: blocks in a wave's ring; K: groups of row output held per
  // wave before a burst; NW: waves per workgroup
  constexpr int RS = NB * BR;               // rows in the ring
  constexpr int G = RS > NR ? RS / NR : 1;  // groups the ring holds rows of
  static_assert(NR == 8 || NR == 16, "ring kernel: 512- or 1024-byte records");
  static_assert(NR % BR == 0, "a block lies inside one record");
  static_assert(RS <= NR ? NR % RS == 0 : (RS == 2 * NR && BR == NR), "static ring indices");
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t* fold = lds + kRepDwords;  // [A4 | A8 | A12 | A16 | A32 | A48]
  const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(lds);
  const TableRegs<NW * 64> tab_regs = table_loads<NW * 64>(p.tabs);
  asm volatile("" ::: "memory");

  const int lane = threadIdx.x & 63;
  const int q = lane & 3;
  const uint32_t s1 = a64_s1((uint32_t)lane);
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(
      blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t g_end = (p.n + 15u) >> 4;
  const bool force = (p.opts & MGENX_OPT_CHECKSUM_FORCE) != 0;
  const bool tcp = (p.opts & MGENX_OPT_TCP) != 0;
  const uint32_t L = p.fixed_len;  // == 64 * NR (host-checked)

  auto rec_idx = [&](uint32_t gg) { return (gg << 4) + (uint32_t)(lane >> 2); };
  // (no short-circuit: the three compares are cheaper than the branches around them)
  auto is_live = [&](uint32_t i) {
    const uint64_t off = (uint64_t)i * p.stride;
    return (bool)((i < p.n) & (off <= p.slab_bytes) & (L <= p.slab_bytes - off));
  };
  // lane's row base (32-bit offset, saddr form); a dead lane reads inside the slab at 64
  auto row_base = [&](uint32_t i, bool live) {
    return (live ? i * (uint32_t)p.stride : 64u) + 16u * (uint32_t)q;
  };
  // quad lane q keeps dwords 2q, 2q + 1 of the record's row: lane masks, not branches
  const uint32_t qm0 = 0u - (uint32_t)(q == 0), qm1 = 0u - (uint32_t)(q == 1);
  const uint32_t qm2 = 0u - (uint32_t)(q == 2), qm3 = 0u - (uint32_t)(q == 3);
  // the loads that bring a group into the ring (the prime, and the reloads with rows of a later
  // group); kNt: non-temporal.  Reloads with later rows of the group being folded (a ring
  // shorter than a record) are always plain loads -- that mix is what was measured, DESIGN 4.1
  auto ld = [&](uint32_t base, int j) {
    const uint8_t* a = p.slab + (uint64_t)base + 64 * j;
    return kNt ? ldnt128(a) : ldu128(a);
  };
  auto decide = [&](const u32x4_t& pf, bool live) {
    const uint32_t w0 = prefix_word(pf, 0);
    const uint32_t w5 = prefix_word(pf, 5);
    const bool v2 = ((w0 >> 16) & 0xffu) == 2u;
    const bool flagged = force || ((((w0 >> 24) & MGENX_FLAG_CHECKSUM) != 0) && v2);
    const uint32_t t = (w5 >> 16) & 0xffu;
    return live && flagged && (tcp || (v2 && (t == 1u || t == 2u)));
  };
  // the quad's 32-B mgenx_rec: lane q holds bytes 8q .. 8q+7 (as unpack_fixed_kernel)
  auto decode = [&](const u32x4_t& pf, uint32_t idx, bool live, uint32_t& o0, uint32_t& o1) {
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = prefix_word(pf, j);
    const uint32_t w10 = prefix_word(pf, 10);
    const uint32_t D = w[5] >> 24;
    const uint32_t hw = (D == 4u) ? w[7] : w10;
    const uint32_t gi = (28u + D + (hw >> 24)) >> 2;
    const uint32_t g3 = (prefix_word(pf, 11) & (0u - (uint32_t)(gi == 8u))) |
                        (prefix_word(pf, 12) & (0u - (uint32_t)(gi == 9u))) |
                        (prefix_word(pf, 14) & (0u - (uint32_t)(gi == 11u))) |
                        (prefix_word(pf, 15) & (0u - (uint32_t)(gi == 12u)));
    uint32_t flow = bswap32(w[1]), seq = bswap32(w[2]), sec = bswap32(w[3]);
    uint32_t usec = bswap32(w[4]), dst4 = w[6];
    uint32_t msg_len = bswap16((uint16_t)(w[0] & 0xffffu));
    uint32_t dport = bswap16((uint16_t)(w[5] & 0xffffu));
    const uint32_t hlen = 44u + D + (hw >> 24);
    uint32_t plen = bswap16((uint16_t)(g3 >> 16));
    if (!(plen != 0 && hlen + plen <= L)) plen = 0;  // mgenMsg.cpp:488-497
    uint32_t flags = w[0] >> 24, err = 0, dtype = (w[5] >> 16) & 0xffu, dlen = D;
    uint32_t ptype = (g3 >> 8) & 0xffu, gps = g3 & 0xffu;
    const bool slow = live && !fast_layout(w[0], w[5], hw);
    if (__any(slow)) {
      Hdr h;
      if (slow && q == 0) parse_header(p.slab + (uint64_t)idx * p.stride, L, false, w, h);
      auto bc = [&](uint32_t& dst, uint32_t v) {
        v = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, false);
        if (slow) dst = v;
      };
      bc(flow, h.flow); bc(seq, h.seq); bc(sec, h.sec); bc(usec, h.usec); bc(dst4, h.dst4);
      bc(msg_len, h.msg_len); bc(dport, h.dst_port); bc(plen, h.plen); bc(flags, h.flags);
      bc(err, h.err); bc(dtype, h.dst_type); bc(dlen, h.dst_len); bc(ptype, h.ptype);
      bc(gps, h.gps);
    }
    const uint32_t a3 = plen | flags << 16 | err << 24;
    const uint32_t c3 = dtype | dlen << 8 | ptype << 16 | gps << 24;
    const uint32_t c2 = msg_len | dport << 16;
    const uint32_t r0 = (flow & qm0) | (sec & qm1) | (dst4 & qm2) | (a3 & qm3);
    const uint32_t r1 = (seq & qm0) | (usec & qm1) | (c2 & qm2) | (c3 & qm3);
    // a dead lane: every field 0, err = OOB
    o0 = live ? r0 : (qm3 & ((uint32_t)MGENX_ERROR_OOB << 24));
    o1 = live ? r1 : 0u;
  };
  // the caller's receive check (mgenTransport.cpp:971): ERROR_CHECKSUM (+ TCP flag) in word 6
  auto verdict = [&](uint32_t& o0, bool crc_bad) {
    const uint32_t fl = tcp ? (uint32_t)MGENX_FLAG_CHECKSUM_ERROR : 0u;
    if (crc_bad && q == 3) o0 = (o0 & 0x00ffffffu) | fl << 16 | (uint32_t)MGENX_ERROR_CHECKSUM << 24;
  };

  // ---- row output held per wave: slot k of buf, `held` groups pending.  A group's row goes
  // to slot `slot` by a wave-uniform indexed move (no shift of the held rows); a burst's
  // first slot is K - (groups in that burst), so at flush time slot k always belongs to
  // group last_g - (K - 1 - k) * n_waves
  typedef uint32_t held_t __attribute__((ext_vector_type(K)));
  held_t b0 = 0u, b1 = 0u;
  uint32_t held = 0, last_g = 0;
  // groups this wave still has to push (wave-uniform)
  uint32_t left = __builtin_amdgcn_readfirstlane(
      wave_id < g_end ? (g_end - 1u - wave_id) / n_waves + 1u : 0u);
  uint32_t slot = (uint32_t)K - (left < (uint32_t)K ? left : (uint32_t)K);
  auto push = [&](uint32_t o0, uint32_t o1, uint32_t gg) {
    const uint32_t us = __builtin_amdgcn_readfirstlane(slot);  // one indexed move each
    b0[us] = o0;
    b1[us] = o1;
    slot++;
    held++;
    left--;
    last_g = gg;
  };
  auto flush = [&]() {  // buf[k] belongs to group last_g - (K - 1 - k) * n_waves
#pragma unroll
    for (int k = 0; k < K; k++) {
      const uint32_t back = (uint32_t)(K - 1 - k);
      const uint32_t gg = last_g - back * n_waves;
      const uint32_t idx = rec_idx(gg);
      const bool in = back < held && idx < p.n;
      const uint64_t v = (uint64_t)b1[k] << 32 | b0[k];
      if (back < held)  // wave-uniform
        st_g64_nt(in ? (uint64_t)p.cols.rows + (uint64_t)idx * 32 + 8 * q
                     : (uint64_t)p.sink + 8u * (uint32_t)lane, v);
    }
    held = 0;
    slot = (uint32_t)K - (left < (uint32_t)K ? left : (uint32_t)K);
  };

  u32x4_t d[RS];
  // The ring holds rows of G consecutive groups of the wave: slot s (ring rows s * NR ..) those
  // of group g + s * n_waves.  idxq / liveq: record index and liveness of those groups' lanes;
  // base: the row base of group g (only a ring shorter than a record reads more of group g).
  uint32_t g = wave_id;
  uint32_t idxq[G];
  bool liveq[G];
  uint32_t base = 0;
  // the whole ring, from group g on (a group past the wave's last: group g's rows again)
  auto prime = [&]() {
    const uint32_t g0 = g < g_end ? g : 0u;
#pragma unroll
    for (int s = 0; s < G; s++) {
      const uint32_t gs = g + (uint32_t)s * n_waves;
      idxq[s] = rec_idx(gs < g_end ? gs : g0);
      liveq[s] = is_live(idxq[s]);
      const uint32_t b = row_base(idxq[s], liveq[s]);
      if (s == 0) base = b;
#pragma unroll
      for (int j = 0; j < (RS < NR ? RS : NR); j++) {
        d[s * NR + j] = ld(b, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  prime();
  table_writes(lds, tab_regs);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (g >= g_end) return;

  // One pipelined group: group g, whose rows sit in slot S of the ring.  When the last row of
  // a block has been read out of the ring, the block's BR registers are reloaded in place, back
  // to back, with the rows RS further on in the wave's row stream: later rows of group g (a
  // ring shorter than a record), or the same block of group g + G * n_waves.  So NB - 1 blocks
  // are in flight while one is folded.  Returns whether the wave's next group is pipelined too.
  // `run` (wave-uniform; constant true unless G = 2) = false: there is no such group, and the
  // step only requests the slot's last block again, so that the loads in flight are in the
  // same order on every path through the loop (the compiler's waits count on that order).
  auto step = [&](auto slot_c, bool run) -> bool {
    constexpr int S = decltype(slot_c)::value;
    constexpr auto ri = [](int j) { return (S * NR + j) % RS; };  // ring index of g's row j
    const uint32_t idx = idxq[0];
    const bool live = liveq[0];
    const bool has_next = g + n_waves < g_end;
    const uint32_t gn = g + (uint32_t)G * n_waves;  // the group whose rows are requested here
    const uint32_t idx_n = rec_idx(gn < g_end ? gn : g);
    const bool live_n = is_live(idx_n);
    const uint32_t base_n = row_base(idx_n, live_n);
    bool needs_crc = false, any = false;
    uint32_t o0 = 0u, o1 = 0u, f0 = 0u, f1 = 0u, f2 = 0u, f3 = 0u;
    if (run) {
      const u32x4_t hdr = d[ri(0)];  // row 0 = the 64-byte header prefix (aligned)
      needs_crc = decide(hdr, live);
      any = __any(needs_crc);
      decode(hdr, idx, live, o0, o1);
      uint32_t ha[4] = {0u, 0u, 0u, 0u}, hb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < NR - 1; j++) {
        const u32x4_t x = d[ri(j)];
        const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
        uint32_t c4[4];
#pragma unroll
        for (int b = 0; b < 4; b++) c4[b] = xor3(ha[b], hb[b], xw[b]);
        __builtin_amdgcn_sched_barrier(0);
        // the block's last row is out of the ring: reload the block
        if ((j % BR) == BR - 1) {
#pragma unroll
          for (int t = j - (BR - 1); t <= j; t++) {
            if (t + RS < NR) d[ri(t)] = ldu128(p.slab + (uint64_t)base + 64 * (t + RS));
            else d[ri(t)] = ld(base_n, (t + RS) % NR);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 4; b++) a64_parts(ldsb, c4[b], s1, ha[b], hb[b]);
      }
      const u32x4_t xf = d[ri(NR - 1)];
      f0 = xor3(ha[0], hb[0], xf.x);
      f1 = xor3(ha[1], hb[1], xf.y);
      f2 = xor3(ha[2], hb[2], xf.z);
      f3 = xor3(ha[3], hb[3], q == 3 ? bswap32(xf.w) : xf.w);
    }
    asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = NR - BR; t < NR; t++) d[ri(t)] = ld(base_n, (t + RS) % NR);
    __builtin_amdgcn_sched_barrier(0);
    if (run) {
      const uint32_t v = shift_tab(fold + 3 * 1024, f0) ^ shift_tab(fold + 2 * 1024, f1) ^
                         shift_tab(fold + 1 * 1024, f2) ^ shift_tab(fold, f3);
      const uint32_t* lt = fold + (q == 0 ? 5 : (q == 1 ? 4 : 3)) * 1024;  // A48/A32/A16
      uint32_t sum = (q == 3) ? v : shift_tab(lt, v);
      sum ^= __shfl_xor(sum, 1);
      sum ^= __shfl_xor(sum, 2);
      verdict(o0, needs_crc && sum != expect);
      push(o0, o1, g);
      if (held == (uint32_t)K) flush();
      g += n_waves;
#pragma unroll
      for (int s = 0; s + 1 < G; s++) {
        idxq[s] = idxq[s + 1];
        liveq[s] = liveq[s + 1];
      }
      idxq[G - 1] = idx_n;
      liveq[G - 1] = live_n;
      if (G == 1) base = base_n;
    }
    // a group without checksummed records: its successors run header-only (the rows of
    // the following groups in flight are simply overwritten later)
    return run && has_next && any;
  };

  // Two modes, each in its own loop.  The pipelined loop is the only place that redefines
  // the ring inside a loop, and it does so in place; G groups per trip, so that every ring
  // index is static.  The header-only loop never touches the ring, and the switch back
  // re-primes the whole of it outside both.  (In one mixed loop the header-only path's second
  // definition of the ring made LLVM copy the whole ring at the back edge.)
  for (;;) {
    // ---- pipelined groups: slot 0 of the ring holds the rows of group g
    if (G == 1) {
      while (step(std::integral_constant<int, 0>{}, true)) {
      }
    } else {
      // Two groups per trip, and no way out of the loop between them: the compiler
      // structurizes this loop (its body has divergent branches), which turns an exit after the
      // first step into a path around the second one to the back edge.  Along that path the
      // first slot's reloads would be the youngest loads, and every wait of the first step
      // would become a drain of both blocks (seen in the assembly: vmcnt(7) .. (0)).
      bool more;
      do {
        const bool two = step(std::integral_constant<int, 0>{}, true);
        more = step(std::integral_constant<int, G - 1>{}, two);
      } while (more);
    }
    // ---- header-only groups: header first, body only when a record needs the CRC
    for (; g < g_end; g += n_waves) {
      const uint32_t i = rec_idx(g);
      const bool lv = is_live(i);
      // (a plain load: the line is read again if the group turns out to need the CRC)
      const u32x4_t ph = ldu128(p.slab + (uint64_t)row_base(i, lv));
      if (__any(decide(ph, lv))) break;
      uint32_t o0, o1;
      decode(ph, i, lv, o0, o1);
      push(o0, o1, g);
      if (held == (uint32_t)K) flush();
    }
    if (g >= g_end) break;
    // ---- back to the pipelined mode at group g
    prime();
  }
  if (held) flush();
}

template <int NR, int MODE = 0, bool kRows = false, bool kAligned = false>
static hipError_t launch_fixed(const UnpackParams& p, int grid, hipStream_t stream) {
  const auto kernel = unpack_fixed_kernel<NR, MODE, kRows, kAligned>;
  hipError_t e = set_max_lds((const void*)kernel, (int)kUnpackLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kUnpackThreads), kUnpackLdsBytes, stream, p,
                     p.expect_fixed);
  return hipGetLastError();
}

// The ring kernel sizes its own grid: one workgroup of NW waves per CU, a group per wave at
// least -- min(ceil(groups / NW), CUs).
template <int NR, int BR = 4, int NB = 1, int K = 16, int NW = 16, bool kNt = false>
static hipError_t launch_ring(const UnpackParams& p, int cus, hipStream_t stream) {
  const auto kernel = unpack_fixed_ring_kernel<NR, BR, NB, K, NW, kNt>;
  hipError_t e = set_max_lds((const void*)kernel, (int)kUnpackLdsBytes);
  if (e != hipSuccess) return e;
  const uint64_t groups = ((uint64_t)p.n + 15) / 16;
  uint64_t grid = (groups + NW - 1) / NW;
  if (grid > (uint64_t)cus) grid = (uint64_t)cus;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(NW * 64), kUnpackLdsBytes, stream, p,
                     p.expect_fixed);
  return hipGetLastError();
}

// Non-temporal ring loads, by batch size (scripts/ring_shapes.py, plain against non-temporal,
// us per launch on one MI355X, the same slab read again by every launch):
//   1024-B records   65,536: 16.9 / 16.5   131,072: 27.0 / 26.3   1,048,576: 185.5 / 172.6
//    512-B records  131,072: 15.6 / 16.2   262,144: 26.1 / 26.9   393,216: 36.5 / 36.4
//                   524,288: 47.2 / 46.1   1,048,576: 97.5 / 85.3
// So 1024-byte records always load non-temporally, 512-byte records from 393,216 records
// (24,576 groups) up.
constexpr uint32_t kRingNt512Groups = 24576;

typedef hipError_t (*fixed_launcher)(const UnpackParams&, int, hipStream_t);
#define MGENX_FIXED_TABLE(R)                                                              \
  {nullptr, nullptr, launch_fixed<2, 0, R>, launch_fixed<3, 0, R>, launch_fixed<4, 0, R>,    \
   launch_fixed<5, 0, R>, launch_fixed<6, 0, R>, launch_fixed<7, 0, R>, launch_fixed<8, 0, R>, \
   launch_fixed<9, 0, R>, launch_fixed<10, 0, R>, launch_fixed<11, 0, R>,                    \
   launch_fixed<12, 0, R>, launch_fixed<13, 0, R>, launch_fixed<14, 0, R>,                   \
   launch_fixed<15, 0, R>, launch_fixed<16, 0, R>}
static const fixed_launcher kFixedLaunch[17] = MGENX_FIXED_TABLE(false);
static const fixed_launcher kFixedLaunchRows[17] = MGENX_FIXED_TABLE(true);
#undef MGENX_FIXED_TABLE

hipError_t launch_fixed_product(const UnpackParams& p, int grid, int cus, hipStream_t stream) {
  const mgenx_cols& c = p.cols;
  // 256 / 512 / 1024-byte records: the aligned variant (header = row 0)
  switch (p.fixed_len) {
    case 256: return c.rows ? launch_fixed<4, 0, true, true>(p, grid, stream)
                            : launch_fixed<4, 0, false, true>(p, grid, stream);
    case 512:
      if (!c.rows) return launch_fixed<8, 0, false, true>(p, grid, stream);
      return (p.n + 15u) / 16u >= kRingNt512Groups
                 ? launch_ring<8, 4, 1, 16, 16, true>(p, cus, stream)
                 : launch_ring<8, 4, 1, 16, 16, false>(p, cus, stream);
    case 1024: return c.rows ? launch_ring<16, 4, 1, 16, 16, true>(p, cus, stream)
                             : launch_fixed<16, 0, false, true>(p, grid, stream);
    default: break;
  }
  return (c.rows ? kFixedLaunchRows : kFixedLaunch)[(p.fixed_len + 63) / 64](p, grid, stream);
}

#if MGENX_DIAG
template <int M, bool kAligned>
hipError_t launch_fixed_1024(const UnpackParams& p, int grid, int, hipStream_t stream) {
  return p.cols.rows ? launch_fixed<16, M, true, kAligned>(p, grid, stream)
                     : launch_fixed<16, M, false, kAligned>(p, grid, stream);
}
template <int BR, int NB, int K, int NW, bool kNt>
hipError_t launch_ring_shape(const UnpackParams& p, int, int cus, hipStream_t stream) {
  return p.fixed_len == 1024 ? launch_ring<16, BR, NB, K, NW, kNt>(p, cus, stream)
                             : launch_ring<8, BR, NB, K, NW, kNt>(p, cus, stream);
}
// launch_unpack's variants 12 and 13, 1024 + M, and 17, 18, 28
#define MGENX_LAUNCHER(...) \
  template hipError_t __VA_ARGS__(const UnpackParams&, int, int, hipStream_t);
MGENX_LAUNCHER(launch_fixed_1024<0, false>)
MGENX_LAUNCHER(launch_fixed_1024<0, true>)
#define MGENX_ABL(M) MGENX_LAUNCHER(launch_fixed_1024<M, true>)
MGENX_FIXED_ABL_MODES(MGENX_ABL)
#undef MGENX_ABL
MGENX_LAUNCHER(launch_ring_shape<4, 1, 16, 16, false>)
MGENX_LAUNCHER(launch_ring_shape<8, 2, 32, 8, false>)
MGENX_LAUNCHER(launch_ring_shape<4, 1, 16, 16, true>)
#undef MGENX_LAUNCHER
#endif  // MGENX_DIAG

}  // namespace mgenx
