// mgenx_unpack_var.hpp -- unpack + receive CRC for batches with per-record lengths: the kernel
// and its launcher.  Compiled as part of mgenx_unpack.hip (see there) and nowhere else.
#pragma once

#include "mgenx_unpack.hpp"

namespace mgenx {

// Variable-length records (per-record lengths: config 3, TCP / SINK scan output), with the
// rows streamed through a load ring across groups.  The braid CRC and the column output
// are those of unpack_kernel<true>; what differs is the schedule:
//   * each wave takes tiles of 64 consecutive records, ranks them by row count R (64 lane
//     compares) and runs them as four groups of 16 records of similar length;
//   * a group's virtual rows are V = max R of its records rounded up to an even count >= 4
//     (shorter records front-padded with zero rows, which leave the zero CRC state as is);
//   * the wave's rows form ONE stream over its groups, with RS = 4 rows in flight: row
//     r + 4 of the stream is loaded as row r is consumed -- during a group's last four rows
//     that is the next group's first four rows (its header follows the group's column
//     stores) -- so the loads never drain at group boundaries (the next tile is ranked one group ahead,
//     its placements loaded one tile ahead).
// No header-first mode: every record's rows are read (for batches without checksummed
// records this reads the bodies too; the payload stays unread by the CRC work otherwise).
// Row output (r03): the rows of the last KB groups are held in registers (lo / hi word of
// the quad lane's 8 bytes and the record index) and stored in one burst every KB groups, as
// the ring kernel does, instead of one row store per group mixed into the read stream.
// Config 3 (`scripts/var_shapes.py`): per-group stores 0.250 ms, KB = 4 0.236 ms, every row
// store sent to one scratch line (MODE 1, the bound of any store schedule) 0.223 ms.  KB = 8
// spills 23 VGPRs at the 128-VGPR limit of 16 waves per CU (0.240 ms); 12 waves per CU with
// KB = 8 or 16 fit the registers but lose the loads in flight (0.245-0.253 ms); flushing at
// each tile's end with the indices recomputed from the rank permutation 0.239 ms;
// non-temporal row stores 0.241-0.246 ms; tiles handed out by an atomic ticket (dynamic
// balance) 0.32-0.44 ms; (r04) a tile's 64 rows gathered by lane permutes and stored as 2 KiB
// of whole lines (two 16-B stores per lane instead of four scattered 8-B ones) 0.2359 ms
// against 0.2361 (15 VGPRs spilled; the partial-line writes are not what costs).
// One block of kUnpackThreads threads per CU (the LDS tables), KB = 4 groups of rows held.
// MODE (ablations, diagnostics build; 0 = the product kernel): bit 1: every core store to the
// sink; bit 8: non-temporal row stores; bit 16: every row load 64-byte aligned (wrong data,
// timing only).
template <int MODE>
__global__ void __launch_bounds__(kUnpackThreads)
unpack_var_kernel(UnpackParams p) {
  constexpr int KB = 4;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t* fold = lds + kRepDwords;  // [A4 | A8 | A12 | A16 | A32 | A48]
  stage_tables(lds, p.tabs);
  __syncthreads();
  const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(lds);

  const int lane = threadIdx.x & 63;
  const int q = lane & 3;
  const uint32_t s1 = a64_s1((uint32_t)lane);
  const uint64_t wave_id = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t n_tiles = ((uint64_t)p.n + 63) >> 6;
  if (wave_id >= n_tiles) return;  // (no barrier below)
  const bool force = (p.opts & MGENX_OPT_CHECKSUM_FORCE) != 0;
  const bool tcp = (p.opts & MGENX_OPT_TCP) != 0;
  const bool want_ext = p.cols.dst_addr || p.cols.host_addr;
  // any_ext_cols(p.cols), written out: through the call this kernel's register allocation
  // changes throughout (compared as assembly), and the kernel was tuned as it is
  const mgenx_cols& cc = p.cols;
  const bool any_ext = cc.hdr_len || cc.payload_off || cc.host_port || cc.host_type ||
                       cc.host_len || cc.lat_raw || cc.lon_raw || cc.alt || cc.dst_addr ||
                       cc.host_addr || cc.decoded;
  const uint8_t* dummy = reinterpret_cast<const uint8_t*>(p.tabs);
  const u32x4_t zero = {0u, 0u, 0u, 0u};

  // ---- tiles: placements of the 64 records (lane j: record t0 + j) and their order ----
  auto place = [&](uint64_t t, uint64_t& off, uint32_t& L) {
    const uint64_t ri = (t << 6) + (uint64_t)lane;
    off = 0;
    L = 0;
    if (t < n_tiles && ri < p.n) {
      off = p.rec_off ? p.rec_off[ri] : ri * p.stride;
      L = p.rec_len ? p.rec_len[ri] : p.fixed_len;
    }
  };
  auto n_valid_of = [&](uint64_t t) { return (uint32_t)min((uint64_t)64, (uint64_t)p.n - (t << 6)); };
  // sorted position r -> the tile lane holding it
  auto rank_tile = [&](uint64_t t, uint32_t L) {
    const uint32_t key = (uint32_t)lane < n_valid_of(t) ? (L + 63u) >> 6 : 0xFFFFu;
    uint32_t rank = 0;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
      const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
      rank += (kj < key || (kj == key && j < lane)) ? 1u : 0u;
    }
    return __builtin_amdgcn_ds_permute((int)(rank << 2), lane);
  };
  // the wave's tiles: wave_id, + n_waves, ...
  uint64_t t_c = wave_id, off_c, off_p;
  uint64_t t_p = t_c + n_waves;
  uint32_t len_c, len_p;
  place(t_c, off_c, len_c);
  int src_c = rank_tile(t_c, len_c), src_p = lane;
  place(t_p, off_p, len_p);
  bool p_ranked = false;

  // ---- rows held per group: lo / hi word of the quad lane's 8 bytes, record index
  // (~0: the record's row is not the burst's -- a slow-layout or out-of-bounds record, stored
  // at once by quad lane 0)
  uint32_t b0[KB], b1[KB], bi[KB];
#pragma unroll
  for (int j = 0; j < KB; j++) b0[j] = b1[j] = 0u, bi[j] = 0xFFFFFFFFu;
  uint32_t held = 0;
  const bool burst = p.cols.rows != nullptr && !(MODE & 1);
  auto st_row = [&](uint64_t a, uint64_t v) {
    if (MODE & 8) st_g64_nt(a, v);
    else st_g64(a, v);
  };
  auto flush = [&]() {
#pragma unroll
    for (int j = 0; j < KB; j++) {
      const uint32_t back = (uint32_t)(KB - 1 - j);
      if (back < held)  // wave-uniform
        st_row(bi[j] != 0xFFFFFFFFu ? (uint64_t)p.cols.rows + (uint64_t)bi[j] * 32 + 8u * q
                                    : (uint64_t)p.sink + 8u * (uint32_t)lane,
               (uint64_t)b1[j] << 32 | b0[j]);
    }
    held = 0;
  };

  // ---- a group: the quad's record and its row geometry ----
  struct Grp {
    uint64_t off;
    uint32_t idx, L;
    int pos0, pad;        // row 0 position in the record (+16q), virtual rows before row 0
    bool valid, live, oob;
    uint32_t V;           // virtual rows (wave-uniform, even, >= 4)
  };
  auto make = [&](uint64_t t, int k, uint64_t offs, uint32_t lens, int src) {
    Grp g;
    const int li = __builtin_amdgcn_ds_bpermute((16 * k + (lane >> 2)) << 2, src);
    const int at = li << 2;
    g.idx = (uint32_t)(t << 6) + (uint32_t)li;
    g.off = (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)(uint32_t)offs) |
            (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)(uint32_t)(offs >> 32)) << 32;
    g.L = (uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)lens);
    g.valid = (uint32_t)li < n_valid_of(t);
    g.oob = g.valid && (g.L > 65535u || g.off > p.slab_bytes || g.L > p.slab_bytes - g.off);
    g.live = g.valid && !g.oob;
    const int R = (g.live && g.L >= 32) ? (int)((g.L + 63u) >> 6) : 0;
    int m = R;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) m = max(m, __shfl_xor(m, sft));
    g.V = (uint32_t)max(4, (__builtin_amdgcn_readfirstlane(m) + 1) & ~1);
    g.pad = (int)g.V - R;
    g.pos0 = (int)g.L - 64 * R + 16 * q;
    return g;
  };
  auto row_ptr = [&](const Grp& g, int j) {
    const int real = j - g.pad;
    if (MODE & 16) {  // (ablation, timing only: every row load 64-byte aligned, wrong data)
      const uint64_t a = (g.off + (uint64_t)max(g.pos0 - 16 * q + 64 * real, 0)) & ~(uint64_t)63;
      return (real >= 0) ? p.slab + a + 16u * (uint32_t)q : dummy;
    }
    return (real >= 0) ? p.slab + g.off + (uint64_t)max(g.pos0 + 64 * real, 0) : dummy;
  };
  auto hdr_ptr = [&](const Grp& g) {
    return (g.live && g.L >= 16u * (q + 1)) ? p.slab + g.off + 16 * q : dummy;
  };
  // row j's 16 bytes as the braid consumes them: row 0 of a record that does not start on
  // a row boundary is shifted up (its bytes before the record read as zero)
  auto row_data = [&](const Grp& g, const u32x4_t& x, int j) {
    const int real = j - g.pad;
    u32x4_t y = real >= 0 ? x : zero;
    const int s0 = g.pos0 < 0 ? -g.pos0 : 0;
    if (__any(real == 0 && s0 > 0)) {
      const u32x4_t sh = s0 < 16 ? shl_bytes(x, s0 & 15) : zero;
      if (real == 0) y = sh;
    }
    return y;
  };

  // ---- the first group ----
  int k = 0;
  int rho = 0;  // ring slot of the current group's row 0
  Grp G = make(t_c, 0, off_c, len_c, src_c);
  u32x4_t d[4];
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = ldu128(row_ptr(G, j));
  u32x4_t pf = ldu128(hdr_ptr(G));
  uint32_t expect = p.expect[G.live ? G.L : 0u];

  for (;;) {
    // the next group: this tile's group k + 1, or the next tile's first (ranked here)
    bool has_next = true, next_tile = false;
    Grp N;
    if (k + 1 < 4 && (uint32_t)(16 * (k + 1)) < n_valid_of(t_c)) {
      N = make(t_c, k + 1, off_c, len_c, src_c);
    } else if (t_p < n_tiles) {
      if (!p_ranked) {
        src_p = rank_tile(t_p, len_p);
        p_ranked = true;
      }
      N = make(t_p, 0, off_p, len_p, src_p);
      next_tile = true;
    } else {
      has_next = false;
      N = G;
      N.V = 4;
      N.pad = 4;  // all padding: the ring loads the dummy line
    }

    // ---- stream G's rows: chunks of 4, the last chunk feeding N's first rows ----
    uint32_t ha[4] = {0u, 0u, 0u, 0u}, hb[4] = {0u, 0u, 0u, 0u};
    auto consume = [&](const u32x4_t& y) {
      const uint32_t xw[4] = {y.x, y.y, y.z, y.w};
      uint32_t c4[4];
#pragma unroll
      for (int b = 0; b < 4; b++) c4[b] = xor3(ha[b], hb[b], xw[b]);
#pragma unroll
      for (int b = 0; b < 4; b++) a64_parts(ldsb, c4[b], s1, ha[b], hb[b]);
    };
    // G's row r sits in ring slot (r + rho) & 3 (rho in {0, 2}: V is even, not necessarily a
    // multiple of 4, so a group may start mid-ring); each variant keeps every slot index
    // static (a register copy of an in-flight row would make LLVM drain the ring)
    auto tail = [&](auto RT, int jl) {  // the last 4 rows, reloading N's rows 0..3
      constexpr int T = decltype(RT)::value;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const u32x4_t y = row_data(G, d[(j + T) & 3], jl + j);
        __builtin_amdgcn_sched_barrier(0);
        d[(j + T) & 3] = ldu128(row_ptr(N, j));
        __builtin_amdgcn_sched_barrier(0);
        consume(y);
      }
      u32x4_t xf = row_data(G, d[(3 + T) & 3], jl + 3);
      __builtin_amdgcn_sched_barrier(0);
      d[(3 + T) & 3] = ldu128(row_ptr(N, 3));
      __builtin_amdgcn_sched_barrier(0);
      if (q == 3) xf.w = bswap32(xf.w);  // the big-endian trailer, in stream order
      const uint32_t v = shift_tab(fold + 3 * 1024, xor3(ha[0], hb[0], xf.x)) ^
                         shift_tab(fold + 2 * 1024, xor3(ha[1], hb[1], xf.y)) ^
                         shift_tab(fold + 1 * 1024, xor3(ha[2], hb[2], xf.z)) ^
                         shift_tab(fold, xor3(ha[3], hb[3], xf.w));
      const uint32_t* lt = fold + (q == 0 ? 5 : (q == 1 ? 4 : 3)) * 1024;  // A48/A32/A16
      uint32_t t = (q == 3) ? v : shift_tab(lt, v);
      t ^= __shfl_xor(t, 1);
      t ^= __shfl_xor(t, 2);
      return t;
    };
    auto run = [&](auto RHO) {
      constexpr int R0 = decltype(RHO)::value;
      const int nc = (int)((G.V - 4) >> 2);  // whole chunks before the tail
#pragma unroll 1
      for (int c = 0; c < nc; c++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const u32x4_t y = row_data(G, d[(j + R0) & 3], 4 * c + j);
          __builtin_amdgcn_sched_barrier(0);
          d[(j + R0) & 3] = ldu128(row_ptr(G, 4 * c + 4 + j));
          __builtin_amdgcn_sched_barrier(0);
          consume(y);
        }
      }
      const int r0 = 4 * nc;
      if (G.V & 2u) {  // two rows more, then the tail two slots further round the ring
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const u32x4_t y = row_data(G, d[(j + R0) & 3], r0 + j);
          __builtin_amdgcn_sched_barrier(0);
          d[(j + R0) & 3] = ldu128(row_ptr(G, r0 + 4 + j));
          __builtin_amdgcn_sched_barrier(0);
          consume(y);
        }
        return tail(std::integral_constant<int, R0 ^ 2>{}, r0 + 2);
      }
      return tail(std::integral_constant<int, R0>{}, r0);
    };
    uint32_t tot = rho ? run(std::integral_constant<int, 2>{}) : run(std::integral_constant<int, 0>{});
    rho = (rho + (int)G.V) & 3;

    // ---- G's columns (as unpack_kernel) ----
    {
      uint32_t pw[16];
      quad_bcast<0>(pf, pw);
      quad_bcast<1>(pf, pw);
      quad_bcast<2>(pf, pw);
      quad_bcast<3>(pf, pw);
      const uint8_t* rec = p.slab + G.off;
      const uint32_t buf_len = tcp ? min(G.L, (uint32_t)MGENX_TX_BUFFER_SIZE) : G.L;
      // fast layouts: every quad lane derives the fields from the prefix words and the
      // quad stores them branch-free (lane q: column group q); other records: quad lane 0
      const uint32_t D = pw[5] >> 24;
      const uint32_t hw = (D == 4u) ? pw[7] : pw[10];
      const bool fast = G.live && buf_len >= 64 && fast_layout(pw[0], pw[5], hw);
      {
        const uint32_t gi = (28u + D + (hw >> 24)) >> 2;
        const uint32_t g3 = (pw[11] & (0u - (uint32_t)(gi == 8u))) |
                            (pw[12] & (0u - (uint32_t)(gi == 9u))) |
                            (pw[14] & (0u - (uint32_t)(gi == 11u))) |
                            (pw[15] & (0u - (uint32_t)(gi == 12u)));
        const uint32_t hl = 44u + D + (hw >> 24);
        Core v;
        v.plen = bswap16((uint16_t)(g3 >> 16));
        if (!(v.plen != 0 && hl + v.plen <= buf_len)) v.plen = 0;  // mgenMsg.cpp:488-497
        const bool needs_crc = force || (((pw[0] >> 24) & MGENX_FLAG_CHECKSUM) != 0);
        uint8_t flags = (uint8_t)(pw[0] >> 24), err = 0;
        crc_verdict(!needs_crc || tot == expect, tcp, err, flags);
        v.flow = bswap32(pw[1]); v.seq = bswap32(pw[2]); v.sec = bswap32(pw[3]);
        v.usec = bswap32(pw[4]); v.dst4 = pw[6];
        v.msg_len = bswap16((uint16_t)(pw[0] & 0xffffu));
        v.dport = bswap16((uint16_t)(pw[5] & 0xffffu));
        v.flags = flags; v.err = err; v.dtype = (pw[5] >> 16) & 0xffu; v.dlen = D;
        v.ptype = (g3 >> 8) & 0xffu; v.gps = g3 & 0xffu;
        if (burst) {
          const uint32_t m0 = 0u - (uint32_t)(q == 0), m1 = 0u - (uint32_t)(q == 1);
          const uint32_t m2 = 0u - (uint32_t)(q == 2), m3 = 0u - (uint32_t)(q == 3);
          auto pick = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
            return (a & m0) | (b & m1) | (c & m2) | (d & m3);
          };
#pragma unroll
          for (int j = 0; j < KB - 1; j++) b0[j] = b0[j + 1], b1[j] = b1[j + 1];
          b0[KB - 1] = pick(v.flow, v.sec, v.dst4, (v.plen & 0xffffu) | v.flags << 16 | v.err << 24);
          b1[KB - 1] = pick(v.seq, v.usec, (v.msg_len & 0xffffu) | v.dport << 16,
                            v.dtype | v.dlen << 8 | v.ptype << 16 | v.gps << 24);
#pragma unroll
          for (int j = 0; j < KB - 1; j++) bi[j] = bi[j + 1];
          bi[KB - 1] = fast ? G.idx : 0xFFFFFFFFu;
          held++;
        } else {
          store_core_quad_m(p, G.idx, fast && !(MODE & 1), lane, q, v);
        }
      }
      if (fast && any_ext) store_fast_ext(p.cols, G.idx, [&](int kk) { return pw[kk]; }, buf_len, q == 0);
      if (!fast && G.live && q == 0) {
        uint32_t w[8];
        if (G.L >= 32) {
#pragma unroll
          for (int j = 0; j < 8; j++) w[j] = pw[j];
        } else if (G.L >= MGENX_MIN_SIZE) {
          load_fixed(rec, buf_len, w);
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) w[j] = 0;
        }
        const bool flagged = force || (((w[0] >> 24) & MGENX_FLAG_CHECKSUM) != 0 &&
                                       buf_len >= MGENX_MIN_SIZE && ((w[0] >> 16) & 0xffu) == 2u);
        const bool needs_crc = flagged && (tcp ? (G.L >= 4) : fixed_ok(buf_len, w));
        const bool vec_crc = needs_crc && G.L >= 32;
        Hdr h;
        parse_header(rec, buf_len, want_ext, w, h);
        const bool crc_ok = !needs_crc || (vec_crc ? (tot == expect) : small_crc_ok(rec, G.L));
        store_hdr_q0(p.cols, G.idx, h, crc_ok, tcp);
      } else if (G.oob && q == 0) {
        store_oob_q0(p.cols, G.idx);
      }
    }

    if (burst && held == (uint32_t)KB) flush();
    if (!has_next) break;
    // N's header: needed only after N's rows, so loaded after G's column stores
    pf = ldu128(hdr_ptr(N));
    expect = p.expect[N.live ? N.L : 0u];
    if (next_tile) {
      t_c = t_p;
      t_p = t_c + n_waves;
      off_c = off_p;
      len_c = len_p;
      src_c = src_p;
      place(t_p, off_p, len_p);
      p_ranked = false;
      k = 0;
    } else {
      k++;
    }
    G = N;
  }
  if (burst && held) flush();
}

template <int MODE>
static hipError_t launch_var(const UnpackParams& p, int grid, int, hipStream_t stream) {
  const auto kernel = unpack_var_kernel<MODE>;
  hipError_t e = set_max_lds((const void*)kernel, (int)kUnpackLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kUnpackThreads), kUnpackLdsBytes, stream, p);
  return hipGetLastError();
}

}  // namespace mgenx
