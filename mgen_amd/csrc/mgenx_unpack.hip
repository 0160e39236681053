// mgenx_unpack.hip -- batched MgenMsg::Unpack + receive-side CRC-32 check on gfx950.
//
// Reference semantics: MgenMsg::Unpack (src/common/mgenMsg.cpp:315-500) on a fresh
// MgenMsg, followed by the receive CRC check of the UDP / SINK / TCP callers
// (src/common/mgenTransport.cpp:958-975, 2092-2112, 1516-1564).
//
// Work mapping (one persistent 1024-thread workgroup per CU):
//   * a quad of 4 lanes owns one record; a wave owns 16 consecutive records;
//   * the record is covered by 64-byte rows aligned to the record END, so a quad's four
//     16-byte loads per row are one contiguous (unaligned) 64-byte span: coalesced, and
//     the CRC trailer always lands in word 3 of lane 3 of the last row;
//   * CRC: residue check.  The stream Y = [zero pad][payload bytes][LE(trailer)] is
//     reduced with zero initial state; the record is intact iff crc_raw(Y) equals
//     expect[L] = A_4(A_{L-4}(~0) ^ ~0) (init handled by linearity, no per-byte masking).
//     Each lane keeps 4 independent "braid" states (one per word of its 16-byte unit),
//     advanced row to row by the 64-byte shift operator A_64 -- one conflict-free LDS
//     table lookup per input byte (the A_64 tables are replicated 32x so lane l always
//     reads bank l).  The last row folds the braids with A_4 and the quad folds its four
//     lanes with A_16 / A_32 (shuffles);
//   * lane 0 of the quad decodes the header fields and writes the SoA columns.
// This file: the general kernel (any placement, any columns) and launch_unpack, the dispatch
// over the kernel families (mgenx_unpack.hpp lists them).
#include "mgenx_unpack.hpp"

namespace mgenx {

// MODE (diagnostic ablations, never the product path): 0 = full kernel, 1 = row loads +
// XOR only (no LDS table lookups), 2 = table lookups on one L1-resident row (no streaming).
template <bool kCrc, int MODE = 0>
__global__ void __launch_bounds__(kUnpackThreads)
unpack_kernel(UnpackParams p) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* rep = lds;
  uint32_t* fold = lds + kRepDwords;  // [A4 | A8 | A12 | A16 | A32 | A48]

  // ---- stage the shift-operator tables (A_64 replicated 32x) ----
  if (kCrc) {
    stage_tables(lds, p.tabs);
    __syncthreads();
  }
  const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(rep);

  const int lane = threadIdx.x & 63;
  const int q = lane & 3;
  const uint32_t s1 = a64_s1((uint32_t)lane);
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint64_t wave_id = (uint64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
  const uint64_t n_groups = ((uint64_t)p.n + 15) >> 4;
  const bool force = (p.opts & MGENX_OPT_CHECKSUM_FORCE) != 0;
  const bool tcp = (p.opts & MGENX_OPT_TCP) != 0;
  const bool want_ext = p.cols.dst_addr || p.cols.host_addr;
  const bool any_ext = any_ext_cols(p.cols);

  // Per-wave predictor: while recent groups carried checksummed records, issue the row
  // loads speculatively together with the header load (one memory round per group); a
  // group without any CRC work turns speculation off (header first, body only if needed).
  bool spec = true;
  // one group: the quad's record rec_idx (valid: < n), the wave's 16 records together
  // (off, L: its placement, read by the caller)
  auto group = [&](const uint64_t rec_idx, const bool valid, const uint64_t off, const uint32_t L) {
    const bool oob = valid && (L > 65535u || off > p.slab_bytes || L > p.slab_bytes - off);
    const bool live = valid && !oob;
    const uint8_t* rec = p.slab + off;
    const uint32_t buf_len = tcp ? min(L, (uint32_t)MGENX_TX_BUFFER_SIZE) : L;

    // Header prefix: lane q of the quad loads bytes [16q, 16q+16) (64 bytes per record,
    // enough for every layout but IPv6 dst + IPv6 host); quad lane 0 gathers the words by
    // DPP quad broadcast when it parses.  Loads are unconditional (clamped to a dummy line)
    // so no divergent branch forces a full vmcnt wait.
    const bool pfx = live && L >= 32;           // prefix words 0..7 valid
    const bool pfx64 = live && buf_len >= 64;   // prefix words 0..15 valid
    const uint8_t* dummy = reinterpret_cast<const uint8_t*>(p.tabs);
    u32x4_t pf = {0u, 0u, 0u, 0u};
    uint32_t w[8];
    uint32_t expect = 0;
    auto load_header = [&]() {
      pf = ldu128((live && L >= 16u * (q + 1)) ? rec + 16 * q : dummy);
      if (kCrc) expect = p.expect[live ? L : 0u];
    };
    // prefix words 0..15 of the quad's record, gathered by DPP with every lane active
    auto gather = [&](uint32_t (&pw)[16]) {
      quad_bcast<0>(pf, pw);
      quad_bcast<1>(pf, pw);
      quad_bcast<2>(pf, pw);
      quad_bcast<3>(pf, pw);
    };
    auto unpack_words = [&](const uint32_t (&pw)[16]) {
      if (pfx) {
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = pw[j];
      } else if (live && L >= MGENX_MIN_SIZE) {
        load_fixed(rec, buf_len, w);  // 28..31-byte records
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = 0;
      }
    };
    bool needs_crc = false;
    auto decide = [&]() {
      uint32_t pw[16];
      gather(pw);
      if (kCrc && live && q == 0) {  // quad lane 0 decides and stores
        unpack_words(pw);
        const bool flagged = force || (((w[0] >> 24) & MGENX_FLAG_CHECKSUM) != 0 &&
                                       buf_len >= MGENX_MIN_SIZE &&
                                       ((w[0] >> 16) & 0xffu) == 2u);
        needs_crc = flagged && (tcp ? (L >= 4) : fixed_ok(buf_len, w));
      }
    };

    uint32_t tot = 0;
    const bool speculate = kCrc && (spec || force);
    bool run_crc = speculate;
    if (!speculate) {
      load_header();
      if (kCrc) {
        decide();
        run_crc = __any(needs_crc);
      }
    }
    if (kCrc && run_crc) {
      // ---- braid CRC over end-aligned 64-byte rows ----
      // R depends only on L, so the row loads need nothing from the header.  Quads are
      // front-padded with zero rows to the wave-uniform count V (leading zeros leave a
      // zero-initialised CRC unchanged): all lanes run the same updates.
      const int R = (live && L >= 32) ? (int)((L + 63u) >> 6) : 0;
      const bool vec = R > 0;
      const int64_t row0 = (int64_t)L - 64 * (int64_t)R + 16 * q;  // position of row 0
      int Rmax = R;
#pragma unroll
      for (int sft = 1; sft < 64; sft <<= 1) Rmax = max(Rmax, __shfl_xor(Rmax, sft));
      const int V = __builtin_amdgcn_readfirstlane(Rmax);  // virtual rows 0..V-1 (V-1 final)
      const int pad = V - R;
      const bool multi = R >= 2;
      const uint8_t* base = multi ? rec + row0 : reinterpret_cast<const uint8_t*>(p.tabs);
      const int hi_row = multi ? R - 1 : 0;
      auto row_addr = [&](int j) {
        const int real = j - pad;
        const int rr = real < 1 ? 1 : (real > hi_row ? hi_row : real);
        return base + 64 * (multi ? (MODE == 2 ? 1 : rr) : 0);
      };
      // braid state word b = ha[b] ^ hb[b] (kept split so the next row folds in one XOR3)
      uint32_t ha[4] = {0u, 0u, 0u, 0u}, hb[4] = {0u, 0u, 0u, 0u};
      const u32x4_t zero = {0u, 0u, 0u, 0u};
      u32x4_t xr = zero, xf = zero;
      // row 0 may start before the record: it is loaded from max(row0, 0) and its bytes
      // shifted up by s0 (0 when aligned); a row entirely before the record is padding
      const int s0 = row0 >= 0 ? 0 : (int)(-row0);
      auto load_row0 = [&]() { xr = ldu128(vec ? rec + (row0 >= 0 ? row0 : 0) : dummy); };
      auto load_final = [&]() { xf = ldu128(base + 64 * hi_row); };  // unused if R < 2
      auto row0_data = [&]() { return (vec && s0 < 16) ? shl_bytes(xr, s0) : zero; };
      auto consume = [&](const u32x4_t& dv, int j) {
        const int real = j - pad;
        const u32x4_t x = (real == 0) ? row0_data() : zero;
        u32x4_t xin;
        xin.x = real > 0 ? dv.x : (real == 0 ? x.x : 0u);
        xin.y = real > 0 ? dv.y : (real == 0 ? x.y : 0u);
        xin.z = real > 0 ? dv.z : (real == 0 ? x.z : 0u);
        xin.w = real > 0 ? dv.w : (real == 0 ? x.w : 0u);
        const uint32_t xw[4] = {xin.x, xin.y, xin.z, xin.w};
        if (MODE == 1) {
#pragma unroll
          for (int b = 0; b < 4; b++) ha[b] = (ha[b] << 1) ^ xw[b];
        } else {
          // all 16 lookups of the row are independent: every address first, the 16 LDS
          // reads back to back, then the folds (one LDS round trip per row)
#pragma unroll
          for (int b = 0; b < 4; b++) a64_parts(ldsb, xor3(ha[b], hb[b], xw[b]), s1, ha[b], hb[b]);
        }
      };
      // One block of N middle rows (virtual rows j0..j0+N-1, all in 1..V-2): all loads
      // issued first (unconditional, clamped addresses), then -- first block only -- row 0,
      // the final row and the header, then consumption in order with counted waits.  The
      // empty asm with a memory clobber keeps LLVM from sinking a load into its consumer.
      auto block = [&](auto n_tag, int j0, int cnt, bool first) {
        constexpr int N = decltype(n_tag)::value;
        u32x4_t d[N];
        // issue order = consumption order: row 0, the block, then the final row + header
        if (first) load_row0();
#pragma unroll
        for (int k = 0; k < N; k++) d[k] = ldu128(row_addr(j0 + k));
        if (first) {
          load_final();
          if (speculate) load_header();
        }
        asm volatile("" ::: "memory");
        if (first && V >= 2) consume(zero, 0);  // virtual row 0: row 0 (from xr) or padding
#pragma unroll
        for (int k = 0; k < N; k++)
          if (k < cnt) consume(d[k], j0 + k);
      };
      using B14 = std::integral_constant<int, 14>;
      using B6 = std::integral_constant<int, 6>;
      using B2 = std::integral_constant<int, 2>;
      const int mid = V - 2;  // middle rows 1..V-2 (wave-uniform)
      if (mid <= 2) {
        block(B2{}, 1, mid, true);
      } else if (mid <= 6) {
        block(B6{}, 1, mid, true);
      } else {
        block(B14{}, 1, min(14, mid), true);
        for (int j0 = 15; j0 <= mid; j0 += 14) block(B14{}, j0, min(14, mid + 1 - j0), false);
      }
      u32x4_t x = multi ? xf : row0_data();
      if (speculate) decide();
      // last row: byte-swap the big-endian trailer into little-endian stream order
      if (q == 3) x.w = bswap32(x.w);
      // fold: word b of lane q sits 64-16q-4b bytes before the record end, so
      //   v_q = A16(g0) ^ A12(g1) ^ A8(g2) ^ A4(g3),  tot = XOR_q A_{48-16q}(v_q)
      // (16 independent lookups, then one per-lane lookup and a quad XOR-reduce)
      const uint32_t v = shift_tab(fold + 3 * 1024, xor3(ha[0], hb[0], x.x)) ^
                         shift_tab(fold + 2 * 1024, xor3(ha[1], hb[1], x.y)) ^
                         shift_tab(fold + 1 * 1024, xor3(ha[2], hb[2], x.z)) ^
                         shift_tab(fold, xor3(ha[3], hb[3], x.w));
      const uint32_t* lt = fold + (q == 0 ? 5 : (q == 1 ? 4 : 3)) * 1024;  // A48/A32/A16
      uint32_t s = (q == 3) ? v : shift_tab(lt, v);
      s ^= __shfl_xor(s, 1);
      s ^= __shfl_xor(s, 2);
      tot = s;
      spec = __any(needs_crc);
    } else if (kCrc) {
      spec = false;
    }
    if (!kCrc) load_header();
    const bool vec_crc = needs_crc && live && L >= 32;

    uint32_t pw[16];
    gather(pw);
    if (live && q == 0) {
      // each parse path stores its own record (no join merging two decoded headers)
      if (pfx64 && fast_layout(pw[0], pw[5], (pw[5] >> 24) == 4u ? pw[7] : pw[10])) {
        store_fast_q0(p.cols, rec_idx, pw, buf_len, !needs_crc || tot == expect, tcp);
        if (any_ext) store_fast_ext(p.cols, rec_idx, [&](int k) { return pw[k]; }, buf_len, true);
      } else {
        Hdr h;
        unpack_words(pw);
        parse_header(rec, buf_len, want_ext, w, h);
        const bool crc_ok =
            !needs_crc || (vec_crc ? (tot == expect) : small_crc_ok(rec, L));
        store_hdr_q0(p.cols, rec_idx, h, crc_ok, tcp);
      }
    } else if (oob && q == 0) {
      store_oob_q0(p.cols, rec_idx);
    }
  };

  auto place = [&](uint64_t ri, uint64_t& off, uint32_t& L) {
    off = 0;
    L = 0;
    if (ri < p.n) {
      off = p.rec_off ? p.rec_off[ri] : ri * p.stride;
      L = p.rec_len ? p.rec_len[ri] : p.fixed_len;
    }
  };
  for (uint64_t g = wave_id; g < n_groups; g += n_waves) {
    const uint64_t ri = (g << 4) + (uint64_t)(lane >> 2);
    uint64_t off;
    uint32_t L;
    place(ri, off, L);
    group(ri, ri < p.n, off, L);
  }
}

}  // namespace mgenx

// The var and the long kernel have a file each but are compiled here, after the general
// kernel: on their own their machine code comes out different (the order in which the shared
// forced-inline helpers enter the module decides the order they are inlined in, and with it
// block layout and register allocation), and these kernels were tuned as they are.
#include "mgenx_unpack_var.hpp"
#include "mgenx_unpack_long.hpp"

namespace mgenx {

template <int MODE>
static hipError_t launch_general(const UnpackParams& p, int grid, int, hipStream_t stream) {
  const auto kernel = unpack_kernel<true, MODE>;
  hipError_t e = set_max_lds((const void*)kernel, (int)kUnpackLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kUnpackThreads), kUnpackLdsBytes, stream, p);
  return hipGetLastError();
}

#if MGENX_DIAG
// The diagnostics build's variants (MGENX_TUNE_UNPACK_VARIANT != 0), all of them.  A variant
// runs when the batch is of its kind; otherwise -- and for a number that is not here -- the
// batch goes on to the long / var / general dispatch below (never to the fixed-length product
// path).  A number with one meaning per kind of batch would be one entry per kind.
// Shapes that were measured and lost are not kept: DESIGN 4.1 has their numbers.
enum BatchKind {
  kAnyBatch,     // every batch
  kFixed1024,    // meets `fixed` (below), 1024-byte records
  kFixedRowRing, // meets `fixed`, 512- or 1024-byte records, row output
  kRecLen,       // per-record lengths
};
struct UnpackVariant {
  int variant;
  BatchKind kind;
  int which;  // the MGENX_UNPACK_K_* it reports
  unpack_launcher launch;
  const char* what;
};
static const UnpackVariant kUnpackVariants[] = {
    // ablations of the general kernel, and the general kernel on any batch
    {1, kAnyBatch, MGENX_UNPACK_K_OTHER, launch_general<1>, "general: row loads + XOR only"},
    {2, kAnyBatch, MGENX_UNPACK_K_OTHER, launch_general<2>, "general: lookups on one cached row"},
    {3, kAnyBatch, MGENX_UNPACK_K_OTHER, launch_general<0>, "general kernel, whatever the batch"},
    // the fixed-length kernel on 1024-byte records as it was before the ring kernel
    {12, kFixed1024, MGENX_UNPACK_K_OTHER, launch_fixed_1024<0, false>, "separate header load"},
    {13, kFixed1024, MGENX_UNPACK_K_OTHER, launch_fixed_1024<0, true>, "aligned, stores interleaved"},
    // ring kernel (block rows, blocks, groups held, waves, non-temporal loads)
    {17, kFixedRowRing, MGENX_UNPACK_K_FIXED_RING, launch_ring_shape<4, 1, 16, 16, false>,
     "product shape, plain loads"},
    {18, kFixedRowRing, MGENX_UNPACK_K_FIXED_RING, launch_ring_shape<8, 2, 32, 8, false>,
     "two 8-row blocks at 8 waves (tests/test_gpu_unpack_ring_blocks.py)"},
    {28, kFixedRowRing, MGENX_UNPACK_K_FIXED_RING, launch_ring_shape<4, 1, 16, 16, true>,
     "product shape, non-temporal loads"},
    // var kernel
    {20, kRecLen, MGENX_UNPACK_K_VAR, launch_var<1>, "every core store to the sink"},
    {32, kRecLen, MGENX_UNPACK_K_VAR, launch_var<8>, "non-temporal row stores"},
    {33, kRecLen, MGENX_UNPACK_K_VAR, launch_var<16>, "64-byte-aligned row loads (timing only)"},
    // ablation mask M of the aligned 1024-byte kernel (unpack_fixed_kernel's MODE)
#define MGENX_ABL(M) \
  {1024 + M, kFixed1024, MGENX_UNPACK_K_OTHER, launch_fixed_1024<M, true>, "aligned 1024 B, MODE " #M},
    MGENX_FIXED_ABL_MODES(MGENX_ABL)
#undef MGENX_ABL
};
#endif  // MGENX_DIAG

hipError_t launch_unpack(const UnpackParams& p, int grid, int cus, hipStream_t stream,
                         int* which) {
  *which = MGENX_UNPACK_K_OTHER;
  if (p.opts & MGENX_OPT_SKIP_CRC) {
    *which = MGENX_UNPACK_K_HEADER;
    hipLaunchKernelGGL((unpack_kernel<false>), dim3(grid), dim3(kUnpackThreads), 0, stream, p);
    return hipGetLastError();
  }
  // fixed stride + one length in [65, 1024] + core columns: the pipelined kernel
  const mgenx_cols& c = p.cols;
  const uint32_t nr = (p.fixed_len + 63) / 64;
  const bool fixed = !p.rec_off && !p.rec_len && p.fixed_len >= 65 && p.fixed_len <= 1024 &&
                     p.stride > 0 && p.n <= 0xFFFFFFF0u && !any_ext_cols(c) &&
                     p.slab_bytes < 0xFFFF0000ull && p.slab_bytes >= 64ull * (nr + 1) + 16 &&
                     p.slab_bytes >= p.fixed_len;
  if (p.variant == 0 && fixed) {
    *which = (c.rows && (p.fixed_len == 512 || p.fixed_len == 1024)) ? MGENX_UNPACK_K_FIXED_RING
                                                                    : MGENX_UNPACK_K_FIXED;
    return launch_fixed_product(p, grid, cus, stream);
  }
#if MGENX_DIAG
  for (const UnpackVariant& v : kUnpackVariants) {
    if (v.variant != p.variant) continue;
    const bool len1024 = p.fixed_len == 1024, len512 = p.fixed_len == 512;
    const bool applies = v.kind == kAnyBatch || (v.kind == kFixed1024 && fixed && len1024) ||
                         (v.kind == kFixedRowRing && fixed && c.rows && (len512 || len1024)) ||
                         (v.kind == kRecLen && p.rec_len);
    if (!applies) continue;
    *which = v.which;
    return v.launch(p, grid, cus, stream);
  }
#endif  // MGENX_DIAG
  // long records (a TCP stream of 16-KiB records: the mean length from the slab) -- one wave
  // per record, 1-KiB contiguous loads
  const uint64_t mean = p.rec_len ? (p.n ? p.slab_bytes / p.n : 0) : p.fixed_len;
  if (mean >= kLongMin) {
    *which = MGENX_UNPACK_K_LONG;
    return launch_long(p, grid, cus, stream);
  }
  // per-record lengths: sorted groups with the rows in a load ring -- when every wave gets
  // at least two 64-record tiles; fewer, larger records (a 1 GiB stream of 16-KiB TCP
  // records is 1024 tiles for 4096 waves) keep the general kernel's one group per wave and
  // its 14-row load blocks, which keep more bytes in flight per record
  const uint64_t tiles = ((uint64_t)p.n + 63) / 64;
  const uint64_t waves = (uint64_t)grid * (kUnpackThreads / 64);
  if (p.rec_len && tiles >= 2 * waves) {
    *which = MGENX_UNPACK_K_VAR;
    return launch_var<0>(p, grid, cus, stream);
  }
  *which = MGENX_UNPACK_K_GENERAL;
  return launch_general<0>(p, grid, cus, stream);
}

int unpack_threads() { return kUnpackThreads; }

}  // namespace mgenx
