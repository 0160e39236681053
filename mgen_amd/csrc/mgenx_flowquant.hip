// mgenx_flowquant.hip -- exact latency percentiles per flow and window on gfx950
// (mgenx_flow_series_quantiles, include/mgenx.h): for every cell (flow, window of receive time)
// the r-th smallest latency of its records, for up to MGENX_FLOW_SERIES_MAX_Q ranks at once.
//
// Two phases, ordered by separate launches; no kernel waits on another workgroup.
//   1. Group by cell.  flow_quant_cell_kernel reads the five columns once, coalesced, and leaves
//      per record its cell id f * n_bins + b (MGENX_FLOW_NONE for a record that counts nowhere)
//      and its latency as a biased key (sign bit flipped: unsigned order = signed order).  The
//      records are ordered by cell with mgenx::flow_sort_run, the radix ordering mgenx_flow_dist
//      uses, keyed on the cell id and restricted to the bits the cell count needs; its bnd[]
//      gives every cell's segment [bnd[c], bnd[c + 1]).  flow_quant_gather_kernel then lays the
//      keys out in sorted order: seg[].  The order inside a segment plays no part below.
//   2. Select per cell, the tier chosen from the segment's length (the edges: kTinyMax,
//      kWaveMax, kGroupMax, kWideMax in mgenx_flowquant.hpp):
//        empty, tiny   flow_quant_tiny_kernel, a lane per cell: INT64_MIN for an empty cell; up
//                      to kTinyMax keys in registers through a 19-comparator network.  The lane
//                      of a longer cell appends the cell to its tier's list (one atomic per wave
//                      and tier; the order of a list does not reach the output).
//        wave          flow_quant_lds_kernel<kWaveMax, 64>: a wave per cell, bitonic sort in LDS
//        group         flow_quant_lds_kernel<kGroupMax, 256>: a workgroup per cell, 16 KiB
//        wide group    flow_quant_lds_kernel<kWideMax, 1024>: 128 KiB, one workgroup per CU
//        large         radix select over the segment in global memory, 8 passes of one byte from
//                      the top: flow_quant_hist_kernel counts, over many workgroups per cell, the
//                      byte's values among the keys that still match a wanted rank's prefix (one
//                      histogram per distinct prefix, LDS first, then one atomic per non-zero
//                      bin); flow_quant_pick_kernel (a workgroup per cell) scans the 256 counts,
//                      extends each rank's prefix by the byte that holds it and clears the
//                      histogram.  After the eighth pass the prefix is the key.
//      Every list is walked by a grid of fixed size with a stride: the trip counts are the list
//      lengths and segment lengths, all read at kernel entry.
// Every element of the output has one writer: the lane, wave or workgroup that owns its cell.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include "mgenx_flowquant.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

constexpr uint32_t kMaxQ = MGENX_FLOW_SERIES_MAX_Q;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;
constexpr uint64_t kBias = 1ull << 63;
constexpr uint32_t kHistLanes = 1024;  // flow_quant_hist_kernel's workgroup
constexpr uint32_t kHistSplit = 64;    // workgroups sharing one large cell
constexpr uint32_t kDigits = 8;        // bytes of a key

struct QuantQ {
  uint32_t q[kMaxQ];
};

struct QuantCols {
  const uint32_t *flow, *txs, *txu, *rxs, *rxu;
};

// the cells of the tiers above tiny: list[t][0 .. count[t]), capacity cap[t]
struct QuantLists {
  uint32_t* count;  // [kLists]
  uint32_t* list[kLists];
  uint32_t cap[kLists];
};

__global__ void flow_quant_fill_kernel(int64_t* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = INT64_MIN;
}

// phase 1: cell id and biased latency per record
__global__ void flow_quant_cell_kernel(QuantCols col, uint32_t n, uint32_t n_flows, int64_t t0,
                                       uint64_t width, uint32_t n_bins,
                                       uint32_t* __restrict__ cell, uint64_t* __restrict__ key) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = col.flow[i];
  const int64_t rs = col.rxs[i], ru = col.rxu[i], ts = col.txs[i], tu = col.txu[i];
  const int64_t rx = rs * 1000000 + ru;
  const int64_t lat = (rs - ts) * 1000000 + ru - tu;
  uint32_t c = kNoCell;
  // 0 <= rx < 2^53, so rx - t0 fits 64 unsigned bits whenever it is not negative
  if (f < n_flows && rx >= t0) {
    const uint64_t b = ((uint64_t)rx - (uint64_t)t0) / width;
    if (b < (uint64_t)n_bins) c = f * n_bins + (uint32_t)b;  // < 2^31
  }
  cell[i] = c;
  key[i] = (uint64_t)lat ^ kBias;
}

// the keys in sorted order: position p < bnd[n_cells] holds record order[p]
__global__ void flow_quant_gather_kernel(const uint32_t* __restrict__ order,
                                         const uint32_t* __restrict__ bnd, uint32_t n_cells,
                                         uint32_t n, const uint64_t* __restrict__ key,
                                         uint64_t* __restrict__ seg) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || p >= bnd[n_cells]) return;
  const uint32_t r = order[p];
  if (r < n) seg[p] = key[r];
}

__device__ __forceinline__ void quant_cx(uint64_t& a, uint64_t& b) {
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// one atomic per wave: the lanes with `want` append their cells
__device__ __forceinline__ void quant_append(bool want, uint32_t cell, uint32_t* count,
                                             uint32_t* list, uint32_t cap) {
  const unsigned long long m = __ballot(want);
  if (!m) return;  // (the whole wave)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t leader = (uint32_t)__builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, leader);
  if (want) {
    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap) list[pos] = cell;
  }
}

// phase 2, a lane per cell: the empty and the tiny cells answered, the others listed
__global__ void __launch_bounds__(256)
flow_quant_tiny_kernel(const uint32_t* __restrict__ bnd, const uint64_t* __restrict__ seg,
                       uint32_t n_cells, QuantQ qs, uint32_t n_q, int64_t* __restrict__ out,
                       QuantLists ls) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = cell < n_cells;
  uint32_t b0 = 0, c = 0;
  if (in) {
    b0 = bnd[cell];
    c = bnd[cell + 1u] - b0;
  }
  const int tier = in ? quant_tier(c) : kTierTiny;
  if (in && tier == kTierTiny) {
    int64_t* o = out + (size_t)cell * n_q;
    if (c == 0u) {
      for (uint32_t j = 0; j < n_q; j++) o[j] = INT64_MIN;
    } else {
      static_assert(kTinyMax == 8, "the network below sorts eight keys");
      uint64_t x[kTinyMax];
#pragma unroll
      for (uint32_t k = 0; k < kTinyMax; k++) x[k] = k < c ? seg[b0 + k] : ~0ull;
      if (c > 1u) {
        quant_cx(x[0], x[2]); quant_cx(x[1], x[3]); quant_cx(x[4], x[6]); quant_cx(x[5], x[7]);
        quant_cx(x[0], x[4]); quant_cx(x[1], x[5]); quant_cx(x[2], x[6]); quant_cx(x[3], x[7]);
        quant_cx(x[0], x[1]); quant_cx(x[2], x[3]); quant_cx(x[4], x[5]); quant_cx(x[6], x[7]);
        quant_cx(x[2], x[4]); quant_cx(x[3], x[5]);
        quant_cx(x[1], x[4]); quant_cx(x[3], x[6]);
        quant_cx(x[1], x[2]); quant_cx(x[3], x[4]); quant_cx(x[5], x[6]);
      }
      for (uint32_t j = 0; j < n_q; j++) {
        const uint32_t r = quant_rank(qs.q[j], c) - 1u;
        uint64_t v = x[0];
#pragma unroll
        for (uint32_t k = 1; k < kTinyMax; k++) v = r == k ? x[k] : v;
        o[j] = (int64_t)(v ^ kBias);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kLists; t++)
    quant_append(tier == t, cell, ls.count + t, ls.list[t], ls.cap[t]);
}

// phase 2, a workgroup of T lanes per listed cell of at most CAP keys: bitonic sort in LDS over
// the next power of two, padded with the largest key (a rank never exceeds the cell's size, so
// the padding is never the answer unless it equals it)
template <uint32_t CAP, uint32_t T>
__global__ void __launch_bounds__(T)
flow_quant_lds_kernel(const uint32_t* __restrict__ bnd, const uint64_t* __restrict__ seg,
                      const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                      uint32_t cap, QuantQ qs, uint32_t n_q, int64_t* __restrict__ out) {
  static_assert((CAP & (CAP - 1u)) == 0u && CAP >= 2u * T, "a power of two, a pair per lane");
  __shared__ uint64_t s[CAP];
  const uint32_t t = threadIdx.x;
  const uint32_t cnt = min(*count, cap);
  for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
    const uint32_t cell = list[i];
    const uint32_t b0 = bnd[cell];
    const uint32_t c = min(bnd[cell + 1u] - b0, CAP);  // (the list holds cells of 2..CAP keys)
    const uint32_t p = quant_pow2(c);  // 2 <= p <= CAP
    for (uint32_t k = t; k < p; k += T) s[k] = k < c ? seg[b0 + k] : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= p; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (uint32_t k = t; k < (p >> 1); k += T) {
          const uint32_t lo = 2u * k - (k & (stride - 1u)), hi = lo + stride;
          const bool asc = (lo & size) == 0u;
          const uint64_t a = s[lo], b = s[hi];
          if ((a > b) == asc) {
            s[lo] = b;
            s[hi] = a;
          }
        }
        __syncthreads();
      }
    }
    for (uint32_t j = t; j < n_q; j += T)
      out[(size_t)cell * n_q + j] = (int64_t)(s[quant_rank(qs.q[j], c) - 1u] ^ kBias);
    __syncthreads();
  }
}

// the first rank that shares rank j's prefix: ranks with one prefix share its histogram
__device__ __forceinline__ uint32_t quant_lead(const uint64_t* pre, uint32_t j) {
  uint32_t lead = j;
  for (uint32_t k = 0; k < j; k++)
    if (pre[k] == pre[j]) {
      lead = k;
      break;
    }
  return lead;
}

// phase 2, large cells, the counting half of pass `pass` (0 = the top byte): hist[(l * n_q + j)
// * 256 + d] += the keys of cell list[l] whose bytes above the pass's byte equal pre[l * n_q + j]
// and whose byte is d, for every j that leads its prefix.  gridDim.x workgroups share a cell.
__global__ void __launch_bounds__(kHistLanes)
flow_quant_hist_kernel(uint32_t pass, const uint32_t* __restrict__ bnd,
                       const uint64_t* __restrict__ seg, const uint32_t* __restrict__ list,
                       const uint32_t* __restrict__ count, uint32_t cap, uint32_t n_q,
                       const uint64_t* __restrict__ pre, uint32_t* hist) {
  __shared__ uint32_t s_h[kMaxQ * 256u];
  __shared__ uint64_t s_pre[kMaxQ];
  __shared__ uint32_t s_lead[kMaxQ];
  const uint32_t t = threadIdx.x;
  const uint32_t cnt = min(*count, cap);
  const uint32_t shift = 56u - 8u * pass;
  for (uint32_t l = blockIdx.y; l < cnt; l += gridDim.y) {
    const uint32_t cell = list[l];
    const uint32_t b0 = bnd[cell], c = bnd[cell + 1u] - b0;
    for (uint32_t k = t; k < n_q * 256u; k += kHistLanes) s_h[k] = 0u;
    if (t < n_q) s_pre[t] = pass ? pre[(size_t)l * n_q + t] : 0ull;
    __syncthreads();
    if (t < n_q) s_lead[t] = quant_lead(s_pre, t);
    __syncthreads();
    // (c < 2^31 and the stride is 2^16: k does not wrap)
    for (uint32_t k = blockIdx.x * kHistLanes + t; k < c; k += gridDim.x * kHistLanes) {
      const uint64_t v = seg[b0 + k];
      const uint32_t d = (uint32_t)(v >> shift) & 255u;
      const uint64_t hi = pass ? v >> (shift + 8u) : 0ull;
      for (uint32_t j = 0; j < n_q; j++)
        if (s_lead[j] == j && s_pre[j] == hi) atomicAdd(&s_h[j * 256u + d], 1u);
    }
    __syncthreads();
    for (uint32_t k = t; k < n_q * 256u; k += kHistLanes) {
      const uint32_t v = s_h[k];
      if (v) atomicAdd(&hist[(size_t)l * n_q * 256u + k], v);
    }
    __syncthreads();
  }
}

// the choosing half: a workgroup of 256 lanes per large cell, lane d holding byte value d.  Rank
// j's prefix grows by the byte whose run of the (inclusive) scan holds the rank left, rem; the
// rank left becomes its position in that byte's keys.  The last pass writes the answers.
__global__ void __launch_bounds__(256)
flow_quant_pick_kernel(uint32_t pass, const uint32_t* __restrict__ bnd,
                       const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                       uint32_t cap, QuantQ qs, uint32_t n_q, uint64_t* pre, uint32_t* rem,
                       uint32_t* hist, int64_t* __restrict__ out) {
  __shared__ uint64_t s_pre[kMaxQ], s_new[kMaxQ];
  __shared__ uint32_t s_lead[kMaxQ], s_rem[kMaxQ], s_left[kMaxQ], s_w[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t cnt = min(*count, cap);
  for (uint32_t l = blockIdx.x; l < cnt; l += gridDim.x) {
    const uint32_t cell = list[l];
    const uint32_t c = bnd[cell + 1u] - bnd[cell];
    const size_t at = (size_t)l * n_q;
    if (t < n_q) {
      s_pre[t] = pass ? pre[at + t] : 0ull;
      s_rem[t] = pass ? rem[at + t] : quant_rank(qs.q[t], c);
      s_new[t] = 0ull;
      s_left[t] = 1u;
    }
    __syncthreads();
    if (t < n_q) s_lead[t] = quant_lead(s_pre, t);
    __syncthreads();
    for (uint32_t j = 0; j < n_q; j++) {
      const uint32_t h = hist[(at + s_lead[j]) * 256u + t];
      uint32_t x = h;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(x, d);
        if (lane >= d) x += o;
      }
      if (lane == 63u) s_w[w] = x;
      __syncthreads();
      for (uint32_t k = 0; k < w; k++) x += s_w[k];
      const uint32_t r = s_rem[j], before = x - h;
      if (before < r && r <= x) {  // (one lane: the counts sum to at least r)
        s_new[j] = (s_pre[j] << 8) | t;
        s_left[j] = r - before;
      }
      __syncthreads();
    }
    for (uint32_t j = 0; j < n_q; j++) hist[(at + j) * 256u + t] = 0u;
    if (t < n_q) {
      if (pass == kDigits - 1u) {
        out[(size_t)cell * n_q + t] = (int64_t)(s_new[t] ^ kBias);
      } else {
        pre[at + t] = s_new[t];
        rem[at + t] = s_left[t];
      }
    }
    __syncthreads();
  }
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (workspace owned by the context: struct mgenx_ctx, mgenx_internal.hpp)
// ------------------------------------------------------------------------------------
using namespace mgenx;

namespace {

struct QuantPlan {
  uint32_t cap[kLists];
  size_t cell_b, key_b, sort_b, seg_b, count_b, list_b[kLists], pre_b, rem_b, hist_b, total;
};

QuantPlan quant_plan(uint32_t n, uint32_t n_cells) {
  const uint32_t edge[kLists] = {kTinyMax, kWaveMax, kGroupMax, kWideMax};
  QuantPlan p;
  p.cell_b = a256((size_t)n * 4u);
  p.key_b = a256((size_t)n * 8u);
  p.sort_b = a256(mgenx::flow_sort_ws(n, n_cells));
  p.seg_b = a256((size_t)n * 8u);
  p.count_b = a256(kLists * 4u);
  p.total = p.cell_b + p.key_b + p.sort_b + p.seg_b + p.count_b;
  for (int t = 0; t < kLists; t++) {
    p.cap[t] = quant_tier_cap(n, n_cells, edge[t]);
    p.list_b[t] = a256((size_t)p.cap[t] * 4u);
    p.total += p.list_b[t];
  }
  const size_t slots = (size_t)p.cap[kListLarge] * kMaxQ;
  p.pre_b = a256(slots * 8u);
  p.rem_b = a256(slots * 4u);
  p.hist_b = a256(slots * 256u * 4u);
  p.total += p.pre_b + p.rem_b + p.hist_b;
  return p;
}

}  // namespace

// n_flows >= 1, n_flows * n_bins < 2^31, 1 <= n_q <= MGENX_FLOW_SERIES_MAX_Q, n < 2^31
int mgenx::flow_quant_run(DevBuf& ws, int cu_count, const uint32_t* flow_idx, const uint32_t* txs,
                          const uint32_t* txu, const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                          int64_t t0, uint64_t width, uint32_t n_bins, uint32_t n_flows,
                          const uint32_t* permille, uint32_t n_q, int64_t* out, hipStream_t stream,
                          char* err, size_t errn) {
  const uint32_t n_cells = n_flows * n_bins;
  if (n == 0) {
    const uint64_t m = (uint64_t)n_cells * n_q;
    hipLaunchKernelGGL(flow_quant_fill_kernel, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0,
                       stream, out, m);
    return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
  }
  const QuantPlan pl = quant_plan(n, n_cells);
  if (ws.reserve(pl.total) != hipSuccess) {
    snprintf(err, errn, "flow_series_quantiles: workspace of %zu bytes", pl.total);
    return MGENX_EDEVICE;
  }
  Carve take(ws.p);
  uint32_t* cell = (uint32_t*)take(pl.cell_b);
  uint64_t* key = (uint64_t*)take(pl.key_b);
  void* sort_mem = take(pl.sort_b);
  uint64_t* seg = (uint64_t*)take(pl.seg_b);
  QuantLists ls;
  ls.count = (uint32_t*)take(pl.count_b);
  for (int t = 0; t < kLists; t++) {
    ls.list[t] = (uint32_t*)take(pl.list_b[t]);
    ls.cap[t] = pl.cap[t];
  }
  uint64_t* pre = (uint64_t*)take(pl.pre_b);
  uint32_t* rem = (uint32_t*)take(pl.rem_b);
  uint32_t* hist = (uint32_t*)take(pl.hist_b);
  QuantQ qs = {};
  for (uint32_t j = 0; j < n_q; j++) qs.q[j] = permille[j];
  const uint32_t cu = cu_count > 0 ? (uint32_t)cu_count : 256u;

  if (hipMemsetAsync(ls.count, 0, kLists * 4u, stream) != hipSuccess) return MGENX_EDEVICE;
  const QuantCols col = {flow_idx, txs, txu, rxs, rxu};
  hipLaunchKernelGGL(flow_quant_cell_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, col, n,
                     n_flows, t0, width, n_bins, cell, key);
  const uint32_t *keys, *order, *bnd;
  const int rc = mgenx::flow_sort_run(sort_mem, cell, n, n_cells, &keys, &order, &bnd, stream, err,
                                     errn);
  if (rc != MGENX_OK) return rc;
  hipLaunchKernelGGL(flow_quant_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, order,
                     bnd, n_cells, n, key, seg);
  hipLaunchKernelGGL(flow_quant_tiny_kernel, dim3((n_cells + 255u) / 256u), dim3(256), 0, stream,
                     bnd, seg, n_cells, qs, n_q, out, ls);
  // a tier runs when n records can form one of its cells; its grid walks the list with a stride
  if (pl.cap[kListWave]) {
    const uint32_t g = pl.cap[kListWave] < cu * 32u ? pl.cap[kListWave] : cu * 32u;
    hipLaunchKernelGGL((flow_quant_lds_kernel<kWaveMax, 64>), dim3(g), dim3(64), 0, stream, bnd,
                       seg, ls.list[kListWave], ls.count + kListWave, ls.cap[kListWave], qs, n_q,
                       out);
  }
  if (pl.cap[kListGroup]) {
    const uint32_t g = pl.cap[kListGroup] < cu * 8u ? pl.cap[kListGroup] : cu * 8u;
    hipLaunchKernelGGL((flow_quant_lds_kernel<kGroupMax, 256>), dim3(g), dim3(256), 0, stream, bnd,
                       seg, ls.list[kListGroup], ls.count + kListGroup, ls.cap[kListGroup], qs,
                       n_q, out);
  }
  if (pl.cap[kListWide]) {
    const uint32_t g = pl.cap[kListWide] < cu ? pl.cap[kListWide] : cu;
    hipLaunchKernelGGL((flow_quant_lds_kernel<kWideMax, 1024>), dim3(g), dim3(1024), 0, stream,
                       bnd, seg, ls.list[kListWide], ls.count + kListWide, ls.cap[kListWide], qs,
                       n_q, out);
  }
  if (pl.cap[kListLarge]) {
    const uint32_t cap = pl.cap[kListLarge];
    if (hipMemsetAsync(hist, 0, (size_t)cap * n_q * 256u * 4u, stream) != hipSuccess)
      return MGENX_EDEVICE;
    const uint32_t gy = cap < 32u ? cap : 32u, gp = cap < cu * 4u ? cap : cu * 4u;
    for (uint32_t pass = 0; pass < kDigits; pass++) {
      hipLaunchKernelGGL(flow_quant_hist_kernel, dim3(kHistSplit, gy), dim3(kHistLanes), 0, stream,
                         pass, bnd, seg, ls.list[kListLarge], ls.count + kListLarge, cap, n_q, pre,
                         hist);
      hipLaunchKernelGGL(flow_quant_pick_kernel, dim3(gp), dim3(256), 0, stream, pass, bnd,
                         ls.list[kListLarge], ls.count + kListLarge, cap, qs, n_q, pre, rem, hist,
                         out);
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "flow_series_quantiles: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}
