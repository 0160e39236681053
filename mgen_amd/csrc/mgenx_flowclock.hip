// mgenx_flowclock.hip -- per-flow clock offset and skew removal on gfx950 (mgenx_flow_clock,
// include/mgenx.h): per flow the edge of the lower convex hull of its (send time, latency)
// points that lies over the mean send time (Moon, Skelly, Towsley, INFOCOM 1999), and per
// record the latency above that line.  Integers only; the arithmetic is mgenx_flowclock.hpp's.
//
// Separate launches order the phases; no kernel waits on another workgroup.
//   1. Group by flow.  mgenx::flow_sort_run (the stable radix ordering of mgenx_flow_dist) gives
//      order[] and every flow's segment [bnd[f], bnd[f + 1]).  flow_clock_pack_kernel reads the
//      columns once, coalesced, and leaves every record's point as a 16-B {x, d} pair;
//      flow_clock_gather_kernel lays the points out in sorted order, one 16-B gather per record.
//      The sort is stable, so inside a segment a lower position is a lower record index: "the
//      lowest record holding a point" is the lowest position.
//   2. Fit per flow: a wave for a flow of up to kClockWaveMax points (flow_clock_wave_kernel,
//      which also writes the empty flows and lists the larger ones), a workgroup of
//      kClockGroupLanes for a listed flow (flow_clock_group_kernel).  Either runs clock_fit:
//        a. one pass reduces S = sum x (128 bits), L = the leftmost point (lowest d, lowest
//           position), R = the rightmost (lowest d, lowest position) and the lowest-d point;
//        b. the chord search: over the points strictly between L and R in x, the minimum of
//           (key, x, position), key = clock_key(L, R, point).  No negative key: (L, R) is the
//           hull edge over the mean.  Otherwise the minimiser M is a hull vertex (the lowest x
//           among equal keys: an interior point of a hull edge parallel to the chord is no
//           vertex), and it replaces L when n x_M <= S, else R.  x_R - x_L shrinks every round;
//           the loop is bounded by the flow's record count plus two all the same, and a flow
//           that hit the bound gets ia = ib = MGENX_CLOCK_NONE;
//        c. one pass for resid_sum / resid_max against the chosen line.
//      A lane walks the points with kClockUnroll loads in flight (clock_each).  Every reduction
//      leaves its result in all lanes, so the control flow of a round is uniform.
//      One lane writes the flow's struct: one writer per element, no atomics on the output.
//   3. flow_clock_apply_kernel, a lane per record in input order, reads its flow's line and
//      writes the optional per-record outputs (launched only when one is given).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include "mgenx_blockscan.hpp"
#include "mgenx_flowclock.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

struct ClockPt {
  uint64_t x;
  int64_t d;
};
static_assert(sizeof(ClockPt) == 16, "one 16-B load per point");

struct ClockCols {
  const uint32_t *flow, *txs, *txu, *rxs, *rxu;
};

// A candidate of a minimum search: compared by (k_hi, k_lo, x, d, p), all ascending.  The
// 128-bit word k orders what the search is about (a biased key, a complemented x, ...).
struct ClockCand {
  uint64_t k_hi, k_lo, x;
  int64_t d;
  uint32_t p, pad;
};
struct ClockSum {  // S as 128 bits
  uint64_t lo, hi;
};
struct ClockRes {
  uint64_t sum;
  int64_t max;
};

constexpr uint64_t kClockBias = 1ull << 63;

__device__ __forceinline__ ClockCand clock_none() {
  return ClockCand{~0ull, ~0ull, ~0ull, INT64_MAX, MGENX_CLOCK_NONE, 0u};
}
__device__ __forceinline__ bool clock_less(const ClockCand& a, const ClockCand& b) {
  if (a.k_hi != b.k_hi) return a.k_hi < b.k_hi;
  if (a.k_lo != b.k_lo) return a.k_lo < b.k_lo;
  if (a.x != b.x) return a.x < b.x;
  if (a.d != b.d) return a.d < b.d;
  return a.p < b.p;
}
// the operators of the reductions (mgenx_blockscan.hpp's shape)
struct ClockMinOp {
  static __device__ ClockCand of(const ClockCand& a, const ClockCand& b) {
    return clock_less(b, a) ? b : a;
  }
};
struct ClockSumOp {
  static __device__ ClockSum of(const ClockSum& a, const ClockSum& b) {
    const clock_u128 s = (((clock_u128)a.hi << 64) | a.lo) + (((clock_u128)b.hi << 64) | b.lo);
    return ClockSum{(uint64_t)s, (uint64_t)(s >> 64)};
  }
};
struct ClockResOp {
  static __device__ ClockRes of(const ClockRes& a, const ClockRes& b) {
    return ClockRes{a.sum + b.sum, a.max > b.max ? a.max : b.max};
  }
};

constexpr uint32_t kClockSlotBytes = 40;  // the largest value reduced (ClockCand)

// the reduction of v over the T lanes that serve a flow (a wave, or the whole workgroup), the
// result in every lane.  T > 64: `slots` holds T / 64 values in LDS; all lanes of the workgroup
// call this together.
template <uint32_t T, class Op, class V>
__device__ __forceinline__ V clock_reduce(V v, unsigned char* slots) {
  static_assert(sizeof(V) <= kClockSlotBytes, "a slot holds the value");
  v = wave_reduce<Op>(v);
  if constexpr (T > 64) {
    V* s = reinterpret_cast<V*>(slots);
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    V r = s[0];
#pragma unroll
    for (uint32_t k = 1; k < T / 64u; k++) r = Op::of(r, s[k]);
    __syncthreads();
    v = r;
  }
  return v;
}

__device__ __forceinline__ void clock_write_empty(struct mgenx_flow_clock* o) {
  o->n = 0;
  o->xa = 0;
  o->da = 0;
  o->xb = 0;
  o->db = 0;
  o->resid_sum = 0;
  o->resid_max = INT64_MIN;
  o->ia = MGENX_CLOCK_NONE;
  o->ib = MGENX_CLOCK_NONE;
}

// f(point, position) for the points pt[b0 + k], k = t, t + T, ... < c, kClockUnroll loads issued
// before the first is used.  c < 2^31 and T <= 2^10: no index wraps.
template <uint32_t T, class F>
__device__ __forceinline__ void clock_each(const ClockPt* __restrict__ pt, uint32_t b0, uint32_t c,
                                           uint32_t t, F f) {
  static_assert(kClockUnroll == 4, "four loads below");
  uint32_t k = t;
  for (; k + 3u * T < c; k += 4u * T) {
    const ClockPt q0 = pt[b0 + k], q1 = pt[b0 + k + T], q2 = pt[b0 + k + 2u * T],
                  q3 = pt[b0 + k + 3u * T];
    f(q0, b0 + k);
    f(q1, b0 + k + T);
    f(q2, b0 + k + 2u * T);
    f(q3, b0 + k + 3u * T);
  }
  for (; k < c; k += T) f(pt[b0 + k], b0 + k);
}

// The fit of one flow: its c >= 1 points pt[b0 .. b0 + c), lane t of T.  All T lanes call it.
template <uint32_t T>
__device__ void clock_fit(const ClockPt* __restrict__ pt, const uint32_t* __restrict__ order,
                          uint32_t b0, uint32_t c, uint32_t t, bool offset_only,
                          struct mgenx_flow_clock* out, unsigned char* slots) {
  // a. S, the leftmost, the rightmost and the lowest point
  ClockSum s = {0, 0};
  ClockCand l = clock_none(), r = clock_none(), low = clock_none();
  clock_each<T>(pt, b0, c, t, [&](const ClockPt& q, uint32_t p) {
    s = ClockSumOp::of(s, ClockSum{q.x, 0});
    const ClockCand cl = {0, 0, q.x, q.d, p, 0u};
    const ClockCand cr = {0, ~q.x, q.x, q.d, p, 0u};
    const ClockCand cd = {0, (uint64_t)q.d ^ kClockBias, q.x, q.d, p, 0u};
    l = ClockMinOp::of(l, cl);
    r = ClockMinOp::of(r, cr);
    low = ClockMinOp::of(low, cd);
  });
  s = clock_reduce<T, ClockSumOp>(s, slots);
  l = clock_reduce<T, ClockMinOp>(l, slots);
  r = clock_reduce<T, ClockMinOp>(r, slots);
  low = clock_reduce<T, ClockMinOp>(low, slots);

  // b. the edge over the mean
  bool found = true;
  if (offset_only) {
    l = low;
    r = low;
  } else if (l.x == r.x) {
    r = l;
  } else {
    found = false;
    for (uint32_t round = 0; round < c + 2u; round++) {
      ClockCand m = clock_none();
      clock_each<T>(pt, b0, c, t, [&](const ClockPt& q, uint32_t p) {
        if (q.x > l.x && q.x < r.x) {
          const clock_i128 key = clock_key(l.x, l.d, r.x, r.d, q.x, q.d);
          const ClockCand cm = {(uint64_t)((clock_u128)key >> 64) ^ kClockBias, (uint64_t)key,
                                q.x, q.d, p, 0u};
          m = ClockMinOp::of(m, cm);
        }
      });
      m = clock_reduce<T, ClockMinOp>(m, slots);
      if (m.k_hi >= kClockBias) {  // no point below the chord (none between its ends included)
        found = true;
        break;
      }
      if (clock_left(c, m.x, s.lo, s.hi)) l = m;
      else r = m;
    }
  }
  const uint64_t xa = found ? l.x : 0, xb = found ? r.x : 0;
  const int64_t da = found ? l.d : 0, db = found ? r.d : 0;

  // c. the residuals against the line
  ClockRes res = {0, INT64_MIN};
  clock_each<T>(pt, b0, c, t, [&](const ClockPt& q, uint32_t) {
    const int64_t ci = clock_resid(xa, da, xb, db, q.x, q.d);
    res = ClockResOp::of(res, ClockRes{(uint64_t)ci, ci});
  });
  res = clock_reduce<T, ClockResOp>(res, slots);
  if (t == 0) {
    out->n = c;
    out->xa = xa;
    out->da = da;
    out->xb = xb;
    out->db = db;
    out->resid_sum = (int64_t)res.sum;
    out->resid_max = res.max;
    out->ia = found ? order[l.p] : MGENX_CLOCK_NONE;  // (l.p, r.p lie in [b0, b0 + c))
    out->ib = found ? order[r.p] : MGENX_CLOCK_NONE;
  }
}

__global__ void flow_clock_fill_kernel(struct mgenx_flow_clock* flows, uint32_t n_flows) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n_flows) clock_write_empty(flows + f);
}

// every record's point, input order (a skipped record's too: nothing reads it)
__global__ void flow_clock_pack_kernel(ClockCols col, uint32_t n, ClockPt* __restrict__ raw) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ts = col.txs[i], tu = col.txu[i];
  raw[i] = ClockPt{clock_x(ts, tu), clock_d(ts, tu, col.rxs[i], col.rxu[i])};
}

// the points in sorted order: position p < bnd[n_flows] holds record order[p]
__global__ void flow_clock_gather_kernel(const ClockPt* __restrict__ raw, uint32_t n,
                                         uint32_t n_flows, const uint32_t* __restrict__ order,
                                         const uint32_t* __restrict__ bnd,
                                         ClockPt* __restrict__ pt) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || p >= bnd[n_flows]) return;
  const uint32_t i = order[p];
  if (i < n) pt[p] = raw[i];
}

// a wave per flow over all flows: the empty ones written, the small ones fitted, the others
// listed (the order of the list does not reach the output)
__global__ void __launch_bounds__(256)
flow_clock_wave_kernel(const ClockPt* __restrict__ pt, const uint32_t* __restrict__ order,
                       const uint32_t* __restrict__ bnd, uint32_t n_flows, uint32_t offset_only,
                       struct mgenx_flow_clock* __restrict__ flows, uint32_t* count,
                       uint32_t* __restrict__ list, uint32_t cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * 4u;
  for (uint64_t f64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); f64 < n_flows;
       f64 += waves) {
    const uint32_t f = (uint32_t)f64;
    const uint32_t b0 = bnd[f], c = bnd[f + 1u] - b0;
    if (c == 0u) {
      if (lane == 0u) clock_write_empty(flows + f);
    } else if (clock_wave_tier(c)) {
      clock_fit<kClockWaveLanes>(pt, order, b0, c, lane, offset_only != 0u, flows + f, nullptr);
    } else if (lane == 0u) {
      const uint32_t pos = atomicAdd(count, 1u);
      if (pos < cap) list[pos] = f;
    }
  }
}

__global__ void __launch_bounds__(kClockGroupLanes)
flow_clock_group_kernel(const ClockPt* __restrict__ pt, const uint32_t* __restrict__ order,
                        const uint32_t* __restrict__ bnd, uint32_t offset_only,
                        struct mgenx_flow_clock* __restrict__ flows,
                        const uint32_t* __restrict__ count, const uint32_t* __restrict__ list,
                        uint32_t cap) {
  __shared__ __attribute__((aligned(16))) unsigned char slots[kClockGroupLanes / 64u *
                                                              kClockSlotBytes];
  const uint32_t cnt = min(*count, cap);
  for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
    const uint32_t f = list[k];
    const uint32_t b0 = bnd[f], c = bnd[f + 1u] - b0;
    clock_fit<kClockGroupLanes>(pt, order, b0, c, threadIdx.x, offset_only != 0u, flows + f,
                                slots);
  }
}

// a lane per record, input order: the optional per-record outputs
__global__ void flow_clock_apply_kernel(ClockCols col, uint32_t n, uint32_t n_flows,
                                        const struct mgenx_flow_clock* __restrict__ flows,
                                        int64_t* __restrict__ resid, uint32_t* __restrict__ sec_out,
                                        uint32_t* __restrict__ usec_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = col.flow[i];
  const uint32_t rs = col.rxs[i], ru = col.rxu[i];
  int64_t c = INT64_MIN;
  uint32_t so = rs, uo = ru;
  if (f < n_flows) {
    const uint32_t ts = col.txs[i], tu = col.txu[i];
    const struct mgenx_flow_clock* fl = flows + f;
    const uint64_t x = clock_x(ts, tu);
    c = clock_resid(fl->xa, fl->da, fl->xb, fl->db, x, clock_d(ts, tu, rs, ru));
    clock_stamp(x, c, &so, &uo);
  }
  if (resid) resid[i] = c;
  if (sec_out) {
    sec_out[i] = so;
    usec_out[i] = uo;
  }
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (workspace owned by the context: struct mgenx_ctx, mgenx_internal.hpp)
// ------------------------------------------------------------------------------------
using namespace mgenx;

// n_flows >= 1; n, n_flows < 2^31
int mgenx::flow_clock_run(DevBuf& ws, int cu_count, const uint32_t* flow_idx, const uint32_t* txs,
                          const uint32_t* txu, const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                          uint32_t n_flows, uint32_t opts, struct mgenx_flow_clock* flows,
                          int64_t* resid, uint32_t* sec_out, uint32_t* usec_out,
                          hipStream_t stream, char* err, size_t errn) {
  if (n == 0) {
    hipLaunchKernelGGL(flow_clock_fill_kernel, dim3((n_flows + 255u) / 256u), dim3(256), 0, stream,
                       flows, n_flows);
    return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
  }
  const uint32_t cap = clock_list_cap(n, n_flows);
  const size_t sort_b = a256(mgenx::flow_sort_ws(n, n_flows)), pt_b = a256((size_t)n * 16u),
               count_b = a256(4u), list_b = a256((size_t)cap * 4u);
  const size_t total = sort_b + 2u * pt_b + count_b + list_b;
  if (ws.reserve(total) != hipSuccess) {
    snprintf(err, errn, "flow_clock: workspace of %zu bytes", total);
    return MGENX_EDEVICE;
  }
  Carve take(ws.p);
  void* sort_mem = take(sort_b);
  ClockPt* raw = (ClockPt*)take(pt_b);
  ClockPt* pt = (ClockPt*)take(pt_b);
  uint32_t* count = (uint32_t*)take(count_b);
  uint32_t* list = (uint32_t*)take(list_b);
  const uint32_t cu = cu_count > 0 ? (uint32_t)cu_count : 256u;
  const uint32_t offset_only = (opts & MGENX_CLOCK_OFFSET_ONLY) ? 1u : 0u;

  if (hipMemsetAsync(count, 0, 4u, stream) != hipSuccess) return MGENX_EDEVICE;
  const ClockCols col = {flow_idx, txs, txu, rxs, rxu};
  hipLaunchKernelGGL(flow_clock_pack_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, col, n,
                     raw);
  const uint32_t *keys, *order, *bnd;
  const int rc = mgenx::flow_sort_run(sort_mem, flow_idx, n, n_flows, &keys, &order, &bnd, stream,
                                     err, errn);
  if (rc != MGENX_OK) return rc;
  hipLaunchKernelGGL(flow_clock_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, raw,
                     n, n_flows, order, bnd, pt);
  // a wave per flow, the grid walking the flows with a stride once they outnumber it
  const uint32_t want = (n_flows + 3u) / 4u, most = cu * 64u;
  hipLaunchKernelGGL(flow_clock_wave_kernel, dim3(want < most ? want : most), dim3(256), 0, stream,
                     pt, order, bnd, n_flows, offset_only, flows, count, list, cap);
  if (cap) {
    const uint32_t g = cap < cu * 2u ? cap : cu * 2u;
    hipLaunchKernelGGL(flow_clock_group_kernel, dim3(g), dim3(kClockGroupLanes), 0, stream, pt,
                       order, bnd, offset_only, flows, count, list, cap);
  }
  if (resid || sec_out)
    hipLaunchKernelGGL(flow_clock_apply_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, col,
                       n, n_flows, flows, resid, sec_out, usec_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "flow_clock: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}

int mgenx_flow_clock(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_tx_sec,
                     const uint32_t* dev_tx_usec, const uint32_t* dev_rx_sec,
                     const uint32_t* dev_rx_usec, uint32_t n, uint32_t n_flows, uint32_t opts,
                     struct mgenx_flow_clock* dev_flows, int64_t* dev_resid,
                     uint32_t* dev_rx_sec_out, uint32_t* dev_rx_usec_out, void* stream) {
  if (!ctx || !dev_flows || (opts & ~(uint32_t)MGENX_CLOCK_OFFSET_ONLY) || n > 0x7FFFFFFFu ||
      n_flows > 0x7FFFFFFFu || (!dev_rx_sec_out != !dev_rx_usec_out))
    return MGENX_EINVAL;
  if (n && (!dev_flow_idx || !dev_tx_sec || !dev_tx_usec || !dev_rx_sec || !dev_rx_usec))
    return MGENX_EINVAL;
  if (n_flows == 0) return MGENX_OK;
  hipSetDevice(ctx->device);
  return mgenx::flow_clock_run(ctx->flowclock_ws, ctx->cu_count, dev_flow_idx, dev_tx_sec,
                              dev_tx_usec, dev_rx_sec, dev_rx_usec, n, n_flows, opts, dev_flows,
                              dev_resid, dev_rx_sec_out, dev_rx_usec_out, (hipStream_t)stream,
                              ctx->err, sizeof(ctx->err));
}
