// mgenx_flowdist.hip -- per-flow delivery statistics on gfx950 (mgenx_flow_dist, include/mgenx.h):
// latency histogram, jitter, receive gaps and reordering, in integer microseconds.
//
// Every term but one is local once the records are ordered by flow with the receive order kept:
// the jitter and gap of a record need its predecessor in the flow, the histogram bin needs the
// record alone.  Only "reordered" needs the running maximum M of the flow's earlier sequence
// numbers.  So:
//   0. flow_dist_snap_kernel copies what the batch's first record of a flow pairs with
//      (last_lat, last_rx, seq_max) out of the states, which the main pass updates in place;
//   1. the records are ordered by flow, stably (mgenx::flow_sort_run: flow_reduce's radix path),
//      and flow_dist_pack_kernel writes each record's latency, receive time, seq and length as
//      one 32-B record, so that the passes below gather one line per record, not six;
//   2. the sorted positions are cut into chunks of kChunk, whatever the flow edges are: one
//      dominant flow spreads over as many workgroups as its records fill.
//      flow_dist_tail_kernel writes per chunk the largest seq of its last flow's records and
//      whether that run continues the previous chunk's; flow_dist_carry_kernel (one workgroup)
//      scans those (segmented max), giving every chunk the M its first run starts from.
//      No kernel waits on another workgroup;
//   3. flow_dist_main_kernel: a lane per sorted position, a segmented inclusive max scan of seq
//      over the chunk, then per run of one flow either (runs of kLong lanes or more) an LDS
//      histogram and a workgroup reduction flushed with one atomic per field and non-zero bin,
//      or (shorter runs) atomics straight from the lanes.  Sums, minima and maxima of integers
//      commute, so the bytes left do not depend on the order the workgroups finish in.
// Passes 1 and 2 are mgenx::flow_prep_run, which mgenx_flow_series (mgenx_flowseries.hip) runs too;
// what both main passes use of them is DistRec (mgenx_flowdist.hpp) and kChunk with the
// segmented scan (mgenx_blockscan.hpp).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include "mgenx_blockscan.hpp"
#include "mgenx_flowdist.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

// (the header gives the struct and the function one name: the type needs its keyword)
typedef struct mgenx_flow_dist DistState;
static_assert(sizeof(DistState) == 160, "mgenx_flow_dist is 160 B");

constexpr uint32_t kLong = 128;     // a run of this many lanes takes the LDS path
constexpr uint32_t kMaxLong = kChunk / kLong;

// what a flow's first record of the batch pairs with
struct DistSnap {
  int64_t last_lat, last_rx;
  int64_t seq_max;  // kNone while the flow has no record
  int64_t rsv;
};

// ---- the reduced fields: index, operation, identity ----
enum { kAdd = 0, kMin = 1, kMax = 2 };
constexpr int kFields = 13;
// 0 counts (n | lat_neg << 16 | lat_over << 32 | reordered << 48: at most kChunk each)
// 1 bytes  2 lat_sum  3 lat_min  4 lat_max  5 jitter_sum  6 jitter_max  7 gap_min  8 gap_max
// 9 reorder_sum  10 reorder_max  11 seq_min  12 seq_max
__host__ __device__ constexpr int field_op(int k) {
  return (k == 3 || k == 7 || k == 11) ? kMin
         : (k == 4 || k == 6 || k == 8 || k == 10 || k == 12) ? kMax : kAdd;
}
__host__ __device__ constexpr int64_t field_ident(int k) {
  return field_op(k) == kMin ? INT64_MAX : field_op(k) == kMax ? INT64_MIN : 0;
}
__device__ __forceinline__ int64_t field_combine(int op, int64_t a, int64_t b) {
  return op == kMin ? (a < b ? a : b) : op == kMax ? (a > b ? a : b)
                                                    : (int64_t)((uint64_t)a + (uint64_t)b);
}

// one reduced field into the state (an identity adds nothing)
__device__ __forceinline__ void field_flush(DistState* d, int k, int64_t v) {
  typedef unsigned long long ull;
  if (v == field_ident(k)) return;
  switch (k) {
    case 0: {
      const uint64_t c = (uint64_t)v;
      atomicAdd((ull*)&d->n, (ull)(c & 0xFFFFu));
      if ((c >> 16) & 0xFFFFu) atomicAdd((ull*)&d->lat_neg, (ull)((c >> 16) & 0xFFFFu));
      if ((c >> 32) & 0xFFFFu) atomicAdd((ull*)&d->lat_over, (ull)((c >> 32) & 0xFFFFu));
      if (c >> 48) atomicAdd((ull*)&d->reordered, (ull)(c >> 48));
      break;
    }
    case 1: atomicAdd((ull*)&d->bytes, (ull)v); break;
    case 2: atomicAdd((ull*)&d->lat_sum, (ull)v); break;
    case 3: atomicMin((long long*)&d->lat_min, (long long)v); break;
    case 4: atomicMax((long long*)&d->lat_max, (long long)v); break;
    case 5: atomicAdd((ull*)&d->jitter_sum, (ull)v); break;
    case 6: atomicMax((ull*)&d->jitter_max, (ull)v); break;
    case 7: atomicMin((long long*)&d->gap_min, (long long)v); break;
    case 8: atomicMax((long long*)&d->gap_max, (long long)v); break;
    case 9: atomicAdd((ull*)&d->reorder_sum, (ull)v); break;
    case 10: atomicMax(&d->reorder_max, (uint32_t)v); break;
    case 11: atomicMin(&d->seq_min, (uint32_t)v); break;
    case 12: atomicMax(&d->seq_max, (uint32_t)v); break;
  }
}

__global__ void flow_dist_init_kernel(DistState* dist, uint32_t n_flows) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_flows) return;
  DistState d = {};
  d.lat_min = INT64_MAX;
  d.lat_max = INT64_MIN;
  d.gap_min = INT64_MAX;
  d.gap_max = INT64_MIN;
  d.seq_min = 0xFFFFFFFFu;
  dist[f] = d;
}

__global__ void flow_dist_snap_kernel(const DistState* __restrict__ dist, uint32_t n_flows,
                                      DistSnap* __restrict__ snap) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_flows) return;
  const DistState& d = dist[f];
  DistSnap s;
  s.last_lat = d.last_lat;
  s.last_rx = d.last_rx;
  s.seq_max = d.n ? (int64_t)d.seq_max : kNone;
  s.rsv = 0;
  snap[f] = s;
}

struct DistCols {
  const uint32_t *seq, *txs, *txu;
  const uint16_t* len;
  const uint32_t *rxs, *rxu;
};

__global__ void flow_dist_pack_kernel(DistCols col, uint32_t n, DistRec* __restrict__ rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t rs = col.rxs[i], ru = col.rxu[i], ts = col.txs[i], tu = col.txu[i];
  DistRec r;
  r.rx = rs * 1000000 + ru;
  r.lat = (rs - ts) * 1000000 + ru - tu;
  r.seq = col.seq[i];
  r.len = col.len[i];
  r.rsv0 = r.rsv1 = 0u;
  rec[i] = r;
}

// pass 1: per chunk, the largest seq among the records of its last flow, and whether that run
// is the whole chunk and continues the previous chunk's last flow
__global__ void __launch_bounds__(kChunk)
flow_dist_tail_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                      const uint32_t* __restrict__ bnd, uint32_t n_flows,
                      const uint32_t* __restrict__ seq, int64_t* __restrict__ tail_max,
                      uint32_t* __restrict__ tail_cont) {
  __shared__ int64_t s_v[kWaves];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) {  // no counted record here
    if (t == 0) {
      tail_max[c] = kNone;
      tail_cont[c] = 0u;
    }
    return;
  }
  const uint32_t pl = (uint32_t)min((uint64_t)nv, p0 + kChunk) - 1u;  // the last counted position
  const uint32_t fl = keys[pl];
  const uint32_t p = (uint32_t)p0 + t;
  int64_t v = kNone;
  // (the seq column, 4 B per record, stays in cache where the 32-B records do not: 80 against
  // 151 us at 8.4 M records)
  if (p <= pl && keys[p] == fl) v = (int64_t)seq[order[p]];
  v = wave_reduce<MaxOp>(v);
  if ((t & 63u) == 0u) s_v[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < kWaves; w++) v = v > s_v[w] ? v : s_v[w];
    tail_max[c] = v;
    // the run covers the chunk from its first position and started before it
    tail_cont[c] = (bnd[fl] < (uint32_t)p0) ? 1u : 0u;
  }
}

// pass 2 (one workgroup): scan[c] = the largest seq of chunk c's last flow over chunk c and the
// chunks before it that this flow fills (a segmented inclusive max over the chunks)
__global__ void __launch_bounds__(kChunk)
flow_dist_carry_kernel(const int64_t* __restrict__ tail_max, const uint32_t* __restrict__ tail_cont,
                       uint32_t n_chunks, int64_t* __restrict__ scan) {
  __shared__ int64_t s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  __shared__ int64_t s_run;
  chunk_carry<MaxOp>(
      n_chunks, kNone,
      [&](uint32_t c, int64_t& v) {
        v = tail_max[c];
        return tail_cont[c] == 0u;
      },
      [&](uint32_t c, int64_t v) { scan[c] = v; }, s_v, s_h, &s_run);
}

// pass 3: the statistics.  A lane per sorted position.
template <bool kHist>
__global__ void __launch_bounds__(kChunk)
flow_dist_main_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                      const uint32_t* __restrict__ bnd, uint32_t n_flows,
                      const DistRec* __restrict__ rec,
                      const DistSnap* __restrict__ snap, const int64_t* __restrict__ scan,
                      DistState* dist, uint64_t* hist) {
  __shared__ int64_t s_lat[kChunk], s_rx[kChunk], s_incl[kChunk];
  __shared__ int64_t s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  __shared__ int64_t s_red[kWaves][kFields];
  __shared__ uint32_t s_hist[kHist ? MGENX_FLOW_DIST_BINS : 1];
  __shared__ uint32_t s_long[kMaxLong][3];
  __shared__ uint32_t s_nlong;

  const uint32_t c = blockIdx.x, t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) return;  // (the whole workgroup)
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;
  if (t == 0) s_nlong = 0u;

  uint32_t f = 0, a = 0, b = 0, seq = 0, len = 0;
  int64_t lat = 0, rx = 0;
  bool head_flow = false, tail_flow = false;
  DistSnap sn = {0, 0, kNone, 0};
  if (active) {
    f = keys[p];
    const uint32_t r = order[p];
    const uint32_t f0 = bnd[f], f1 = bnd[f + 1u];  // the flow's run of sorted positions
    head_flow = p == f0;
    tail_flow = p == f1 - 1u;
    a = f0 > (uint32_t)p0 ? f0 - (uint32_t)p0 : 0u;
    b = (uint32_t)min((uint64_t)f1 - p0, (uint64_t)kChunk);
    const DistRec me = rec[r];
    seq = me.seq;
    len = me.len;
    rx = me.rx;
    lat = me.lat;
    if (head_flow) sn = snap[f];
  }
  s_lat[t] = lat;
  s_rx[t] = rx;

  // the running maximum: a run that starts its flow starts from the state's seq_max, the
  // chunk's first run otherwise from the chunks before it
  const bool seg_head = t == 0u || head_flow || !active;
  int64_t base = kNone;
  if (active && seg_head) {
    if (head_flow) {
      base = sn.seq_max;
    } else {  // t == 0 inside a flow: c > 0
      const int64_t m0 = snap[f].seq_max, m1 = scan[c - 1u];
      base = m0 > m1 ? m0 : m1;
    }
  }
  int64_t sv = active ? (int64_t)seq : kNone;
  if (base > sv) sv = base;
  const int64_t incl = seg_scan<MaxOp>(sv, seg_head, s_v, s_h);
  s_incl[t] = incl;
  __syncthreads();

  // this record's terms
  int64_t v[kFields];
#pragma unroll
  for (int k = 0; k < kFields; k++) v[k] = field_ident(k);
  uint32_t bin = MGENX_FLOW_DIST_BINS;
  bool is_long = false;
  if (active) {
    const int64_t m = seg_head ? base : s_incl[t - 1u];
    bool has_prev;
    int64_t plat, prx;
    if (head_flow) {
      has_prev = sn.seq_max != kNone;
      plat = sn.last_lat;
      prx = sn.last_rx;
    } else if (t > 0u) {
      has_prev = true;
      plat = s_lat[t - 1u];
      prx = s_rx[t - 1u];
    } else {
      has_prev = true;
      const DistRec pr = rec[order[p - 1u]];
      prx = pr.rx;
      plat = pr.lat;
    }
    const bool neg = lat < 0, over = lat >= (1ll << 32);
    const bool reo = (int64_t)seq < m;
    v[0] = (int64_t)(1ull | ((uint64_t)neg << 16) | ((uint64_t)over << 32) | ((uint64_t)reo << 48));
    v[1] = len;
    v[2] = lat;
    v[3] = lat;
    v[4] = lat;
    if (has_prev) {
      const int64_t dl = lat - plat;
      v[5] = dl < 0 ? -dl : dl;
      v[6] = v[5];
      v[7] = rx - prx;
      v[8] = v[7];
    }
    if (reo) {
      v[9] = m - (int64_t)seq;
      v[10] = v[9];
    }
    v[11] = seq;
    v[12] = seq;
    if (!neg && !over) bin = flow_dist_bin((uint64_t)lat);
    is_long = b - a >= kLong;
    if (is_long && t == a) {
      const uint32_t i = atomicAdd(&s_nlong, 1u);
      s_long[i][0] = a;
      s_long[i][1] = b;
      s_long[i][2] = f;
    }
    // carried for the next batch: written by the lanes that hold the flow's ends
    DistState* d = dist + f;
    if (head_flow && !has_prev) d->first_rx = rx;
    if (tail_flow) {
      d->last_rx = rx;
      d->last_lat = lat;
    }
    if (!is_long) {  // a short run: straight to global memory
#pragma unroll
      for (int k = 0; k < kFields; k++) field_flush(d, k, v[k]);
      if (kHist && bin < MGENX_FLOW_DIST_BINS)
        atomicAdd((unsigned long long*)&hist[(size_t)f * MGENX_FLOW_DIST_BINS + bin], 1ull);
    }
  }
  __syncthreads();

  // the long runs, one after the other: LDS histogram, workgroup reduction, one atomic per
  // field and non-zero bin
  const uint32_t n_long = s_nlong;
  for (uint32_t i = 0; i < n_long; i++) {
    const uint32_t ra = s_long[i][0], rb = s_long[i][1], rf = s_long[i][2];
    const bool in = active && t >= ra && t < rb;
    if (kHist) {
      if (t < MGENX_FLOW_DIST_BINS) s_hist[t] = 0u;
      __syncthreads();
      if (in && bin < MGENX_FLOW_DIST_BINS) atomicAdd(&s_hist[bin], 1u);
    }
    const uint32_t w0 = w * 64u;
    if (w0 < rb && w0 + 64u > ra) {  // (wave-uniform) the wave holds lanes of the run
      int64_t x[kFields];
#pragma unroll
      for (int k = 0; k < kFields; k++) {
        x[k] = in ? v[k] : field_ident(k);
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1)
          x[k] = field_combine(field_op(k), x[k], __shfl_xor((long long)x[k], d));
      }
      if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < kFields; k++) s_red[w][k] = x[k];
      }
    } else if (lane < (uint32_t)kFields) {
      int64_t id = 0;
#pragma unroll
      for (int k = 0; k < kFields; k++) id = lane == (uint32_t)k ? field_ident(k) : id;
      s_red[w][lane] = id;
    }
    __syncthreads();
    if (t < (uint32_t)kFields) {
      // (the packed counts of field 0 stay below 2^16 each: at most kChunk records)
#pragma unroll
      for (int k = 0; k < kFields; k++) {
        if (t == (uint32_t)k) {
          int64_t r = s_red[0][k];
          for (uint32_t ww = 1; ww < kWaves; ww++) r = field_combine(field_op(k), r, s_red[ww][k]);
          field_flush(dist + rf, k, r);
        }
      }
    }
    if (kHist && t < MGENX_FLOW_DIST_BINS) {
      const uint32_t cnt = s_hist[t];
      if (cnt)
        atomicAdd((unsigned long long*)&hist[(size_t)rf * MGENX_FLOW_DIST_BINS + t],
                  (unsigned long long)cnt);
    }
    __syncthreads();
  }
}

// ---- quantiles: one wave per flow, a scan over the bins for each requested rank ----
constexpr uint32_t kQGroup = 32;
struct DistQ {
  uint32_t q[kQGroup];
};

__global__ void flow_dist_quantiles_kernel(const DistState* __restrict__ dist,
                                           const uint64_t* __restrict__ hist, uint32_t n_flows,
                                           DistQ qs, uint32_t q_first, uint32_t q_count,
                                           uint32_t n_q, int64_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f = blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6);
  if (f >= n_flows) return;  // (the whole wave)
  const uint64_t n = dist[f].n, n_neg = dist[f].lat_neg;
  const uint64_t* h = hist + (size_t)f * MGENX_FLOW_DIST_BINS;
  for (uint32_t j = 0; j < q_count; j++) {
    int64_t val;
    if (n == 0) {
      val = INT64_MIN;
    } else {
      uint64_t r = ((uint64_t)qs.q[j] * n + 999u) / 1000u;
      if (r < 1u) r = 1u;
      if (r <= n_neg) {
        val = -1;
      } else {
        r -= n_neg;
        val = 1ll << 32;  // past every bin: among the overflows
        uint64_t run = 0;
        for (uint32_t b0 = 0; b0 < MGENX_FLOW_DIST_BINS; b0 += 64u) {
          uint64_t x = h[b0 + lane];  // (896 = 14 x 64)
#pragma unroll
          for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up((unsigned long long)x, d);
            if (lane >= d) x += o;
          }
          const unsigned long long hit = __ballot(run + x >= r);
          if (hit) {
            const uint32_t b = b0 + (uint32_t)__builtin_ctzll(hit);
            val = (int64_t)(flow_dist_bin_lo(b + 1u) - 1u);
            break;
          }
          run += __shfl((unsigned long long)x, 63);
        }
      }
    }
    if (lane == 0u) out[(size_t)f * n_q + q_first + j] = val;
  }
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (workspace owned by the context: struct mgenx_ctx, mgenx_internal.hpp)
// ------------------------------------------------------------------------------------
using namespace mgenx;


int mgenx::flow_dist_init_run(struct mgenx_flow_dist* dist, uint64_t* hist, uint32_t n_flows,
                              hipStream_t stream) {
  if (!n_flows) return MGENX_OK;
  hipLaunchKernelGGL(flow_dist_init_kernel, dim3((n_flows + 255u) / 256u), dim3(256), 0, stream,
                     dist, n_flows);
  if (hipGetLastError() != hipSuccess) return MGENX_EDEVICE;
  if (hist && hipMemsetAsync(hist, 0, (size_t)n_flows * MGENX_FLOW_DIST_BINS * 8u, stream) !=
                  hipSuccess)
    return MGENX_EDEVICE;
  return MGENX_OK;
}

// the passes mgenx_flow_dist and mgenx_flow_series share (mgenx_flowdist.hpp)
size_t mgenx::flow_prep_ws(uint32_t n, uint32_t n_flows) {
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  return a256(mgenx::flow_sort_ws(n, n_flows)) + 2 * a256((size_t)n_chunks * 8u) +
         a256((size_t)n_chunks * 4u) + a256((size_t)n * sizeof(DistRec));
}

int mgenx::flow_prep_run(void* mem, const uint32_t* flow_idx, const uint32_t* seq,
                         const uint32_t* txs, const uint32_t* txu, const uint16_t* len,
                         const uint32_t* rxs, const uint32_t* rxu, uint32_t n, uint32_t n_flows,
                         const uint32_t** keys, const uint32_t** order, const uint32_t** bnd,
                         const DistRec** rec_out, const int64_t** scan_out, hipStream_t stream,
                         char* err, size_t errn) {
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  const size_t c8 = a256((size_t)n_chunks * 8u), c4 = a256((size_t)n_chunks * 4u);
  Carve take(mem);
  void* sort_mem = take(mgenx::flow_sort_ws(n, n_flows));
  int64_t* tail_max = (int64_t*)take(c8);
  int64_t* scan = (int64_t*)take(c8);
  uint32_t* tail_cont = (uint32_t*)take(c4);
  DistRec* rec = (DistRec*)take((size_t)n * sizeof(DistRec));
  const int rc = mgenx::flow_sort_run(sort_mem, flow_idx, n, n_flows, keys, order, bnd, stream, err,
                                     errn);
  if (rc != MGENX_OK) return rc;
  const DistCols col = {seq, txs, txu, len, rxs, rxu};
  hipLaunchKernelGGL(flow_dist_pack_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, col, n,
                     rec);
  hipLaunchKernelGGL(flow_dist_tail_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, *keys, *order,
                     *bnd, n_flows, seq, tail_max, tail_cont);
  hipLaunchKernelGGL(flow_dist_carry_kernel, dim3(1), dim3(kChunk), 0, stream, tail_max, tail_cont,
                     n_chunks, scan);
  *rec_out = rec;
  *scan_out = scan;
  return MGENX_OK;
}

int mgenx::flow_dist_run(DevBuf& ws, const uint32_t* flow_idx, const uint32_t* seq,
                         const uint32_t* txs, const uint32_t* txu, const uint16_t* len,
                         const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                         struct mgenx_flow_dist* dist, uint64_t* hist, uint32_t n_flows,
                         hipStream_t stream, char* err, size_t errn) {
  if (n == 0 || n_flows == 0) return MGENX_OK;
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  const size_t snap_b = a256((size_t)n_flows * sizeof(DistSnap));
  const size_t need = snap_b + mgenx::flow_prep_ws(n, n_flows);
  if (ws.reserve(need) != hipSuccess) {
    snprintf(err, errn, "flow_dist: workspace of %zu bytes", need);
    return MGENX_EDEVICE;
  }
  DistSnap* snap = (DistSnap*)ws.p;
  hipLaunchKernelGGL(flow_dist_snap_kernel, dim3((n_flows + 255u) / 256u), dim3(256), 0, stream,
                     dist, n_flows, snap);
  const uint32_t *keys, *order, *bnd;
  const DistRec* rec;
  const int64_t* scan;
  const int rc = mgenx::flow_prep_run(static_cast<char*>(ws.p) + snap_b, flow_idx, seq, txs, txu,
                                     len, rxs, rxu, n, n_flows, &keys, &order, &bnd, &rec, &scan,
                                     stream, err, errn);
  if (rc != MGENX_OK) return rc;
  if (hist)
    hipLaunchKernelGGL(flow_dist_main_kernel<true>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                       order, bnd, n_flows, rec, snap, scan, dist, hist);
  else
    hipLaunchKernelGGL(flow_dist_main_kernel<false>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                       order, bnd, n_flows, rec, snap, scan, dist, hist);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "flow_dist: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}

int mgenx::flow_dist_quantiles_run(const struct mgenx_flow_dist* dist, const uint64_t* hist,
                                   uint32_t n_flows, const uint32_t* permille, uint32_t n_q,
                                   int64_t* out, hipStream_t stream) {
  for (uint32_t q0 = 0; q0 < n_q; q0 += kQGroup) {
    DistQ qs = {};
    const uint32_t cnt = n_q - q0 < kQGroup ? n_q - q0 : kQGroup;
    for (uint32_t j = 0; j < cnt; j++) qs.q[j] = permille[q0 + j];
    hipLaunchKernelGGL(flow_dist_quantiles_kernel, dim3((n_flows + 3u) / 4u), dim3(256), 0, stream,
                       dist, hist, n_flows, qs, q0, cnt, n_q, out);
  }
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}
