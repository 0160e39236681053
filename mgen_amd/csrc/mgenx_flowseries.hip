// mgenx_flowseries.hip -- per-flow time series on gfx950 (mgenx_flow_series, include/mgenx.h):
// records, bytes, latency, jitter and the movement of the sequence numbers per flow and per
// window of receive time, all flows on one time axis.
//
// Ordered by flow with the receive order kept, a record needs its predecessor in the flow (the
// jitter) and the running maximum M of the flow's earlier sequence numbers (fresh / late /
// advance); everything else is the record's own.  The first passes are mgenx_flow_dist's
// (mgenx::flow_prep_run, mgenx_flowdist.hip): the stable sort by flow, one 32-B record per input
// record, and per chunk of kChunk sorted positions the M its first run starts from.  Then:
//   0. flow_series_snap_kernel copies what the batch's first record of a flow pairs with
//      (n, last_lat, seq_max) out of the states, which the main pass overwrites;
//   1. flow_series_main_kernel: a lane per sorted position.  A segmented max scan of seq gives
//      each lane its M.  Each lane computes its terms and its key (flow, bin); adjacent lanes
//      with equal keys form a run, reduced by a segmented scan (wave shuffles, then LDS across
//      the waves), and the run's last lane issues one atomic per field that is not its identity.
//      A narrow window gives runs of a record or two (atomics straight from the lanes), a wide
//      one a run per flow and chunk.  A receive time that goes backwards only cuts runs shorter:
//      sums, minima and maxima of integers commute, so the bytes left do not depend on how the
//      runs fall or on the order the workgroups finish in.
//      The state has one writer per flow: the lane holding the flow's last record of the batch
//      (n, last_lat, seq_max).  Only `outside` is added to, by the runs that fell outside the bins.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include "mgenx_blockscan.hpp"
#include "mgenx_flowdist.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

typedef struct mgenx_flow_series_bin SeriesBin;
typedef struct mgenx_flow_series_state SeriesState;
static_assert(sizeof(SeriesBin) == 64, "mgenx_flow_series_bin is 64 B");
static_assert(sizeof(SeriesState) == 32, "mgenx_flow_series_state is 32 B");

constexpr uint32_t kOutside = 0xFFFFFFFFu;  // the bin of a record outside [0, n_bins)
constexpr uint64_t kNoKey = ~0ull;          // the key of a lane past the counted records

// what a flow's first record of the batch pairs with
struct SeriesSnap {
  uint64_t n;
  int64_t last_lat;
  int64_t seq_max;  // kNone while the flow has no record
  int64_t rsv;
};

// the terms of one record, or of a run of records of one (flow, bin); its own operator for
// seg_scan (mgenx_blockscan.hpp)
struct SeriesAcc {
  uint64_t cnt;  // n | fresh << 16 | late << 32: at most kChunk each
  uint64_t bytes, lat_sum, jitter, advance;
  int64_t lat_min, lat_max;

  static __device__ __forceinline__ SeriesAcc of(SeriesAcc a, const SeriesAcc& b) {
    a.cnt += b.cnt;
    a.bytes += b.bytes;
    a.lat_sum += b.lat_sum;
    a.jitter += b.jitter;
    a.advance += b.advance;
    a.lat_min = a.lat_min < b.lat_min ? a.lat_min : b.lat_min;
    a.lat_max = a.lat_max > b.lat_max ? a.lat_max : b.lat_max;
    return a;
  }
};

__global__ void flow_series_init_kernel(SeriesState* state, SeriesBin* bins, uint32_t n_flows,
                                        uint32_t n_cells) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_flows) {
    SeriesState s = {};
    state[i] = s;
  }
  if (i < n_cells) {
    SeriesBin b = {};
    b.lat_min = INT64_MAX;
    b.lat_max = INT64_MIN;
    bins[i] = b;
  }
}

__global__ void flow_series_snap_kernel(const SeriesState* __restrict__ state, uint32_t n_flows,
                                        SeriesSnap* __restrict__ snap) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_flows) return;
  const SeriesState& d = state[f];
  SeriesSnap s;
  s.n = d.n;
  s.last_lat = d.last_lat;
  s.seq_max = d.n ? (int64_t)d.seq_max : kNone;
  s.rsv = 0;
  snap[f] = s;
}

// the statistics: a lane per sorted position
__global__ void __launch_bounds__(kChunk)
flow_series_main_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                        const uint32_t* __restrict__ bnd, uint32_t n_flows,
                        const DistRec* __restrict__ rec, const SeriesSnap* __restrict__ snap,
                        const int64_t* __restrict__ scan, int64_t t0, uint64_t width,
                        uint32_t n_bins, SeriesState* state, SeriesBin* bins) {
  typedef unsigned long long ull;
  __shared__ int64_t s_lat[kChunk], s_incl[kChunk];
  __shared__ uint64_t s_key[kChunk];
  __shared__ int64_t s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  __shared__ SeriesAcc s_a[kWaves];

  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) return;  // (the whole workgroup)
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;

  uint32_t f = 0, seq = 0, len = 0, bin = kOutside;
  int64_t lat = 0;
  bool head_flow = false, tail_flow = false;
  SeriesSnap sn = {0, 0, kNone, 0};
  uint64_t key = kNoKey;
  if (active) {
    f = keys[p];
    const uint32_t f0 = bnd[f], f1 = bnd[f + 1u];  // the flow's run of sorted positions
    head_flow = p == f0;
    tail_flow = p == f1 - 1u;
    const DistRec me = rec[order[p]];
    seq = me.seq;
    len = me.len;
    lat = me.lat;
    // 0 <= rx < 2^53, so rx - t0 fits 64 unsigned bits whenever it is not negative
    if (me.rx >= t0) {
      const uint64_t b = ((uint64_t)me.rx - (uint64_t)t0) / width;
      if (b < (uint64_t)n_bins) bin = (uint32_t)b;
    }
    if (head_flow || tail_flow) sn = snap[f];
    key = ((uint64_t)f << 32) | bin;
  }
  s_lat[t] = lat;
  s_key[t] = key;

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
  SeriesAcc a = {0, 0, 0, 0, 0, INT64_MAX, INT64_MIN};
  bool run_head = true, run_tail = false;
  if (active) {
    const int64_t m = seg_head ? base : s_incl[t - 1u];
    bool has_prev;
    int64_t plat;
    if (head_flow) {
      has_prev = sn.seq_max != kNone;
      plat = sn.last_lat;
    } else if (t > 0u) {
      has_prev = true;
      plat = s_lat[t - 1u];
    } else {
      has_prev = true;
      plat = rec[order[p - 1u]].lat;
    }
    const bool fresh = m == kNone || (int64_t)seq > m, late = (int64_t)seq < m;
    a.cnt = 1ull | ((uint64_t)fresh << 16) | ((uint64_t)late << 32);
    a.bytes = len;
    a.lat_sum = (uint64_t)lat;
    a.lat_min = a.lat_max = lat;
    if (has_prev) {
      const int64_t dl = lat - plat;
      a.jitter = (uint64_t)(dl < 0 ? -dl : dl);
    }
    if (fresh) a.advance = m == kNone ? 1ull : (uint64_t)((int64_t)seq - m);
    run_head = t == 0u || s_key[t - 1u] != key;
    run_tail = t == kChunk - 1u || s_key[t + 1u] != key;
    // carried for the next batch: one writer per flow
    if (tail_flow) {
      SeriesState* d = state + f;
      d->n = sn.n + (uint64_t)(bnd[f + 1u] - bnd[f]);
      d->last_lat = lat;
      d->seq_max = (uint32_t)incl;
    }
  }
  a = seg_scan<SeriesAcc, false>(a, run_head, s_a, s_h);

  if (active && run_tail) {
    const uint64_t n = a.cnt & 0xFFFFu;
    if (bin == kOutside) {
      atomicAdd((ull*)&state[f].outside, (ull)n);
    } else {
      SeriesBin* b = bins + ((size_t)f * n_bins + bin);
      const uint32_t fresh = (uint32_t)(a.cnt >> 16) & 0xFFFFu, late = (uint32_t)(a.cnt >> 32);
      atomicAdd((ull*)&b->n, (ull)n);
      if (a.bytes) atomicAdd((ull*)&b->bytes, (ull)a.bytes);
      if (a.lat_sum) atomicAdd((ull*)&b->lat_sum, (ull)a.lat_sum);
      atomicMin((long long*)&b->lat_min, (long long)a.lat_min);
      atomicMax((long long*)&b->lat_max, (long long)a.lat_max);
      if (a.jitter) atomicAdd((ull*)&b->jitter_sum, (ull)a.jitter);
      if (a.advance) atomicAdd((ull*)&b->advance, (ull)a.advance);
      if (fresh) atomicAdd(&b->fresh, fresh);
      if (late) atomicAdd(&b->late, late);
    }
  }
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (workspace owned by the context: struct mgenx_ctx, mgenx_internal.hpp)
// ------------------------------------------------------------------------------------
using namespace mgenx;

// n_flows >= 1, n_flows * n_bins < 2^31
int mgenx::flow_series_init_run(struct mgenx_flow_series_state* state,
                                struct mgenx_flow_series_bin* bins, uint32_t n_flows,
                                uint32_t n_bins, hipStream_t stream) {
  const uint32_t n_cells = n_flows * n_bins;
  const uint32_t m = n_cells > n_flows ? n_cells : n_flows;
  hipLaunchKernelGGL(flow_series_init_kernel, dim3((m + 255u) / 256u), dim3(256), 0, stream, state,
                     bins, n_flows, n_cells);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

int mgenx::flow_series_run(DevBuf& ws, const uint32_t* flow_idx, const uint32_t* seq,
                           const uint32_t* txs, const uint32_t* txu, const uint16_t* len,
                           const uint32_t* rxs, const uint32_t* rxu, uint32_t n, int64_t t0,
                           uint64_t width, uint32_t n_bins, struct mgenx_flow_series_state* state,
                           struct mgenx_flow_series_bin* bins, uint32_t n_flows, hipStream_t stream,
                           char* err, size_t errn) {
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  const size_t snap_b = a256((size_t)n_flows * sizeof(SeriesSnap));
  const size_t need = snap_b + mgenx::flow_prep_ws(n, n_flows);
  if (ws.reserve(need) != hipSuccess) {
    snprintf(err, errn, "flow_series: workspace of %zu bytes", need);
    return MGENX_EDEVICE;
  }
  SeriesSnap* snap = (SeriesSnap*)ws.p;
  hipLaunchKernelGGL(flow_series_snap_kernel, dim3((n_flows + 255u) / 256u), dim3(256), 0, stream,
                     state, n_flows, snap);
  const uint32_t *keys, *order, *bnd;
  const DistRec* rec;
  const int64_t* scan;
  const int rc = mgenx::flow_prep_run(static_cast<char*>(ws.p) + snap_b, flow_idx, seq, txs, txu,
                                     len, rxs, rxu, n, n_flows, &keys, &order, &bnd, &rec, &scan,
                                     stream, err, errn);
  if (rc != MGENX_OK) return rc;
  hipLaunchKernelGGL(flow_series_main_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, order,
                     bnd, n_flows, rec, snap, scan, t0, width, n_bins, state, bins);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "flow_series: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}
