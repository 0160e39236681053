// mgenx_match.hip -- a sender's log joined with a receiver's log on gfx950 (mgenx_msg_match,
// mgenx_msg_match_ex, mgenx_match_side; include/mgenx.h): an equi-join of two record sets on the
// message identity, then per-flow delivery accounting in the sender's order.
//
//   0. match_init_kernel writes the empty per-flow values, zeroes the global counters and
//      empties the hash table;
//   1. match_build_kernel: a lane per send record.  An open-addressing table of send indices
//      (a power of two >= 2 ns slots of 4 B, kEmpty = no record), linear probing from a 64-bit
//      mix of the identity.  A lane takes an empty slot with a compare-and-swap; on a slot whose
//      record has the equal identity (compared through the columns, never through the hash) it
//      atomicMin's its own index in.  Equal identities share one probe sequence and a slot never
//      changes identity, so each identity ends in exactly one slot holding its lowest index,
//      whatever the interleaving.  Only atomics touch the table inside this launch; the probe
//      loop is bounded by the slot count and no lane waits on another;
//   2. match_mark_kernel: own[i] = the index its identity's slot holds (i itself for an owner);
//   3. match_probe_kernel: a lane per recv record finds the owner or none, writes recv_send,
//      counts into send_rx_count (atomicAdd) and send_first_rx (atomicMin); the orphans of a
//      flow and the global counters are summed per wave before their atomics;
//   4. the send records ordered by flow, stably (mgenx::flow_sort_run, as mgenx_flow_dist runs
//      it), and cut into chunks of kChunk sorted positions that ignore the flow edges.
//      Every position is U (an undelivered owner), D (a delivered owner) or X (a send
//      duplicate, which neither counts nor breaks a run).  A loss run is a segment of a
//      segmented sum of the U flags, segments starting at a flow's first position and at every
//      D; bit 31 of the summed word marks a segment that started with its flow (no D yet).
//      match_pack_kernel classifies, leaves one 16-B record per position and per chunk the sum
//      after its last segment start and whether it has one; match_carry_kernel (one workgroup)
//      scans those over the chunks; match_main_kernel repeats the scan with the carry and
//      counts a run once, where it ends: at the D that follows it, or at the flow's last
//      position.  lost_head and lost_tail fall out of the same word and have one writer per
//      flow.  The other fields are reduced per run of a flow inside the chunk (a second
//      segmented scan; the 18 histogram counts ride along as 12-bit fields of four words) and
//      go out as one atomic per field that is not its identity.  Integer sums, minima and
//      maxima commute, so the bytes left do not depend on the order the workgroups finish in.
//   5. mgenx_msg_match_ex's timeline, only when asked for: match_mark_kernel writes own[] into
//      the caller's owner column; match_pack_kernel<true> also leaves each position's send stamp
//      and a second chunk summary (the first and last U after the last segment start);
//      match_series_kernel reduces the positions of one (flow, window of send time) that follow
//      each other and adds them to the cell with atomics; match_carry_fl_kernel,
//      match_runs_kernel<false>, match_run_base_kernel and match_runs_kernel<true> find each run
//      where the main pass counts it, with its first and last U, count the listed ones per
//      chunk, scan the counts and write the list in the order of the sorted positions.
// The identity, the table with its build and mark kernels and the carry kernel are in
// mgenx_match.hpp, shared with mgenx_matchmulti.hip; the segmented scan is mgenx_blockscan.hpp's.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include "mgenx_match.hpp"

namespace mgenx {

typedef struct mgenx_flow_match FlowMatch;
static_assert(sizeof(FlowMatch) == 256, "mgenx_flow_match is 256 B");

constexpr uint32_t kFromFlowStart = 1u << 31;  // the segment began with its flow: no D yet
constexpr uint32_t kLenMask = kFromFlowStart - 1u;
enum : uint8_t { kX = 0, kU = 1, kD = 2 };

// one sorted position as the main pass reads it
struct alignas(16) MatchRec {
  int64_t lat;   // D only
  uint32_t len;  // U and D
  uint32_t rxc;  // D: send_rx_count
};
static_assert(sizeof(MatchRec) == 16, "MatchRec is 16 B");

__global__ void match_init_kernel(FlowMatch* flows, uint32_t n_flows, MatchStats* stats,
                                  uint32_t* table, uint32_t n_slots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_flows) {
    FlowMatch f = {};
    f.lat_min = INT64_MAX;
    f.lat_max = INT64_MIN;
    flows[i] = f;
  }
  if (i < n_slots) table[i] = kEmpty;
  if (i == 0) {
    MatchStats s = {};
    *stats = s;
  }
}

__global__ void match_probe_kernel(MatchSide send, MatchSide recv, uint32_t nr, uint32_t n_flows,
                                   bool use_time, const uint32_t* __restrict__ table,
                                   uint32_t mask, uint32_t* send_rx_count, uint32_t* send_first_rx,
                                   uint32_t* __restrict__ recv_send, FlowMatch* flows,
                                   MatchStats* stats) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  bool skipped = false, orphan = false;
  uint32_t f = 0;
  if (j < nr) {
    f = recv.flow[j];
    uint32_t o = kEmpty;
    if (f >= n_flows) {
      skipped = true;
    } else {
      o = table_find(table, mask, send, use_time, ident_of(recv, j, use_time));
      if (o == kEmpty) {
        orphan = true;
      } else {
        atomicAdd(&send_rx_count[o], 1u);
        atomicMin(&send_first_rx[o], j);
      }
    }
    recv_send[j] = o;
  }
  wave_count_add(&stats->recv_skipped, skipped);
  wave_count_add(&stats->recv_unmatched, orphan);
  // the orphans of one flow among the wave's lanes: one add per flow
  unsigned long long left = __ballot(orphan);
  const uint32_t lane = threadIdx.x & 63u;
  while (left) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t lf = __shfl(f, lead);
    const unsigned long long same = __ballot(orphan && f == lf) & left;
    if (lane == lead)
      atomicAdd((unsigned long long*)&flows[lf].rx_orphan, (unsigned long long)__popcll(same));
    left &= ~same;
  }
}

// a position's word in the loss-run scan and whether it starts a segment
__device__ __forceinline__ uint32_t run_word(uint8_t cls, bool head_flow, bool* head) {
  *head = head_flow || cls == kD;
  if (cls == kD) return 0u;
  return (cls == kU ? 1u : 0u) | (head_flow ? kFromFlowStart : 0u);
}

// ---- the first and the last U of a loss run (mgenx_msg_match_ex's run list) ----
// The scan of run_word's segments with another operator: a U at lane t is the word
// (0x800 - t) << 16 | (t + 1), every other position 0 (no U), and the halves combine by maximum:
// the high half ends as 0x800 - the lowest lane with a U, the low half as the highest + 1.
struct FlOp {
  static __device__ __forceinline__ uint32_t of(uint32_t a, uint32_t b) {
    const uint32_t ah = a & 0xFFFF0000u, bh = b & 0xFFFF0000u, al = a & 0xFFFFu, bl = b & 0xFFFFu;
    return (ah > bh ? ah : bh) | (al > bl ? al : bl);
  }
};
__device__ __forceinline__ uint32_t fl_word(uint8_t cls, uint32_t t) {
  return cls == kU ? ((0x800u - t) << 16) | (t + 1u) : 0u;
}
// sorted positions from a chunk's word: the first U (kEmpty: none) and the last U + 1 (0: none)
__device__ __forceinline__ uint32_t fl_first(uint32_t w, uint32_t p0) {
  const uint32_t h = (w >> 16) & 0xFFFu;
  return h ? p0 + 0x800u - h : kEmpty;
}
__device__ __forceinline__ uint32_t fl_last1(uint32_t w, uint32_t p0) {
  const uint32_t l = w & 0xFFFFu;
  return l ? p0 + l : 0u;
}

struct PackCols {
  const uint32_t *own, *rx_count, *first_rx, *len, *t_sec, *t_usec, *rx_sec, *rx_usec;
};

// pass 4a: classify, pack, and the chunk's summary.  kTimeline (mgenx_msg_match_ex with a series
// or a run list): the position's send stamp rides along, and trail_fl[c] is the chunk's first
// and last U after its last segment start (fl_word).
template <bool kTimeline>
__global__ void __launch_bounds__(kChunk)
match_pack_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                  const uint32_t* __restrict__ bnd, uint32_t n_flows, PackCols col,
                  MatchRec* __restrict__ rec, uint8_t* __restrict__ cls_out,
                  uint32_t* __restrict__ trail, uint32_t* __restrict__ has_head,
                  int64_t* __restrict__ stamp, uint32_t* __restrict__ trail_fl) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) {  // no counted record here
    if (t == 0) {
      trail[c] = 0u;
      has_head[c] = 1u;
      if (kTimeline) trail_fl[c] = 0u;
    }
    return;
  }
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;
  uint8_t cls = kX;
  bool head = true;
  uint32_t v = 0u;
  if (active) {
    const uint32_t f = keys[p], i = order[p];
    MatchRec r = {0, 0u, 0u};
    if (col.own[i] == i) {
      const uint32_t cnt = col.rx_count[i];
      r.len = col.len[i];
      if (cnt) {
        const uint32_t j = col.first_rx[i];
        cls = kD;
        r.rxc = cnt;
        r.lat = ((int64_t)col.rx_sec[j] - (int64_t)col.t_sec[i]) * 1000000 +
                (int64_t)col.rx_usec[j] - (int64_t)col.t_usec[i];
      } else {
        cls = kU;
      }
    }
    // (a send duplicate's stamp places nothing: it only keeps the series' key runs whole)
    if (kTimeline) stamp[p] = (int64_t)col.t_sec[i] * 1000000 + (int64_t)col.t_usec[i];
    rec[p] = r;
    cls_out[p] = cls;
    v = run_word(cls, p == bnd[f], &head);
  }
  const uint32_t incl = seg_scan<SumOp>(v, head, s_v, s_h);
  const int any = __syncthreads_or(active && head);
  const uint32_t last = (uint32_t)min((uint64_t)nv - p0, (uint64_t)kChunk) - 1u;
  if (t == last) {
    trail[c] = incl;
    has_head[c] = any ? 1u : 0u;
  }
  if (kTimeline) {
    const uint32_t fl = seg_scan<FlOp>(fl_word(cls, t), head, s_v, s_h);
    if (t == last) trail_fl[c] = fl;
  }
}

// the terms of one position, or of a run of positions of one flow; its own operator for seg_scan
struct MatchAcc {
  uint64_t cnt;  // sent | send_dup << 16 | delivered << 32 | loss_runs << 48: at most kChunk each
  uint64_t sent_bytes, delivered_bytes, rx_dup, lat_sum, run_max;
  int64_t lat_min, lat_max;
  uint64_t hist[4];  // loss_run_hist[k] in bits 12 (k % 5) .. of word k / 5: at most kChunk each

  static __device__ __forceinline__ MatchAcc of(MatchAcc a, const MatchAcc& b) {
    a.cnt += b.cnt;
    a.sent_bytes += b.sent_bytes;
    a.delivered_bytes += b.delivered_bytes;
    a.rx_dup += b.rx_dup;
    a.lat_sum += b.lat_sum;
    a.run_max = a.run_max > b.run_max ? a.run_max : b.run_max;
    a.lat_min = a.lat_min < b.lat_min ? a.lat_min : b.lat_min;
    a.lat_max = a.lat_max > b.lat_max ? a.lat_max : b.lat_max;
#pragma unroll
    for (int k = 0; k < 4; k++) a.hist[k] += b.hist[k];
    return a;
  }
};

// pass 4c: the accounting.  A lane per sorted position.
__global__ void __launch_bounds__(kChunk)
match_main_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ bnd,
                  uint32_t n_flows, const MatchRec* __restrict__ rec,
                  const uint8_t* __restrict__ cls_in, const uint32_t* __restrict__ carry,
                  FlowMatch* flows) {
  typedef unsigned long long ull;
  __shared__ uint32_t s_incl[kChunk], s_key[kChunk];
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ MatchAcc s_a[kWaves];

  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) return;  // (the whole workgroup)
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;

  uint32_t f = kEmpty;
  uint8_t cls = kX;
  bool head_flow = false, tail_flow = false, head = true;
  MatchRec me = {0, 0u, 0u};
  uint32_t v = 0u, cin = 0u;
  if (active) {
    f = keys[p];
    head_flow = p == bnd[f];
    tail_flow = p == bnd[f + 1u] - 1u;
    cls = cls_in[p];
    me = rec[p];
    v = run_word(cls, head_flow, &head);
    // the chunk's first position inside a flow continues the chunks before it (c > 0)
    if (t == 0u && !head_flow) {
      cin = carry[c - 1u];
      if (cls != kD) v += cin;
    }
  }
  s_key[t] = f;
  const uint32_t incl = seg_scan<SumOp>(v, head, s_v, s_h);
  s_incl[t] = incl;
  __syncthreads();

  MatchAcc a = {0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN, {0, 0, 0, 0}};
  bool run_head = true, run_tail = false;
  if (active) {
    // a loss run is counted where it ends: at the D after it, or at the flow's last position
    uint32_t ended = 0u;
    if (cls == kD)
      ended = head_flow ? 0u : t == 0u ? cin : s_incl[t - 1u];
    else if (tail_flow)
      ended = incl;
    const uint32_t run = ended & kLenMask;
    FlowMatch* d = flows + f;
    if (run) {
      // one writer per flow and field: the first D of the flow, or its last position
      if (ended & kFromFlowStart)
        d->lost_head = run;
      else if (cls != kD)
        d->lost_tail = run;
      const uint32_t k = min(31u - (uint32_t)__builtin_clz(run), 17u);
      // (static indices: a runtime one would put the terms in scratch memory)
#pragma unroll
      for (uint32_t w = 0; w < 4u; w++) a.hist[w] = k / 5u == w ? 1ull << (12u * (k % 5u)) : 0ull;
      a.run_max = run;
    }
    a.cnt = (uint64_t)(cls != kX) | ((uint64_t)(cls == kX) << 16) | ((uint64_t)(cls == kD) << 32) |
            ((uint64_t)(run != 0u) << 48);
    a.sent_bytes = me.len;
    if (cls == kD) {
      a.delivered_bytes = me.len;
      a.rx_dup = me.rxc - 1u;
      a.lat_sum = (uint64_t)me.lat;
      a.lat_min = a.lat_max = me.lat;
    }
    run_head = t == 0u || s_key[t - 1u] != f;
    run_tail = t == kChunk - 1u || s_key[t + 1u] != f;
  }
  a = seg_scan<MatchAcc, false>(a, run_head, s_a, s_h);

  if (active && run_tail) {
    FlowMatch* d = flows + f;
    const uint64_t sent = a.cnt & 0xFFFFu, dup = (a.cnt >> 16) & 0xFFFFu,
                   dlv = (a.cnt >> 32) & 0xFFFFu, runs = a.cnt >> 48;
    if (sent) atomicAdd((ull*)&d->sent, (ull)sent);
    if (a.sent_bytes) atomicAdd((ull*)&d->sent_bytes, (ull)a.sent_bytes);
    if (dup) atomicAdd((ull*)&d->send_dup, (ull)dup);
    if (dlv) {
      atomicAdd((ull*)&d->delivered, (ull)dlv);
      if (a.delivered_bytes) atomicAdd((ull*)&d->delivered_bytes, (ull)a.delivered_bytes);
      if (a.rx_dup) atomicAdd((ull*)&d->rx_dup, (ull)a.rx_dup);
      if (a.lat_sum) atomicAdd((ull*)&d->lat_sum, (ull)a.lat_sum);
      atomicMin((long long*)&d->lat_min, (long long)a.lat_min);
      atomicMax((long long*)&d->lat_max, (long long)a.lat_max);
    }
    if (runs) {
      atomicAdd((ull*)&d->loss_runs, (ull)runs);
      atomicMax((ull*)&d->loss_run_max, (ull)a.run_max);
#pragma unroll
      for (uint32_t k = 0; k < 18u; k++) {
        const uint64_t n = (a.hist[k / 5u] >> (12u * (k % 5u))) & 0xFFFu;
        if (n) atomicAdd((ull*)&d->loss_run_hist[k], (ull)n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// the timeline (mgenx_msg_match_ex): the series per send-time window and the run list.
// Both read what passes 4a and 4b left (cls, MatchRec, the stamps, the carries) and run after
// them, only when asked for.
// ------------------------------------------------------------------------------------
typedef struct mgenx_match_bin MatchBin;
typedef struct mgenx_loss_run LossRun;
static_assert(sizeof(MatchBin) == 64, "mgenx_match_bin is 64 B");
static_assert(sizeof(LossRun) == 40, "mgenx_loss_run is 40 B");
constexpr uint32_t kOutside = 1u << 31;  // a series key outside the windows: kOutside | flow

// every cell, every outside count and the run count: written on every call
__global__ void match_tl_init_kernel(MatchBin* bins, uint32_t n_cells, uint64_t* outside,
                                     uint32_t n_flows, uint64_t* n_runs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_cells) {
    MatchBin b = {};
    b.lat_min = INT64_MAX;
    b.lat_max = INT64_MIN;
    bins[i] = b;
  }
  if (i < n_flows && outside) outside[i] = 0ull;
  if (i == 0 && n_runs) *n_runs = 0ull;
}

// the terms of one position, or of a run of positions of one (flow, window); its own operator
// for seg_scan
struct MatchBinAcc {
  uint32_t cnt;  // sent | delivered << 16: at most kChunk each
  uint64_t sent_bytes, delivered_bytes, rx_dup, lat_sum;
  int64_t lat_min, lat_max;

  static __device__ __forceinline__ MatchBinAcc of(MatchBinAcc a, const MatchBinAcc& b) {
    a.cnt += b.cnt;
    a.sent_bytes += b.sent_bytes;
    a.delivered_bytes += b.delivered_bytes;
    a.rx_dup += b.rx_dup;
    a.lat_sum += b.lat_sum;
    a.lat_min = a.lat_min < b.lat_min ? a.lat_min : b.lat_min;
    a.lat_max = a.lat_max > b.lat_max ? a.lat_max : b.lat_max;
    return a;
  }
};

// the series.  A lane per sorted position; the positions of one (flow, window) that follow each
// other are reduced on chip and leave one atomic per field that is not its identity.  A cell
// that comes up again (a log out of time order, a later chunk) is combined by those atomics.
__global__ void __launch_bounds__(kChunk)
match_series_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ bnd,
                    uint32_t n_flows, const MatchRec* __restrict__ rec,
                    const uint8_t* __restrict__ cls_in, const int64_t* __restrict__ stamp,
                    int64_t t0, uint64_t width, uint32_t n_bins, MatchBin* bins,
                    uint64_t* outside) {
  typedef unsigned long long ull;
  __shared__ uint32_t s_key[kChunk];
  __shared__ uint32_t s_h[kWaves];
  __shared__ MatchBinAcc s_a[kWaves];

  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) return;  // (the whole workgroup)
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;

  uint32_t key = kEmpty, f = 0u;
  MatchBinAcc a = {0u, 0, 0, 0, 0, INT64_MAX, INT64_MIN};
  if (active) {
    f = keys[p];
    const uint8_t cls = cls_in[p];
    const MatchRec me = rec[p];
    // t0 lies in [-2^62, 2^62] and a stamp in [0, 2^53): the difference fits; a negative floor
    // is outside whatever its value
    const int64_t d = stamp[p] - t0;
    const uint64_t b = d < 0 ? (uint64_t)n_bins : (uint64_t)d / width;
    key = b < n_bins ? f * n_bins + (uint32_t)b : kOutside | f;
    if (cls != kX) {
      a.cnt = 1u;
      a.sent_bytes = me.len;
    }
    if (cls == kD) {
      a.cnt |= 1u << 16;
      a.delivered_bytes = me.len;
      a.rx_dup = me.rxc - 1u;
      a.lat_sum = (uint64_t)me.lat;
      a.lat_min = a.lat_max = me.lat;
    }
  }
  s_key[t] = key;
  __syncthreads();
  const bool run_head = !active || t == 0u || s_key[t - 1u] != key;
  const bool run_tail = active && (t == kChunk - 1u || s_key[t + 1u] != key);
  a = seg_scan<MatchBinAcc, false>(a, run_head, s_a, s_h);

  if (run_tail) {
    const uint32_t sent = a.cnt & 0xFFFFu, dlv = a.cnt >> 16;
    if (key & kOutside) {
      if (sent) atomicAdd((ull*)&outside[f], (ull)sent);
    } else if (sent) {
      MatchBin* d = bins + key;
      atomicAdd((ull*)&d->sent, (ull)sent);
      if (a.sent_bytes) atomicAdd((ull*)&d->sent_bytes, (ull)a.sent_bytes);
      if (dlv) {
        atomicAdd((ull*)&d->delivered, (ull)dlv);
        if (a.delivered_bytes) atomicAdd((ull*)&d->delivered_bytes, (ull)a.delivered_bytes);
        if (a.rx_dup) atomicAdd((ull*)&d->rx_dup, (ull)a.rx_dup);
        if (a.lat_sum) atomicAdd((ull*)&d->lat_sum, (ull)a.lat_sum);
        atomicMin((long long*)&d->lat_min, (long long)a.lat_min);
        atomicMax((long long*)&d->lat_max, (long long)a.lat_max);
      }
    }
  }
}

// (one workgroup) over the chunks, as match_carry_kernel: carry_first[c] / carry_last1[c] = the
// sorted position of the first U and of the last U + 1 (kEmpty / 0: none) in the segment that
// is open after chunk c's last position
__global__ void __launch_bounds__(kChunk)
match_carry_fl_kernel(const uint32_t* __restrict__ trail_fl, const uint32_t* __restrict__ has_head,
                      uint32_t n_chunks, uint32_t* __restrict__ carry_first,
                      uint32_t* __restrict__ carry_last1) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_first, s_last1;
  // (two walks over the chunks, one word each: one walk of a two-word value would double s_v)
  chunk_carry<MinOp>(
      n_chunks, kEmpty,
      [&](uint32_t c, uint32_t& v) {
        v = fl_first(trail_fl[c], c * kChunk);
        return has_head[c] != 0u;
      },
      [&](uint32_t c, uint32_t v) { carry_first[c] = v; }, s_v, s_h, &s_first);
  chunk_carry<MaxOp>(
      n_chunks, 0u,
      [&](uint32_t c, uint32_t& v) {
        v = fl_last1(trail_fl[c], c * kChunk);
        return has_head[c] != 0u;
      },
      [&](uint32_t c, uint32_t v) { carry_last1[c] = v; }, s_v, s_h, &s_last1);
}

// the run list.  A run is found where match_main_kernel counts it: at the D that follows it or
// at its flow's last position, so the list's order is the order of the sorted positions: by
// flow, then by send index.  kWrite false: chunk_n[c] = the listed runs that end in chunk c.
// kWrite true (after match_run_base_kernel): each is written at chunk_base[c] + its rank in the
// chunk, unless the list does not fit.
template <bool kWrite>
__global__ void __launch_bounds__(kChunk)
match_runs_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                  const uint32_t* __restrict__ bnd, uint32_t n_flows,
                  const uint8_t* __restrict__ cls_in, const int64_t* __restrict__ stamp,
                  const uint32_t* __restrict__ carry, const uint32_t* __restrict__ carry_first,
                  const uint32_t* __restrict__ carry_last1, uint32_t min_run,
                  uint32_t* __restrict__ chunk_n, const uint32_t* __restrict__ chunk_base,
                  const uint64_t* __restrict__ n_runs, LossRun* __restrict__ runs,
                  uint64_t run_cap) {
  __shared__ uint32_t s_incl[kChunk], s_fl[kChunk];
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_cin[3];

  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) {  // (the whole workgroup)
    if (!kWrite && t == 0) chunk_n[c] = 0u;
    return;
  }
  if (kWrite && *n_runs > run_cap) return;  // too small a list: not one byte of it changes
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;

  uint32_t f = kEmpty;
  uint8_t cls = kX;
  bool head_flow = false, tail_flow = false, head = true;
  uint32_t v = 0u;
  if (t == 0u) {
    s_cin[0] = 0u;
    s_cin[1] = kEmpty;
    s_cin[2] = 0u;
  }
  if (active) {
    f = keys[p];
    head_flow = p == bnd[f];
    tail_flow = p == bnd[f + 1u] - 1u;
    cls = cls_in[p];
    v = run_word(cls, head_flow, &head);
    // the chunk's first position inside a flow continues the chunks before it (c > 0)
    if (t == 0u && !head_flow) {
      s_cin[0] = carry[c - 1u];
      s_cin[1] = carry_first[c - 1u];
      s_cin[2] = carry_last1[c - 1u];
      if (cls != kD) v += s_cin[0];
    }
  }
  bool open_fl;
  const uint32_t incl = seg_scan<SumOp>(v, head, s_v, s_h);
  const uint32_t fl = seg_scan<FlOp>(fl_word(cls, t), head, s_v, s_h, &open_fl) |
                      (open_fl ? 1u << 31 : 0u);  // bit 31: the segment began before the chunk
  s_incl[t] = incl;
  s_fl[t] = fl;
  __syncthreads();

  uint32_t ended = 0u, first = kEmpty, last1 = 0u;
  if (active) {
    uint32_t w = 0u;
    bool local = false;
    if (cls == kD) {
      if (!head_flow) {
        if (t == 0u) {
          ended = s_cin[0];
          first = s_cin[1];
          last1 = s_cin[2];
        } else {
          ended = s_incl[t - 1u];
          w = s_fl[t - 1u];
          local = true;
        }
      }
    } else if (tail_flow) {
      ended = incl;
      w = fl;
      local = true;
    }
    if (local) {
      first = fl_first(w, (uint32_t)p0);
      last1 = fl_last1(w, (uint32_t)p0);
      if (w >> 31) {
        first = MinOp::of(s_cin[1], first);
        last1 = MaxOp::of(s_cin[2], last1);
      }
    }
  }
  const uint32_t run = ended & kLenMask;
  // (a run has a U: first and last1 - 1 are positions below nv; the test keeps a wrong carry
  // from becoming a wild read)
  const bool listed = run >= min_run && first < nv && last1 - 1u < nv;
  if (!kWrite) {
    const int n = __syncthreads_count(listed);
    if (t == 0u) chunk_n[c] = (uint32_t)n;
    return;
  }
  const uint32_t rank1 = seg_scan<SumOp>(listed ? 1u : 0u, t == 0u, s_v, s_h);
  if (listed) {
    const uint64_t at = (uint64_t)chunk_base[c] + rank1 - 1u;
    if (at < run_cap) {
      LossRun r;
      r.flow_idx = f;
      r.length = run;
      r.first_send = order[first];
      r.last_send = order[last1 - 1u];
      r.flags = ((ended & kFromFlowStart) ? MGENX_RUN_HEAD : 0u) |
                (cls != kD ? MGENX_RUN_TAIL : 0u);
      r.rsv = 0u;
      r.t_first_us = stamp[first];
      r.t_last_us = stamp[last1 - 1u];
      runs[at] = r;
    }
  }
}

// (one workgroup) chunk_base[c] = the listed runs of the chunks before c; *n_runs = all of them
__global__ void __launch_bounds__(kChunk)
match_run_base_kernel(const uint32_t* __restrict__ chunk_n, uint32_t n_chunks,
                      uint32_t* __restrict__ chunk_base, uint64_t* n_runs) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_sum;
  uint32_t n = 0u;  // this lane's entry of the round
  const uint32_t all = chunk_carry<SumOp>(
      n_chunks, 0u,
      [&](uint32_t c, uint32_t& v) {
        v = n = chunk_n[c];
        return false;  // one sum over all the chunks
      },
      [&](uint32_t c, uint32_t incl) { chunk_base[c] = incl - n; }, s_v, s_h, &s_sum);
  if (threadIdx.x == 0) *n_runs = all;
}

// one lane per parsed line (mgenx_match_side; src_out may be src)
__global__ void match_side_kernel(const uint8_t* __restrict__ event,
                                  const uint8_t* __restrict__ status, const mgenx_addr* src,
                                  uint32_t n, uint32_t want_event, mgenx_addr* src_out,
                                  uint8_t* __restrict__ err_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  err_out[i] = (status[i] == MGENX_PARSE_OK && event[i] == want_event) ? 0
                                                                      : MGENX_ERROR_NOT_RECV;
  mgenx_addr a = {};
  a.port = src[i].port;
  src_out[i] = a;
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (workspace owned by the context: struct mgenx_ctx, mgenx_internal.hpp)
// ------------------------------------------------------------------------------------
using namespace mgenx;


int mgenx::match_side_run(const uint8_t* event, const uint8_t* status, const mgenx_addr* src,
                          uint32_t n, uint32_t want_event, mgenx_addr* src_out, uint8_t* err_out,
                          hipStream_t stream) {
  hipLaunchKernelGGL(match_side_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, event,
                     status, src, n, want_event, src_out, err_out);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

// ns <= 2^30 (the slot count fits 32 bits); nr, n_flows < 2^31
int mgenx::msg_match_run(DevBuf& ws, const uint32_t* s_flow, const uint32_t* s_seq,
                         const uint32_t* s_sec, const uint32_t* s_usec, const uint32_t* s_len,
                         uint32_t ns, const uint32_t* r_flow, const uint32_t* r_seq,
                         const uint32_t* r_txs, const uint32_t* r_txu, const uint32_t* r_rxs,
                         const uint32_t* r_rxu, uint32_t nr, uint32_t n_flows, uint32_t opts,
                         uint32_t* send_rx_count, uint32_t* send_first_rx, uint32_t* recv_send,
                         struct mgenx_flow_match* flows, struct mgenx_match_stats* stats,
                         const mgenx_match_timeline* tl, hipStream_t stream, char* err,
                         size_t errn) {
  // the timeline's parts; with none of them the launches and the bytes are mgenx_msg_match's
  const bool series = tl && tl->n_bins > 0, listed = tl && tl->dev_n_runs;
  const bool timeline = series || listed;
  uint32_t n_slots = 64;  // a power of two >= 2 ns
  while (n_slots < 2u * ns) n_slots <<= 1;
  const bool account = ns > 0 && n_flows > 0;
  const uint32_t n_chunks = (ns + kChunk - 1u) / kChunk;
  const size_t tab_b = a256((size_t)n_slots * 4u), own_b = a256((size_t)ns * 4u),
               sort_b = account ? a256(mgenx::flow_sort_ws(ns, n_flows)) : 0,
               rec_b = a256((size_t)ns * sizeof(MatchRec)), cls_b = a256((size_t)ns),
               c4 = a256((size_t)n_chunks * 4u);
  const size_t stamp_b = timeline ? a256((size_t)ns * 8u) : 0, tl4 = timeline ? c4 : 0;
  const size_t need = tab_b + own_b + sort_b + rec_b + cls_b + 3 * c4 + stamp_b + 5 * tl4;
  if (ws.reserve(need) != hipSuccess) {
    snprintf(err, errn, "msg_match: workspace of %zu bytes", need);
    return MGENX_EDEVICE;
  }
  Carve take(ws.p);
  uint32_t* table = (uint32_t*)take(tab_b);
  uint32_t* own = (uint32_t*)take(own_b);
  void* sort_mem = take(sort_b);
  MatchRec* rec = (MatchRec*)take(rec_b);
  uint8_t* cls = (uint8_t*)take(cls_b);
  uint32_t* trail = (uint32_t*)take(c4);
  uint32_t* has_head = (uint32_t*)take(c4);
  uint32_t* carry = (uint32_t*)take(c4);
  int64_t* stamp = (int64_t*)take(stamp_b);
  uint32_t* trail_fl = (uint32_t*)take(tl4);
  uint32_t* carry_first = (uint32_t*)take(tl4);
  uint32_t* carry_last1 = (uint32_t*)take(tl4);
  uint32_t* chunk_n = (uint32_t*)take(tl4);
  uint32_t* chunk_base = (uint32_t*)take(tl4);
  if (tl && tl->dev_send_owner && ns) own = tl->dev_send_owner;  // the owner column, in place

  const bool use_time = !(opts & MGENX_MATCH_NO_TIME);
  const uint32_t mask = n_slots - 1u;
  const MatchSide send = {s_flow, s_seq, s_sec, s_usec}, recv = {r_flow, r_seq, r_txs, r_txu};
  const uint32_t n_init = n_slots > n_flows ? n_slots : n_flows;
  hipLaunchKernelGGL(match_init_kernel, dim3((n_init + 255u) / 256u), dim3(256), 0, stream, flows,
                     n_flows, stats, table, n_slots);
  if (ns) {
    hipLaunchKernelGGL(match_build_kernel, dim3((ns + 255u) / 256u), dim3(256), 0, stream, send, ns,
                       n_flows, use_time, table, mask, send_rx_count, send_first_rx);
    hipLaunchKernelGGL(match_mark_kernel, dim3((ns + 255u) / 256u), dim3(256), 0, stream, send, ns,
                       n_flows, use_time, table, mask, own, stats);
  }
  if (nr)
    hipLaunchKernelGGL(match_probe_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, stream, send,
                       recv, nr, n_flows, use_time, table, mask, send_rx_count, send_first_rx,
                       recv_send, flows, stats);
  if (timeline) {
    const uint32_t n_cells = series ? n_flows * tl->n_bins : 0u;
    const uint32_t n_tl = n_cells > n_flows ? n_cells : n_flows ? n_flows : 1u;
    hipLaunchKernelGGL(match_tl_init_kernel, dim3((n_tl + 255u) / 256u), dim3(256), 0, stream,
                       series ? tl->dev_bins : nullptr, n_cells,
                       series ? tl->dev_outside : nullptr, n_flows,
                       listed ? tl->dev_n_runs : nullptr);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "msg_match: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  if (!account) return MGENX_OK;
  const uint32_t *keys, *order, *bnd;
  const int rc = mgenx::flow_sort_run(sort_mem, s_flow, ns, n_flows, &keys, &order, &bnd, stream,
                                     err, errn);
  if (rc != MGENX_OK) return rc;
  const PackCols col = {own, send_rx_count, send_first_rx, s_len, s_sec, s_usec, r_rxs, r_rxu};
  if (timeline)
    hipLaunchKernelGGL(match_pack_kernel<true>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                       order, bnd, n_flows, col, rec, cls, trail, has_head, stamp, trail_fl);
  else
    hipLaunchKernelGGL(match_pack_kernel<false>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                       order, bnd, n_flows, col, rec, cls, trail, has_head, (int64_t*)nullptr,
                       (uint32_t*)nullptr);
  hipLaunchKernelGGL(match_carry_kernel, dim3(1), dim3(kChunk), 0, stream, trail, has_head,
                     n_chunks, carry);
  hipLaunchKernelGGL(match_main_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, bnd,
                     n_flows, rec, cls, carry, flows);
  if (series)
    hipLaunchKernelGGL(match_series_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, bnd,
                       n_flows, rec, cls, stamp, tl->t0_us, tl->width_us, tl->n_bins, tl->dev_bins,
                       tl->dev_outside);
  if (listed) {
    const uint32_t min_run = tl->min_run ? tl->min_run : 1u;
    hipLaunchKernelGGL(match_carry_fl_kernel, dim3(1), dim3(kChunk), 0, stream, trail_fl, has_head,
                       n_chunks, carry_first, carry_last1);
    hipLaunchKernelGGL(match_runs_kernel<false>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                       order, bnd, n_flows, cls, stamp, carry, carry_first, carry_last1, min_run,
                       chunk_n, chunk_base, tl->dev_n_runs, tl->dev_runs, tl->run_cap);
    hipLaunchKernelGGL(match_run_base_kernel, dim3(1), dim3(kChunk), 0, stream, chunk_n, n_chunks,
                       chunk_base, tl->dev_n_runs);
    if (tl->run_cap)
      hipLaunchKernelGGL(match_runs_kernel<true>, dim3(n_chunks), dim3(kChunk), 0, stream, keys,
                         order, bnd, n_flows, cls, stamp, carry, carry_first, carry_last1, min_run,
                         chunk_n, chunk_base, tl->dev_n_runs, tl->dev_runs, tl->run_cap);
  }
  e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "msg_match: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}
