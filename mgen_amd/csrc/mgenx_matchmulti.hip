// mgenx_matchmulti.hip -- one sender's log joined with many receivers' logs on gfx950
// (mgenx_msg_match_multi; include/mgenx.h): the join of mgenx_match.hip with a receiver index on
// every recv record, and the delivery matrix per (flow, receiver) in the sender's order.
//
//   0. multi_init_kernel writes the empty value of every output and empties both tables;
//   1. match_build_kernel, match_mark_kernel (mgenx_match.hpp): the identity table of the send
//      records and own[i], as mgenx_msg_match runs them;
//   2. multi_probe_kernel: a lane per recv record finds the owner, writes recv_send, ORs bit rcv
//      into the owner's 64-bit mask and enters the record into a second open-addressing table
//      (a power of two >= 2 nr slots of 4 B) keyed by (owner, rcv).  The slot holds a recv index;
//      two records with an owner have the same owner iff their identities are equal, so
//      equality is compared through the recv columns and rcv, which no launch writes.  A lane
//      takes an empty slot with a compare-and-swap and atomicMin's its index into its key's
//      slot: each (owner, rcv) ends in one slot holding its first arrival.  Only atomics touch
//      the table here; the probe loop is bounded by the slot count; no lane waits on another;
//   3. multi_first_kernel: a lane per recv record reads its key's slot (plain loads: the table
//      is complete), writes recv_first and adds to its cell: delivered, delivered_bytes and the
//      latency for a first arrival, rx_dup otherwise.  The lanes of a wave that hit one cell are
//      summed before the atomics (a log is long runs of one receiver);
//   4. the send records ordered by flow, stably (mgenx::flow_sort_run), in chunks of kChunk sorted
//      positions that ignore the flow edges.  multi_count_kernel leaves per chunk the owners
//      after its last flow start; match_carry_kernel scans them over the chunks;
//      multi_main_kernel gives every owner its rank among its flow's owners (a segmented sum with
//      the carry) and reduces per wave and flow: per receiver the first and the last lane with
//      its bit set (a ballot per receiver, kept by the lane of that number) go out as one
//      64-bit atomicMin / atomicMax of rank << 32 | send index; the reach histogram is a ballot
//      per value, kept the same way, so no array is indexed at run time; the sums go out once
//      per wave and flow.  multi_series_kernel reduces the owners of one (flow, window) per wave;
//   5. multi_finish_kernel: a lane per cell turns the two packed words into lost_head,
//      lost_tail, first_send, last_send;
//   6. mgenx_msg_match_multi_ex only: multi_main_kernel also leaves every owner's rank per sorted
//      position, and mgenx_matchloss.hip's passes (multi_loss_run) follow: the loss runs per
//      (flow, receiver), their list, and the loss that pairs of receivers share.
// Integer sums, minima, maxima and ORs commute: the bytes left do not depend on the order the
// workgroups finish in.
#include <stdio.h>

#include "mgenx_match.hpp"

namespace mgenx {

typedef struct mgenx_rcv_cell RcvCell;
typedef struct mgenx_flow_fanout FlowFanout;
typedef struct mgenx_multi_bin MultiBin;
static_assert(sizeof(RcvCell) == 80, "mgenx_rcv_cell is 80 B");
static_assert(sizeof(FlowFanout) == 560, "mgenx_flow_fanout is 560 B");
static_assert(sizeof(MultiBin) == 64, "mgenx_multi_bin is 64 B");

constexpr uint32_t kOutsideKey = 1u << 31;  // a series key outside the windows: kOutsideKey | flow
constexpr uint32_t kCellRounds = 8;         // cells a wave combines before its lanes go alone

typedef unsigned long long ull;

// the (owner, rcv) table's first slot for a recv record of identity `d` at receiver r
__device__ __forceinline__ uint32_t pair_slot(const Ident& d, uint32_t r, uint32_t mask) {
  const uint64_t a = ((uint64_t)d.flow << 32) | d.seq, b = ((uint64_t)d.sec << 32) | d.usec;
  return (uint32_t)mix64(mix64(a) ^ (b * 0x9E3779B97F4A7C15ull) ^
                         ((uint64_t)(r + 1u) * 0xD6E8FEB86659FD93ull)) & mask;
}

struct MultiOut {
  uint64_t* send_mask;   // [ns]
  RcvCell* cells;        // [n_flows * n_rcv]
  FlowFanout* fanout;    // [n_flows]
  MatchStats* stats;
  MultiBin* bins;        // [n_bin_cells] or null
  uint64_t* outside;     // [n_flows] or null
  uint32_t* table;       // [n_slots]
  uint32_t* pairs;       // [n_pair_slots]
  uint64_t *minp, *maxp;  // [n_cells]: rank << 32 | send index of the first / last delivered owner
};

// every output's empty value, both tables emptied
__global__ void multi_init_kernel(MultiOut o, uint32_t ns, uint32_t n_flows, uint32_t n_cells,
                                  uint32_t n_bin_cells, uint32_t n_slots, uint32_t n_pair_slots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns) o.send_mask[i] = 0ull;
  if (i < n_slots) o.table[i] = kEmpty;
  if (i < n_pair_slots) o.pairs[i] = kEmpty;
  if (i < n_cells) {
    RcvCell c = {};
    c.first_send = c.last_send = kEmpty;
    c.lat_min = INT64_MAX;
    c.lat_max = INT64_MIN;
    o.cells[i] = c;
    o.minp[i] = UINT64_MAX;
    o.maxp[i] = 0ull;
  }
  if (i < n_flows) {
    FlowFanout f = {};
    o.fanout[i] = f;
    if (o.outside) o.outside[i] = 0ull;
  }
  if (i < n_bin_cells) {
    MultiBin b = {};
    b.reach_min = UINT64_MAX;
    o.bins[i] = b;
  }
  if (i == 0) {
    MatchStats s = {};
    *o.stats = s;
  }
}

// pass 2: a lane per recv record
__global__ void multi_probe_kernel(MatchSide send, MatchSide recv,
                                   const uint32_t* __restrict__ rcv, uint32_t nr,
                                   uint32_t n_flows, uint32_t n_rcv, bool use_time,
                                   const uint32_t* __restrict__ table, uint32_t mask,
                                   uint32_t* pairs, uint32_t pmask, uint64_t* send_mask,
                                   uint32_t* __restrict__ recv_send, RcvCell* cells,
                                   MatchStats* stats) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  bool skipped = false, orphan = false;
  uint32_t key = 0;
  if (j < nr) {
    const uint32_t f = recv.flow[j], r = rcv[j];
    uint32_t o = kEmpty;
    if (f >= n_flows || r >= n_rcv) {
      skipped = true;
    } else {
      key = f * n_rcv + r;
      const Ident me = ident_of(recv, j, use_time);
      o = table_find(table, mask, send, use_time, me);
      if (o == kEmpty) {
        orphan = true;
      } else {
        atomicOr((ull*)&send_mask[o], 1ull << r);
        uint32_t slot = pair_slot(me, r, pmask);
        // (at most nr keys in more than nr slots: an empty slot or the key's own comes up)
        for (uint32_t k = 0; k <= pmask; k++) {
          const uint32_t v = atomicCAS(&pairs[slot], kEmpty, j);
          if (v == kEmpty) break;
          if (rcv[v] == r && ident_eq(ident_of(recv, v, use_time), me)) {
            if (j < v) atomicMin(&pairs[slot], j);
            break;
          }
          slot = (slot + 1u) & pmask;
        }
      }
    }
    recv_send[j] = o;
  }
  wave_count_add(&stats->recv_skipped, skipped);
  wave_count_add(&stats->recv_unmatched, orphan);
  // the orphans of one cell among the wave's lanes: one add per cell
  ull left = __ballot(orphan);
  const uint32_t lane = threadIdx.x & 63u;
  while (left) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t lk = __shfl(key, lead);
    const ull same = __ballot(orphan && key == lk) & left;
    if (lane == lead) atomicAdd((ull*)&cells[lk].rx_orphan, (ull)__popcll(same));
    left &= ~same;
  }
}

__device__ __forceinline__ void cell_add(RcvCell* d, uint32_t n_first, uint32_t n_dup,
                                         uint64_t bytes, uint64_t lat_sum, int64_t lat_min,
                                         int64_t lat_max) {
  if (n_dup) atomicAdd((ull*)&d->rx_dup, (ull)n_dup);
  if (n_first) {
    atomicAdd((ull*)&d->delivered, (ull)n_first);
    if (bytes) atomicAdd((ull*)&d->delivered_bytes, (ull)bytes);
    if (lat_sum) atomicAdd((ull*)&d->lat_sum, (ull)lat_sum);
    atomicMin((long long*)&d->lat_min, (long long)lat_min);
    atomicMax((long long*)&d->lat_max, (long long)lat_max);
  }
}

// pass 3: a lane per recv record; the (owner, rcv) table is complete
__global__ void multi_first_kernel(MatchSide send, MatchSide recv,
                                   const uint32_t* __restrict__ rcv,
                                   const uint32_t* __restrict__ rx_sec,
                                   const uint32_t* __restrict__ rx_usec,
                                   const uint32_t* __restrict__ send_len, uint32_t nr,
                                   uint32_t n_rcv, bool use_time,
                                   const uint32_t* __restrict__ pairs, uint32_t pmask,
                                   const uint32_t* __restrict__ recv_send,
                                   uint8_t* __restrict__ recv_first, RcvCell* cells) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  bool has = false, first = false;
  uint32_t key = 0;
  uint64_t bytes = 0, lat_u = 0;
  int64_t lat_lo = INT64_MAX, lat_hi = INT64_MIN;
  if (j < nr) {
    const uint32_t o = recv_send[j];
    if (o != kEmpty) {
      has = true;
      const uint32_t r = rcv[j];
      const Ident me = ident_of(recv, j, use_time);
      key = me.flow * n_rcv + r;
      uint32_t slot = pair_slot(me, r, pmask);
      for (uint32_t k = 0; k <= pmask; k++) {
        const uint32_t v = pairs[slot];
        if (v == j) {
          first = true;
          break;
        }
        if (v == kEmpty || (rcv[v] == r && ident_eq(ident_of(recv, v, use_time), me))) break;
        slot = (slot + 1u) & pmask;
      }
      if (first) {
        // the stamps are the columns' own, whatever the identity compares
        const int64_t lat = ((int64_t)rx_sec[j] - (int64_t)send.sec[o]) * 1000000 +
                            (int64_t)rx_usec[j] - (int64_t)send.usec[o];
        bytes = send_len[o];
        lat_u = (uint64_t)lat;
        lat_lo = lat_hi = lat;
      }
    }
    recv_first[j] = first ? 1 : 0;
  }
  const uint32_t lane = threadIdx.x & 63u;
  ull left = __ballot(has);
  for (uint32_t round = 0; left && round < kCellRounds; round++) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t lk = __shfl(key, lead);
    const bool in = has && key == lk;
    const ull same = __ballot(in);
    const uint32_t n_first = (uint32_t)__popcll(__ballot(in && first));
    const uint32_t n_dup = (uint32_t)__popcll(same) - n_first;
    uint64_t b = 0, ls = 0;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    if (n_first) {  // (the same in every lane)
      b = wave_reduce<SumOp, uint64_t>(in ? bytes : 0ull);
      ls = wave_reduce<SumOp, uint64_t>(in ? lat_u : 0ull);
      lo = wave_reduce<MinOp, int64_t>(in ? lat_lo : INT64_MAX);
      hi = wave_reduce<MaxOp, int64_t>(in ? lat_hi : INT64_MIN);
    }
    if (lane == lead) cell_add(cells + lk, n_first, n_dup, b, ls, lo, hi);
    left &= ~same;
  }
  // a wave that mixes more cells than that: what is left goes lane by lane
  if (has && ((left >> lane) & 1ull))
    cell_add(cells + key, first ? 1u : 0u, first ? 0u : 1u, bytes, lat_u, lat_lo, lat_hi);
}

// pass 4a: trail[c] = the owners after chunk c's last flow start, has_head[c] = it has one
__global__ void __launch_bounds__(kChunk)
multi_count_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                   const uint32_t* __restrict__ bnd, uint32_t n_flows,
                   const uint32_t* __restrict__ own, uint32_t* __restrict__ trail,
                   uint32_t* __restrict__ has_head) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) {  // no counted record here
    if (t == 0) {
      trail[c] = 0u;
      has_head[c] = 1u;
    }
    return;
  }
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;
  bool head = true;
  uint32_t v = 0u;
  if (active) {
    const uint32_t i = order[p];
    head = p == bnd[keys[p]];
    v = own[i] == i ? 1u : 0u;
  }
  const uint32_t incl = seg_scan<SumOp>(v, head, s_v, s_h);
  const int any = __syncthreads_or(active && head);
  const uint32_t last = (uint32_t)min((uint64_t)nv - p0, (uint64_t)kChunk) - 1u;
  if (t == last) {
    trail[c] = incl;
    has_head[c] = any ? 1u : 0u;
  }
}

// pass 4c: a lane per sorted position
__global__ void __launch_bounds__(kChunk)
multi_main_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                  const uint32_t* __restrict__ bnd, uint32_t n_flows, uint32_t n_rcv,
                  const uint32_t* __restrict__ own, const uint64_t* __restrict__ send_mask,
                  const uint32_t* __restrict__ send_len, const uint32_t* __restrict__ carry,
                  uint64_t* minp, uint64_t* maxp, FlowFanout* fanout,
                  uint32_t* __restrict__ rank_out) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t nv = bnd[n_flows];
  const uint64_t p0 = (uint64_t)c * kChunk;
  if (p0 >= nv) return;  // (the whole workgroup)
  const uint32_t p = (uint32_t)p0 + t;
  const bool active = p < nv;

  uint32_t f = kEmpty, i = 0u, ln = 0u, v = 0u;
  bool owner = false, head = true;
  uint64_t m = 0ull;
  if (active) {
    f = keys[p];
    i = order[p];
    head = p == bnd[f];
    owner = own[i] == i;
    if (owner) {
      m = send_mask[i];
      ln = send_len[i];
    }
    v = owner ? 1u : 0u;
    // the chunk's first position inside a flow continues the chunks before it (c > 0)
    if (t == 0u && !head) v += carry[c - 1u];
  }
  const uint32_t incl = seg_scan<SumOp>(v, head, s_v, s_h);
  // the owner's rank among its flow's owners, and the word the cells keep
  const uint64_t pk = ((uint64_t)(incl - (owner ? 1u : 0u)) << 32) | i;
  if (rank_out && owner) rank_out[p] = incl - 1u;  // (mgenx_msg_match_multi_ex's passes read it)
  const uint32_t pc = (uint32_t)__popcll(m);

  const uint32_t lane = t & 63u;
  ull left = __ballot(active);
  while (left) {  // once per flow among the wave's lanes
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t lf = __shfl(f, lead);
    const bool in = active && f == lf;
    const bool ow = in && owner;
    const ull same = __ballot(in);
    const uint32_t sent = (uint32_t)__popcll(__ballot(ow));
    const uint32_t dup = (uint32_t)__popcll(same) - sent;
    FlowFanout* d = fanout + lf;
    if (lane == lead && dup) atomicAdd((ull*)&d->send_dup, (ull)dup);
    if (sent) {  // (the same in every lane, as every branch on a ballot below)
      const uint64_t bytes = wave_reduce<SumOp, uint64_t>(ow ? ln : 0u);
      const uint32_t deliv = wave_reduce<SumOp, uint32_t>(ow ? pc : 0u);
      const uint32_t all = (uint32_t)__popcll(__ballot(ow && pc == n_rcv));
      // reach_hist[k], k < n_rcv: lane k keeps the count (no array indexed at run time)
      uint32_t hc = 0u;
      for (uint32_t k = 0; k < n_rcv; k++) {
        const ull b = __ballot(ow && pc == k);
        if (lane == k) hc = (uint32_t)__popcll(b);
      }
      if (hc) atomicAdd((ull*)&d->reach_hist[lane], (ull)hc);
      if (lane == lead) {
        atomicAdd((ull*)&d->sent, (ull)sent);
        if (bytes) atomicAdd((ull*)&d->sent_bytes, (ull)bytes);
        if (deliv) atomicAdd((ull*)&d->deliveries, (ull)deliv);
        if (all) {
          atomicAdd((ull*)&d->reached_all, (ull)all);
          atomicAdd((ull*)&d->reach_hist[n_rcv], (ull)all);
        }
      }
      if (deliv) {
        // receiver r's delivered owners of this flow in the wave: lane r keeps the ballot.
        // Ranks and send indices rise with the lane, so the first and the last set lane hold
        // the least and the greatest word.
        ull mine = 0ull;
        for (uint32_t r = 0; r < n_rcv; r++) {
          const ull b = __ballot(ow && ((m >> r) & 1ull));
          if (lane == r) mine = b;
        }
        const int first_lane = mine ? __builtin_ctzll(mine) : 0;
        const int last_lane = mine ? 63 - __builtin_clzll(mine) : 0;
        const uint64_t pf = __shfl((ull)pk, first_lane);
        const uint64_t pl = __shfl((ull)pk, last_lane);
        if (mine) {  // (lane < n_rcv)
          atomicMin((ull*)&minp[lf * n_rcv + lane], (ull)pf);
          atomicMax((ull*)&maxp[lf * n_rcv + lane], (ull)pl);
        }
      }
    }
    left &= ~same;
  }
}

// the series: a lane per sorted position; the owners of one (flow, window) among a wave's lanes
// are reduced before the atomics
__global__ void __launch_bounds__(kChunk)
multi_series_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                    const uint32_t* __restrict__ bnd, uint32_t n_flows, uint32_t n_rcv,
                    const uint32_t* __restrict__ own, const uint64_t* __restrict__ send_mask,
                    const uint32_t* __restrict__ send_len, const uint32_t* __restrict__ t_sec,
                    const uint32_t* __restrict__ t_usec, int64_t t0, uint64_t width,
                    uint32_t n_bins, MultiBin* bins, uint64_t* outside) {
  const uint32_t nv = bnd[n_flows];
  const uint64_t p64 = (uint64_t)blockIdx.x * kChunk + threadIdx.x;
  bool owner = false;
  uint32_t key = 0u, ln = 0u, pc = 0u;
  if (p64 < nv) {
    const uint32_t p = (uint32_t)p64;
    const uint32_t f = keys[p], i = order[p];
    owner = own[i] == i;
    if (owner) {
      ln = send_len[i];
      pc = (uint32_t)__popcll(send_mask[i]);
      // t0 lies in [-2^62, 2^62] and a stamp in [0, 2^53): the difference fits; a negative
      // floor is outside whatever its value
      const int64_t d = (int64_t)t_sec[i] * 1000000 + (int64_t)t_usec[i] - t0;
      const uint64_t b = d < 0 ? (uint64_t)n_bins : (uint64_t)d / width;
      key = b < n_bins ? f * n_bins + (uint32_t)b : kOutsideKey | f;
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  ull left = __ballot(owner);
  while (left) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t lk = __shfl(key, lead);
    const bool in = owner && key == lk;
    const ull same = __ballot(in);
    const uint32_t sent = (uint32_t)__popcll(same);
    if (lk & kOutsideKey) {
      if (lane == lead) atomicAdd((ull*)&outside[lk & ~kOutsideKey], (ull)sent);
    } else {
      const uint64_t bytes = wave_reduce<SumOp, uint64_t>(in ? ln : 0u);
      const uint32_t deliv = wave_reduce<SumOp, uint32_t>(in ? pc : 0u);
      const uint64_t dbytes = wave_reduce<SumOp, uint64_t>(in ? (uint64_t)ln * pc : 0ull);
      const uint32_t any = (uint32_t)__popcll(__ballot(in && pc > 0u));
      const uint32_t all = (uint32_t)__popcll(__ballot(in && pc == n_rcv));
      const uint32_t lo = wave_reduce<MinOp, uint32_t>(in ? pc : 0xFFFFFFFFu);
      const uint32_t hi = wave_reduce<MaxOp, uint32_t>(in ? pc : 0u);
      if (lane == lead) {
        MultiBin* d = bins + lk;
        atomicAdd((ull*)&d->sent, (ull)sent);
        if (bytes) atomicAdd((ull*)&d->sent_bytes, (ull)bytes);
        if (deliv) atomicAdd((ull*)&d->deliveries, (ull)deliv);
        if (dbytes) atomicAdd((ull*)&d->delivered_bytes, (ull)dbytes);
        if (any) atomicAdd((ull*)&d->reached_any, (ull)any);
        if (all) atomicAdd((ull*)&d->reached_all, (ull)all);
        atomicMin((ull*)&d->reach_min, (ull)lo);
        if (hi) atomicMax((ull*)&d->reach_max, (ull)hi);
      }
    }
    left &= ~same;
  }
}

// pass 5: a lane per cell (the fanout and the packed words are complete)
__global__ void multi_finish_kernel(const uint64_t* __restrict__ minp,
                                    const uint64_t* __restrict__ maxp,
                                    const FlowFanout* __restrict__ fanout, uint32_t n_cells,
                                    uint32_t n_rcv, RcvCell* cells) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const uint64_t sent = fanout[c / n_rcv].sent;
  const uint64_t lo = minp[c], hi = maxp[c];
  RcvCell* d = cells + c;
  if (lo == UINT64_MAX) {  // no owner delivered here
    d->lost_head = sent;
  } else {
    d->lost_head = lo >> 32;
    d->lost_tail = sent - 1u - (hi >> 32);
    d->first_send = (uint32_t)lo;
    d->last_send = (uint32_t)hi;
  }
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side (the workspace is the context's, shared with mgenx_msg_match)
// ------------------------------------------------------------------------------------
using namespace mgenx;

// ns, nr <= 2^30 (both slot counts fit 32 bits); 1 <= n_rcv <= 64; n_flows * n_rcv and
// n_flows * n_bins < 2^31
int mgenx::msg_match_multi_run(DevBuf& ws, const uint32_t* s_flow, const uint32_t* s_seq,
                               const uint32_t* s_sec, const uint32_t* s_usec,
                               const uint32_t* s_len, uint32_t ns, const uint32_t* r_flow,
                               const uint32_t* r_seq, const uint32_t* r_txs,
                               const uint32_t* r_txu, const uint32_t* r_rxs,
                               const uint32_t* r_rxu, const uint32_t* r_rcv, uint32_t nr,
                               uint32_t n_rcv, uint32_t n_flows, uint32_t opts,
                               uint64_t* send_mask, uint32_t* recv_send, uint8_t* recv_first,
                               struct mgenx_rcv_cell* cells, struct mgenx_flow_fanout* fanout,
                               struct mgenx_match_stats* stats, const mgenx_multi_timeline* tl,
                               const mgenx_multi_loss* lx, hipStream_t stream, char* err,
                               size_t errn) {
  const bool series = tl && tl->n_bins > 0 && n_flows > 0;
  // mgenx_msg_match_multi_ex's parts; with none of them the launches and the bytes are
  // mgenx_msg_match_multi's
  const bool loss = lx && (lx->dev_rcv_runs || lx->dev_n_runs || lx->dev_pairs);
  uint32_t n_slots = 64, n_pairs = 64;  // powers of two >= 2 ns, 2 nr
  while (n_slots < 2u * ns) n_slots <<= 1;
  while (n_pairs < 2u * nr) n_pairs <<= 1;
  const bool account = ns > 0 && n_flows > 0;
  const uint32_t n_chunks = (ns + kChunk - 1u) / kChunk;
  const uint32_t n_cells = n_flows * n_rcv, n_bin_cells = series ? n_flows * tl->n_bins : 0u;
  const size_t tab_b = a256((size_t)n_slots * 4u), pair_b = a256((size_t)n_pairs * 4u),
               own_b = a256((size_t)ns * 4u),
               sort_b = account ? a256(mgenx::flow_sort_ws(ns, n_flows)) : 0,
               cell_b = a256((size_t)n_cells * 8u), c4 = a256((size_t)n_chunks * 4u);
  const size_t loss_b = loss ? a256(mgenx::multi_loss_ws(ns, n_flows, n_rcv)) : 0;
  const size_t need = tab_b + pair_b + own_b + sort_b + 2 * cell_b + 3 * c4 + loss_b;
  if (ws.reserve(need) != hipSuccess) {
    snprintf(err, errn, "msg_match_multi: workspace of %zu bytes", need);
    return MGENX_EDEVICE;
  }
  Carve take(ws.p);
  uint32_t* table = (uint32_t*)take(tab_b);
  uint32_t* pairs = (uint32_t*)take(pair_b);
  uint32_t* own = (uint32_t*)take(own_b);
  void* sort_mem = take(sort_b);
  uint64_t* minp = (uint64_t*)take(cell_b);
  uint64_t* maxp = (uint64_t*)take(cell_b);
  uint32_t* trail = (uint32_t*)take(c4);
  uint32_t* has_head = (uint32_t*)take(c4);
  uint32_t* carry = (uint32_t*)take(c4);
  void* loss_mem = take(loss_b);

  const bool use_time = !(opts & MGENX_MATCH_NO_TIME);
  const uint32_t mask = n_slots - 1u, pmask = n_pairs - 1u;
  const MatchSide send = {s_flow, s_seq, s_sec, s_usec}, recv = {r_flow, r_seq, r_txs, r_txu};
  const MultiOut out = {send_mask, cells, fanout, stats, series ? tl->dev_bins : nullptr,
                        series ? tl->dev_outside : nullptr, table, pairs, minp, maxp};
  uint32_t n_init = n_slots > n_pairs ? n_slots : n_pairs;
  if (n_cells > n_init) n_init = n_cells;
  if (n_bin_cells > n_init) n_init = n_bin_cells;  // (ns < n_slots, n_flows <= n_cells)
  hipLaunchKernelGGL(multi_init_kernel, dim3((n_init + 255u) / 256u), dim3(256), 0, stream, out, ns,
                     n_flows, n_cells, n_bin_cells, n_slots, n_pairs);
  if (ns) {
    hipLaunchKernelGGL(match_build_kernel, dim3((ns + 255u) / 256u), dim3(256), 0, stream, send, ns,
                       n_flows, use_time, table, mask, (uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(match_mark_kernel, dim3((ns + 255u) / 256u), dim3(256), 0, stream, send, ns,
                       n_flows, use_time, table, mask, own, stats);
  }
  if (nr) {
    hipLaunchKernelGGL(multi_probe_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, stream, send,
                       recv, r_rcv, nr, n_flows, n_rcv, use_time, table, mask, pairs, pmask,
                       send_mask, recv_send, cells, stats);
    hipLaunchKernelGGL(multi_first_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, stream, send,
                       recv, r_rcv, r_rxs, r_rxu, s_len, nr, n_rcv, use_time, pairs, pmask,
                       recv_send, recv_first, cells);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "msg_match_multi: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  mgenx::MultiLossIn lin = {};
  lin.own = own;
  lin.send_mask = send_mask;
  lin.minp = minp;
  lin.maxp = maxp;
  lin.fanout = fanout;
  lin.t_sec = s_sec;
  lin.t_usec = s_usec;
  lin.ns = ns;
  lin.n_flows = n_flows;
  lin.n_rcv = n_rcv;
  if (!account)  // (no owner: the empty values are the result)
    return loss ? mgenx::multi_loss_run(loss_mem, lin, lx, false, stream, err, errn) : MGENX_OK;
  const uint32_t *keys, *order, *bnd;
  const int rc = mgenx::flow_sort_run(sort_mem, s_flow, ns, n_flows, &keys, &order, &bnd, stream,
                                     err, errn);
  if (rc != MGENX_OK) return rc;
  hipLaunchKernelGGL(multi_count_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, order, bnd,
                     n_flows, own, trail, has_head);
  hipLaunchKernelGGL(match_carry_kernel, dim3(1), dim3(kChunk), 0, stream, trail, has_head,
                     n_chunks, carry);
  hipLaunchKernelGGL(multi_main_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, order, bnd,
                     n_flows, n_rcv, own, send_mask, s_len, carry, minp, maxp, fanout,
                     loss ? mgenx::multi_loss_rank(loss_mem) : (uint32_t*)nullptr);
  if (series)
    hipLaunchKernelGGL(multi_series_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, keys, order,
                       bnd, n_flows, n_rcv, own, send_mask, s_len, s_sec, s_usec, tl->t0_us,
                       tl->width_us, tl->n_bins, tl->dev_bins, tl->dev_outside);
  hipLaunchKernelGGL(multi_finish_kernel, dim3((n_cells + 255u) / 256u), dim3(256), 0, stream, minp,
                     maxp, fanout, n_cells, n_rcv, cells);
  e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "msg_match_multi: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  if (loss) {
    lin.keys = keys;
    lin.order = order;
    lin.bnd = bnd;
    return mgenx::multi_loss_run(loss_mem, lin, lx, true, stream, err, errn);
  }
  return MGENX_OK;
}
