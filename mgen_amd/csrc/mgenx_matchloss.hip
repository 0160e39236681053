// mgenx_matchloss.hip -- what mgenx_msg_match_multi_ex adds to the join of mgenx_matchmulti.hip on
// gfx950 (include/mgenx.h): per (flow, receiver) the loss runs with their list, and per flow and
// pair of receivers the loss they share.  It runs after multi_main_kernel, on what the join holds
// by then: send_mask, every owner's rank in its flow (multi_main_kernel leaves it per sorted
// position when asked), the flows' sent and every cell's packed first and last delivered owner.
//
//   0. loss_init_kernel writes the empty value of every output asked for;
//   1. loss_obase_kernel (one workgroup): obase[f] = the owners of the flows before f, a sum over
//      mgenx_flow_fanout.sent; obase[n_flows] = all owners.  loss_compact_kernel, a lane per sorted
//      position: the owner of rank k in flow f goes to q = obase[f] + k with its flow, its send
//      index and its mask.  In q the owners stand in (flow, send-log) order with nothing between
//      them: send duplicates and skipped records are gone, a run of ranks is a run of q, its
//      length a difference, and a neighbour is q + 1;
//   2. a tile is 64 consecutive q, one wave: 64 owners by 64 receivers is a 64 x 64 bit matrix,
//      transposed with one ballot per receiver, lane r keeping ballot r: its delivery word.  The
//      flow heads and tails of the tile are one more ballot word each;
//   3. the runs (loss_runs_kernel, 16 tiles per workgroup).  A run starts after the last breaker
//      below it: a delivered owner or a flow head.  `start`, the q at which the run open after a
//      position began, only grows with q, so its carry is a running maximum with 0 for "no
//      breaker here": per tile from clz of the lane's word and of the head word, over a
//      workgroup's tiles through LDS, over the chunks by loss_carry_kernel (a workgroup per
//      receiver walks the per-(chunk, receiver) summary that loss_runs_kernel<0> left).  A run is
//      known at its last undelivered owner: the next owner is delivered (bit j + 1, or bit 0 of
//      the next tile, read from its mask) or the flow ends.  loss_runs_kernel<1> walks the ends
//      of the lane's word (ctz; the bound is their popcount), adds the statistics of the runs of
//      one flow with one atomic per field that is not its identity, and counts the listed ends
//      per chunk; loss_base_kernel scans the counts; loss_runs_kernel<2> transposes the listed
//      ends back (lane j: the receivers whose run ends at owner j), scans their popcounts over
//      the workgroup and writes each run at its place: by flow, last_send, receiver;
//   4. the pairs (loss_pairs_kernel, one wave per kPairTiles tiles).  Per flow segment of a tile
//      lane b holds receiver b's span as a bit mask; for a < n_rcv, a's word and span are
//      wave-uniform and lane b adds popcounts over the common span to its own column of two
//      LDS arrays [a][b] (two 16-bit counts a word: a wave sees at most 64 kPairTiles owners).
//      Lane b alone touches column b, so there is no barrier and no bank conflict.  The columns
//      go out with atomics at a flow edge and at the end of the wave's range.
// Every loop's bound is known before it starts, no lane waits on another, no shift is by 64.
// Integer sums and maxima commute: the bytes left do not depend on the order the workgroups
// finish in.
#include <stdio.h>

#include <limits.h>

#include "mgenx_blockscan.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

typedef struct mgenx_rcv_runs RcvRuns;
typedef struct mgenx_rcv_loss_run RcvLossRun;
typedef struct mgenx_rcv_pair RcvPair;
static_assert(sizeof(RcvRuns) == 160, "mgenx_rcv_runs is 160 B");
static_assert(sizeof(RcvLossRun) == 40, "mgenx_rcv_loss_run is 40 B");
static_assert(sizeof(RcvPair) == 32, "mgenx_rcv_pair is 32 B");

constexpr uint32_t kPairTiles = 64;  // tiles a wave of loss_pairs_kernel walks
static_assert(kPairTiles * 64u < 65536u, "a wave's pair counts fit 16 bits");

constexpr uint32_t kNoFlow = 0xFFFFFFFFu;  // no flow yet (no flow index is that high)

typedef unsigned long long ull;

__device__ __forceinline__ uint32_t msb64(ull x) { return 63u - (uint32_t)__builtin_clzll(x); }

__global__ void loss_init_kernel(uint64_t* runs_w, uint64_t n_runs_w, uint64_t* pairs_w,
                                 uint64_t n_pairs_w, uint64_t* n_runs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_runs_w) runs_w[i] = 0ull;
  if (i < n_pairs_w) pairs_w[i] = 0ull;
  if (i == 0 && n_runs) *n_runs = 0ull;
}

// (one workgroup) obase[f] = the owners of the flows before f; obase[n_flows] = all of them
__global__ void __launch_bounds__(kChunk)
loss_obase_kernel(const struct mgenx_flow_fanout* __restrict__ fanout, uint32_t n_flows,
                  uint32_t* __restrict__ obase) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) obase[0] = 0u;
  chunk_carry<SumOp>(
      n_flows, 0u,
      [&](uint32_t f, uint32_t& v) {
        v = (uint32_t)fanout[f].sent;
        return false;  // one sum over all the flows
      },
      [&](uint32_t f, uint32_t incl) { obase[f + 1u] = incl; }, s_v, s_h, &s_sum);
}

// a lane per sorted position: the owners, compacted
__global__ void __launch_bounds__(kChunk)
loss_compact_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                    const uint32_t* __restrict__ bnd, uint32_t n_flows, uint32_t ns,
                    const uint32_t* __restrict__ own, const uint32_t* __restrict__ rank,
                    const uint64_t* __restrict__ send_mask, const uint32_t* __restrict__ obase,
                    uint32_t* __restrict__ c_flow, uint32_t* __restrict__ c_send,
                    uint64_t* __restrict__ c_mask) {
  const uint64_t p64 = (uint64_t)blockIdx.x * kChunk + threadIdx.x;
  if (p64 >= bnd[n_flows]) return;
  const uint32_t p = (uint32_t)p64, i = order[p];
  if (own[i] != i) return;
  const uint32_t f = keys[p];
  const uint32_t q = obase[f] + rank[p];
  if (q >= ns) return;  // (never: the owners are at most ns; it keeps a wrong rank in bounds)
  c_flow[q] = f;
  c_send[q] = i;
  c_mask[q] = send_mask[i];
}

// 64 consecutive owners from q0, transposed
struct Tile {
  ull w;             // lane r < n_rcv: bit j = owner q0 + j was delivered to r; other lanes 0
  ull heads, tails;  // bit j: owner q0 + j is its flow's first / last
  ull valid;         // bit j: q0 + j is an owner
  uint32_t f;        // the flow of owner q0 + lane (kNoFlow: none)
};
__device__ __forceinline__ Tile load_tile(uint32_t q0, uint32_t n_own, uint32_t n_flows,
                                          uint32_t n_rcv,
                                          const uint32_t* __restrict__ c_flow,
                                          const uint64_t* __restrict__ c_mask,
                                          const uint32_t* __restrict__ obase) {
  const uint32_t lane = threadIdx.x & 63u, q = q0 + lane;
  bool valid = q < n_own;
  Tile t;
  t.f = kNoFlow;
  ull m = 0ull;
  bool head = false, tail = false;
  if (valid) t.f = c_flow[q];
  // (never: every q below n_own was written with its flow; it keeps a wrong one from indexing)
  if (t.f >= n_flows) {
    valid = false;
    t.f = kNoFlow;
  }
  if (valid) {
    m = c_mask[q];
    head = q == obase[t.f];
    tail = q + 1u == obase[t.f + 1u];
  }
  t.w = 0ull;
  for (uint32_t r = 0; r < n_rcv; r++) {
    const ull b = __ballot((m >> r) & 1ull);
    if (lane == r) t.w = b;
  }
  t.heads = __ballot(head);
  t.tails = __ballot(tail);
  t.valid = __ballot(valid);
  return t;
}

// the run statistics of one lane (one receiver) over the runs of one flow
struct RunAcc {
  uint32_t f, n;
  uint64_t mx, h0, h1;  // loss_run_hist[k] in bits 7 (k % 9) .. of h0 (k < 9) or h1: at most 32 each
};
__device__ __forceinline__ void run_acc_flush(RunAcc& a, RcvRuns* out, uint32_t n_rcv,
                                              uint32_t r) {
  if (a.n) {
    RcvRuns* d = out + (size_t)a.f * n_rcv + r;
    atomicAdd((ull*)&d->loss_runs, (ull)a.n);
    atomicMax((ull*)&d->loss_run_max, (ull)a.mx);
#pragma unroll
    for (uint32_t k = 0; k < 18u; k++) {
      const uint64_t n = ((k < 9u ? a.h0 : a.h1) >> (7u * (k % 9u))) & 0x7Full;
      if (n) atomicAdd((ull*)&d->loss_run_hist[k], (ull)n);
    }
  }
  a.n = 0u;
  a.mx = a.h0 = a.h1 = 0ull;
}

struct RunsArgs {
  const uint32_t *c_flow, *c_send, *obase;
  const uint64_t* c_mask;
  const uint32_t *t_sec, *t_usec;
  uint32_t ns, n_flows, n_rcv, n_chunks, min_run;
  uint32_t* summary;        // [n_rcv * n_chunks]: the start of the run open after chunk c, 0: none
  const uint32_t* carry;    // [n_rcv * n_chunks]: the same over the chunks up to c
  uint32_t* chunk_n;        // [n_chunks]: the listed runs that end in chunk c (null: no list)
  const uint64_t* chunk_base;
  RcvRuns* stats;           // null: not wanted
  const uint64_t* n_runs;
  RcvLossRun* runs;
  uint64_t run_cap;
};

// kMode 0: the chunk's summary.  1: the statistics and the listed runs per chunk.  2: the list.
template <int kMode>
__global__ void __launch_bounds__(kChunk) loss_runs_kernel(RunsArgs a) {
  __shared__ uint32_t s_loc[kWaves][64];
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint64_t s_recv[kMode == 2 ? kChunk : 1], s_off[kMode == 2 ? kChunk : 1];

  const uint32_t c = blockIdx.x, t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t n_own = a.obase[a.n_flows];
  const uint64_t qc = (uint64_t)c * kChunk;
  if (qc >= n_own) {  // (the whole workgroup) no owner here
    if (kMode == 0 && t < a.n_rcv) a.summary[(size_t)t * a.n_chunks + c] = 0u;
    if (kMode == 1 && t == 0 && a.chunk_n) a.chunk_n[c] = 0u;
    return;
  }
  if (kMode == 2 && *a.n_runs > a.run_cap) return;  // too small a list: not one byte changes
  const uint32_t q0 = (uint32_t)qc + wv * 64u;
  const Tile tl = load_tile(q0, n_own, a.n_flows, a.n_rcv, a.c_flow, a.c_mask, a.obase);
  const bool rcv_lane = lane < a.n_rcv;

  // where the run open after this tile began: after its last delivered owner or at its last flow
  // head; 0 when the tile has neither (owner 0 is a flow head: 0 means the same either way)
  uint32_t loc = 0u;
  if (rcv_lane) {
    if (tl.w) loc = q0 + msb64(tl.w) + 1u;
    if (tl.heads) loc = max(loc, q0 + msb64(tl.heads));
  }
  s_loc[wv][lane] = loc;
  __syncthreads();
  if (kMode == 0) {
    if (t < a.n_rcv) {
      uint32_t m = 0u;
      for (uint32_t k = 0; k < kWaves; k++) m = max(m, s_loc[k][t]);
      a.summary[(size_t)t * a.n_chunks + c] = m;
    }
    return;
  }

  // the ends of lane r's runs in this tile, and where each began
  uint32_t cin = 0u;
  ull ends = 0ull;
  if (rcv_lane) {
    if (c > 0u) cin = a.carry[(size_t)lane * a.n_chunks + c - 1u];
    for (uint32_t k = 0; k < wv; k++) cin = max(cin, s_loc[k][lane]);
    // the owner after the tile: a tile that ends inside a flow has one
    const uint32_t qn = q0 + 64u;
    const ull next = qn < n_own ? (a.c_mask[qn] >> lane) & 1ull : 0ull;
    ends = ~tl.w & tl.valid & (tl.tails | (tl.w >> 1) | (next << 63));
  }
  auto start_of = [&](uint32_t j) -> uint32_t {
    const ull below = (2ull << j) - 1ull;  // bits 0 .. j (j = 63: all)
    const ull d = tl.w & below, h = tl.heads & below;
    int s = -1;
    if (d) s = (int)msb64(d) + 1;
    if (h) s = max(s, (int)msb64(h));
    return s >= 0 ? q0 + (uint32_t)s : cin;
  };

  ull listed = 0ull;
  RunAcc acc = {kNoFlow, 0u, 0ull, 0ull, 0ull};
  {
    ull left = ends;
    for (uint32_t n = (uint32_t)__popcll(ends); n > 0u; n--) {
      const uint32_t j = (uint32_t)__builtin_ctzll(left);
      left &= left - 1ull;
      const uint32_t qe = q0 + j, st = start_of(j);
      if (st > qe) continue;  // (never: it keeps a wrong carry from becoming a wild length)
      const uint32_t len = qe - st + 1u;
      if (len >= a.min_run) listed |= 1ull << j;
      if (kMode == 1 && a.stats) {
        const uint32_t f = a.c_flow[qe];
        if (f != acc.f) {
          run_acc_flush(acc, a.stats, a.n_rcv, lane);
          acc.f = f;
        }
        const uint32_t k = min(31u - (uint32_t)__builtin_clz(len), 17u);
        acc.n++;
        acc.mx = max(acc.mx, (uint64_t)len);
        if (k < 9u)
          acc.h0 += 1ull << (7u * k);
        else
          acc.h1 += 1ull << (7u * (k - 9u));
      }
    }
    if (kMode == 1 && a.stats) run_acc_flush(acc, a.stats, a.n_rcv, lane);
  }
  if (kMode == 1) {
    if (!a.chunk_n) return;
    const uint32_t incl = seg_scan<SumOp>((uint32_t)__popcll(listed), t == 0u, s_v, s_h);
    if (t == kChunk - 1u) a.chunk_n[c] = incl;
    return;
  }

  if (kMode == 2) {
    // back to a lane per owner: the receivers whose listed run ends at owner q0 + lane
    ull rcvs = 0ull;
    for (uint32_t j = 0; j < 64u; j++) {
      const ull b = __ballot((listed >> j) & 1ull);
      if (lane == j) rcvs = b;
    }
    const uint32_t cnt = (uint32_t)__popcll(rcvs);
    const uint32_t incl = seg_scan<SumOp>(cnt, t == 0u, s_v, s_h);
    s_recv[t] = rcvs;
    s_off[t] = a.chunk_base[c] + incl - cnt;
    __syncthreads();
    ull left = listed;
    for (uint32_t n = (uint32_t)__popcll(listed); n > 0u; n--) {
      const uint32_t j = (uint32_t)__builtin_ctzll(left);
      left &= left - 1ull;
      const uint32_t qe = q0 + j, st = start_of(j);
      const uint64_t at =
          s_off[wv * 64u + j] + (uint32_t)__popcll(s_recv[wv * 64u + j] & ((1ull << lane) - 1ull));
      if (at >= a.run_cap) continue;
      const uint32_t f = a.c_flow[qe], i0 = a.c_send[st], i1 = a.c_send[qe];
      if (i0 >= a.ns || i1 >= a.ns) continue;  // (never: the compacted send indices are below ns)
      RcvLossRun r;
      r.flow_idx = f;
      r.length = qe - st + 1u;
      r.first_send = i0;
      r.last_send = i1;
      r.flags = (st == a.obase[f] ? MGENX_RUN_HEAD : 0u) |
                (qe + 1u == a.obase[f + 1u] ? MGENX_RUN_TAIL : 0u);
      r.rcv = lane;
      r.t_first_us = (int64_t)a.t_sec[i0] * 1000000 + (int64_t)a.t_usec[i0];
      r.t_last_us = (int64_t)a.t_sec[i1] * 1000000 + (int64_t)a.t_usec[i1];
      a.runs[at] = r;
    }
  }
}

// (a workgroup per receiver) carry[r][c] = the greatest summary of receiver r over the chunks up
// to c: where the run open after chunk c began
__global__ void __launch_bounds__(kChunk)
loss_carry_kernel(const uint32_t* __restrict__ summary, uint32_t n_chunks,
                  uint32_t* __restrict__ carry) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_run;
  const size_t row = (size_t)blockIdx.x * n_chunks;
  chunk_carry<MaxOp>(
      n_chunks, 0u,
      [&](uint32_t c, uint32_t& v) {
        v = summary[row + c];
        return false;  // one running maximum over all the chunks
      },
      [&](uint32_t c, uint32_t v) { carry[row + c] = v; }, s_v, s_h, &s_run);
}

// (one workgroup) chunk_base[c] = the listed runs of the chunks before c; *n_runs = all of them
__global__ void __launch_bounds__(kChunk)
loss_base_kernel(const uint32_t* __restrict__ chunk_n, uint32_t n_chunks,
                 uint64_t* __restrict__ chunk_base, uint64_t* n_runs) {
  __shared__ uint64_t s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  __shared__ uint64_t s_sum;
  uint64_t n = 0ull;  // this lane's entry of the round
  const uint64_t all = chunk_carry<SumOp>(
      n_chunks, (uint64_t)0,
      [&](uint32_t c, uint64_t& v) {
        v = n = chunk_n[c];
        return false;
      },
      [&](uint32_t c, uint64_t incl) { chunk_base[c] = incl - n; }, s_v, s_h, &s_sum);
  if (threadIdx.x == 0) *n_runs = all;
}

// the pair matrix: one wave walks kPairTiles tiles
__global__ void __launch_bounds__(64)
loss_pairs_kernel(const uint32_t* __restrict__ c_flow, const uint64_t* __restrict__ c_mask,
                  const uint32_t* __restrict__ obase, const uint64_t* __restrict__ minp,
                  const uint64_t* __restrict__ maxp, uint32_t n_flows, uint32_t n_rcv,
                  RcvPair* pairs) {
  // [a][b], column b lane b's own: span | lost_both << 16 and lost_a | lost_b << 16
  __shared__ uint32_t s_x[64][64], s_y[64][64];
  const uint32_t lane = threadIdx.x;
  const uint32_t n_own = obase[n_flows];
  const uint64_t qb = (uint64_t)blockIdx.x * (kPairTiles * 64u);
  if (qb >= n_own) return;
  for (uint32_t k = 0; k < n_rcv; k++) s_x[k][lane] = s_y[k][lane] = 0u;

  auto flush = [&](uint32_t f) {
    if (lane >= n_rcv) return;
    for (uint32_t k = 0; k < n_rcv; k++) {
      const uint32_t x = s_x[k][lane], y = s_y[k][lane];
      if ((x | y) == 0u) continue;
      RcvPair* d = pairs + ((size_t)f * n_rcv + k) * n_rcv + lane;
      if (x & 0xFFFFu) atomicAdd((ull*)&d->span, (ull)(x & 0xFFFFu));
      if (x >> 16) atomicAdd((ull*)&d->lost_both, (ull)(x >> 16));
      if (y & 0xFFFFu) atomicAdd((ull*)&d->lost_a, (ull)(y & 0xFFFFu));
      if (y >> 16) atomicAdd((ull*)&d->lost_b, (ull)(y >> 16));
      s_x[k][lane] = s_y[k][lane] = 0u;
    }
  };

  const uint64_t rest = (uint64_t)n_own - qb;
  const uint32_t n_tiles = rest >= kPairTiles * 64u ? kPairTiles : (uint32_t)((rest + 63u) / 64u);
  uint32_t cur = kNoFlow;  // the flow the columns hold (the same in every lane)
  for (uint32_t ti = 0; ti < n_tiles; ti++) {
    const uint32_t q0 = (uint32_t)qb + ti * 64u;
    const Tile tl = load_tile(q0, n_own, n_flows, n_rcv, c_flow, c_mask, obase);
    // the flow segments of the tile: one from bit 0 and one from every other flow head
    ull left = tl.valid;
    for (uint32_t n = (uint32_t)__popcll(tl.heads | 1ull); n > 0u && left; n--) {
      const uint32_t lead = (uint32_t)__builtin_ctzll(left);
      const ull nh = tl.heads & left & (left - 1ull);  // the heads above the segment's first bit
      const ull seg = nh ? left & ((1ull << __builtin_ctzll(nh)) - 1ull) : left;
      left &= ~seg;
      const uint32_t f = __shfl(tl.f, lead);
      if (f != cur) {
        if (cur != kNoFlow) flush(cur);
        cur = f;
      }
      // receiver `lane`'s span inside the segment
      ull sp = 0ull;
      if (lane < n_rcv) {
        const uint64_t lo = minp[(size_t)f * n_rcv + lane], hi = maxp[(size_t)f * n_rcv + lane];
        if (lo != UINT64_MAX) {
          const uint64_t base = obase[f];
          const uint64_t qlo = base + (lo >> 32), qhi = base + (hi >> 32);
          if (qhi >= q0 && qlo <= (uint64_t)q0 + 63u) {
            const uint32_t jl = qlo > q0 ? (uint32_t)(qlo - q0) : 0u;
            const uint32_t jh = qhi < (uint64_t)q0 + 63u ? (uint32_t)(qhi - q0) : 63u;
            sp = seg & (~0ull << jl) & (~0ull >> (63u - jh));
          }
        }
      }
      for (uint32_t k = 0; k < n_rcv; k++) {
        const ull wa = __shfl(tl.w, k), sa = __shfl(sp, k);
        const ull cm = sa & sp;
        if (cm) {
          s_x[k][lane] += (uint32_t)__popcll(cm) | ((uint32_t)__popcll(cm & ~wa & ~tl.w) << 16);
          s_y[k][lane] += (uint32_t)__popcll(cm & ~wa) | ((uint32_t)__popcll(cm & ~tl.w) << 16);
        }
      }
    }
  }
  if (cur != kNoFlow) flush(cur);
}

}  // namespace mgenx

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
using namespace mgenx;

namespace {
struct LossWs {
  size_t rank_b, flow_b, send_b, mask_b, obase_b, sum_b, n_b, base_b;
  LossWs(uint32_t ns, uint32_t n_flows, uint32_t n_rcv) {
    const size_t n_chunks = (ns + kChunk - 1u) / kChunk;
    rank_b = flow_b = send_b = a256((size_t)ns * 4u);
    mask_b = a256((size_t)ns * 8u);
    obase_b = a256(((size_t)n_flows + 1u) * 4u);
    sum_b = a256(n_chunks * n_rcv * 4u);
    n_b = a256(n_chunks * 4u);
    base_b = a256(n_chunks * 8u);
  }
  size_t total() const {
    return rank_b + flow_b + send_b + mask_b + obase_b + 2 * sum_b + n_b + base_b;
  }
};
}  // namespace

size_t mgenx::multi_loss_ws(uint32_t ns, uint32_t n_flows, uint32_t n_rcv) {
  return LossWs(ns, n_flows, n_rcv).total();
}

// (the first piece of the workspace: multi_main_kernel writes it)
uint32_t* mgenx::multi_loss_rank(void* mem) { return (uint32_t*)mem; }

int mgenx::multi_loss_run(void* mem, const MultiLossIn& in, const mgenx_multi_loss* lx,
                          bool account, hipStream_t stream, char* err, size_t errn) {
  const uint32_t ns = in.ns, n_flows = in.n_flows, n_rcv = in.n_rcv;
  const bool listed = lx->dev_n_runs != nullptr;
  const uint64_t n_cells = (uint64_t)n_flows * n_rcv;
  const uint64_t runs_w = lx->dev_rcv_runs ? n_cells * (sizeof(RcvRuns) / 8u) : 0ull;
  const uint64_t pairs_w = lx->dev_pairs ? n_cells * n_rcv * (sizeof(RcvPair) / 8u) : 0ull;
  const uint64_t n_init = runs_w > pairs_w ? runs_w : pairs_w;
  hipLaunchKernelGGL(loss_init_kernel, dim3((uint32_t)((n_init + 255u) / 256u + 1u)), dim3(256), 0,
                     stream, (uint64_t*)lx->dev_rcv_runs, runs_w, (uint64_t*)lx->dev_pairs, pairs_w,
                     lx->dev_n_runs);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && account) {
    const LossWs sz(ns, n_flows, n_rcv);
    Carve take(mem);
    uint32_t* rank = (uint32_t*)take(sz.rank_b);
    uint32_t* c_flow = (uint32_t*)take(sz.flow_b);
    uint32_t* c_send = (uint32_t*)take(sz.send_b);
    uint64_t* c_mask = (uint64_t*)take(sz.mask_b);
    uint32_t* obase = (uint32_t*)take(sz.obase_b);
    uint32_t* summary = (uint32_t*)take(sz.sum_b);
    uint32_t* carry = (uint32_t*)take(sz.sum_b);
    uint32_t* chunk_n = (uint32_t*)take(sz.n_b);
    uint64_t* chunk_base = (uint64_t*)take(sz.base_b);
    const uint32_t n_chunks = (ns + kChunk - 1u) / kChunk;

    hipLaunchKernelGGL(loss_obase_kernel, dim3(1), dim3(kChunk), 0, stream, in.fanout, n_flows,
                       obase);
    hipLaunchKernelGGL(loss_compact_kernel, dim3(n_chunks), dim3(kChunk), 0, stream, in.keys,
                       in.order, in.bnd, n_flows, ns, in.own, rank, in.send_mask, obase, c_flow,
                       c_send, c_mask);
    if (lx->dev_rcv_runs || listed) {
      RunsArgs a = {};
      a.c_flow = c_flow;
      a.c_send = c_send;
      a.obase = obase;
      a.c_mask = c_mask;
      a.t_sec = in.t_sec;
      a.t_usec = in.t_usec;
      a.ns = ns;
      a.n_flows = n_flows;
      a.n_rcv = n_rcv;
      a.n_chunks = n_chunks;
      a.min_run = lx->min_run ? lx->min_run : 1u;
      a.summary = summary;
      a.carry = carry;
      a.chunk_n = listed ? chunk_n : nullptr;
      a.chunk_base = chunk_base;
      a.stats = lx->dev_rcv_runs;
      a.n_runs = lx->dev_n_runs;
      a.runs = lx->dev_runs;
      a.run_cap = lx->run_cap;
      hipLaunchKernelGGL(loss_runs_kernel<0>, dim3(n_chunks), dim3(kChunk), 0, stream, a);
      hipLaunchKernelGGL(loss_carry_kernel, dim3(n_rcv), dim3(kChunk), 0, stream, summary,
                         n_chunks, carry);
      hipLaunchKernelGGL(loss_runs_kernel<1>, dim3(n_chunks), dim3(kChunk), 0, stream, a);
      if (listed) {
        hipLaunchKernelGGL(loss_base_kernel, dim3(1), dim3(kChunk), 0, stream, chunk_n, n_chunks,
                           chunk_base, lx->dev_n_runs);
        if (lx->run_cap)
          hipLaunchKernelGGL(loss_runs_kernel<2>, dim3(n_chunks), dim3(kChunk), 0, stream, a);
      }
    }
    if (lx->dev_pairs) {
      const uint32_t n_waves = (ns + kPairTiles * 64u - 1u) / (kPairTiles * 64u);
      hipLaunchKernelGGL(loss_pairs_kernel, dim3(n_waves), dim3(64), 0, stream, c_flow, c_mask,
                         obase, in.minp, in.maxp, n_flows, n_rcv, lx->dev_pairs);
    }
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    snprintf(err, errn, "msg_match_multi_ex: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}
