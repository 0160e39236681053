// mgenx_match.hpp -- what the two joins share (mgenx_match.hip: one receiver; mgenx_matchmulti.hip:
// many): the identity of a message, the open-addressing table of send indices with its build and
// mark kernels, the per-wave counter add, and the carry of the loss-run word over the chunks (the
// scan itself: mgenx_blockscan.hpp).  The kernels are `static`: each file that includes this
// header gets its own copy in its own code object, launched from that file alone.
#pragma once

#include <hip/hip_runtime.h>

#include <limits.h>

#include "mgenx_blockscan.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {

typedef struct mgenx_match_stats MatchStats;
static_assert(sizeof(MatchStats) == 32, "mgenx_match_stats is 32 B");

constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // an empty slot; MGENX_MATCH_NONE in the outputs

struct MatchSide {  // the identity columns of one side
  const uint32_t *flow, *seq, *sec, *usec;
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

struct Ident {
  uint32_t flow, seq, sec, usec;
};
__device__ __forceinline__ Ident ident_of(const MatchSide& s, uint32_t i, bool use_time) {
  Ident d;
  d.flow = s.flow[i];
  d.seq = s.seq[i];
  d.sec = use_time ? s.sec[i] : 0u;
  d.usec = use_time ? s.usec[i] : 0u;
  return d;
}
__device__ __forceinline__ bool ident_eq(const Ident& a, const Ident& b) {
  return a.flow == b.flow && a.seq == b.seq && a.sec == b.sec && a.usec == b.usec;
}
__device__ __forceinline__ uint32_t ident_slot(const Ident& d, uint32_t mask) {
  const uint64_t a = ((uint64_t)d.flow << 32) | d.seq, b = ((uint64_t)d.sec << 32) | d.usec;
  return (uint32_t)mix64(mix64(a) ^ (b * 0x9E3779B97F4A7C15ull)) & mask;
}

// the slot's record index for identity `d`, or kEmpty (the table is complete: plain loads)
__device__ __forceinline__ uint32_t table_find(const uint32_t* __restrict__ table, uint32_t mask,
                                               const MatchSide& send, bool use_time,
                                               const Ident& d) {
  uint32_t slot = ident_slot(d, mask);
  for (uint32_t k = 0; k <= mask; k++) {
    const uint32_t v = table[slot];
    if (v == kEmpty) return kEmpty;
    if (ident_eq(ident_of(send, v, use_time), d)) return v;
    slot = (slot + 1u) & mask;
  }
  return kEmpty;
}

// the sum of the lanes' counts of one wave, added by its first lane
__device__ __forceinline__ void wave_count_add(uint64_t* dst, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63u) == 0u)
    atomicAdd((unsigned long long*)dst, (unsigned long long)__popcll(m));
}

// send_rx_count / send_first_rx: mgenx_msg_match's per-record outputs, emptied here; both null
// for a caller that has none (mgenx_msg_match_multi)
static __global__ void match_build_kernel(MatchSide send, uint32_t ns, uint32_t n_flows,
                                          bool use_time, uint32_t* table, uint32_t mask,
                                          uint32_t* send_rx_count, uint32_t* send_first_rx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  if (send_rx_count) {
    send_rx_count[i] = 0u;
    send_first_rx[i] = kEmpty;
  }
  if (send.flow[i] >= n_flows) return;
  const Ident me = ident_of(send, i, use_time);
  uint32_t slot = ident_slot(me, mask);
  // (at most ns identities in more than ns slots: an empty slot or the identity's own comes up)
  for (uint32_t k = 0; k <= mask; k++) {
    const uint32_t v = atomicCAS(&table[slot], kEmpty, i);
    if (v == kEmpty) return;
    if (ident_eq(ident_of(send, v, use_time), me)) {
      if (i < v) atomicMin(&table[slot], i);
      return;
    }
    slot = (slot + 1u) & mask;
  }
}

static __global__ void match_mark_kernel(MatchSide send, uint32_t ns, uint32_t n_flows,
                                         bool use_time, const uint32_t* __restrict__ table,
                                         uint32_t mask, uint32_t* __restrict__ own,
                                         MatchStats* stats) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool skipped = false, dup = false;
  if (i < ns) {
    uint32_t o = kEmpty;
    if (send.flow[i] >= n_flows) {
      skipped = true;
    } else {
      o = table_find(table, mask, send, use_time, ident_of(send, i, use_time));
      dup = o != i;
    }
    own[i] = o;
  }
  wave_count_add(&stats->send_skipped, skipped);
  wave_count_add(&stats->send_dup, dup);
}

// (one workgroup) carry[c] = the summed word after chunk c's last position, over chunk c and the
// chunks before it back to the last segment start.  trail[c]: the sum after chunk c's last
// segment start; has_head[c]: the chunk has one.
static __global__ void __launch_bounds__(kChunk)
match_carry_kernel(const uint32_t* __restrict__ trail, const uint32_t* __restrict__ has_head,
                   uint32_t n_chunks, uint32_t* __restrict__ carry) {
  __shared__ uint32_t s_v[kWaves], s_h[kWaves];
  __shared__ uint32_t s_run;
  chunk_carry<SumOp>(
      n_chunks, 0u,
      [&](uint32_t c, uint32_t& v) {
        v = trail[c];
        return has_head[c] != 0u;
      },
      [&](uint32_t c, uint32_t v) { carry[c] = v; }, s_v, s_h, &s_run);
}

}  // namespace mgenx
