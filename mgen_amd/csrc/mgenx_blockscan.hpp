// mgenx_blockscan.hpp -- the workgroup primitives of the per-flow passes (mgenx_flowdist.hip,
// mgenx_flowseries.hip, mgenx_match.hip, mgenx_matchmulti.hip, mgenx_flowclock.hip): the chunk
// size, word-wise lane shuffles of any value, a reduction over a wave, a segmented inclusive scan
// over the kChunk lanes of a workgroup, and that scan walked over any number of entries by one
// workgroup.  Device code: .hip files only.
//
// An operator is a type with a static `of(earlier, later)` that is associative; every one in use
// is commutative too.  A value is trivially copyable and a whole number of 32-bit words.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

namespace mgenx {

constexpr uint32_t kChunk = 1024;   // sorted positions (= lanes) per workgroup
constexpr uint32_t kWaves = kChunk / 64;
constexpr int64_t kNone = -1;       // "no earlier record" as a running maximum of u32 values

struct SumOp {
  template <class T>
  static __device__ __forceinline__ T of(T a, T b) { return a + b; }
};
struct MinOp {
  template <class T>
  static __device__ __forceinline__ T of(T a, T b) { return a < b ? a : b; }
};
struct MaxOp {
  template <class T>
  static __device__ __forceinline__ T of(T a, T b) { return a > b ? a : b; }
};

// v of the lane d below (lane_shfl_up; the lanes under d keep their own) or of lane ^ mask
// (lane_shfl_xor) within the wave, one 32-bit shuffle per word
template <class V, class F>
__device__ __forceinline__ V lane_shfl_words(const V& v, F f) {
  static_assert(std::is_trivially_copyable<V>::value && sizeof(V) % 4 == 0, "whole words");
  constexpr int kW = sizeof(V) / 4;
  union {
    V v;
    uint32_t w[kW];
  } a, b;
  a.v = v;
#pragma unroll
  for (int k = 0; k < kW; k++) b.w[k] = (uint32_t)f((int)a.w[k]);
  return b.v;
}
template <class V>
__device__ __forceinline__ V lane_shfl_up(const V& v, uint32_t d) {
  return lane_shfl_words(v, [d](int w) { return __shfl_up(w, d); });
}
template <class V>
__device__ __forceinline__ V lane_shfl_xor(const V& v, int mask) {
  return lane_shfl_words(v, [mask](int w) { return __shfl_xor(w, mask); });
}

// the reduction of v over the 64 lanes of a wave; every lane calls, every lane gets the result
template <class Op, class V>
__device__ __forceinline__ V wave_reduce(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = Op::of(v, lane_shfl_xor(v, o));
  return v;
}

// ---- segmented inclusive scan over the kChunk lanes of a workgroup ----
// `head` starts a segment at this lane.  Returns Op over the values of the lanes from the lane's
// segment start (or lane 0) to the lane.  With `open`, *open = no segment starts at or before the
// lane: what came before lane 0 continues into it.  Without, nothing is computed for it.
// s_v / s_h: kWaves entries each, in LDS.  All kChunk lanes call it together.
//
// Barriers.  On entry no lane may still read s_v / s_h from an earlier use; the scan's two inner
// barriers order its own accesses.  kSync (the default): a closing barrier, so on return every
// lane is past the scan's last read and the caller may write s_v / s_h again at once, as the
// next scan over the same arrays does.  !kSync: no closing barrier.  The value returned and
// *open are complete either way (they are the lane's own registers); what the caller gives up is
// the reuse: it must pass a barrier of its own before any lane writes s_v or s_h again.
template <class Op, bool kSync = true, class V>
__device__ __forceinline__ V seg_scan(V v, bool head, V* s_v, uint32_t* s_h,
                                      bool* open = nullptr) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t h = head ? 1u : 0u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const V pv = lane_shfl_up(v, d);
    const uint32_t ph = __shfl_up(h, d);
    if (lane >= d && !h) {
      v = Op::of(pv, v);
      h = ph;
    }
  }
  if (lane == 63u) {
    s_v[w] = v;
    s_h[w] = h;
  }
  __syncthreads();
  if (w == 0) {
    // (the idle lanes hold a copy of wave 0's total under a head flag: no identity is needed)
    V wv = s_v[lane < kWaves ? lane : 0u];
    uint32_t wh = lane < kWaves ? s_h[lane] : 1u;
#pragma unroll
    for (uint32_t d = 1; d < kWaves; d <<= 1) {
      const V pv = lane_shfl_up(wv, d);
      const uint32_t ph = __shfl_up(wh, d);
      if (lane >= d && !wh) {
        wv = Op::of(pv, wv);
        wh = ph;
      }
    }
    if (lane < kWaves) {
      s_v[lane] = wv;
      if (open) s_h[lane] = wh;
    }
  }
  __syncthreads();
  if (w > 0 && !h) {  // the segment started in an earlier wave
    v = Op::of(s_v[w - 1], v);
    if (open) h = s_h[w - 1];
  }
  if (open) *open = h == 0u;
  if (kSync) __syncthreads();
  return v;
}

// ---- the scan over n entries by one workgroup, kChunk entries a round ----
// in(c, v) loads entry c < n into v and returns its head flag; out(c, v) takes the scanned value
// of entry c: Op over the entries from its segment start (or entry 0) to it.  `idle` is Op's
// identity: what runs into entry 0, and the value of the lanes past n (which start no segment).
// Returns the value after the last entry (idle when n == 0) in every lane.  A scan without
// segments is an `in` that never returns a head.  s_v / s_h as seg_scan's; s_run: one value.
template <class Op, class V, class In, class Out>
__device__ __forceinline__ V chunk_carry(uint32_t n, V idle, In in, Out out, V* s_v,
                                         uint32_t* s_h, V* s_run) {
  const uint32_t t = threadIdx.x;
  if (t == 0) *s_run = idle;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kChunk) {
    const uint32_t c = base + t;
    V v = idle;
    bool head = false, open;
    if (c < n) head = in(c, v);
    v = seg_scan<Op>(v, head, s_v, s_h, &open);
    if (open) v = Op::of(*s_run, v);
    if (c < n) out(c, v);
    __syncthreads();  // every lane has read s_run
    if (t == kChunk - 1u) *s_run = v;
    __syncthreads();
  }
  return *s_run;
}

}  // namespace mgenx
