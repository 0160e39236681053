// The latency histogram's bin arithmetic (mgenx_flow_dist): one definition for the kernels and
// the exported host functions mgenx_flow_dist_bin / mgenx_flow_dist_bin_lo.  Below it, what
// mgenx_flow_dist and mgenx_flow_series share: the chunk size, the packed record and the
// segmented max scan of the sort / pack / carry passes behind mgenx::flow_prep_run
// (mgenx_flowdist.hip; declared in mgenx_internal.hpp).
//
// 0 <= v < 2^32 microseconds in MGENX_FLOW_DIST_BINS = 896 bins: one bin per value below 64, then
// 32 sub-bins per octave (a relative width of 1/32 .. 1/64):
//   bin(v) = v                                              v < 64
//          = 64 + (e - 6) * 32 + ((v >> (e - 5)) - 32)      e = floor(log2 v) >= 6
// Bin b >= 64 starts at (32 + (b - 64) % 32) << ((b - 64) / 32 + 1) and is
// 1 << ((b - 64) / 32 + 1) wide; bin_lo(896) = 2^32 closes the last bin.
#pragma once
#include <stdint.h>

#include "mgenx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGENX_HD __host__ __device__
#else
#define MGENX_HD
#endif

namespace mgenx {

// v < 2^32; any larger value maps to MGENX_FLOW_DIST_BINS (no bin)
MGENX_HD inline uint32_t flow_dist_bin(uint64_t v) {
  if (v < 64u) return (uint32_t)v;
  if (v >> 32) return MGENX_FLOW_DIST_BINS;
  const uint32_t e = 31u - (uint32_t)__builtin_clz((uint32_t)v);
  return 64u + (e - 6u) * 32u + (((uint32_t)v >> (e - 5u)) - 32u);
}

// the lowest value of bin b; b >= MGENX_FLOW_DIST_BINS gives 2^32
MGENX_HD inline uint64_t flow_dist_bin_lo(uint32_t b) {
  if (b < 64u) return b;
  if (b >= MGENX_FLOW_DIST_BINS) return 1ull << 32;
  const uint32_t k = b - 64u;
  return (uint64_t)(32u + k % 32u) << (k / 32u + 1u);
}

// ---- what the per-flow passes share (mgenx_flowdist.hip, mgenx_flowseries.hip) ----
constexpr uint32_t kChunk = 1024;   // sorted positions (= lanes) per workgroup
constexpr uint32_t kWaves = kChunk / 64;
constexpr int64_t kNone = -1;       // "no earlier record" as a running maximum of u32 values

// One record as the passes read it: the sorted order puts a flow's consecutive records about
// n_flows records apart, so a lane gathering six columns touches six cache lines for 22 bytes.
// flow_dist_pack_kernel reads the columns once, coalesced, and leaves one 32-B record per input
// record (latency and receive time already in microseconds): one gather per lane instead of six.
struct alignas(16) DistRec {
  int64_t lat, rx;
  uint32_t seq, len, rsv0, rsv1;
};
static_assert(sizeof(DistRec) == 32, "DistRec is 32 B");

#if defined(__HIPCC__)
// ---- segmented inclusive max scan over the kChunk lanes of a workgroup ----
// `head` starts a segment at this lane.  Returns the maximum of v over the lanes from the
// lane's segment start (or lane 0) to the lane; *open = no segment starts at or before it.
// s_v / s_h: kWaves entries each.  Ends with every lane past the last barrier's reads.
__device__ __forceinline__ int64_t block_segmax(int64_t v, bool head, int64_t* s_v, uint32_t* s_h,
                                                bool* open) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t h = head ? 1u : 0u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const int64_t pv = __shfl_up((long long)v, d);
    const uint32_t ph = __shfl_up(h, d);
    if (lane >= d && !h) {
      v = v > pv ? v : pv;
      h = ph;
    }
  }
  if (lane == 63u) {
    s_v[w] = v;
    s_h[w] = h;
  }
  __syncthreads();
  if (w == 0) {
    int64_t wv = lane < kWaves ? s_v[lane] : kNone;
    uint32_t wh = lane < kWaves ? s_h[lane] : 1u;
#pragma unroll
    for (uint32_t d = 1; d < kWaves; d <<= 1) {
      const int64_t pv = __shfl_up((long long)wv, d);
      const uint32_t ph = __shfl_up(wh, d);
      if (lane >= d && !wh) {
        wv = wv > pv ? wv : pv;
        wh = ph;
      }
    }
    if (lane < kWaves) {
      s_v[lane] = wv;
      s_h[lane] = wh;
    }
  }
  __syncthreads();
  if (w > 0 && !h) {
    const int64_t pv = s_v[w - 1];
    v = v > pv ? v : pv;
    h = s_h[w - 1];
  }
  *open = h == 0u;
  __syncthreads();
  return v;
}
#endif

}  // namespace mgenx
