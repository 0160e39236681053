// The latency histogram's bin arithmetic (mgenx_flow_dist): one definition for the kernels and
// the exported host functions mgenx_flow_dist_bin / mgenx_flow_dist_bin_lo.  Below it, the packed
// record that mgenx::flow_prep_run (mgenx_flowdist.hip; declared in mgenx_internal.hpp) leaves
// for mgenx_flow_dist and mgenx_flow_series.  Plain C++ as well as HIP; the chunk size and the
// scan the two share are device code, in mgenx_blockscan.hpp.
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

// One record as the passes read it: the sorted order puts a flow's consecutive records about
// n_flows records apart, so a lane gathering six columns touches six cache lines for 22 bytes.
// flow_dist_pack_kernel reads the columns once, coalesced, and leaves one 32-B record per input
// record (latency and receive time already in microseconds): one gather per lane instead of six.
struct alignas(16) DistRec {
  int64_t lat, rx;
  uint32_t seq, len, rsv0, rsv1;
};
static_assert(sizeof(DistRec) == 32, "DistRec is 32 B");

}  // namespace mgenx
