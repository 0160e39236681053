// The exact integer arithmetic of mgenx_flow_clock that host and device share
// (mgenx_flowclock.hip): a record's point (x, d), the chord key of the hull search, the side of
// the mean a vertex lies on, the floored line, the split of a corrected receive time into its
// two stamps, and the tier edges.  128-bit where the products need it (about 2^106).  No HIP
// needed: tests/cpp/flow_clock_arith_host.cpp runs these under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include "mgenx.h"

#ifndef MGENX_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGENX_HD __host__ __device__
#else
#define MGENX_HD
#endif
#endif

namespace mgenx {

typedef __int128 clock_i128;
typedef unsigned __int128 clock_u128;

// ---- the tiers: a flow of c points is served by one wave up to kClockWaveMax, by a workgroup
// of kClockGroupLanes above; the lanes of either walk the flow's points in chunks of their count,
// kClockUnroll chunks at a time while that many are left
constexpr uint32_t kClockUnroll = 4;
constexpr uint32_t kClockWaveLanes = 64;
constexpr uint32_t kClockGroupLanes = 1024;
constexpr uint32_t kClockWaveMax = 2048;
// every size at which the code takes another path (tests/test_gpu_flow_clock.py walks them)
constexpr uint32_t kClockEdges[] = {kClockWaveLanes, kClockUnroll * kClockWaveLanes,
                                    kClockGroupLanes, kClockWaveMax,
                                    kClockUnroll * kClockGroupLanes};

MGENX_HD inline bool clock_wave_tier(uint32_t c) { return c <= kClockWaveMax; }

// how many flows of more than kClockWaveMax records n records can form, within n_flows
inline uint32_t clock_list_cap(uint32_t n, uint32_t n_flows) {
  const uint32_t by_n = n / (kClockWaveMax + 1u);
  return by_n < n_flows ? by_n : n_flows;
}

// ---- a record's point: send time and latency in microseconds (a tx_usec >= 10^6 as it is) ----
MGENX_HD inline uint64_t clock_x(uint32_t tx_sec, uint32_t tx_usec) {
  return (uint64_t)tx_sec * 1000000u + tx_usec;  // < 2^52
}
MGENX_HD inline int64_t clock_d(uint32_t tx_sec, uint32_t tx_usec, uint32_t rx_sec,
                                uint32_t rx_usec) {
  return ((int64_t)rx_sec - (int64_t)tx_sec) * 1000000 + (int64_t)rx_usec - (int64_t)tx_usec;
}

// ---- the chord key: twice the signed area of (L, R, P); negative iff P lies below the line
// through L and R (x_l < x_r), and the more negative the farther below.  |terms| < 2^106.
MGENX_HD inline clock_i128 clock_key(uint64_t xl, int64_t dl, uint64_t xr, int64_t dr, uint64_t x,
                                     int64_t d) {
  const clock_i128 dx = (clock_i128)xr - (clock_i128)xl, dd = (clock_i128)dr - (clock_i128)dl;
  return dx * ((clock_i128)d - (clock_i128)dl) - dd * ((clock_i128)x - (clock_i128)xl);
}

// ---- the vertex-side test: n * x <= S, S = s_hi * 2^64 + s_lo the sum of the flow's x ----
MGENX_HD inline bool clock_left(uint64_t n, uint64_t x, uint64_t s_lo, uint64_t s_hi) {
  const clock_u128 s = ((clock_u128)s_hi << 64) | s_lo;
  return (clock_u128)n * x <= s;
}

// ---- line(x) = da + floor((db - da) (x - xa) / (xb - xa)), the floor toward -inf; da when
// xa == xb.  xa <= xb.
MGENX_HD inline int64_t clock_line(uint64_t xa, int64_t da, uint64_t xb, int64_t db, uint64_t x) {
  if (xa >= xb) return da;
  const clock_i128 num = ((clock_i128)db - (clock_i128)da) * ((clock_i128)x - (clock_i128)xa);
  const uint64_t den = xb - xa;  // 1 .. 2^52
  int64_t q;
  if (num >= -((clock_i128)1 << 62) && num < ((clock_i128)1 << 62)) {  // the common case
    const int64_t n64 = (int64_t)num, d64 = (int64_t)den;
    q = n64 / d64;
    if (n64 % d64 < 0) q -= 1;
  } else {
    clock_i128 q128 = num / (clock_i128)den;
    if (num % (clock_i128)den < 0) q128 -= 1;
    q = (int64_t)(uint64_t)(clock_u128)q128;  // modulo 2^64 (the contract: c is kept so)
  }
  return (int64_t)((uint64_t)da + (uint64_t)q);
}

// c = d - line(x), as the 64-bit difference
MGENX_HD inline int64_t clock_resid(uint64_t xa, int64_t da, uint64_t xb, int64_t db, uint64_t x,
                                    int64_t d) {
  return (int64_t)((uint64_t)d - (uint64_t)clock_line(xa, da, xb, db, x));
}

// ---- the corrected receive time r = x + c on the sender's clock, as stamps ----
MGENX_HD inline void clock_stamp(uint64_t x, int64_t c, uint32_t* sec, uint32_t* usec) {
  const uint64_t r = x + (uint64_t)c;
  *sec = (uint32_t)(r / 1000000u);  // mod 2^32
  *usec = (uint32_t)(r % 1000000u);
}

}  // namespace mgenx
