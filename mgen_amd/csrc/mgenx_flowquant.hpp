// The integer arithmetic of mgenx_flow_series_quantiles that host and device share
// (mgenx_flowquant.hip): the tier edges, the tier of a cell, the rank of a permille value, the
// padded size of an in-LDS sort and the capacity of a tier's list.  No HIP needed:
// tests/cpp/flow_quant_arith_host.cpp runs these under the address and undefined-behaviour
// sanitizers.
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

// ---- the tier edges: a cell of c records takes the first tier with c <= its edge ----
constexpr uint32_t kTinyMax = 8;       // a lane per cell, keys in registers
constexpr uint32_t kWaveMax = 256;     // a wave per cell, 2 KiB of LDS
constexpr uint32_t kGroupMax = 2048;   // 256 lanes per cell, 16 KiB of LDS
constexpr uint32_t kWideMax = 16384;   // 1024 lanes per cell, 128 KiB of LDS; above: radix select

// the tiers above tiny keep a list of their cells
enum { kListWave = 0, kListGroup = 1, kListWide = 2, kListLarge = 3, kLists = 4 };
constexpr int kTierTiny = -1;  // (empty cells included)

MGENX_HD inline int quant_tier(uint32_t c) {
  return c <= kTinyMax ? kTierTiny
         : c <= kWaveMax ? kListWave
         : c <= kGroupMax ? kListGroup
         : c <= kWideMax ? kListWide : kListLarge;
}

// rank of permille q (1..1000) among c >= 1 values: 1 <= r <= c
MGENX_HD inline uint32_t quant_rank(uint32_t q, uint32_t c) {
  const uint64_t r = ((uint64_t)q * c + 999u) / 1000u;
  return r < 1u ? 1u : (uint32_t)r;
}

// the power of two a bitonic sort of c keys runs over: 2 <= p, c <= p < 2 c (c >= 2), c <= 2^31
MGENX_HD inline uint32_t quant_pow2(uint32_t c) {
  return c > 2u ? 1u << (32u - (uint32_t)__builtin_clz(c - 1u)) : 2u;
}

// how many cells of more than `edge` records n records can form, within n_cells
inline uint32_t quant_tier_cap(uint32_t n, uint32_t n_cells, uint32_t edge) {
  const uint32_t by_n = n / (edge + 1u);
  return by_n < n_cells ? by_n : n_cells;
}

}  // namespace mgenx
