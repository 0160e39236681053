// The integer arithmetic of mgenx_flow_series_quantiles (mgen_amd/csrc/mgenx_flowquant.hpp) as a
// host program under the address and undefined-behaviour sanitizers: the rank rule against
// 128-bit arithmetic up to the largest cell, the tier of every size around every edge, the
// padded size of the in-LDS sort and the capacity of the tier lists.  No HIP, no GPU.
// Prints "flow_quant_arith_host ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mgen_amd/csrc/mgenx_flowquant.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

int main() {
  using namespace mgenx;
  const uint32_t edges[kLists] = {kTinyMax, kWaveMax, kGroupMax, kWideMax};
  static_assert(MGENX_FLOW_SERIES_MAX_Q == 32, "the ranks of one call");

  // sizes worth looking at: small ones, around every edge and power of two, the largest
  std::vector<uint32_t> sizes;
  for (uint32_t c = 1; c <= 2100; c++) sizes.push_back(c);
  for (uint32_t b = 12; b < 31; b++)
    for (int d = -1; d <= 1; d++) sizes.push_back((1u << b) + d);
  sizes.push_back(0x7FFFFFFFu);

  for (uint32_t c : sizes) {
    uint32_t prev = 1;
    for (uint32_t q = 1; q <= 1000; q++) {
      const unsigned __int128 wide = ((unsigned __int128)q * c + 999u) / 1000u;
      const uint32_t r = quant_rank(q, c);
      CHECK(r == (wide < 1 ? 1 : (uint32_t)wide) && r >= 1 && r <= c && r >= prev);
      prev = r;
    }
    CHECK(quant_rank(1000, c) == c && quant_rank(1, c) == (c + 999u) / 1000u);
    if (c <= (1u << 30)) {
      const uint32_t p = quant_pow2(c);
      CHECK((p & (p - 1u)) == 0u && p >= 2u && p >= c && (c < 2u || p < 2u * c));
    }
  }
  CHECK(quant_rank(1, 1000) == 1 && quant_rank(1, 1001) == 2);

  // tiers: empty and up to the first edge tiny, then the first list whose edge holds the size
  CHECK(quant_tier(0) == kTierTiny && quant_tier(1) == kTierTiny);
  for (int t = 0; t < kLists; t++) {
    CHECK(t == 0 || edges[t] > edges[t - 1]);
    CHECK(quant_tier(edges[t]) == (t == 0 ? kTierTiny : t - 1));
    CHECK(quant_tier(edges[t] + 1u) == t);
  }
  CHECK(quant_tier(0xFFFFFFFFu) == kListLarge);
  // an in-LDS tier's padded size never exceeds its edge
  for (uint32_t c = kTinyMax + 1u; c <= kWideMax; c++) CHECK(quant_pow2(c) <= edges[quant_tier(c) + 1]);

  // list capacities: enough for every cell n records can form above the edge, never past n_cells
  const uint32_t ns[] = {1, 8, 9, 17, 18, 257, 514, 16385, 32770, 265795, 8388608, 0x7FFFFFFFu};
  for (uint32_t n : ns)
    for (uint32_t n_cells : {1u, 7u, 1000u, 0x7FFFFFFFu})
      for (int t = 0; t < kLists; t++) {
        const uint32_t cap = quant_tier_cap(n, n_cells, edges[t]);
        CHECK(cap <= n_cells && (uint64_t)cap * (edges[t] + 1u) <= n);
        CHECK(cap == n_cells || ((uint64_t)cap + 1u) * (edges[t] + 1u) > n);
      }
  std::printf("flow_quant_arith_host ok: %zu sizes\n", sizes.size());
  return 0;
}
