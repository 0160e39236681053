// C++ host-layer test of mgenx::FlowClock (include/mgenx.hpp): about 6000 records in 4 flows whose
// receive stamps carry a clock offset, a drift and a random delay, against a serial loop in this
// program: Andrew's monotone chain over each flow's points with __int128, then the edge over the
// mean send time, the floored line and the residuals.  Flow 0 dominates (a workgroup serves it),
// flow 3 stays empty, some records are skipped.  Also the offset-only option and the accessors.
// Prints "flow_clock_host ok" and exits 0.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "mgenx.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

typedef __int128 i128;
struct Pt {
  uint64_t x;
  int64_t d;
};

static i128 cross(const Pt& o, const Pt& a, const Pt& b) {
  return ((i128)a.x - (i128)o.x) * ((i128)b.d - (i128)o.d) -
         ((i128)a.d - (i128)o.d) * ((i128)b.x - (i128)o.x);
}

static int64_t line_at(const Pt& a, const Pt& b, uint64_t x) {
  if (a.x == b.x) return a.d;
  const i128 num = ((i128)b.d - a.d) * ((i128)x - (i128)a.x), den = (i128)(b.x - a.x);
  i128 q = num / den;
  if (num % den != 0 && num < 0) q -= 1;
  return (int64_t)(a.d + q);
}

int main() {
  using namespace mgenx;
  const uint32_t n = 6007, n_flows = 4;
  Context ctx(0);
  FlowClock::Columns col;
  uint64_t r = 24680;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  // per flow: receive clock = (1 + skew) * t + offset, plus a delay of 200 us and up
  const int64_t off[3] = {2500000, -3000000, 17};
  const int64_t ppm[3] = {40, -50, 0};
  const int64_t base = 1700000000ll * 1000000;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = rnd() % 8 < 6 ? 0 : 1 + rnd() % 2;
    const int64_t tx = base + (int64_t)i * 1531 + rnd() % 700;
    const int64_t delay = 200 + (rnd() % 16 == 0 ? rnd() % 20000 : rnd() % 900);
    const int64_t rx = tx + off[f] + (tx - base) * ppm[f] / 1000000 + delay;
    col.flow_idx.push_back(i % 401 == 400 ? MGENX_FLOW_NONE : (i % 977 == 5 ? n_flows + 3 : f));
    col.tx_sec.push_back((uint32_t)(tx / 1000000));
    col.tx_usec.push_back((uint32_t)(tx % 1000000));
    col.rx_sec.push_back((uint32_t)(rx / 1000000));
    col.rx_usec.push_back((uint32_t)(rx % 1000000));
  }

  for (int pass = 0; pass < 2; pass++) {
    const bool offset_only = pass == 1;
    FlowClock fc(ctx, n_flows, offset_only ? MGENX_CLOCK_OFFSET_ONLY : 0u);
    const std::vector<FlowClock::Flow> got = fc.Run(col);
    const std::vector<int64_t> resid = fc.Residuals();
    const std::vector<uint32_t> rxs = fc.RxSec(), rxu = fc.RxUsec();
    CHECK(got.size() == n_flows && resid.size() == n && rxs.size() == n && rxu.size() == n);

    std::vector<Pt> pt(n);
    for (uint32_t i = 0; i < n; i++) {
      pt[i].x = (uint64_t)col.tx_sec[i] * 1000000u + col.tx_usec[i];
      pt[i].d = ((int64_t)col.rx_sec[i] - (int64_t)col.tx_sec[i]) * 1000000 +
                (int64_t)col.rx_usec[i] - (int64_t)col.tx_usec[i];
    }
    uint64_t counted = 0;
    for (uint32_t f = 0; f < n_flows; f++) {
      std::vector<Pt> p;
      unsigned __int128 sum = 0;
      for (uint32_t i = 0; i < n; i++)
        if (col.flow_idx[i] == f) {
          p.push_back(pt[i]);
          sum += pt[i].x;
        }
      const FlowClock::Flow& g = got[f];
      CHECK(g.n == p.size());
      if (p.empty()) {
        CHECK(g.xa == 0 && g.xb == 0 && g.da == 0 && g.db == 0 && g.resid_sum == 0 &&
              g.resid_max == INT64_MIN && g.ia == MGENX_CLOCK_NONE && g.ib == MGENX_CLOCK_NONE);
        continue;
      }
      counted += p.size();
      std::sort(p.begin(), p.end(), [](const Pt& a, const Pt& b) {
        return a.x != b.x ? a.x < b.x : a.d < b.d;
      });
      Pt a, b;
      if (offset_only) {
        a = p[0];
        for (const Pt& q : p)
          if (q.d < a.d) a = q;  // (sorted by x: the first of the lowest has the lowest x)
        b = a;
      } else {
        std::vector<Pt> h;  // the lower hull: strict turns only, the lowest d of an x only
        for (const Pt& q : p) {
          if (!h.empty() && h.back().x == q.x) continue;
          while (h.size() >= 2 && cross(h[h.size() - 2], h.back(), q) <= 0) h.pop_back();
          h.push_back(q);
        }
        a = b = h[0];
        for (size_t k = 0; k + 1 < h.size(); k++)
          if ((unsigned __int128)p.size() * h[k].x <= sum && sum < (unsigned __int128)p.size() * h[k + 1].x) {
            a = h[k];
            b = h[k + 1];
          }
        CHECK(h.size() == 1 || a.x < b.x);
      }
      CHECK(g.xa == a.x && g.da == a.d && g.xb == b.x && g.db == b.d);
      CHECK(g.ia < n && pt[g.ia].x == a.x && pt[g.ia].d == a.d && col.flow_idx[g.ia] == f);
      CHECK(g.ib < n && pt[g.ib].x == b.x && pt[g.ib].d == b.d && col.flow_idx[g.ib] == f);
      for (uint32_t i = 0; i < g.ia; i++)
        CHECK(!(col.flow_idx[i] == f && pt[i].x == a.x && pt[i].d == a.d));
      for (uint32_t i = 0; i < g.ib; i++)
        CHECK(!(col.flow_idx[i] == f && pt[i].x == b.x && pt[i].d == b.d));
      int64_t rsum = 0, rmax = INT64_MIN;
      for (uint32_t i = 0; i < n; i++) {
        if (col.flow_idx[i] != f) continue;
        const int64_t c = pt[i].d - line_at(a, b, pt[i].x);
        CHECK(c >= 0 && resid[i] == c);
        const uint64_t rr = pt[i].x + (uint64_t)c;
        CHECK(rxs[i] == (uint32_t)(rr / 1000000u) && rxu[i] == (uint32_t)(rr % 1000000u));
        rsum += c;
        rmax = std::max(rmax, c);
      }
      CHECK(g.resid_sum == rsum && g.resid_max == rmax);
      if (!offset_only && f < 3) {
        // the drift the data were made with, within the slack a floor of 200 us leaves
        const double ppm_got = FlowClock::skew_ppm(g);
        CHECK(ppm_got > (double)ppm[f] - 25.0 && ppm_got < (double)ppm[f] + 25.0);
        CHECK(FlowClock::offset_us(g) == (double)g.da);
        const double at_b = FlowClock::offset_us(g, g.xb);
        CHECK(at_b > (double)g.db - 1.0 && at_b < (double)g.db + 1.0);
      }
      if (offset_only) CHECK(FlowClock::skew_ppm(g) == 0.0);
    }
    for (uint32_t i = 0; i < n; i++)
      if (col.flow_idx[i] >= n_flows)
        CHECK(resid[i] == INT64_MIN && rxs[i] == col.rx_sec[i] && rxu[i] == col.rx_usec[i]);
    CHECK(counted > 5900 && counted < n && got[0].n > 2048 && got[3].n == 0);
  }
  std::printf("flow_clock_host ok: %u records in %u flows\n", n, n_flows);
  return 0;
}
