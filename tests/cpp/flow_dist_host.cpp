// C++ host-layer test of mgenx::FlowDistribution (include/mgenx.hpp): about 5000 records in 3
// flows, packed, received and decoded, then the per-flow delivery statistics in two Update
// calls against a serial loop over the same records.  Prints "flow_dist_host ok" and exits 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mgenx.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

uint32_t bin_of(uint64_t v) {  // restated from the definition, not the library's
  if (v < 64) return (uint32_t)v;
  uint32_t e = 0;
  while ((v >> (e + 1)) != 0) e++;
  return 64 + (e - 6) * 32 + (uint32_t)((v >> (e - 5)) - 32);
}

struct Want {
  uint64_t n = 0, bytes = 0, neg = 0, over = 0, jsum = 0, jmax = 0, reo = 0, rsum = 0;
  int64_t lsum = 0, lmin = INT64_MAX, lmax = INT64_MIN, gmin = INT64_MAX, gmax = INT64_MIN;
  int64_t first_rx = 0, last_rx = 0, last_lat = 0;
  uint32_t rmax = 0, smin = UINT32_MAX, smax = 0;
  std::vector<uint64_t> hist = std::vector<uint64_t>(MGENX_FLOW_DIST_BINS, 0);
};

}  // namespace

int main() {
  using namespace mgenx;
  const uint32_t n = 5001, n_flows = 3, slot = 128;
  Context ctx(0);
  SendBatch sb(ctx);
  const uint8_t lo[4] = {127, 0, 0, 1};
  uint32_t fl[n_flows];
  for (uint32_t f = 0; f < n_flows; f++) fl[f] = sb.AddFlow(f + 1, IPv4, lo, (uint16_t)(5000 + f));

  // flow of record i, its seq (now and then behind), tx time; rx = tx + a latency that moves,
  // with the receive clock behind the sender's for a few records
  std::vector<uint32_t> idx(n), seq(n), rxs(n), rxu(n);
  std::vector<uint16_t> size(n);
  std::vector<int64_t> tx(n), rx(n);
  uint32_t next[n_flows] = {0, 0, 0};
  uint64_t r = 12345;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = rnd() % 7 < 4 ? 0 : 1 + rnd() % 2;  // flow 0 dominates
    idx[i] = i % 500 == 499 ? MGENX_FLOW_NONE : f;
    seq[i] = next[f]++;
    if (rnd() % 20 == 0 && seq[i] > 6) seq[i] -= 1 + rnd() % 6;
    tx[i] = 1700000000ll * 1000000 + (int64_t)i * 137 + rnd() % 100;
    rx[i] = tx[i] + 40 + rnd() % 3000 - (i % 911 == 5 ? 5000 : 0);
    size[i] = (uint16_t)(64 + rnd() % 65);
    struct timeval tv;
    tv.tv_sec = (time_t)(tx[i] / 1000000);
    tv.tv_usec = (suseconds_t)(tx[i] % 1000000);
    sb.Add(fl[f], seq[i], tv, size[i]);
    rxs[i] = (uint32_t)(rx[i] / 1000000);
    rxu[i] = (uint32_t)(rx[i] % 1000000);
  }
  const std::vector<uint32_t>& len = sb.Pack(/*checksum=*/true, false, 0, slot);

  // the serial walk
  std::vector<Want> want(n_flows);
  for (uint32_t i = 0; i < n; i++) {
    if (idx[i] >= n_flows) continue;
    Want& w = want[idx[i]];
    const int64_t lat = rx[i] - tx[i];
    if (w.n) {
      const uint64_t j = (uint64_t)(lat > w.last_lat ? lat - w.last_lat : w.last_lat - lat);
      const int64_t g = rx[i] - w.last_rx;
      w.jsum += j;
      w.jmax = std::max(w.jmax, j);
      w.gmin = std::min(w.gmin, g);
      w.gmax = std::max(w.gmax, g);
      if (seq[i] < w.smax) {
        w.reo++;
        w.rsum += w.smax - seq[i];
        w.rmax = std::max(w.rmax, w.smax - seq[i]);
      }
    } else {
      w.first_rx = rx[i];
    }
    w.n++;
    w.bytes += size[i];
    w.lsum += lat;
    w.lmin = std::min(w.lmin, lat);
    w.lmax = std::max(w.lmax, lat);
    if (lat < 0) w.neg++;
    else if (lat >= (1ll << 32)) w.over++;
    else w.hist[bin_of((uint64_t)lat)]++;
    w.smin = std::min(w.smin, seq[i]);
    w.smax = std::max(w.smax, seq[i]);
    w.last_rx = rx[i];
    w.last_lat = lat;
  }

  // two batches through the device
  FlowDistribution fd(ctx, n_flows);
  const uint32_t cuts[3] = {0, 1777, n};
  for (int k = 0; k < 2; k++) {
    const uint32_t a = cuts[k], m = cuts[k + 1] - a;
    RecvBatch rb(ctx, m, slot);
    for (uint32_t i = 0; i < m; i++) {
      CHECK(len[a + i] == size[a + i]);
      std::memcpy(rb.Slot(i), sb.Datagram(a + i), len[a + i]);
      rb.SetLength(i, len[a + i]);
    }
    rb.Unpack(m);
    CHECK(rb[0].GetError() == ERROR_NONE && rb[m - 1].GetSeqNum() == seq[a + m - 1]);
    fd.Update(rb, std::vector<uint32_t>(idx.begin() + a, idx.begin() + a + m),
              std::vector<uint32_t>(rxs.begin() + a, rxs.begin() + a + m),
              std::vector<uint32_t>(rxu.begin() + a, rxu.begin() + a + m));
  }
  const std::vector<FlowDistribution::State> got = fd.Dist();
  const std::vector<uint64_t> hist = fd.Histogram();
  const std::vector<int64_t> q = fd.Quantiles({500, 1000});
  uint64_t total = 0, reordered = 0, negative = 0;
  for (uint32_t f = 0; f < n_flows; f++) {
    const Want& w = want[f];
    const FlowDistribution::State& g = got[f];
    CHECK(g.n == w.n && g.bytes == w.bytes && g.lat_neg == w.neg && g.lat_over == w.over);
    CHECK(g.lat_sum == w.lsum && g.lat_min == w.lmin && g.lat_max == w.lmax);
    CHECK(g.jitter_sum == w.jsum && g.jitter_max == w.jmax);
    CHECK(g.gap_min == w.gmin && g.gap_max == w.gmax);
    CHECK(g.reordered == w.reo && g.reorder_sum == w.rsum && g.reorder_max == w.rmax);
    CHECK(g.seq_min == w.smin && g.seq_max == w.smax);
    CHECK(g.first_rx == w.first_rx && g.last_rx == w.last_rx && g.last_lat == w.last_lat);
    for (uint32_t b = 0; b < MGENX_FLOW_DIST_BINS; b++)
      CHECK(hist[(size_t)f * MGENX_FLOW_DIST_BINS + b] == w.hist[b]);
    // the largest latency lies in the last bin with a count, whose upper edge is the maximum
    CHECK(q[f * 2 + 1] >= w.lmax && (uint64_t)w.lmax >= mgenx_flow_dist_bin_lo(
                                        mgenx_flow_dist_bin((uint64_t)w.lmax)));
    CHECK(q[f * 2] <= q[f * 2 + 1] && q[f * 2] >= -1);
    total += g.n;
    reordered += g.reordered;
    negative += g.lat_neg;
  }
  CHECK(total == n - n / 500 && reordered > 100 && negative >= 5);
  CHECK(got[0].n > got[1].n + got[2].n);
  std::printf("flow_dist_host ok: %" PRIu64 " records, %" PRIu64 " reordered, %" PRIu64
              " with a negative latency\n", total, reordered, negative);
  return 0;
}
