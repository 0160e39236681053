// C++ host-layer test of mgenx::FlowSeries (include/mgenx.hpp): about 5000 records in 3 flows,
// packed, received and decoded, then the per-flow time series in two Update calls against a
// serial loop over the same records.  The windows leave the first and the last records outside.
// Prints "flow_series_host ok" and exits 0.
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

struct WantBin {
  uint64_t n = 0, bytes = 0, jsum = 0, advance = 0;
  int64_t lsum = 0, lmin = INT64_MAX, lmax = INT64_MIN;
  uint32_t fresh = 0, late = 0;
};
struct WantState {
  uint64_t n = 0, outside = 0;
  int64_t last_lat = 0;
  uint32_t smax = 0;
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

  // flow of record i, its seq (now and then behind, now and then a gap), tx time; rx = tx + a
  // latency that moves, with the receive clock behind the sender's for a few records
  std::vector<uint32_t> idx(n), seq(n), rxs(n), rxu(n);
  std::vector<uint16_t> size(n);
  std::vector<int64_t> tx(n), rx(n);
  uint32_t next[n_flows] = {0, 0, 0};
  uint64_t r = 54321;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = rnd() % 7 < 4 ? 0 : 1 + rnd() % 2;  // flow 0 dominates
    idx[i] = i % 500 == 499 ? MGENX_FLOW_NONE : f;
    if (rnd() % 50 == 0) next[f] += 1 + rnd() % 4;  // lost on the way
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

  // windows of 7 ms over the middle of the 0.69 s the records span
  const int64_t t0 = 1700000000ll * 1000000 + 50000;
  const uint64_t width = 7000;
  const uint32_t n_bins = 80;

  // the serial walk
  std::vector<WantState> ws(n_flows);
  std::vector<WantBin> wb((size_t)n_flows * n_bins);
  for (uint32_t i = 0; i < n; i++) {
    if (idx[i] >= n_flows) continue;
    WantState& s = ws[idx[i]];
    const int64_t lat = rx[i] - tx[i];
    const int64_t d = rx[i] - t0;
    const int64_t b = d >= 0 ? d / (int64_t)width : -((-d + (int64_t)width - 1) / (int64_t)width);
    if (b >= 0 && b < (int64_t)n_bins) {
      WantBin& w = wb[(size_t)idx[i] * n_bins + (size_t)b];
      w.n++;
      w.bytes += size[i];
      w.lsum += lat;
      w.lmin = std::min(w.lmin, lat);
      w.lmax = std::max(w.lmax, lat);
      if (s.n) w.jsum += (uint64_t)(lat > s.last_lat ? lat - s.last_lat : s.last_lat - lat);
      if (!s.n) {
        w.fresh++;
        w.advance++;
      } else if (seq[i] > s.smax) {
        w.fresh++;
        w.advance += seq[i] - s.smax;
      } else if (seq[i] < s.smax) {
        w.late++;
      }
    } else {
      s.outside++;
    }
    s.smax = s.n ? std::max(s.smax, seq[i]) : seq[i];
    s.last_lat = lat;
    s.n++;
  }

  // two batches through the device
  FlowSeries fs(ctx, n_flows, t0, width, n_bins);
  CHECK(fs.NumBins() == n_bins && fs.BinStart(2) == t0 + 14000);
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
    fs.Update(rb, std::vector<uint32_t>(idx.begin() + a, idx.begin() + a + m),
              std::vector<uint32_t>(rxs.begin() + a, rxs.begin() + a + m),
              std::vector<uint32_t>(rxu.begin() + a, rxu.begin() + a + m));
  }
  const std::vector<FlowSeries::State> st = fs.States();
  const std::vector<FlowSeries::Bin> bins = fs.Bins();
  CHECK(st.size() == n_flows && bins.size() == (size_t)n_flows * n_bins);
  uint64_t total = 0, inside = 0, outside = 0, late = 0, skipped = 0;
  for (uint32_t f = 0; f < n_flows; f++) {
    CHECK(st[f].n == ws[f].n && st[f].outside == ws[f].outside);
    CHECK(st[f].last_lat == ws[f].last_lat && st[f].seq_max == ws[f].smax && st[f].rsv == 0);
    total += st[f].n;
    outside += st[f].outside;
    for (uint32_t b = 0; b < n_bins; b++) {
      const WantBin& w = wb[(size_t)f * n_bins + b];
      const FlowSeries::Bin& g = bins[(size_t)f * n_bins + b];
      CHECK(g.n == w.n && g.bytes == w.bytes && g.jitter_sum == w.jsum);
      CHECK(g.lat_sum == w.lsum && g.lat_min == w.lmin && g.lat_max == w.lmax);
      CHECK(g.advance == w.advance && g.fresh == w.fresh && g.late == w.late);
      inside += g.n;
      late += g.late;
      skipped += g.advance - g.fresh;
    }
  }
  CHECK(total == n - n / 500 && inside + outside == total);
  CHECK(outside > 300 && inside > 3000 && late > 100 && skipped > 100);
  CHECK(st[0].n > st[1].n + st[2].n);
  std::printf("flow_series_host ok: %" PRIu64 " records, %" PRIu64 " outside the windows, %" PRIu64
              " late, %" PRIu64 " sequence numbers skipped\n", total, outside, late, skipped);
  return 0;
}
