// C++ host-layer test of mgenx::FlowSeriesQuantiles (include/mgenx.hpp): about 5000 records in 3
// flows, packed, received and decoded, then the exact latency percentiles per flow and window
// against a serial loop with std::sort over the same records.  The windows leave the first
// records outside and run past the last; flow 0 dominates, so the cells run from empty to a few
// hundred records.  Prints "flow_quant_host ok" and exits 0.
#include <algorithm>
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

int main() {
  using namespace mgenx;
  const uint32_t n = 5001, n_flows = 3, slot = 128;
  Context ctx(0);
  SendBatch sb(ctx);
  const uint8_t lo[4] = {127, 0, 0, 1};
  uint32_t fl[n_flows];
  for (uint32_t f = 0; f < n_flows; f++) fl[f] = sb.AddFlow(f + 1, IPv4, lo, (uint16_t)(5000 + f));

  // rx = tx + a latency that moves, with the receive clock behind the sender's now and then
  std::vector<uint32_t> idx(n), rxs(n), rxu(n);
  std::vector<int64_t> tx(n), rx(n);
  uint32_t next[n_flows] = {0, 0, 0};
  uint64_t r = 97531;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = rnd() % 7 < 4 ? 0 : 1 + rnd() % 2;
    idx[i] = i % 500 == 499 ? MGENX_FLOW_NONE : f;
    tx[i] = 1700000000ll * 1000000 + (int64_t)i * 137 + rnd() % 100;
    rx[i] = tx[i] + 40 + rnd() % 3000 - (i % 311 == 5 ? 5000 : 0);
    struct timeval tv;
    tv.tv_sec = (time_t)(tx[i] / 1000000);
    tv.tv_usec = (suseconds_t)(tx[i] % 1000000);
    sb.Add(fl[f], next[f]++, tv, (uint16_t)(64 + rnd() % 65));
    rxs[i] = (uint32_t)(rx[i] / 1000000);
    rxu[i] = (uint32_t)(rx[i] % 1000000);
  }
  const std::vector<uint32_t>& len = sb.Pack(/*checksum=*/true, false, 0, slot);

  // windows of 100 ms from 50 ms into the 0.69 s the records span; the last one stays empty
  const int64_t t0 = 1700000000ll * 1000000 + 50000;
  const uint64_t width = 100000;
  const uint32_t n_bins = 8;
  const std::vector<uint32_t> permille = {1, 500, 950, 990, 1000};
  const size_t nq = permille.size();

  // the serial walk
  std::vector<std::vector<int64_t>> cell((size_t)n_flows * n_bins);
  uint64_t inside = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (idx[i] >= n_flows) continue;
    const int64_t d = rx[i] - t0;
    const int64_t b = d >= 0 ? d / (int64_t)width : -((-d + (int64_t)width - 1) / (int64_t)width);
    if (b < 0 || b >= (int64_t)n_bins) continue;
    cell[(size_t)idx[i] * n_bins + (size_t)b].push_back(rx[i] - tx[i]);
    inside++;
  }

  RecvBatch rb(ctx, n, slot);
  for (uint32_t i = 0; i < n; i++) {
    std::memcpy(rb.Slot(i), sb.Datagram(i), len[i]);
    rb.SetLength(i, len[i]);
  }
  rb.Unpack(n);
  CHECK(rb[0].GetError() == ERROR_NONE);
  const std::vector<int64_t> got =
      FlowSeriesQuantiles(ctx, rb, idx, rxs, rxu, n_flows, t0, width, n_bins, permille);
  CHECK(got.size() == cell.size() * nq);

  size_t empty = 0, largest = 0, negative = 0;
  for (size_t c = 0; c < cell.size(); c++) {
    std::vector<int64_t>& v = cell[c];
    std::sort(v.begin(), v.end());
    largest = std::max(largest, v.size());
    for (size_t j = 0; j < nq; j++) {
      int64_t want = INT64_MIN;
      if (!v.empty()) {
        uint64_t rank = ((uint64_t)permille[j] * v.size() + 999u) / 1000u;
        if (rank < 1) rank = 1;
        want = v[rank - 1];
      }
      CHECK(got[c * nq + j] == want);
      if (want < 0 && want != INT64_MIN) negative++;
    }
    if (v.empty()) empty++;
  }
  CHECK(inside > 3000 && inside < n - n / 500 && largest > 256 && negative > 0 && empty >= n_flows);
  std::printf("flow_quant_host ok: %" PRIu64 " records in %zu cells, %zu empty, the largest %zu\n",
              inside, cell.size(), empty, largest);
  return 0;
}
