// C++ host-layer test of mgenx::MessageMatchMulti (include/mgenx.hpp): about 9000 sent messages
// in 4 flows and 5 receivers (one joins late, one leaves early, one logs some messages twice,
// all lose a few), some send lines repeated, a few records of either side without a flow,
// through RunSeries against a serial loop over the same records.
// Prints "msg_match_multi_host ok" and exits 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
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
  const uint32_t ns = 9001, n_flows = 4, n_rcv = 5, n_bins = 16;
  Context ctx(0);
  uint64_t r = 24680;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };

  MessageMatchMulti::SendColumns s;
  const int64_t t_first = 1700000000ll * 1000000 + 999000;
  uint32_t next[n_flows] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < ns; i++) {
    const uint32_t f = rnd() % 9 < 5 ? 0 : 1 + rnd() % 3;  // flow 0 dominates
    const int64_t t = t_first + (int64_t)i * 211;
    if (i > 100 && rnd() % 300 == 0) {  // the line of an earlier message again
      const uint32_t j = i - 1 - rnd() % 100;
      s.flow_idx.push_back(s.flow_idx[j]);
      s.seq.push_back(s.seq[j]);
      s.t_sec.push_back(s.t_sec[j]);
      s.t_usec.push_back(s.t_usec[j]);
      s.len.push_back(s.len[j]);
      continue;
    }
    s.flow_idx.push_back(i % 1000 == 999 ? MGENX_FLOW_NONE : f);
    s.seq.push_back(next[f]++);
    s.t_sec.push_back((uint32_t)(t / 1000000));
    s.t_usec.push_back((uint32_t)(t % 1000000));
    s.len.push_back(64 + rnd() % 1200);
  }

  // the receivers' logs, one after the other
  MessageMatchMulti::RecvColumns q;
  std::vector<uint32_t> rcv;
  auto log_line = [&](uint32_t i, uint32_t k, uint32_t seq_xor) {
    const int64_t rx = (int64_t)s.t_sec[i] * 1000000 + s.t_usec[i] + 150 + rnd() % 4000 - 40 * k;
    q.flow_idx.push_back(s.flow_idx[i]);
    q.seq.push_back(s.seq[i] ^ seq_xor);
    q.tx_sec.push_back(s.t_sec[i]);
    q.tx_usec.push_back(s.t_usec[i]);
    q.rx_sec.push_back((uint32_t)(rx / 1000000));
    q.rx_usec.push_back((uint32_t)(rx % 1000000));
    rcv.push_back(k);
  };
  for (uint32_t k = 0; k < n_rcv; k++) {
    const uint32_t from = k == 1 ? 2500 : 0, to = k == 3 ? 7000 : ns;
    for (uint32_t i = from; i < to; i++) {
      if (rnd() % 50 == 0) continue;                  // lost on the way
      log_line(i, k, 0);
      if (k == 2 && rnd() % 40 == 0) log_line(i, k, 0);         // logged twice
      if (rnd() % 500 == 0) log_line(i, k, 0x40000000u);        // nobody sent this one
    }
  }
  log_line(5, n_rcv, 0);  // a receiver out of range
  const uint32_t nr = (uint32_t)rcv.size();

  const int64_t t0 = t_first + 100000;
  const uint64_t width = 110000;  // the windows end before the log does
  MessageMatchMulti mm(ctx, n_flows, n_rcv);
  mm.RunSeries(s, q, rcv, t0, width, n_bins);
  const auto cells = mm.Cells();
  const auto fan = mm.Fanout();
  const auto st = mm.Stats();
  const auto mask = mm.SendMask();
  const auto rs = mm.RecvSend();
  const auto first = mm.RecvFirst();
  const auto bins = mm.Bins();
  const auto outside = mm.Outside();
  CHECK(cells.size() == n_flows * n_rcv && fan.size() == n_flows && mask.size() == ns);
  CHECK(rs.size() == nr && first.size() == nr && bins.size() == n_flows * n_bins);

  // ---- the serial loop ----
  typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Id;
  std::map<Id, uint32_t> owner;
  std::vector<std::vector<uint32_t>> owners(n_flows);
  std::vector<MessageMatchMulti::FlowFanout> wf(n_flows);
  MessageMatchMulti::MatchStats ws = {};
  for (auto& f : wf) f = {};
  for (uint32_t i = 0; i < ns; i++) {
    const uint32_t f = s.flow_idx[i];
    if (f >= n_flows) {
      ws.send_skipped++;
      continue;
    }
    if (!owner.emplace(Id(f, s.seq[i], s.t_sec[i], s.t_usec[i]), i).second) {
      ws.send_dup++;
      wf[f].send_dup++;
    } else {
      owners[f].push_back(i);
    }
  }
  std::vector<uint64_t> wmask(ns, 0);
  std::vector<MessageMatchMulti::Cell> wc(n_flows * n_rcv);
  for (auto& c : wc) {
    c = {};
    c.first_send = c.last_send = MGENX_MATCH_NONE;
    c.lat_min = INT64_MAX;
    c.lat_max = INT64_MIN;
  }
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> arrival;
  for (uint32_t j = 0; j < nr; j++) {
    const uint32_t f = q.flow_idx[j], k = rcv[j];
    uint32_t o = MGENX_MATCH_NONE;
    uint8_t is_first = 0;
    if (f >= n_flows || k >= n_rcv) {
      ws.recv_skipped++;
    } else {
      auto it = owner.find(Id(f, q.seq[j], q.tx_sec[j], q.tx_usec[j]));
      auto& c = wc[f * n_rcv + k];
      if (it == owner.end()) {
        ws.recv_unmatched++;
        c.rx_orphan++;
      } else {
        o = it->second;
        if (arrival.emplace(std::make_pair(o, k), j).second) {
          is_first = 1;
          wmask[o] |= 1ull << k;
          const int64_t lat = ((int64_t)q.rx_sec[j] - (int64_t)s.t_sec[o]) * 1000000 +
                              (int64_t)q.rx_usec[j] - (int64_t)s.t_usec[o];
          c.delivered++;
          c.delivered_bytes += s.len[o];
          c.lat_sum += lat;
          c.lat_min = std::min(c.lat_min, lat);
          c.lat_max = std::max(c.lat_max, lat);
        } else {
          c.rx_dup++;
        }
      }
    }
    CHECK(rs[j] == o);
    CHECK(first[j] == is_first);
  }
  std::vector<MessageMatchMulti::Bin> wb(n_flows * n_bins);
  for (auto& b : wb) {
    b = {};
    b.reach_min = UINT64_MAX;
  }
  std::vector<uint64_t> wout(n_flows, 0);
  for (uint32_t f = 0; f < n_flows; f++) {
    wf[f].sent = owners[f].size();
    for (uint32_t k = 0; k < n_rcv; k++) wc[f * n_rcv + k].lost_head = wf[f].sent;
    for (uint32_t rank = 0; rank < owners[f].size(); rank++) {
      const uint32_t i = owners[f][rank];
      const uint32_t pc = (uint32_t)__builtin_popcountll(wmask[i]);
      wf[f].sent_bytes += s.len[i];
      wf[f].deliveries += pc;
      wf[f].reached_all += pc == n_rcv;
      wf[f].reach_hist[pc]++;
      for (uint32_t k = 0; k < n_rcv; k++) {
        if (!((wmask[i] >> k) & 1)) continue;
        auto& c = wc[f * n_rcv + k];
        if (c.first_send == MGENX_MATCH_NONE) {
          c.first_send = i;
          c.lost_head = rank;
        }
        c.last_send = i;
        c.lost_tail = wf[f].sent - 1 - rank;
      }
      const int64_t d = (int64_t)s.t_sec[i] * 1000000 + s.t_usec[i] - t0;
      if (d < 0 || (uint64_t)d / width >= n_bins) {
        wout[f]++;
        continue;
      }
      auto& b = wb[f * n_bins + (uint64_t)d / width];
      b.sent++;
      b.sent_bytes += s.len[i];
      b.deliveries += pc;
      b.delivered_bytes += (uint64_t)s.len[i] * pc;
      b.reached_any += pc > 0;
      b.reached_all += pc == n_rcv;
      b.reach_min = std::min<uint64_t>(b.reach_min, pc);
      b.reach_max = std::max<uint64_t>(b.reach_max, pc);
    }
  }

  for (uint32_t i = 0; i < ns; i++) CHECK(mask[i] == wmask[i]);
  for (uint32_t c = 0; c < n_flows * n_rcv; c++) {
    const auto &g = cells[c], &w = wc[c];
    CHECK(g.delivered == w.delivered && g.delivered_bytes == w.delivered_bytes);
    CHECK(g.rx_dup == w.rx_dup && g.rx_orphan == w.rx_orphan);
    CHECK(g.lost_head == w.lost_head && g.lost_tail == w.lost_tail);
    CHECK(g.first_send == w.first_send && g.last_send == w.last_send);
    CHECK(g.lat_sum == w.lat_sum && g.lat_min == w.lat_min && g.lat_max == w.lat_max);
  }
  for (uint32_t f = 0; f < n_flows; f++) {
    const auto &g = fan[f], &w = wf[f];
    CHECK(g.sent == w.sent && g.sent_bytes == w.sent_bytes && g.send_dup == w.send_dup);
    CHECK(g.deliveries == w.deliveries && g.reached_all == w.reached_all);
    for (uint32_t k = 0; k < 65; k++) CHECK(g.reach_hist[k] == w.reach_hist[k]);
    CHECK(outside[f] == wout[f]);
  }
  for (uint32_t c = 0; c < n_flows * n_bins; c++) {
    const auto &g = bins[c], &w = wb[c];
    CHECK(g.sent == w.sent && g.sent_bytes == w.sent_bytes && g.deliveries == w.deliveries);
    CHECK(g.delivered_bytes == w.delivered_bytes && g.reached_any == w.reached_any);
    CHECK(g.reached_all == w.reached_all && g.reach_min == w.reach_min);
    CHECK(g.reach_max == w.reach_max);
  }
  CHECK(st.send_skipped == ws.send_skipped && st.recv_skipped == ws.recv_skipped);
  CHECK(st.recv_unmatched == ws.recv_unmatched && st.send_dup == ws.send_dup);
  // the case is what it claims to be
  CHECK(ws.send_dup > 5 && ws.send_skipped > 5 && ws.recv_unmatched > 20 && ws.recv_skipped > 20);
  CHECK(wc[1].lost_head > 1000 && wc[3].lost_tail > 500 && wc[2].rx_dup > 50);
  CHECK(wf[0].reached_all > 100 && wf[0].reach_hist[3] > 100 && wout[0] > 100);

  // Run without the series on the same object: the same cells
  mm.Run(s, q, rcv);
  const auto again = mm.Cells();
  for (uint32_t c = 0; c < n_flows * n_rcv; c++)
    CHECK(again[c].delivered == wc[c].delivered && again[c].lost_head == wc[c].lost_head);
  CHECK(mm.Bins().empty() && mm.Outside().empty());

  std::printf("msg_match_multi_host ok: %u sent, %u received at %u receivers, %" PRIu64
              " deliveries in flow 0\n", ns, nr, n_rcv, fan[0].deliveries);
  return 0;
}
