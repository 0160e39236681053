// C++ host-layer test of mgenx::MessageMatch (include/mgenx.hpp): about 9000 sent messages in 4
// flows, some repeated in the sender's log, some lost in bursts, some received twice, a few
// records of either side without a flow, against a serial loop over the same records.
// Prints "msg_match_host ok" and exits 0.
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

namespace {

struct Want {
  uint64_t sent = 0, sent_bytes = 0, send_dup = 0, delivered = 0, delivered_bytes = 0, rx_dup = 0,
           rx_orphan = 0, lost_head = 0, lost_tail = 0, runs = 0, run_max = 0, hist[18] = {};
  int64_t lsum = 0, lmin = INT64_MAX, lmax = INT64_MIN;
  uint64_t run = 0;  // the undelivered owners since the last delivered one
  bool any = false;
  void Close() {
    runs++;
    run_max = std::max(run_max, run);
    uint32_t k = 0;
    while ((run >> (k + 1)) && k < 17) k++;
    hist[k]++;
  }
};

}  // namespace

int main() {
  using namespace mgenx;
  const uint32_t ns = 9001, n_flows = 4;
  Context ctx(0);
  uint64_t r = 97531;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };

  MessageMatch::SendColumns s;
  std::vector<bool> lost(ns, false);
  uint32_t next[n_flows] = {0, 0, 0, 0}, burst = 0;
  for (uint32_t i = 0; i < ns; i++) {
    const uint32_t f = rnd() % 9 < 5 ? 0 : 1 + rnd() % 3;  // flow 0 dominates
    const int64_t t = 1700000000ll * 1000000 + 999000 + (int64_t)i * 211;
    if (i > 100 && rnd() % 300 == 0) {  // the line of an earlier message again
      const uint32_t j = i - 1 - rnd() % 100;
      s.flow_idx.push_back(s.flow_idx[j]);
      s.seq.push_back(s.seq[j]);
      s.t_sec.push_back(s.t_sec[j]);
      s.t_usec.push_back(s.t_usec[j]);
      s.len.push_back(s.len[j]);
      lost[i] = true;  // (what happens to the message is decided at its first line)
      continue;
    }
    s.flow_idx.push_back(i % 700 == 699 ? MGENX_FLOW_NONE : f);
    s.seq.push_back(next[f]++);
    s.t_sec.push_back((uint32_t)(t / 1000000));
    s.t_usec.push_back((uint32_t)(t % 1000000));
    s.len.push_back(28 + rnd() % 70000);
    if (!burst && rnd() % 60 == 0) burst = 1 + rnd() % 40;
    if (i < 40 || i > ns - 30) burst = burst ? burst : 1;  // the head and the tail are lost
    if (burst) {
      lost[i] = true;
      burst--;
    }
  }
  MessageMatch::RecvColumns rc;
  auto receive = [&](uint32_t i, uint32_t flow) {
    const int64_t rx = (int64_t)s.t_sec[i] * 1000000 + s.t_usec[i] + (int64_t)(rnd() % 4000) - 500;
    rc.flow_idx.push_back(flow);
    rc.seq.push_back(s.seq[i]);
    rc.tx_sec.push_back(s.t_sec[i]);
    rc.tx_usec.push_back(s.t_usec[i]);
    rc.rx_sec.push_back((uint32_t)(rx / 1000000));
    rc.rx_usec.push_back((uint32_t)(rx % 1000000));
  };
  for (uint32_t i = 0; i < ns; i++) {
    if (lost[i]) continue;
    receive(i, rnd() % 800 == 0 ? n_flows : s.flow_idx[i]);  // (a few with no flow)
    if (rnd() % 50 == 0) receive(i >= 7 ? i - 7 : i, s.flow_idx[i >= 7 ? i - 7 : i]);
    if (rnd() % 400 == 0) {  // a message the sender never logged
      receive(i, s.flow_idx[i]);
      rc.seq.back() += 1000000;
    }
  }
  const uint32_t nr = (uint32_t)rc.flow_idx.size();

  // the serial walk
  typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Ident;
  std::map<Ident, uint32_t> owner;
  std::vector<uint32_t> cnt(ns, 0), first(ns, MGENX_MATCH_NONE), rs(nr, MGENX_MATCH_NONE);
  std::vector<bool> is_owner(ns, false);
  std::vector<Want> w(n_flows);
  uint64_t send_skipped = 0, recv_skipped = 0, unmatched = 0, dups = 0;
  for (uint32_t i = 0; i < ns; i++) {
    if (s.flow_idx[i] >= n_flows) {
      send_skipped++;
      continue;
    }
    const Ident id(s.flow_idx[i], s.seq[i], s.t_sec[i], s.t_usec[i]);
    if (owner.count(id)) {
      w[s.flow_idx[i]].send_dup++;
      dups++;
    } else {
      owner[id] = i;
      is_owner[i] = true;
    }
  }
  for (uint32_t j = 0; j < nr; j++) {
    if (rc.flow_idx[j] >= n_flows) {
      recv_skipped++;
      continue;
    }
    auto it = owner.find(Ident(rc.flow_idx[j], rc.seq[j], rc.tx_sec[j], rc.tx_usec[j]));
    if (it == owner.end()) {
      unmatched++;
      w[rc.flow_idx[j]].rx_orphan++;
      continue;
    }
    rs[j] = it->second;
    if (!cnt[it->second]++) first[it->second] = j;
  }
  for (uint32_t i = 0; i < ns; i++) {
    if (!is_owner[i]) continue;
    Want& f = w[s.flow_idx[i]];
    f.sent++;
    f.sent_bytes += s.len[i];
    if (!cnt[i]) {
      f.run++;
      continue;
    }
    if (f.run) {
      f.Close();
      if (!f.any) f.lost_head = f.run;
    }
    f.run = 0;
    f.any = true;
    f.delivered++;
    f.delivered_bytes += s.len[i];
    f.rx_dup += cnt[i] - 1;
    const uint32_t j = first[i];
    const int64_t lat = ((int64_t)rc.rx_sec[j] - (int64_t)s.t_sec[i]) * 1000000 +
                        (int64_t)rc.rx_usec[j] - (int64_t)s.t_usec[i];
    f.lsum += lat;
    f.lmin = std::min(f.lmin, lat);
    f.lmax = std::max(f.lmax, lat);
  }
  for (Want& f : w) {
    if (!f.run) continue;
    f.Close();
    (f.any ? f.lost_tail : f.lost_head) = f.run;
  }

  MessageMatch mm(ctx, n_flows);
  mm.Run(s, rc);
  const std::vector<MessageMatch::Flow> g = mm.Flows();
  const MessageMatch::Stats st = mm.GetStats();
  CHECK(mm.SendRxCount() == cnt && mm.SendFirstRx() == first && mm.RecvSend() == rs);
  CHECK(st.send_skipped == send_skipped && st.recv_skipped == recv_skipped);
  CHECK(st.recv_unmatched == unmatched && st.send_dup == dups);
  uint64_t lost_total = 0, runs = 0, rx_dup = 0;
  for (uint32_t f = 0; f < n_flows; f++) {
    CHECK(g[f].sent == w[f].sent && g[f].sent_bytes == w[f].sent_bytes);
    CHECK(g[f].send_dup == w[f].send_dup && g[f].delivered == w[f].delivered);
    CHECK(g[f].delivered_bytes == w[f].delivered_bytes && g[f].rx_dup == w[f].rx_dup);
    CHECK(g[f].rx_orphan == w[f].rx_orphan && g[f].lost_head == w[f].lost_head);
    CHECK(g[f].lost_tail == w[f].lost_tail && g[f].loss_runs == w[f].runs);
    CHECK(g[f].loss_run_max == w[f].run_max);
    for (int k = 0; k < 18; k++) CHECK(g[f].loss_run_hist[k] == w[f].hist[k]);
    CHECK(g[f].lat_sum == w[f].lsum && g[f].lat_min == w[f].lmin && g[f].lat_max == w[f].lmax);
    lost_total += g[f].sent - g[f].delivered;
    runs += g[f].loss_runs;
    rx_dup += g[f].rx_dup;
  }
  CHECK(lost_total > 1000 && runs > 50 && rx_dup > 50 && dups > 10 && unmatched > 5);
  CHECK(send_skipped > 5 && recv_skipped > 2 && g[0].lost_head > 10 && g[0].sent > g[1].sent);

  // an empty receiver log: everything is lost, one run per flow
  MessageMatch none(ctx, n_flows);
  none.Run(s, MessageMatch::RecvColumns());
  for (const MessageMatch::Flow& f : none.Flows())
    CHECK(f.delivered == 0 && f.lost_head == f.sent && f.loss_runs == 1 && f.lat_min == INT64_MAX);
  std::printf("msg_match_host ok: %" PRIu64 " of %u lost in %" PRIu64 " runs, %" PRIu64
              " received again, %" PRIu64 " repeated SEND lines\n", lost_total, ns, runs, rx_dup,
              dups);
  return 0;
}
