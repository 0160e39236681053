// C++ host-layer test of mgenx::MessageMatch::RunTimeline (include/mgenx.hpp): about 9000 sent
// messages in 4 flows, some repeated in the sender's log, some lost in bursts, some received
// twice, a few records without a flow, against a serial loop over the same records: the series
// per window of send time, the list of loss runs and the owner column.
// Prints "match_timeline_host ok" and exits 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

typedef mgenx::MessageMatch::Bin Bin;
typedef mgenx::MessageMatch::LossRun LossRun;

Bin EmptyBin() {
  Bin b;
  std::memset(&b, 0, sizeof(b));
  b.lat_min = INT64_MAX;
  b.lat_max = INT64_MIN;
  return b;
}

}  // namespace

int main() {
  using namespace mgenx;
  const uint32_t ns = 9001, n_flows = 4, n_bins = 6, min_run = 3;
  const int64_t t_first = 1700000000ll * 1000000 + 999000;
  const int64_t t0 = t_first + 150000;  // the first 150 ms and the last part lie outside
  const uint64_t width = 250000;
  Context ctx(0);
  uint64_t r = 24680;
  auto rnd = [&]() { return (uint32_t)((r = r * 6364136223846793005ull + 1442695040888963407ull) >> 33); };

  MessageMatch::SendColumns s;
  std::vector<bool> lost(ns, false);
  uint32_t next[n_flows] = {0, 0, 0, 0}, burst = 0;
  for (uint32_t i = 0; i < ns; i++) {
    const uint32_t f = rnd() % 9 < 5 ? 0 : 1 + rnd() % 3;  // flow 0 dominates
    const int64_t t = t_first + (int64_t)i * 211;
    if (i > 100 && rnd() % 200 == 0) {  // the line of an earlier message again
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
  auto receive = [&](uint32_t i) {
    const int64_t rx = (int64_t)s.t_sec[i] * 1000000 + s.t_usec[i] + (int64_t)(rnd() % 4000) - 500;
    rc.flow_idx.push_back(s.flow_idx[i]);
    rc.seq.push_back(s.seq[i]);
    rc.tx_sec.push_back(s.t_sec[i]);
    rc.tx_usec.push_back(s.t_usec[i]);
    rc.rx_sec.push_back((uint32_t)(rx / 1000000));
    rc.rx_usec.push_back((uint32_t)(rx % 1000000));
  };
  for (uint32_t i = 0; i < ns; i++) {
    if (lost[i]) continue;
    receive(i);
    if (rnd() % 50 == 0) receive(i >= 7 ? i - 7 : i);
  }
  const uint32_t nr = (uint32_t)rc.flow_idx.size();

  // the serial walk: owners, what arrived of them, then per flow the windows and the runs
  typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Ident;
  std::map<Ident, uint32_t> owner;
  std::vector<uint32_t> own(ns, MGENX_MATCH_NONE), cnt(ns, 0), first(ns, MGENX_MATCH_NONE);
  for (uint32_t i = 0; i < ns; i++) {
    if (s.flow_idx[i] >= n_flows) continue;
    own[i] = owner.emplace(Ident(s.flow_idx[i], s.seq[i], s.t_sec[i], s.t_usec[i]), i).first->second;
  }
  for (uint32_t j = 0; j < nr; j++) {
    if (rc.flow_idx[j] >= n_flows) continue;
    auto it = owner.find(Ident(rc.flow_idx[j], rc.seq[j], rc.tx_sec[j], rc.tx_usec[j]));
    if (it == owner.end()) continue;
    if (!cnt[it->second]++) first[it->second] = j;
  }
  std::vector<Bin> bins((size_t)n_flows * n_bins, EmptyBin());
  std::vector<uint64_t> outside(n_flows, 0);
  std::vector<LossRun> runs;
  auto stamp = [&](uint32_t i) { return (int64_t)s.t_sec[i] * 1000000 + (int64_t)s.t_usec[i]; };
  for (uint32_t f = 0; f < n_flows; f++) {
    std::vector<uint32_t> cur;
    bool delivered_before = false;
    auto close = [&](bool tail) {
      if (cur.size() >= min_run) {
        LossRun q;
        std::memset(&q, 0, sizeof(q));
        q.flow_idx = f;
        q.length = (uint32_t)cur.size();
        q.first_send = cur.front();
        q.last_send = cur.back();
        q.flags = (delivered_before ? 0 : MGENX_RUN_HEAD) | (tail ? MGENX_RUN_TAIL : 0);
        q.t_first_us = stamp(cur.front());
        q.t_last_us = stamp(cur.back());
        runs.push_back(q);
      }
      cur.clear();
    };
    for (uint32_t i = 0; i < ns; i++) {
      if (own[i] != i || s.flow_idx[i] != f) continue;
      const int64_t d = stamp(i) - t0;
      const int64_t b = d >= 0 ? d / (int64_t)width : -1;
      if (b < 0 || b >= (int64_t)n_bins) {
        outside[f]++;
      } else {
        Bin& c = bins[(size_t)f * n_bins + b];
        c.sent++;
        c.sent_bytes += s.len[i];
        if (cnt[i]) {
          const uint32_t j = first[i];
          const int64_t lat = (int64_t)rc.rx_sec[j] * 1000000 + (int64_t)rc.rx_usec[j] - stamp(i);
          c.delivered++;
          c.delivered_bytes += s.len[i];
          c.rx_dup += cnt[i] - 1;
          c.lat_sum += lat;
          c.lat_min = std::min(c.lat_min, lat);
          c.lat_max = std::max(c.lat_max, lat);
        }
      }
      if (!cnt[i]) {
        cur.push_back(i);
      } else {
        close(false);
        delivered_before = true;
      }
    }
    close(true);
  }

  MessageMatch mm(ctx, n_flows);
  mm.RunTimeline(s, rc, t0, width, n_bins, min_run);
  CHECK(mm.SendOwner() == own && mm.SendRxCount() == cnt && mm.SendFirstRx() == first);
  CHECK(mm.Outside() == outside);
  const std::vector<Bin> gb = mm.Bins();
  CHECK(gb.size() == bins.size());
  CHECK(std::memcmp(gb.data(), bins.data(), bins.size() * sizeof(Bin)) == 0);
  const std::vector<LossRun> gr = mm.Runs();
  CHECK(gr.size() == runs.size() && runs.size() > 20);
  CHECK(std::memcmp(gr.data(), runs.data(), runs.size() * sizeof(LossRun)) == 0);
  uint64_t in_bins = 0, out = 0, head = 0, tail = 0;
  for (const Bin& b : gb) in_bins += b.sent;
  for (uint64_t o : outside) out += o;
  for (const LossRun& q : gr) {
    head += (q.flags & MGENX_RUN_HEAD) != 0;
    tail += (q.flags & MGENX_RUN_TAIL) != 0;
  }
  const std::vector<MessageMatch::Flow> g = mm.Flows();
  uint64_t sent = 0;
  for (const MessageMatch::Flow& f : g) sent += f.sent;
  CHECK(in_bins + out == sent && in_bins > 5000 && out > 500 && head >= 1 && tail >= 1);

  // the same object again without a run list worth keeping, then Run: its results are unchanged
  mm.RunTimeline(s, rc, t0, width, 0, 100000);
  CHECK(mm.Runs().empty() && mm.Bins().empty() && mm.Outside().empty() && mm.SendOwner() == own);
  mm.Run(s, rc);
  const std::vector<MessageMatch::Flow> g2 = mm.Flows();
  CHECK(std::memcmp(g.data(), g2.data(), g.size() * sizeof(g[0])) == 0);
  std::printf("match_timeline_host ok: %" PRIu64 " messages in %u windows per flow, %" PRIu64
              " outside, %zu runs of at least %u\n", in_bins, n_bins, out, runs.size(), min_run);
  return 0;
}
