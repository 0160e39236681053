// C++ host-layer test of mgenx::MessageMatchMulti::RunLoss (include/mgenx.hpp) on a case small
// enough to work out by hand: one flow of 12 messages (send records 0 .. 12; record 6 repeats
// record 5's line, so the owners are records 0 .. 5 and 7 .. 12, ranks 0 .. 11) and 3 receivers.
//   receiver 0 misses ranks 4 5 and 9;
//   receiver 1 misses exactly what receiver 0 does;
//   receiver 2 joins late (its first message is rank 3) and misses ranks 5 and 7.
// Runs: receivers 0 and 1 have {4 5} and {9}; receiver 2 has the head {0 1 2}, {5} and {7}.
// Pairs: the spans are 0 .. 11, 0 .. 11 and 3 .. 11.  (0, 1): 12 messages, each lost 3, both 3.
// (0, 2) over ranks 3 .. 11: 9 messages, receiver 0 lost 4 5 9, receiver 2 lost 5 7, both 5.
// Prints "msg_match_multi_ex_host ok" and exits 0.
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
  const uint32_t n_msg = 12, n_rcv = 3, T = 1700000000u;
  Context ctx(0);
  // rank k is send record k (k < 6) or k + 1: record 6 is a send duplicate of record 5
  auto rec_of = [](uint32_t rank) { return rank < 6 ? rank : rank + 1; };
  MessageMatchMulti::SendColumns s;
  for (uint32_t k = 0; k < n_msg; k++) {
    s.flow_idx.push_back(0);
    s.seq.push_back(k);
    s.t_sec.push_back(T);
    s.t_usec.push_back(1000 * k);
    s.len.push_back(64);
    if (k == 5) {  // the same line again
      s.flow_idx.push_back(0);
      s.seq.push_back(k);
      s.t_sec.push_back(T);
      s.t_usec.push_back(1000 * k);
      s.len.push_back(64);
    }
  }
  MessageMatchMulti::RecvColumns q;
  std::vector<uint32_t> rcv;
  auto hears = [](uint32_t r, uint32_t k) {
    if (r < 2) return k != 4 && k != 5 && k != 9;
    return k >= 3 && k != 5 && k != 7;
  };
  for (uint32_t r = 0; r < n_rcv; r++)
    for (uint32_t k = 0; k < n_msg; k++) {
      if (!hears(r, k)) continue;
      q.flow_idx.push_back(0);
      q.seq.push_back(k);
      q.tx_sec.push_back(T);
      q.tx_usec.push_back(1000 * k);
      q.rx_sec.push_back(T);
      q.rx_usec.push_back(1000 * k + 300 + r);
      rcv.push_back(r);
    }

  MessageMatchMulti mm(ctx, 1, n_rcv);
  mm.RunLoss(s, q, rcv);
  const auto cells = mm.Cells();
  const auto stats = mm.RunStats();
  const auto runs = mm.LossRuns();
  const auto pairs = mm.Pairs();
  CHECK(cells.size() == 3 && stats.size() == 3 && pairs.size() == 9);
  CHECK(mm.Fanout()[0].sent == n_msg && mm.Fanout()[0].send_dup == 1);
  CHECK(cells[2].lost_head == 3 && cells[0].lost_head == 0 && cells[2].first_send == 3);

  const uint64_t want_runs[3][2] = {{2, 2}, {2, 2}, {3, 3}};  // loss_runs, loss_run_max
  for (uint32_t r = 0; r < n_rcv; r++) {
    CHECK(stats[r].loss_runs == want_runs[r][0] && stats[r].loss_run_max == want_runs[r][1]);
    uint64_t sum = 0;
    for (int k = 0; k < 18; k++) sum += stats[r].loss_run_hist[k];
    CHECK(sum == stats[r].loss_runs);
  }
  CHECK(stats[0].loss_run_hist[0] == 1 && stats[0].loss_run_hist[1] == 1);
  CHECK(stats[2].loss_run_hist[0] == 2 && stats[2].loss_run_hist[1] == 1);

  // by flow, last_send, rcv: {rcv, length, first rank, last rank, flags}
  const uint32_t want_list[7][5] = {{2, 3, 0, 2, MGENX_RUN_HEAD}, {0, 2, 4, 5, 0}, {1, 2, 4, 5, 0},
                                    {2, 1, 5, 5, 0},              {2, 1, 7, 7, 0}, {0, 1, 9, 9, 0},
                                    {1, 1, 9, 9, 0}};
  CHECK(runs.size() == 7);
  for (size_t k = 0; k < runs.size(); k++) {
    const auto& g = runs[k];
    const uint32_t* w = want_list[k];
    CHECK(g.flow_idx == 0 && g.rcv == w[0] && g.length == w[1] && g.flags == w[4]);
    CHECK(g.first_send == rec_of(w[2]) && g.last_send == rec_of(w[3]));
    CHECK(g.t_first_us == (int64_t)T * 1000000 + 1000 * w[2]);
    CHECK(g.t_last_us == (int64_t)T * 1000000 + 1000 * w[3]);
  }

  const uint64_t want_pairs[3][3][4] = {  // span, lost_a, lost_b, lost_both
      {{12, 3, 3, 3}, {12, 3, 3, 3}, {9, 3, 2, 1}},
      {{12, 3, 3, 3}, {12, 3, 3, 3}, {9, 3, 2, 1}},
      {{9, 2, 3, 1}, {9, 2, 3, 1}, {9, 2, 2, 2}}};
  for (uint32_t a = 0; a < n_rcv; a++)
    for (uint32_t b = 0; b < n_rcv; b++) {
      const auto& g = pairs[a * n_rcv + b];
      const uint64_t* w = want_pairs[a][b];
      CHECK(g.span == w[0] && g.lost_a == w[1] && g.lost_b == w[2] && g.lost_both == w[3]);
    }

  // only the runs of two and more: the list shrinks, the statistics stay
  mm.RunLoss(s, q, rcv, 2);
  CHECK(mm.LossRuns().size() == 3 && mm.RunStats()[2].loss_runs == 3);
  // Run on the same object still gives the cells
  mm.Run(s, q, rcv);
  CHECK(mm.Cells()[2].lost_head == 3);

  std::printf("msg_match_multi_ex_host ok: %zu runs listed\n", runs.size());
  return 0;
}
