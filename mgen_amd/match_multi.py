"""One sender's log joined with the logs of several receivers: the delivery matrix of a
multicast run.

    python -m mgen_amd.match_multi [-n] [-w WIDTH_SEC] [-r MIN_RUN] [-p] <send.log> <recv1.log>
                                   [<recv2.log> ...]

reads the sender's log (SEND lines: `TXLOG`) and up to 64 receivers' logs (RECV lines), each a
text log or a binary log (told apart by the header line inside match_text_logs_multi: no option
here; with a binary sender's log the flows are keyed without the source port), joins them on the GPU (match_text_logs_multi: mgenx_msg_match_multi) and prints one row per
(flow, receiver), the receivers numbered from 0 in the order given:

    flow dst rcv sent delivered lost lost_head lost_tail rx_dup orphans lat_min lat_mean lat_max

lost = sent - delivered is exact; lost_head is what a late joiner missed, lost_tail what a
receiver that left early did.  Latencies are microseconds ("-" while nothing was delivered); the
mean is the floor of lat_sum / delivered.  Then per flow the reach histogram:

    flow dst sent reached_all all_ratio reach_0 reach_1 ... reach_<n_rcv>

reach_k = the messages that reached exactly k receivers; all_ratio = reached_all / sent.

With -w the table gnuplot reads follows, per flow a comment line and one row per window of send
time in which the flow sent something, two blank lines between the flows:

    bin_start_us sent reached_any reached_all delivery_ratio

delivery_ratio = deliveries / (sent * n_rcv), the packet delivery ratio of the window.  Ratios
are six decimals, cut not rounded, computed in integers.  -n joins on (flow, seq) alone
(MGENX_MATCH_NO_TIME).

With -r MIN_RUN (mgenx_msg_match_multi_ex) every (flow, receiver) row gains two columns,
`loss_runs longest_run`: the maximal runs of consecutive messages the receiver missed and the
longest of them.  After everything above comes the outage list, one row per run of at least
MIN_RUN messages, sorted by flow, receiver and first line:

    flow dst rcv length first_line last_line t_first_us t_last_us head tail

first_line and last_line are 1-based lines of the sender's log (the run's first and last lost
message), t_first_us / t_last_us their send stamps, head = 1 when nothing of the flow reached the
receiver before the run, tail = 1 when nothing did after it.

With -p the last table is the loss receivers share, per flow and ordered pair a != b:

    flow dst a b span lost_a lost_b lost_both cond

counted over the messages sent while both receivers were listening (from the later of their first
deliveries to the earlier of their last ones): span = those messages, lost_a / lost_b = what each
missed of them, lost_both = what both missed; cond = lost_both / lost_a, the share of a's losses
that b lost too ("-" when a lost nothing).  Receivers behind one lossy link show cond near 1 both
ways; independent last hops show cond near b's own loss rate.
"""
from __future__ import annotations

import sys

from .series import _addr

CELL_COLUMNS = ("flow", "dst", "rcv", "sent", "delivered", "lost", "lost_head", "lost_tail",
                "rx_dup", "orphans", "lat_min", "lat_mean", "lat_max")
RUN_COLUMNS = ("flow", "dst", "rcv", "length", "first_line", "last_line", "t_first_us",
               "t_last_us", "head", "tail")
PAIR_COLUMNS = ("flow", "dst", "a", "b", "span", "lost_a", "lost_b", "lost_both", "cond")
RUN_HEAD, RUN_TAIL = 1, 2     # MGENX_RUN_HEAD, MGENX_RUN_TAIL
SERIES_COLUMNS = ("bin_start_us", "sent", "reached_any", "reached_all", "delivery_ratio")


def _ratio(num: int, den: int) -> str:
    """num / den with six decimals, cut; "-" for an empty denominator."""
    if den == 0:
        return "-"
    q = num * 10**6 // den
    return "%d.%06d" % (q // 10**6, q % 10**6)


def format_cells(keys, cells, fanout, rcv_runs=None) -> str:
    """One row per (flow, receiver).  keys: REPORT_KEY_DTYPE [n_flows]; cells: RCV_CELL_DTYPE
    [n_flows, n_rcv]; fanout: FLOW_FANOUT_DTYPE [n_flows]; rcv_runs: None or RCV_RUNS_DTYPE
    [n_flows, n_rcv], which adds the columns loss_runs and longest_run.  Integers only."""
    cols = CELL_COLUMNS + (("loss_runs", "longest_run") if rcv_runs is not None else ())
    lines = ["# " + " ".join(cols)]
    for f in range(len(keys)):
        k, sent = keys[f], int(fanout[f]["sent"])
        for r in range(cells.shape[1]):
            e = cells[f, r]
            dlv = int(e["delivered"])
            if dlv:
                lat = (str(int(e["lat_min"])), str(int(e["lat_sum"]) // dlv),
                       str(int(e["lat_max"])))
            else:
                lat = ("-", "-", "-")
            more = ()
            if rcv_runs is not None:
                more = (str(int(rcv_runs[f, r]["loss_runs"])),
                        str(int(rcv_runs[f, r]["loss_run_max"])))
            lines.append(" ".join((
                str(int(k["flow_id"])), _addr(k["dst"]), str(r), str(sent), str(dlv),
                str(sent - dlv), str(int(e["lost_head"])), str(int(e["lost_tail"])),
                str(int(e["rx_dup"])), str(int(e["rx_orphan"]))) + lat + more))
    return "\n".join(lines) + "\n"


def format_outages(keys, runs) -> str:
    """The outage list described above.  keys: REPORT_KEY_DTYPE [n_flows]; runs:
    RCV_LOSS_RUN_DTYPE in any order.  Integers only."""
    lines = ["# " + " ".join(RUN_COLUMNS)]
    rows = sorted(runs, key=lambda r: (int(r["flow_idx"]), int(r["rcv"]), int(r["first_send"])))
    for r in rows:
        k = keys[int(r["flow_idx"])]
        flags = int(r["flags"])
        lines.append(" ".join((
            str(int(k["flow_id"])), _addr(k["dst"]), str(int(r["rcv"])), str(int(r["length"])),
            str(int(r["first_send"]) + 1), str(int(r["last_send"]) + 1),
            str(int(r["t_first_us"])), str(int(r["t_last_us"])),
            str(1 if flags & RUN_HEAD else 0), str(1 if flags & RUN_TAIL else 0))))
    return "\n".join(lines) + "\n"


def format_pairs(keys, pairs) -> str:
    """The shared loss per flow and ordered pair a != b.  keys: REPORT_KEY_DTYPE [n_flows];
    pairs: RCV_PAIR_DTYPE [n_flows, n_rcv, n_rcv].  Integers only."""
    lines = ["# " + " ".join(PAIR_COLUMNS)]
    for f in range(len(keys)):
        k = keys[f]
        n_rcv = pairs.shape[1]
        for a in range(n_rcv):
            for b in range(n_rcv):
                if a == b:
                    continue
                e = pairs[f, a, b]
                la, both = int(e["lost_a"]), int(e["lost_both"])
                lines.append(" ".join((
                    str(int(k["flow_id"])), _addr(k["dst"]), str(a), str(b), str(int(e["span"])),
                    str(la), str(int(e["lost_b"])), str(both), _ratio(both, la))))
    return "\n".join(lines) + "\n"


def format_reach(keys, fanout, n_rcv) -> str:
    """Per flow the reach histogram and reached_all / sent.  Integers only."""
    n_rcv = int(n_rcv)
    lines = ["# flow dst sent reached_all all_ratio " +
             " ".join("reach_%d" % k for k in range(n_rcv + 1))]
    for f in range(len(keys)):
        k, e = keys[f], fanout[f]
        sent, full = int(e["sent"]), int(e["reached_all"])
        lines.append(" ".join(
            [str(int(k["flow_id"])), _addr(k["dst"]), str(sent), str(full), _ratio(full, sent)] +
            [str(int(e["reach_hist"][j])) for j in range(n_rcv + 1)]))
    return "\n".join(lines) + "\n"


def format_multi_series(keys, bins, t0_us, width_us, n_rcv) -> str:
    """The table per window described above.  bins: MULTI_BIN_DTYPE [n_flows, n_bins]."""
    t0_us, width_us, n_rcv = int(t0_us), int(width_us), int(n_rcv)
    out = []
    for f in range(len(keys)):
        k = keys[f]
        lines = ["# flow>%d src>%s dst>%s" % (int(k["flow_id"]), _addr(k["src"]), _addr(k["dst"])),
                 "# " + " ".join(SERIES_COLUMNS)]
        row = bins[f]
        for b in range(len(row)):
            e = row[b]
            sent = int(e["sent"])
            if sent == 0:
                continue
            lines.append(" ".join((
                str(t0_us + b * width_us), str(sent), str(int(e["reached_any"])),
                str(int(e["reached_all"])), _ratio(int(e["deliveries"]), sent * n_rcv))))
        out.append("\n".join(lines) + "\n")
    return "\n\n".join(out)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = ("usage: python -m mgen_amd.match_multi [-n] [-w WIDTH_SEC] [-r MIN_RUN] [-p] "
             "<send.log> <recv1.log> [<recv2.log> ...]\n")
    no_time, width_us, min_run, want_pairs = False, None, None, False
    while argv and argv[0] in ("-n", "-w", "-r", "-p"):
        if argv[0] == "-n":
            no_time = True
            del argv[0]
            continue
        if argv[0] == "-p":
            want_pairs = True
            del argv[0]
            continue
        if len(argv) < 2:
            sys.stderr.write(usage)
            return 2
        if argv[0] == "-r":
            try:
                min_run = int(argv[1])
            except ValueError:
                sys.stderr.write(usage)
                return 2
            if not 0 <= min_run < 2**32:
                sys.stderr.write("match_multi: the shortest run listed is 0 to 2^32 - 1\n")
                return 2
            del argv[:2]
            continue
        from fractions import Fraction
        try:
            width_us = int(Fraction(argv[1]) * 10**6)
        except (ValueError, ZeroDivisionError):
            sys.stderr.write(usage)
            return 2
        if width_us < 1:
            sys.stderr.write("match_multi: the width must be at least one microsecond\n")
            return 2
        del argv[:2]
    if not 2 <= len(argv) <= 65:
        sys.stderr.write(usage)
        return 2
    from . import match_text_logs_multi
    logs = []
    for path in argv:
        with open(path, "rb") as fh:
            logs.append(fh.read())
    n_rcv = len(logs) - 1
    more = {}
    if min_run is not None:
        more["min_run"] = min_run
    if want_pairs:
        more["pairs"] = True
    res = match_text_logs_multi(logs[0], logs[1:], width_us=width_us, no_time=no_time, **more)
    keys, cells, fanout, stats, _mask, n_send_flows = res[:6]
    at = 9 if width_us is not None else 6
    rcv_runs = runs = None
    if min_run is not None:
        rcv_runs, runs = res[at:at + 2]
        at += 2
    sys.stdout.write(format_cells(keys, cells, fanout, rcv_runs))
    sys.stdout.write("\n" + format_reach(keys, fanout, n_rcv))
    if width_us is not None:
        bins, _outside, t0_us = res[6:9]
        sys.stdout.write("\n\n" + format_multi_series(keys, bins, t0_us, width_us, n_rcv))
    if runs is not None:
        sys.stdout.write("\n\n" + format_outages(keys, runs))
    if want_pairs:
        sys.stdout.write("\n\n" + format_pairs(keys, res[at]))
    sys.stderr.write("match_multi: %d flows (%d in the sender's log), %d receivers, %d receiver "
                     "lines without a SEND line, %d repeated SEND lines\n" % (
                         len(keys), n_send_flows, n_rcv, int(stats["recv_unmatched"]),
                         int(stats["send_dup"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
