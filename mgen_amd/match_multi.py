"""One sender's log joined with the logs of several receivers: the delivery matrix of a
multicast run.

    python -m mgen_amd.match_multi [-n] [-w WIDTH_SEC] <send.log> <recv1.log> [<recv2.log> ...]

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
"""
from __future__ import annotations

import sys

from .series import _addr

CELL_COLUMNS = ("flow", "dst", "rcv", "sent", "delivered", "lost", "lost_head", "lost_tail",
                "rx_dup", "orphans", "lat_min", "lat_mean", "lat_max")
SERIES_COLUMNS = ("bin_start_us", "sent", "reached_any", "reached_all", "delivery_ratio")


def _ratio(num: int, den: int) -> str:
    """num / den with six decimals, cut; "-" for an empty denominator."""
    if den == 0:
        return "-"
    q = num * 10**6 // den
    return "%d.%06d" % (q // 10**6, q % 10**6)


def format_cells(keys, cells, fanout) -> str:
    """One row per (flow, receiver).  keys: REPORT_KEY_DTYPE [n_flows]; cells: RCV_CELL_DTYPE
    [n_flows, n_rcv]; fanout: FLOW_FANOUT_DTYPE [n_flows].  Integers only."""
    lines = ["# " + " ".join(CELL_COLUMNS)]
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
            lines.append(" ".join((
                str(int(k["flow_id"])), _addr(k["dst"]), str(r), str(sent), str(dlv),
                str(sent - dlv), str(int(e["lost_head"])), str(int(e["lost_tail"])),
                str(int(e["rx_dup"])), str(int(e["rx_orphan"]))) + lat))
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
    usage = ("usage: python -m mgen_amd.match_multi [-n] [-w WIDTH_SEC] <send.log> <recv1.log> "
             "[<recv2.log> ...]\n")
    no_time, width_us = False, None
    while argv and argv[0] in ("-n", "-w"):
        if argv[0] == "-n":
            no_time = True
            del argv[0]
            continue
        if len(argv) < 2:
            sys.stderr.write(usage)
            return 2
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
    res = match_text_logs_multi(logs[0], logs[1:], width_us=width_us, no_time=no_time)
    keys, cells, fanout, stats, _mask, n_send_flows = res[:6]
    sys.stdout.write(format_cells(keys, cells, fanout))
    sys.stdout.write("\n" + format_reach(keys, fanout, n_rcv))
    if width_us is not None:
        bins, _outside, t0_us = res[6:]
        sys.stdout.write("\n\n" + format_multi_series(keys, bins, t0_us, width_us, n_rcv))
    sys.stderr.write("match_multi: %d flows (%d in the sender's log), %d receivers, %d receiver "
                     "lines without a SEND line, %d repeated SEND lines\n" % (
                         len(keys), n_send_flows, n_rcv, int(stats["recv_unmatched"]),
                         int(stats["send_dup"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
