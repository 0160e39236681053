"""A sender's log joined with a receiver's log on the sender's time axis: offered load, delivered
load and exact loss per window of send time, or the list of outages.

    python -m mgen_amd.match_series [-r MIN] <send.log> <recv.log> <width_sec> [notime]

reads the two logs as `python -m mgen_amd.match` does (text or binary, told apart by the header
line inside match_text_logs_timeline: no option here) and joins them on the GPU
(match_text_logs_timeline: mgenx_msg_match_ex).  Without -r it writes, per flow, a comment line
and one row per window of send time in which the flow sent something:

    # flow>1 src>-/5001 dst>10.0.0.9/5000
    bin_start_us sent sent_bytes delivered delivered_bytes lost rx_dup lat_min lat_max lat_sum

lost = sent - delivered of the messages *sent* in the window, wherever and whenever they were
received; the three latency columns read "-" while nothing sent in the window was delivered.
Two blank lines separate the flows (gnuplot's indexed data sets, as `python -m mgen_amd.series`).

With -r MIN it writes one row per run of at least MIN consecutive lost messages of a flow:

    flow dst length first_send_us last_send_us first_line last_line head tail

first_line and last_line are 1-based lines of the sender's log (the run's first and last lost
message), head = 1 when nothing of the flow was delivered before the run, tail = 1 when nothing
was after it.  `notime` joins on (flow, seq) alone (MGENX_MATCH_NO_TIME).
"""
from __future__ import annotations

import sys

from .series import _addr

COLUMNS = ("bin_start_us", "sent", "sent_bytes", "delivered", "delivered_bytes", "lost", "rx_dup",
           "lat_min", "lat_max", "lat_sum")
RUN_COLUMNS = ("flow", "dst", "length", "first_send_us", "last_send_us", "first_line", "last_line",
               "head", "tail")
RUN_HEAD, RUN_TAIL = 1, 2     # MGENX_RUN_HEAD, MGENX_RUN_TAIL


def format_match_series(keys, bins, t0_us, width_us) -> str:
    """The table per window described above.  keys: REPORT_KEY_DTYPE [n_flows]; bins:
    MATCH_BIN_DTYPE [n_flows, n_bins].  Integers only: no value passes through a float."""
    t0_us, width_us = int(t0_us), int(width_us)
    out = []
    for f in range(len(keys)):
        k = keys[f]
        lines = ["# flow>%d src>%s dst>%s" % (int(k["flow_id"]), _addr(k["src"]), _addr(k["dst"])),
                 "# " + " ".join(COLUMNS)]
        row = bins[f]
        for b in range(len(row)):
            e = row[b]
            sent, dlv = int(e["sent"]), int(e["delivered"])
            if sent == 0:
                continue
            if dlv:
                lat = (str(int(e["lat_min"])), str(int(e["lat_max"])), str(int(e["lat_sum"])))
            else:
                lat = ("-", "-", "-")
            lines.append(" ".join((
                str(t0_us + b * width_us), str(sent), str(int(e["sent_bytes"])), str(dlv),
                str(int(e["delivered_bytes"])), str(sent - dlv), str(int(e["rx_dup"]))) + lat))
        out.append("\n".join(lines) + "\n")
    return "\n\n".join(out)


def format_runs(keys, runs) -> str:
    """The list of runs described above.  keys: REPORT_KEY_DTYPE [n_flows]; runs: LOSS_RUN_DTYPE.
    Integers only."""
    lines = ["# " + " ".join(RUN_COLUMNS)]
    for r in runs:
        k = keys[int(r["flow_idx"])]
        flags = int(r["flags"])
        lines.append(" ".join((
            str(int(k["flow_id"])), _addr(k["dst"]), str(int(r["length"])),
            str(int(r["t_first_us"])), str(int(r["t_last_us"])), str(int(r["first_send"]) + 1),
            str(int(r["last_send"]) + 1), str(1 if flags & RUN_HEAD else 0),
            str(1 if flags & RUN_TAIL else 0))))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = ("usage: python -m mgen_amd.match_series [-r MIN] <send.log> <recv.log> <width_sec> "
             "[notime]\n")
    min_run = None
    if "-r" in argv:
        at = argv.index("-r")
        if at + 1 >= len(argv) or "-r" in argv[at + 2:]:
            sys.stderr.write(usage)
            return 2
        text = argv[at + 1]
        if not (text.isascii() and text.isdigit()) or not 1 <= int(text) < 2**32:
            sys.stderr.write("match_series: -r takes a number of messages, at least 1\n")
            return 2
        min_run = int(text)
        del argv[at:at + 2]
    if len(argv) not in (3, 4) or (len(argv) == 4 and argv[3] != "notime"):
        sys.stderr.write(usage)
        return 2
    from fractions import Fraction
    try:
        width_us = int(Fraction(argv[2]) * 10**6)
    except (ValueError, ZeroDivisionError):
        sys.stderr.write(usage)
        return 2
    if width_us < 1:
        sys.stderr.write("match_series: the width must be at least one microsecond\n")
        return 2
    from . import match_text_logs_timeline
    with open(argv[0], "rb") as fh:
        send = fh.read()
    with open(argv[1], "rb") as fh:
        recv = fh.read()
    keys, flows, stats, bins, outside, runs, t0_us, n_send_flows = match_text_logs_timeline(
        send, recv, width_us, min_run=min_run or 1, no_time=len(argv) == 4)
    if min_run is None:
        sys.stdout.write(format_match_series(keys, bins, t0_us, width_us))
    else:
        sys.stdout.write(format_runs(keys, runs))
    sys.stderr.write("match_series: %d flows (%d in the sender's log), %d windows of %d us from "
                     "%d, %d runs of at least %d lost messages\n" % (
                         len(keys), n_send_flows, bins.shape[1], width_us, t0_us, len(runs),
                         min_run or 1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
