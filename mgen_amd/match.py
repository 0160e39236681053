"""A sender's log joined with a receiver's log: exact per-flow loss as a table.

    python -m mgen_amd.match <send.log> <recv.log> [notime]

reads the sender's text log (SEND lines: `TXLOG`) and the receiver's (RECV lines), joins them on
the GPU (match_text_logs: mgenx_msg_match) and prints one row per flow:

    flow dst sent delivered lost lost_head lost_tail rx_dup orphans loss_runs longest_run
        lat_mean lat_min lat_max

lost = sent - delivered is exact; lost_head + lost_tail is the part that no receiver-only
analysis can see.  Latencies are microseconds ("-" while nothing was delivered); the mean is the
floor of lat_sum / delivered.  `notime` joins on (flow, seq) alone (MGENX_MATCH_NO_TIME): for
SINK-sent logs, whose SEND stamp is the wall clock, and for logs whose time-stamp styles differ.

Either log may be a binary log (`type=binary_log`): match_text_logs tells them apart by the header
line and ingests a binary log with mgenx_binlog_parse, so this tool needs no option for it.  A
binary SEND record holds no source port; with a binary sender's log the flows are keyed without
it, so flows that differ only in source port merge.
"""
from __future__ import annotations

import sys

from .series import _addr

COLUMNS = ("flow", "dst", "sent", "delivered", "lost", "lost_head", "lost_tail", "rx_dup",
           "orphans", "loss_runs", "longest_run", "lat_mean", "lat_min", "lat_max")


def format_match(keys, flows) -> str:
    """The table described above.  keys: REPORT_KEY_DTYPE [n_flows]; flows: FLOW_MATCH_DTYPE
    [n_flows].  Integers only: no value passes through a float."""
    lines = ["# " + " ".join(COLUMNS)]
    for f in range(len(keys)):
        k, e = keys[f], flows[f]
        sent, dlv = int(e["sent"]), int(e["delivered"])
        if dlv:
            lat = (str(int(e["lat_sum"]) // dlv), str(int(e["lat_min"])), str(int(e["lat_max"])))
        else:
            lat = ("-", "-", "-")
        lines.append(" ".join((
            str(int(k["flow_id"])), _addr(k["dst"]), str(sent), str(dlv), str(sent - dlv),
            str(int(e["lost_head"])), str(int(e["lost_tail"])), str(int(e["rx_dup"])),
            str(int(e["rx_orphan"])), str(int(e["loss_runs"])), str(int(e["loss_run_max"]))) + lat))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) not in (2, 3) or (len(argv) == 3 and argv[2] != "notime"):
        sys.stderr.write("usage: python -m mgen_amd.match <send.log> <recv.log> [notime]\n")
        return 2
    from . import match_text_logs
    with open(argv[0], "rb") as fh:
        send = fh.read()
    with open(argv[1], "rb") as fh:
        recv = fh.read()
    keys, flows, stats, _cnt, _first, _rs, n_send_flows = match_text_logs(
        send, recv, no_time=len(argv) == 3)
    sys.stdout.write(format_match(keys, flows))
    sys.stderr.write("match: %d flows (%d in the sender's log), %d receiver lines without a SEND "
                     "line, %d repeated SEND lines\n" % (
                         len(keys), n_send_flows, int(stats["recv_unmatched"]),
                         int(stats["send_dup"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
