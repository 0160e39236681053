"""Per-flow clock offset and skew of an MGEN receiver log as a table.

    python -m mgen_amd.clock <log> [offset]

reads a text log or a binary log (`type=binary_log`: the helper tells them apart by the header
line and ingests a binary log with mgenx_binlog_parse, so this tool needs no option for it), fits
on the GPU (analyze_text_log_clock: mgenx_flow_clock), per flow, the
straight line that lies under every (send time, latency) point and is closest to the points --
the receiver clock's offset and skew plus the minimum path delay (Moon, Skelly, Towsley, INFOCOM
1999) -- and prints one row per flow:

    flow src dst n t_a_us lat_a_us t_b_us lat_b_us skew_ppb resid_mean resid_max

(t_a_us, lat_a_us) and (t_b_us, lat_b_us) are the two records the line passes through: the ends
of the lower hull's edge over the mean send time (one point twice when the flow has one send
time, or with `offset`).  skew_ppb = floor(10^9 (lat_b - lat_a) / (t_b - t_a)), parts per
billion of the sender's clock ("-" where the line has no slope to speak of: one point).
resid_mean = floor(resid_sum / n) and resid_max describe the latency above the line, in
microseconds ("-" for a flow without records).  `offset` forces the slope to 0
(MGENX_CLOCK_OFFSET_ONLY): the line is the flow's lowest latency.
"""
from __future__ import annotations

import sys

from .series import _addr

COLUMNS = ("flow", "src", "dst", "n", "t_a_us", "lat_a_us", "t_b_us", "lat_b_us", "skew_ppb",
           "resid_mean", "resid_max")


def skew_ppb(e):
    """floor(10^9 (db - da) / (xb - xa)) of one FLOW_CLOCK_DTYPE element as a Python integer;
    None for an empty flow or a line through one point."""
    xa, xb = int(e["xa"]), int(e["xb"])
    if int(e["n"]) == 0 or xa == xb:
        return None
    return 10**9 * (int(e["db"]) - int(e["da"])) // (xb - xa)


def format_clock(keys, clock) -> str:
    """The table described above.  keys: REPORT_KEY_DTYPE [n_flows]; clock: FLOW_CLOCK_DTYPE
    [n_flows].  Integers only: no value passes through a float."""
    lines = ["# " + " ".join(COLUMNS)]
    for f in range(len(keys)):
        k, e = keys[f], clock[f]
        n = int(e["n"])
        if n:
            s = skew_ppb(e)
            vals = (str(int(e["xa"])), str(int(e["da"])), str(int(e["xb"])), str(int(e["db"])),
                    "-" if s is None else str(s), str(int(e["resid_sum"]) // n),
                    str(int(e["resid_max"])))
        else:
            vals = ("-",) * 7
        lines.append(" ".join((str(int(k["flow_id"])), _addr(k["src"]), _addr(k["dst"]),
                               str(n)) + vals))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) not in (1, 2) or (len(argv) == 2 and argv[1] != "offset"):
        sys.stderr.write("usage: python -m mgen_amd.clock <log> [offset]\n")
        return 2
    from . import analyze_text_log_clock
    with open(argv[0], "rb") as fh:
        log = fh.read()
    keys, clock, n_lines, n_bad = analyze_text_log_clock(log, offset_only=len(argv) == 2)
    sys.stdout.write(format_clock(keys, clock))
    sys.stderr.write("clock: %d lines, %d malformed, %d flows\n" % (n_lines, n_bad, len(keys)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
