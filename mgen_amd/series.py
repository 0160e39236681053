"""Per-flow time series of an MGEN receiver log as a table to plot.

    python -m mgen_amd.series <log> <width_sec> [outfile]

reads a text log, reduces it on the GPU (analyze_text_log_series: mgenx_flow_series, one time
axis for all flows) and writes, per flow, a comment line and one row per non-empty window:

    # flow>1 src>10.0.0.1/5001 dst>10.0.0.9/5000
    bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum

Two blank lines separate the flows, which is what gnuplot takes as the boundary of indexed data
sets (`plot "f" index 2 using ($1/1e6):($3*8/width)`).  The columns are the integers of struct
mgenx_flow_series_bin: rate = bytes / width, loss as seen in the window = advance - fresh, taken
back later = late, mean latency = lat_sum / n, mean jitter = jitter_sum / n.
"""
from __future__ import annotations

import ipaddress
import sys

COLUMNS = ("bin_start_us", "n", "bytes", "fresh", "late", "advance", "lat_min", "lat_max",
           "lat_sum", "jitter_sum")


def _addr(a) -> str:
    n = int(a["len"])
    raw = bytes(bytearray(int(x) for x in a["addr"][:n]))
    if n == 4:
        host = ".".join(str(x) for x in raw)
    elif n == 16:
        host = str(ipaddress.IPv6Address(raw))
    else:
        host = raw.hex() or "-"
    return "%s/%d" % (host, int(a["port"]))


def format_series(keys, bins, t0_us, width_us) -> str:
    """The table described above.  keys: REPORT_KEY_DTYPE [n_flows]; bins: FLOW_SERIES_BIN_DTYPE
    [n_flows, n_bins].  Integers only: no value passes through a float."""
    t0_us, width_us = int(t0_us), int(width_us)
    out = []
    for f in range(len(keys)):
        k = keys[f]
        lines = ["# flow>%d src>%s dst>%s" % (int(k["flow_id"]), _addr(k["src"]), _addr(k["dst"])),
                 "# " + " ".join(COLUMNS)]
        row = bins[f]
        for b in range(len(row)):
            e = row[b]
            if int(e["n"]) == 0:
                continue
            lines.append(" ".join(str(v) for v in (
                t0_us + b * width_us, int(e["n"]), int(e["bytes"]), int(e["fresh"]),
                int(e["late"]), int(e["advance"]), int(e["lat_min"]), int(e["lat_max"]),
                int(e["lat_sum"]), int(e["jitter_sum"]))))
        out.append("\n".join(lines) + "\n")
    return "\n\n".join(out)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) not in (2, 3):
        sys.stderr.write("usage: python -m mgen_amd.series <log> <width_sec> [outfile]\n")
        return 2
    from fractions import Fraction
    width_us = int(Fraction(argv[1]) * 10**6)
    if width_us < 1:
        sys.stderr.write("series: the width must be at least one microsecond\n")
        return 2
    from . import analyze_text_log_series
    with open(argv[0], "rb") as fh:
        log = fh.read()
    keys, _state, bins, t0_us, n_lines, n_bad = analyze_text_log_series(log, width_us)
    text = format_series(keys, bins, t0_us, width_us)
    if len(argv) == 3:
        with open(argv[2], "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    sys.stderr.write("series: %d lines, %d malformed, %d flows, %d windows of %d us from %d\n" % (
        n_lines, n_bad, len(keys), bins.shape[1], width_us, t0_us))
    return 0


if __name__ == "__main__":
    sys.exit(main())
