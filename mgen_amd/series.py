"""Per-flow time series of an MGEN receiver log as a table to plot.

    python -m mgen_amd.series [-q 500,950,990] [-c fit|offset] <log> <width_sec> [outfile]

reads a text log or a binary log (`type=binary_log`: the helper tells them apart by the header
line and ingests a binary log with mgenx_binlog_parse, so this tool needs no option for it),
reduces it on the GPU (analyze_text_log_series: mgenx_flow_series, one time axis for all flows)
and writes, per flow, a comment line and one row per non-empty window:

    # flow>1 src>10.0.0.1/5001 dst>10.0.0.9/5000
    bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum

Two blank lines separate the flows, which is what gnuplot takes as the boundary of indexed data
sets (`plot "f" index 2 using ($1/1e6):($3*8/width)`).  The columns are the integers of struct
mgenx_flow_series_bin: rate = bytes / width, loss as seen in the window = advance - fresh, taken
back later = late, mean latency = lat_sum / n, mean jitter = jitter_sum / n.

-q takes a comma-separated list of permille values in 1..1000 (at most 32), before or after the
positional arguments, and appends one column per value, lat_p500 lat_p950 lat_p990 for the list
above: the window's exact latency percentiles (mgenx_flow_series_quantiles, the rank rule of
mgenx_flow_dist_quantiles).  Rows exist only for non-empty windows, so every value is a latency.

-c fit (or -c offset), likewise before or after the positional arguments, removes each flow's
clock offset and skew (or its offset alone) first (mgenx_flow_clock): the time axis is then the
sender's clock and every latency column the delay above the flow's fitted line.
"""
from __future__ import annotations

import ipaddress
import sys

MAX_Q = 32   # MGENX_FLOW_SERIES_MAX_Q
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


def parse_permille(text) -> tuple:
    """The argument of -q: "500,950,990" -> (500, 950, 990).  ValueError for an empty list, more
    than MAX_Q values, anything that is not a decimal integer, or a value outside 1..1000."""
    parts = str(text).split(",")
    if not 1 <= len(parts) <= MAX_Q:
        raise ValueError("-q takes 1 to %d permille values" % MAX_Q)
    out = []
    for p in parts:
        if not (p.isascii() and p.isdigit()):
            raise ValueError("-q: %r is not a permille value" % p)
        v = int(p)
        if not 1 <= v <= 1000:
            raise ValueError("-q: %d is outside 1..1000" % v)
        out.append(v)
    return tuple(out)


def parse_clock(text) -> str:
    """The argument of -c: "fit" or "offset".  ValueError for anything else."""
    if text not in ("fit", "offset"):
        raise ValueError("-c takes fit or offset, not %r" % (text,))
    return text


def format_series(keys, bins, t0_us, width_us, quant=None, permille=()) -> str:
    """The table described above.  keys: REPORT_KEY_DTYPE [n_flows]; bins: FLOW_SERIES_BIN_DTYPE
    [n_flows, n_bins]; quant: None, or int64 [n_flows, n_bins, len(permille)] for the columns
    lat_p<permille>.  Integers only: no value passes through a float."""
    t0_us, width_us = int(t0_us), int(width_us)
    columns = COLUMNS
    if quant is not None:
        columns = COLUMNS + tuple("lat_p%d" % int(q) for q in permille)
    out = []
    for f in range(len(keys)):
        k = keys[f]
        lines = ["# flow>%d src>%s dst>%s" % (int(k["flow_id"]), _addr(k["src"]), _addr(k["dst"])),
                 "# " + " ".join(columns)]
        row = bins[f]
        for b in range(len(row)):
            e = row[b]
            if int(e["n"]) == 0:
                continue
            vals = (t0_us + b * width_us, int(e["n"]), int(e["bytes"]), int(e["fresh"]),
                    int(e["late"]), int(e["advance"]), int(e["lat_min"]), int(e["lat_max"]),
                    int(e["lat_sum"]), int(e["jitter_sum"]))
            if quant is not None:
                vals += tuple(int(quant[f][b][j]) for j in range(len(permille)))
            lines.append(" ".join(str(v) for v in vals))
        out.append("\n".join(lines) + "\n")
    return "\n\n".join(out)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = ("usage: python -m mgen_amd.series [-q 500,950,990] [-c fit|offset] <log> <width_sec> "
             "[outfile]\n")
    permille = None
    clock = None
    if "-c" in argv:
        at = argv.index("-c")
        if at + 1 >= len(argv) or "-c" in argv[at + 2:]:
            sys.stderr.write(usage)
            return 2
        try:
            clock = parse_clock(argv[at + 1])
        except ValueError as e:
            sys.stderr.write("series: %s\n" % e)
            return 2
        del argv[at:at + 2]
    if "-q" in argv:
        at = argv.index("-q")
        if at + 1 >= len(argv) or "-q" in argv[at + 2:]:
            sys.stderr.write(usage)
            return 2
        try:
            permille = parse_permille(argv[at + 1])
        except ValueError as e:
            sys.stderr.write("series: %s\n" % e)
            return 2
        del argv[at:at + 2]
    if len(argv) not in (2, 3):
        sys.stderr.write(usage)
        return 2
    from fractions import Fraction
    width_us = int(Fraction(argv[1]) * 10**6)
    if width_us < 1:
        sys.stderr.write("series: the width must be at least one microsecond\n")
        return 2
    from . import analyze_text_log_series
    with open(argv[0], "rb") as fh:
        log = fh.read()
    kw = {} if clock is None else {"clock": clock}
    if permille is None:
        keys, _state, bins, t0_us, n_lines, n_bad = analyze_text_log_series(log, width_us, **kw)
        text = format_series(keys, bins, t0_us, width_us)
    else:
        keys, _state, bins, t0_us, n_lines, n_bad, quant = analyze_text_log_series(
            log, width_us, permille=permille, **kw)
        text = format_series(keys, bins, t0_us, width_us, quant, permille)
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
