"""No GPU: the serial model of the clock offset / skew fit (tests/flow_clock_ref.py) on the
hand-worked case and against a brute-force search of the objective, what its data sets promise,
the struct layout, the table of mgen_amd.clock, the parsing of series' -c, the C entry's argument
errors, and the product's exact arithmetic (mgenx_flowclock.hpp) as a stand-alone program under
the sanitizers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_clock_ref as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "flow_clock_arith_host")


def flow_points(nf, fi, c):
    x, d = C.points(c)
    per = [[] for _ in range(nf)]
    for i in range(len(fi)):
        if int(fi[i]) < nf:
            per[int(fi[i])].append((x[i], d[i]))
    return per


def test_hand_worked_case():
    """Flow 0, send times from 10^9 us: the points (0,10) (4,2) (10,8) (2,6) (4,2) (6,3) (8,4)
    (4,9).  Lower hull: (0,10) (4,2) (8,4) (10,8); (2,6) is collinear on its first edge, (6,3) on
    its second, (4,9) lies above (4,2).  Sum of x = 38 over 8 records: 8*4 <= 38 < 8*8, the edge
    (4,2)-(8,4), slope 1/2.  A is held by records 1 and 6.  Flow 1: (5,-3) and (5,7), one x.
    Record 4 is skipped, flow 2 is empty."""
    nf, fi, c = C.hand_case()
    b = 1_000_000_000
    assert C.lower_hull(flow_points(nf, fi, c)[0]) == [(b, 10), (b + 4, 2), (b + 8, 4), (b + 10, 8)]
    clock, resid, sec, usec = C.model(nf, fi, c)
    assert clock[0].tolist() == (8, b + 4, 2, b + 8, 4, 25, 10, 1, 9)
    assert clock[1].tolist() == (2, b + 5, -3, b + 5, -3, 10, 10, 2, 2)
    assert clock[2].tolist() == (0, 0, 0, 0, 0, 0, C.I64_MIN, C.NONE, C.NONE)
    # line(x) = 2 + floor((x - 4) / 2): 0 at x = 0, 1 at x = 2, 5 at x = 10
    assert resid.tolist() == [10, 0, 0, 3, C.I64_MIN, 5, 0, 0, 10, 0, 7]
    x, _ = C.points(c)
    for i in range(len(fi)):
        if i == 4:      # the skipped record keeps its stamp
            assert (sec[i], usec[i]) == (c["rx_sec"][i], c["rx_usec"][i])
        else:
            assert int(sec[i]) * 10**6 + int(usec[i]) == x[i] + int(resid[i])
    # offset only: the lowest d, the lowest x among those
    off = C.model(nf, fi, c, offset_only=True)
    assert off[0][0].tolist() == (8, b + 4, 2, b + 4, 2, 8 + 0 + 6 + 4 + 0 + 1 + 2 + 7, 8, 1, 1)
    assert off[0][1].tolist() == (2, b + 5, -3, b + 5, -3, 10, 10, 2, 2)


def test_model_minimises_the_objective():
    """Among all lines under every point the chosen edge has the least sum of d - line(x): every
    supporting pair tried with Fractions, on random flows of at most 14 points."""
    rng = np.random.default_rng(11)
    tried = sloped = 0
    for _ in range(400):
        m = int(rng.integers(1, 15))
        span = int(rng.choice([4, 12, 1000]))
        pts = list(zip(rng.integers(0, span, m).tolist(), rng.integers(-span, span, m).tolist()))
        a, b = C.fit(pts)
        best = C.brute_force(pts)
        if best is None:
            assert a == b == (pts[0][0], min(d for _, d in pts))
            continue
        assert a[0] < b[0]
        from fractions import Fraction
        slope = Fraction(b[1] - a[1], b[0] - a[0])
        gaps = [Fraction(d - a[1]) - slope * (x - a[0]) for x, d in pts]
        assert min(gaps) >= 0 and sum(gaps) == best
        tried += 1
        sloped += slope != 0
    assert tried > 300 and sloped > 200


def test_residuals_are_never_negative_and_zero_at_both_ends():
    for nf, fi, c in (C.grid_corpus(), C.tiny_flows(), C.ladder([5, 64])[:3]):
        for opt in (False, True):
            clock, resid, _, _ = C.model(nf, fi, c, offset_only=opt)
            live = np.asarray(fi) < nf
            assert (resid[live] >= 0).all() and (resid[~live] == C.I64_MIN).all()
            full = clock["n"] > 0
            assert (resid[clock["ia"][full]] == 0).all() and (resid[clock["ib"][full]] == 0).all()
            assert (clock["resid_max"][full] >= 0).all()


def test_corpora_cover_what_they_promise():
    nf, fi, c = C.grid_corpus()
    per = flow_points(nf, fi, c)
    assert nf == 2000 and all(1 <= len(p) <= 60 for p in per)
    assert int((fi == C.NONE).sum()) == 700 and int((fi == nf + 5).sum()) == 300
    count = {}
    for p in per:
        for k in C.classify(p):
            count[k] = count.get(k, 0) + 1
    for k in ("all_x_equal", "n1", "n2", "mean_on_vertex", "collinear_on_edge", "a_repeated",
              "negative", "positive", "zero", "one_line"):
        assert count.get(k, 0) >= 10, (k, count)
    # interleaved: no flow's records are contiguous in the input
    assert int((np.diff(fi.astype(np.int64)) != 0).sum()) > len(fi) * 9 // 10
    nf, fi, c = C.tiny_flows()
    sizes = np.bincount(fi[fi < nf], minlength=nf)
    assert nf == 3000 and set(sizes.tolist()) == {0, 1, 2, 3, 4, 5}
    nf, fi, c, names = C.value_domain()
    x, d = C.points(c)
    assert max(x) == (2**32 - 1) * 10**6 + 900_000 and min(x) == 0
    assert max(int(v) for v in c["tx_usec"]) == 2**32 - 1
    assert min(d) < -2**51 and max(d) > 2**51
    clock, resid, _, _ = C.model(nf, fi, c)
    step = clock[names["step"]]
    assert step["xb"] - step["xa"] == 1 and step["db"] - step["da"] > 2**51
    assert step["n"] * step["xa"] == sum(x[i] for i in range(len(fi)) if fi[i] == names["step"])
    far = clock[names["step_far"]]
    assert far["xb"] - far["xa"] == 1 and far["n"] == 5002
    assert 5000 * int(far["db"] - far["da"]) > 2**63          # the residual that wraps
    nf, fi, c = C.parabola(1)
    clock = C.model(nf, fi, c)[0]
    assert clock[0]["n"] == 50_000 and clock[0]["db"] > clock[0]["da"]     # mean right of the vertex
    clock = C.model(*C.parabola(9))[0]
    assert clock[0]["db"] < clock[0]["da"] and clock[0]["xb"] - clock[0]["xa"] == 1


def test_struct_layout_matches_header(tmp_path):
    from mgen_amd import CLOCK_NONE, CLOCK_OFFSET_ONLY, FLOW_CLOCK_DTYPE
    assert FLOW_CLOCK_DTYPE == C.CLOCK_DTYPE and CLOCK_NONE == C.NONE
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %u %u\\n", sizeof(struct mgenx_flow_clock), MGENX_CLOCK_NONE,'
             ' MGENX_CLOCK_OFFSET_ONLY);']
    for f in FLOW_CLOCK_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(struct mgenx_flow_clock, {f}));')
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [64, CLOCK_NONE, CLOCK_OFFSET_ONLY]
    for row in out[1:]:
        if row:
            name, off = row.split()
            assert FLOW_CLOCK_DTYPE.fields[name][1] == int(off), name


def _keys(n):
    from mgen_amd import REPORT_KEY_DTYPE
    keys = np.zeros(n, REPORT_KEY_DTYPE)
    for f in range(n):
        keys[f]["flow_id"] = f + 1
        for side, last, port in (("src", 1 + f, 5001), ("dst", 9, 5000)):
            keys[f][side]["len"] = 4
            keys[f][side]["addr"][:4] = (10, 0, 0, last)
            keys[f][side]["port"] = port
    return keys


def test_format_clock():
    from mgen_amd import FLOW_CLOCK_DTYPE
    from mgen_amd.clock import COLUMNS, format_clock, skew_ppb
    clock = np.zeros(4, FLOW_CLOCK_DTYPE)
    clock[0] = (8, 1_000_000, 2_500_100, 3_000_000, 2_500_180, 25, 10, 1, 9)     # +40 ppm
    clock[1] = (3, 7, -3, 10, -4, -7, 5, 2, 3)          # a negative slope that does not divide
    clock[2] = (0, 0, 0, 0, 0, 0, C.I64_MIN, C.NONE, C.NONE)
    clock[3] = (2, 5, -3, 5, -3, 10, 10, 2, 2)
    assert [skew_ppb(e) for e in clock] == [40_000, -333_333_334, None, None]
    assert format_clock(_keys(4), clock) == (
        "# " + " ".join(COLUMNS) + "\n"
        "1 10.0.0.1/5001 10.0.0.9/5000 8 1000000 2500100 3000000 2500180 40000 3 10\n"
        "2 10.0.0.2/5001 10.0.0.9/5000 3 7 -3 10 -4 -333333334 -3 5\n"
        "3 10.0.0.3/5001 10.0.0.9/5000 0 - - - - - - -\n"
        "4 10.0.0.4/5001 10.0.0.9/5000 2 5 -3 5 -3 - 5 10\n")
    assert " ".join(COLUMNS) == ("flow src dst n t_a_us lat_a_us t_b_us lat_b_us skew_ppb "
                                 "resid_mean resid_max")


def test_c_option_parsing(capsys):
    from mgen_amd import clock, series
    assert series.parse_clock("fit") == "fit" and series.parse_clock("offset") == "offset"
    for bad in ("", "Fit", "skew", "fit,offset", "1", None):
        with pytest.raises(ValueError):
            series.parse_clock(bad)
    # the command line: a bad or missing value ends before any file is opened
    for argv in (["-c", "both", "no.log", "1"], ["no.log", "1", "-c"], ["-c", "fit", "no.log"],
                 ["-c", "fit", "-c", "offset", "no.log", "1"], ["-c", "fit", "-q", "0", "no.log", "1"]):
        assert series.main(argv) == 2
    err = capsys.readouterr().err
    assert "usage" in err and "[-c fit|offset]" in err
    for argv in ([], ["a.log", "fit"], ["a.log", "offset", "x"]):
        assert clock.main(argv) == 2
    assert "usage" in capsys.readouterr().err
    # the analysis helpers refuse an unknown clock before they touch a device
    import mgen_amd
    for fn in (mgen_amd.analyze_text_log_dist, mgen_amd.analyze_text_log_series):
        with pytest.raises(ValueError):
            fn(b"", 1000, clock="skew") if fn is mgen_amd.analyze_text_log_series else \
                fn(b"", clock="skew")


def test_capi_rejects_bad_arguments_without_gpu():
    import mgen_amd
    lib, EINVAL = mgen_amd.load(), -1
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    cols = [p] * 5
    # a null context comes first: no HIP call is made, the pointers are never followed
    assert lib.mgenx_flow_clock(None, *cols, 4, 2, 0, p, None, None, None, None) == EINVAL
    assert lib.mgenx_flow_clock(None, None, None, None, None, None, 0, 0, 0, None, None, None, None,
                                None) == EINVAL


def test_exact_arithmetic_under_sanitizers():
    if not os.path.exists(HOST):      # as the other tests/cpp programs: built on demand
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/flow_clock_arith_host"], check=True)
    rng = np.random.default_rng(12)
    xmax = (2**32 - 1) * 10**6 + 2**32 - 1
    dmax = 2**52 - 1
    rows = []

    def pick(hi, lo=0):
        edge = [lo, lo + 1, hi - 1, hi, (lo + hi) // 2]
        if rng.random() < 0.4:
            return edge[int(rng.integers(0, len(edge)))]
        wide = int(rng.integers(0, 2**62)) * 2**62 + int(rng.integers(0, 2**62))     # 124 bits
        return lo + wide % (hi - lo + 1)

    for _ in range(600):
        ts, tu, rs, ru = (pick(2**32 - 1) for _ in range(4))
        rows.append("pt %d %d %d %d %d %d" % (ts, tu, rs, ru, ts * 10**6 + tu,
                                              (rs - ts) * 10**6 + ru - tu))
    for _ in range(1500):
        xl, xr = sorted((pick(xmax), pick(xmax)))
        if rng.random() < 0.3:
            xr = min(xl + int(rng.integers(1, 4)), xmax)
        dl, dr, d = (pick(dmax, -dmax) for _ in range(3))
        x = pick(xmax)
        rows.append("key %d %d %d %d %d %d %d" % (xl, dl, xr, dr, x, d,
                                                  (xr - xl) * (d - dl) - (dr - dl) * (x - xl)))
        want = dl if xl >= xr else dl + (dr - dl) * (x - xl) // (xr - xl)
        rows.append("line %d %d %d %d %d %d" % (xl, dl, xr, dr, x, C.wrap64(want)))
    for _ in range(600):
        n, x = pick(2**31 - 1, 1), pick(xmax)
        s = n * x + int(rng.integers(-2, 3)) if rng.random() < 0.5 else pick(n * xmax)
        s = max(s, 0)
        rows.append("left %d %d %d %d" % (n, x, s, n * x <= s))
    for _ in range(600):
        x, c = pick(xmax), pick(2**54)
        r = x + c
        rows.append("stamp %d %d %d %d" % (x, c, (r // 10**6) % 2**32, r % 10**6))
    # the corners of the domain: the largest x, d at +-(2^52 - 1), a step of 2^53 across one
    # microsecond, negative numerators with remainders
    rows.append("line %d %d %d %d %d %d" % (xmax - 1, -dmax, xmax, dmax, 0,
                                            C.wrap64(-dmax + 2 * dmax * (0 - (xmax - 1)))))
    rows.append("line 0 0 3 -7 1 -3")
    rows.append("line 0 %d %d %d %d %d" % (dmax, xmax, -dmax, xmax - 1,
                                           dmax + (-2 * dmax) * (xmax - 1) // xmax))
    rows.append("key 0 %d %d %d %d %d %d" % (-dmax, xmax, dmax, xmax, -dmax,
                                             xmax * 0 - 2 * dmax * xmax))
    r = subprocess.run([HOST], input="\n".join(rows) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]        # a sanitizer report exits non-zero
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert "flow_clock_arith_host ok" in r.stdout and "%d vectors" % len(rows) in r.stdout


def test_gpu_tests_tier_edges_are_the_products():
    """CLOCK_EDGES of test_gpu_flow_clock.py restates kClockEdges of mgenx_flowclock.hpp."""
    with open(os.path.join(ROOT, "mgen_amd", "csrc", "mgenx_flowclock.hpp")) as fh:
        hpp = fh.read()
    val = {name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, hpp).group(1))
           for name in ("kClockUnroll", "kClockWaveLanes", "kClockGroupLanes", "kClockWaveMax")}
    listed = re.search(r"constexpr uint32_t kClockEdges\[\] = \{([^}]+)\};", hpp).group(1)
    edges = [eval(e.replace("\n", " "), {}, val) for e in listed.split(",")]
    with open(os.path.join(ROOT, "tests", "test_gpu_flow_clock.py")) as fh:
        mine = re.search(r"^CLOCK_EDGES = \[([0-9, ]+)\]$", fh.read(), re.M).group(1)
    assert [int(v) for v in mine.split(",")] == edges == sorted(edges)
    assert val["kClockWaveMax"] in edges and val["kClockWaveLanes"] in edges
    assert val["kClockGroupLanes"] in edges
