"""No GPU: the serial model of the windowed latency percentiles (tests/flow_quant_ref.py) on the
hand-worked case, its rank rule, the table of mgen_amd.series with and without the percentile
columns, the parsing of -q, the C entry's argument errors, and the product's rank / tier
arithmetic (mgenx_flowquant.hpp) as a stand-alone program under the sanitizers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as D  # noqa: E402
import flow_quant_ref as Q  # noqa: E402
import flow_series_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "flow_quant_arith_host")


def test_hand_worked_case():
    nf, fi, c = D.hand_case()
    lo, hi = S.span(nf, fi, c)
    got = Q.model(nf, 1, fi, c, lo, hi - lo + 1, [1, 500, 950, 990, 999, 1000])
    assert got.dtype == np.int64 and got.shape == (3, 1, 6)
    assert got[0, 0].tolist() == [50, 200, 999050, 999050, 999050, 999050]
    assert got[1, 0].tolist() == [-50, 1100] + [4900000000] * 4       # negative; above 2**32
    assert got[2, 0].tolist() == [70] * 6
    # records outside the windows and the two skipped records belong to no cell
    sizes = {}
    out = Q.model(nf, 2000, fi, c, 1_000_000_420, 500, Q.PERMILLE, sizes=sizes)
    assert sizes == {(0, 0): 1, (0, 1): 2, (1, 0): 1, (0, 1999): 2}
    assert int((out != Q.I64_MIN).sum()) == 4 * len(Q.PERMILLE)
    assert out[0, 1].tolist() == [50, 50, 50, 200, 200, 200, 200]


def test_rank_rule():
    for q in (1, 2, 499, 500, 501, 999, 1000):
        for n in (1, 2, 3, 999, 1000, 1001, 2001, 10**6 + 1, 2**31 - 1):
            assert Q.rank(q, n) == D.rank(q, n) and 1 <= Q.rank(q, n) <= n
    assert Q.rank(1, 1000) == 1 and Q.rank(1, 1001) == 2
    assert Q.rank(1000, 7) == 7 and Q.rank(500, 2) == 1 and Q.rank(501, 2) == 2


def test_signed_floor_of_the_window():
    """A record just before t0 falls in window -1, not in window 0."""
    c = Q.cols_for_lat([999_999, 1_000_000, 1_000_999, 1_001_000], [5, 6, 7, 8])
    fi = np.zeros(4, np.uint32)
    assert Q.model(1, 2, fi, c, 1_000_000, 1000, [1, 1000])[0].tolist() == [[6, 7], [8, 8]]


def test_generators_cover_what_they_promise():
    nf, fi, c, t0, width, n_bins, what = Q.value_domain()
    assert (c["tx_usec"] >= 10**6).any() and nf == len(what) == 9
    sizes = Q.ladder_sizes([8, 256, 2048, 16384])
    assert len(sizes) == len(set(sizes)) == 157 and sum(sizes) == 265_795
    assert all(s in sizes for e in (8, 256, 2048, 16384) for s in (e - 1, e, e + 1))
    assert Q.ladder_sizes([300]) == sizes + [299, 300, 301]


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


def _bins():
    _, bins = S.fresh(2, 3)
    bins[0, 0] = (2, 200, 30, 10, 20, 10, 2, 2, 0)
    bins[0, 2] = (1, 100, -7, -7, -7, 27, 3, 1, 0)
    bins[1, 1] = (3, 300, 2**33 + 3, 1, 2**33, 5, 3, 3, 1)
    return bins


OLD = ("# flow>1 src>10.0.0.1/5001 dst>10.0.0.9/5000\n"
       "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum\n"
       "1000 2 200 2 0 2 10 20 30 10\n"
       "1100 1 100 1 0 3 -7 -7 -7 27\n"
       "\n\n"
       "# flow>2 src>10.0.0.2/5001 dst>10.0.0.9/5000\n"
       "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum\n"
       "1050 3 300 3 1 3 1 8589934592 8589934595 5\n")


def test_format_series_without_quantiles_is_unchanged():
    from mgen_amd.series import format_series
    assert format_series(_keys(2), _bins(), 1000, 50) == OLD
    assert format_series(_keys(2), _bins(), 1000, 50, None, (500,)) == OLD


def test_format_series_with_quantiles():
    from mgen_amd.series import format_series
    quant = np.full((2, 3, 2), Q.I64_MIN, np.int64)
    quant[0, 0] = (10, 20)
    quant[0, 2] = (-7, -7)
    quant[1, 1] = (1, 2**33)
    text = format_series(_keys(2), _bins(), 1000, 50, quant, (500, 990))
    assert text == (
        "# flow>1 src>10.0.0.1/5001 dst>10.0.0.9/5000\n"
        "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum "
        "lat_p500 lat_p990\n"
        "1000 2 200 2 0 2 10 20 30 10 10 20\n"
        "1100 1 100 1 0 3 -7 -7 -7 27 -7 -7\n"
        "\n\n"
        "# flow>2 src>10.0.0.2/5001 dst>10.0.0.9/5000\n"
        "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum "
        "lat_p500 lat_p990\n"
        "1050 3 300 3 1 3 1 8589934592 8589934595 5 1 8589934592\n")
    assert str(Q.I64_MIN) not in text


def test_q_option_parsing(capsys):
    from mgen_amd import series
    assert series.parse_permille("500,950,990") == (500, 950, 990)
    assert series.parse_permille("1") == (1,) and series.parse_permille("1000,1") == (1000, 1)
    assert len(series.parse_permille(",".join(["7"] * 32))) == 32
    for bad in ("", "0", "1001", "500,", ",500", "50.5", "-5", "p50", "500 950", "1e2",
                ",".join(["7"] * 33)):
        with pytest.raises(ValueError):
            series.parse_permille(bad)
    # the command line: a bad or missing list ends before any file is opened
    for argv in (["-q", "0", "no.log", "1"], ["no.log", "1", "-q"], ["no.log", "-q", "5,x", "1"],
                 ["-q", "5", "no.log"], ["-q", "5", "-q", "6", "no.log", "1"]):
        assert series.main(argv) == 2
    assert "usage" in capsys.readouterr().err


def test_capi_rejects_bad_arguments_without_gpu():
    import mgen_amd
    lib = mgen_amd.load()
    q = (ctypes.c_uint32 * 2)(500, 990)
    assert lib.mgenx_flow_series_quantiles(None, None, None, None, None, None, 0, 0, 1000, 4, 2, q,
                                           2, None, None) == -1


def test_rank_and_tier_arithmetic_under_sanitizers():
    if not os.path.exists(HOST):      # as the other tests/cpp programs: built on demand
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/flow_quant_arith_host"], check=True)
    r = subprocess.run([HOST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]        # a sanitizer report exits non-zero
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert "flow_quant_arith_host ok" in r.stdout


def test_gpu_tests_tier_edges_are_the_products():
    """TIER_EDGES of test_gpu_flow_quant.py restates the four constants of mgenx_flowquant.hpp."""
    with open(os.path.join(ROOT, "mgen_amd", "csrc", "mgenx_flowquant.hpp")) as fh:
        hpp = fh.read()
    edges = [int(re.search(r"constexpr uint32_t %s = (\d+);" % name, hpp).group(1))
             for name in ("kTinyMax", "kWaveMax", "kGroupMax", "kWideMax")]
    with open(os.path.join(ROOT, "tests", "test_gpu_flow_quant.py")) as fh:
        listed = re.search(r"^TIER_EDGES = \[([0-9, ]+)\]$", fh.read(), re.M).group(1)
    assert [int(v) for v in listed.split(",")] == edges == sorted(edges)
