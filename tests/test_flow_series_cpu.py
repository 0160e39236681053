"""mgenx_flow_series without a GPU: the serial model (tests/flow_series_ref.py) on a case worked
by hand and against the whole-run model of flow_dist_ref, the ABI layout and argument checks, and
format_series on a hand-made array."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as D  # noqa: E402
import flow_series_ref as S  # noqa: E402

# hand_case with windows of 500 us from 1000.000420 s, 2000 of them: the first records of flows 0
# and 2 fall before the first window, the last two of flow 1 (rx 5000 s) after the last
T0, WIDTH, NBINS = 1_000_000_420, 500, 2000
EMPTY = dict(n=0, bytes=0, lat_sum=0, lat_min=2**63 - 1, lat_max=-2**63, jitter_sum=0, advance=0,
             fresh=0, late=0)
HAND_STATE = {   # worked out by hand from the definitions
    0: dict(n=6, last_lat=64, outside=1, seq_max=20, rsv=0),
    1: dict(n=3, last_lat=1100, outside=2, seq_max=6, rsv=0),
    2: dict(n=1, last_lat=70, outside=1, seq_max=7, rsv=0),
}
HAND_BINS = {
    # flow 0: seq 10 (before the first window) | 12 | 11, 12 | ... | 3, 20
    (0, 0): dict(n=1, bytes=100, lat_sum=700, lat_min=700, lat_max=700, jitter_sum=400,
                 advance=2, fresh=1, late=0),
    (0, 1): dict(n=2, bytes=200, lat_sum=250, lat_min=50, lat_max=200, jitter_sum=650,
                 advance=0, fresh=0, late=1),
    (0, 1999): dict(n=2, bytes=200, lat_sum=999114, lat_min=64, lat_max=999050,
                    jitter_sum=1997986, advance=8, fresh=1, late=1),
    # flow 1: its first record, with a negative latency
    (1, 0): dict(n=1, bytes=64, lat_sum=-50, lat_min=-50, lat_max=-50, jitter_sum=0, advance=1,
                 fresh=1, late=0),
}


def test_model_on_the_hand_case():
    nf, fi, c = D.hand_case()
    state, bins = S.model(nf, NBINS, fi, c, T0, WIDTH)
    for f, want in HAND_STATE.items():
        assert {k: int(state[f][k]) for k in want} == want, f
    for f in range(nf):
        for b in range(NBINS):
            want = HAND_BINS.get((f, b), EMPTY)
            assert {k: int(bins[f, b][k]) for k in want} == want, (f, b)
    # streaming: any cut leaves the same bytes
    for cut in (1, 5, 8, 11):
        s2, b2 = S.fresh(nf, NBINS)
        S.update(s2, b2, fi[:cut], {k: v[:cut] for k, v in c.items()}, T0, WIDTH)
        S.update(s2, b2, fi[cut:], {k: v[cut:] for k, v in c.items()}, T0, WIDTH)
        assert s2.tobytes() == state.tobytes() and b2.tobytes() == bins.tobytes()
    # a negative t0 and a window that covers everything: nothing outside
    s3, b3 = S.model(nf, 1, fi, c, -5, 2**62)
    assert s3["outside"].tolist() == [0, 0, 0] and b3["n"][:, 0].tolist() == [6, 3, 1]
    assert b3["advance"][:, 0].tolist() == [11, 2, 1] and b3["late"][:, 0].tolist() == [2, 0, 0]


@pytest.mark.parametrize("data", [D.hand_case, D.tiny_flows, D.one_flow_every_97th, S.shuffled_rx])
def test_one_bin_equals_the_whole_run_model(data):
    nf, fi, c = data()
    lo, hi = S.span(nf, fi, c)
    state, bins = S.model(nf, 1, fi, c, lo, hi - lo + 1)
    dist, _ = D.model(nf, fi, c)
    assert not state["outside"].any()
    one = bins[:, 0]
    for name in ("n", "bytes", "lat_sum", "lat_min", "lat_max", "jitter_sum"):
        assert np.array_equal(one[name], dist[name]), name
    assert np.array_equal(one["late"], dist["reordered"])
    assert np.array_equal(state["n"], dist["n"]) and np.array_equal(state["seq_max"], dist["seq_max"])
    assert np.array_equal(state["last_lat"], dist["last_lat"])
    for f in np.nonzero(dist["n"])[0]:
        first = int(c["seq"][np.nonzero(np.asarray(fi) == f)[0][0]])
        assert int(one["advance"][f]) == int(dist["seq_max"][f]) - first + 1, f


def test_shuffled_rx_is_what_it_says():
    nf, fi, c = S.shuffled_rx()
    assert nf == 4 and len(fi) == 8000
    rx = S.rx_us(c)
    for f in range(4):
        b = (rx[fi == f] - rx.min()) // 10_000
        assert (np.diff(b) < 0).sum() > 10           # the bins of a flow are not contiguous


def test_layout_matches_header_and_symbols(tmp_path):
    import mgen_amd
    from mgen_amd import FLOW_SERIES_BIN_DTYPE, FLOW_SERIES_STATE_DTYPE
    for s in ("mgenx_flow_series_init", "mgenx_flow_series"):
        assert s in mgen_amd.EXPORTED_SYMBOLS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %zu %d\\n", sizeof(struct mgenx_flow_series_bin), '
             'sizeof(struct mgenx_flow_series_state), MGENX_ABI_VERSION);']
    for st, dt in (("bin", FLOW_SERIES_BIN_DTYPE), ("state", FLOW_SERIES_STATE_DTYPE)):
        for f in dt.names:
            lines.append(f'printf("{st} {f} %zu\\n", offsetof(struct mgenx_flow_series_{st}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["64", "32", "1"]
    assert FLOW_SERIES_BIN_DTYPE.itemsize == 64 == S.BIN.itemsize
    assert FLOW_SERIES_STATE_DTYPE.itemsize == 32 == S.STATE.itemsize
    mine = {"bin": (FLOW_SERIES_BIN_DTYPE, S.BIN), "state": (FLOW_SERIES_STATE_DTYPE, S.STATE)}
    seen = 0
    for line in out[1:]:
        if line:
            st, name, off = line.split()
            assert mine[st][0].fields[name][1] == int(off) == mine[st][1].fields[name][1], line
            seen += 1
    assert seen == len(S.BIN.names) + len(S.STATE.names)


def test_bad_arguments_are_rejected_without_hip():
    from mgen_amd import load
    L = load()
    one = ctypes.c_void_p(16)     # a non-null pointer that is never followed
    cols = (one,) * 7
    assert L.mgenx_flow_series_init(None, one, one, 4, 4, None) == -1
    assert L.mgenx_flow_series(None, *cols, 8, 0, 1000, 4, one, one, 4, None) == -1


def test_format_series_on_a_hand_made_array():
    from mgen_amd import FLOW_SERIES_BIN_DTYPE, REPORT_KEY_DTYPE
    from mgen_amd.series import format_series
    keys = np.zeros(2, REPORT_KEY_DTYPE)
    for f, (fid, host) in enumerate(((7, 1), (4000000000, 2))):
        keys[f]["flow_id"] = fid
        for side, port in (("src", 5001), ("dst", 5000)):
            keys[f][side]["len"] = 4
            keys[f][side]["port"] = port
            keys[f][side]["addr"][:4] = (10, 0, 0, host if side == "src" else 9)
    keys[1]["dst"]["len"] = 16
    keys[1]["dst"]["addr"][:] = [0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1]
    bins, _ = np.zeros((2, 3), FLOW_SERIES_BIN_DTYPE), None
    bins["lat_min"] = 2**63 - 1
    bins["lat_max"] = -2**63
    bins[0, 0] = (2, 2048, 3 * 2**53 + 1, -5, 3 * 2**53, 2**64 - 1, 4, 2, 0)
    bins[0, 2] = (1, 64, 70, 70, 70, 10, 0, 0, 1)
    bins[1, 1] = (1, 28, -30, -30, -30, 0, 1, 1, 0)
    text = format_series(keys, bins, -1500, 1000)
    assert text == (
        "# flow>7 src>10.0.0.1/5001 dst>10.0.0.9/5000\n"
        "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum\n"
        "-1500 2 2048 2 0 4 -5 27021597764222976 27021597764222977 18446744073709551615\n"
        "500 1 64 0 1 0 70 70 70 10\n"
        "\n\n"
        "# flow>4000000000 src>10.0.0.2/5001 dst>2001:db8::1/5000\n"
        "# bin_start_us n bytes fresh late advance lat_min lat_max lat_sum jitter_sum\n"
        "-500 1 28 1 0 1 -30 -30 -30 0\n")
    assert format_series(keys[:0], bins[:0], 0, 1) == ""
