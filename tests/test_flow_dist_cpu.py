"""mgenx_flow_dist without a GPU: the exported bin arithmetic, the ABI layout, argument checks,
and the serial model (tests/flow_dist_ref.py) on a hand-written case."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as R  # noqa: E402


def _values():
    v = list(range(0, 4097))
    for k in range(6, 33):
        v += [x for x in (2**k - 1, 2**k, 2**k + 1) if x < 2**32]
    v += [int(x) for x in np.random.default_rng(7).integers(0, 2**32, 10_000, dtype=np.uint64)]
    return v


def test_exported_bins_match_the_model():
    import mgen_amd
    from mgen_amd import FLOW_DIST_BINS, flow_dist_bin, flow_dist_bin_lo
    assert FLOW_DIST_BINS == R.BINS == 896
    for s in ("mgenx_flow_dist_init", "mgenx_flow_dist", "mgenx_flow_dist_quantiles",
              "mgenx_flow_dist_bin", "mgenx_flow_dist_bin_lo"):
        assert s in mgen_amd.EXPORTED_SYMBOLS
    vals = _values()
    for v in vals:
        b = flow_dist_bin(v)
        assert b == R.bin_of(v), v
        assert flow_dist_bin_lo(b) <= v < flow_dist_bin_lo(b + 1), v
    got = [flow_dist_bin(v) for v in sorted(vals)]
    assert got == sorted(got)                      # monotone
    assert flow_dist_bin(2**32 - 1) == 895 and flow_dist_bin(2**32) == 896
    assert [flow_dist_bin(v) for v in (64, 127, 128)] == [64, 95, 96]
    for b in range(R.BINS + 1):
        assert flow_dist_bin_lo(b) == R.bin_lo(b), b
    assert flow_dist_bin_lo(896) == 2**32
    for b in range(64, R.BINS):                    # the stated edge and width
        k = b - 64
        assert flow_dist_bin_lo(b) == (32 + k % 32) << (k // 32 + 1)
        assert flow_dist_bin_lo(b + 1) - flow_dist_bin_lo(b) == 1 << (k // 32 + 1)
    assert np.array_equal(R.bins_of(np.array(vals)), [R.bin_of(v) for v in vals])


def test_flow_dist_layout_matches_header(tmp_path):
    from mgen_amd import FLOW_DIST_DTYPE
    names = list(FLOW_DIST_DTYPE.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %d\\n", sizeof(struct mgenx_flow_dist), MGENX_FLOW_DIST_BINS);']
    for f in names:
        lines.append(f'printf("{f} %zu\\n", offsetof(struct mgenx_flow_dist, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["160", "896"]
    assert FLOW_DIST_DTYPE.itemsize == 160 == R.DIST.itemsize
    for line in out[1:]:
        if line:
            name, off = line.split()
            assert FLOW_DIST_DTYPE.fields[name][1] == int(off) == R.DIST.fields[name][1], name


def test_null_arguments_are_rejected_without_hip():
    from mgen_amd import load
    L = load()
    one = ctypes.c_void_p(16)     # a non-null pointer that is never followed
    q = (ctypes.c_uint32 * 1)(500)
    assert L.mgenx_flow_dist_init(None, one, one, 4, None) == -1
    assert L.mgenx_flow_dist(None, one, one, one, one, one, one, one, 8, one, one, 4, None) == -1
    assert L.mgenx_flow_dist_quantiles(None, one, one, 4, q, 1, one, None) == -1


HAND = {   # worked out by hand from the definitions
    0: dict(n=6, bytes=600, lat_sum=1000364, lat_min=50, lat_max=999050, lat_neg=0, lat_over=0,
            jitter_sum=1999036, jitter_max=999000, gap_min=-50, gap_max=999090, reordered=2,
            reorder_sum=10, reorder_max=9, seq_min=3, seq_max=20, first_rx=1000000400,
            last_rx=1001000064, last_lat=64),
    1: dict(n=3, bytes=192, lat_sum=4900001050, lat_min=-50, lat_max=4900000000, lat_neg=1,
            lat_over=1, jitter_sum=9799998950, jitter_max=4900000050, gap_min=100,
            gap_max=3999999550, reordered=0, reorder_sum=0, reorder_max=0, seq_min=5, seq_max=6,
            first_rx=1000000450, last_rx=5000000100, last_lat=1100),
    2: dict(n=1, bytes=1400, lat_sum=70, lat_min=70, lat_max=70, lat_neg=0, lat_over=0,
            jitter_sum=0, jitter_max=0, gap_min=2**63 - 1, gap_max=-2**63, reordered=0,
            reorder_sum=0, reorder_max=0, seq_min=7, seq_max=7, first_rx=1000000070,
            last_rx=1000000070, last_lat=70),
}
HAND_BINS = {0: {133: 1, 171: 1, 114: 1, 50: 1, 508: 1, 64: 1}, 1: {194: 1}, 2: {67: 1}}


def test_model_on_the_hand_case():
    nf, fi, c = R.hand_case()
    dist, hist = R.model(nf, fi, c)
    for f, want in HAND.items():
        for k, v in want.items():
            assert int(dist[f][k]) == v, (f, k, int(dist[f][k]), v)
        assert {int(b): int(hist[f][b]) for b in np.nonzero(hist[f])[0]} == HAND_BINS[f]
    # streaming: any cut leaves the same bytes
    for cut in (1, 5, 8, 11):
        d2, h2 = R.fresh(nf)
        R.update(d2, h2, fi[:cut], {k: v[:cut] for k, v in c.items()})
        R.update(d2, h2, fi[cut:], {k: v[cut:] for k, v in c.items()})
        assert d2.tobytes() == dist.tobytes() and h2.tobytes() == hist.tobytes()
    # quantiles of flow 1: one negative < bin 194 (1088..1119) < one past the histogram
    q = R.quantiles(dist, hist, (1, 500, 900, 1000))
    assert q[1].tolist() == [-1, 1119, 2**32, 2**32]
    assert q[2].tolist() == [71, 71, 71, 71]        # bin 67 holds 70..71
    assert q[0].tolist() == [50, 203, 999423, 999423]
    e, eh = R.fresh(1)
    assert R.quantiles(e, eh, (500,))[0, 0] == -2**63
