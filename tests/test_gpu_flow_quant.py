"""GPU: mgenx_flow_series_quantiles (exact latency percentiles per flow and window of receive
time) against the serial model of tests/flow_quant_ref.py.  Every comparison is exact equality of
whole int64 arrays: no cell and no quantile is left out."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as D  # noqa: E402
import flow_quant_ref as Q  # noqa: E402
import flow_series_ref as S  # noqa: E402

# the product's tier edges (kTinyMax, kWaveMax, kGroupMax, kWideMax in mgenx_flowquant.hpp;
# DESIGN.md, "Windowed latency percentiles"): a cell of c records takes the first tier with
# c <= its edge, a cell above the last the radix select
TIER_EDGES = [8, 256, 2048, 16384]
PERMILLE = Q.PERMILLE
I64_MIN = Q.I64_MIN
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def eng(torch):
    from mgen_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def skew():
    """flow_dist_ref's data set 5 with the windows of test_gpu_flow_series.py: 250 ms, placed so
    that the first and the last tenth of the capture time fall outside them."""
    nf, fi, c = D.skew()
    lo, hi = S.span(nf, fi, c)
    t0 = lo + (hi - lo) // 10
    width = 250_000
    n_bins = (hi - (hi - lo) // 10 - t0) // width
    return nf, fi, c, t0, width, n_bins


@pytest.fixture(scope="module")
def ladder():
    """The size ladder and its model, computed once."""
    nf, fi, c, t0, width, n_bins, sizes = Q.ladder(TIER_EDGES)
    cells = {}
    want = Q.model(nf, n_bins, fi, c, t0, width, PERMILLE, sizes=cells)
    want.setflags(write=False)
    return nf, fi, c, t0, width, n_bins, sizes, cells, want


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run(torch, eng, nf, n_bins, fi, c, t0, width, permille=PERMILLE, out=None):
    got = eng.flow_series_quantiles(nf, n_bins, t0, width, permille, dev(torch, fi),
                                    dev(torch, c["tx_sec"]), dev(torch, c["tx_usec"]),
                                    dev(torch, c["rx_sec"]), dev(torch, c["rx_usec"]), out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(nf, n_bins, len(permille))


def check(got, want):
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(bad[0])
        assert False, (len(bad), bad[:8].tolist(), int(got[at]), int(want[at]))


def fitted(nf, fi, c, width):
    lo, hi = S.span(nf, fi, c)
    return lo, (hi - lo) // width + 1


def model_and_sizes(nf, n_bins, fi, c, t0, width, permille=PERMILLE):
    cells = {}
    return Q.model(nf, n_bins, fi, c, t0, width, permille, sizes=cells), cells


# ---- 1. the existing data sets against the model --------------------------------------------
def test_hand_case_with_records_outside_the_bins(torch, eng):
    nf, fi, c = D.hand_case()
    t0, width, n_bins = 1_000_000_420, 500, 2000
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, width)
    assert cells == {(0, 0): 1, (0, 1): 2, (1, 0): 1, (0, 1999): 2}
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_many_tiny_flows(torch, eng):
    nf, fi, c = D.tiny_flows()
    t0, n_bins = fitted(nf, fi, c, 100_000)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, 100_000)
    assert len(cells) == 5662 and max(cells.values()) == 3
    check(run(torch, eng, nf, n_bins, fi, c, t0, 100_000), want)


def test_boundary_sweep(torch, eng):
    nf, fi, c = D.boundary_sweep()
    t0, n_bins = fitted(nf, fi, c, 50_000)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, 50_000)
    assert len(cells) == 55_179 and max(cells.values()) == 8 == TIER_EDGES[0]
    check(run(torch, eng, nf, n_bins, fi, c, t0, 50_000), want)


@pytest.mark.parametrize("width", [300, 2**40])
def test_one_flow_narrow_windows_and_one_window(torch, eng, width):
    nf, fi, c = D.one_flow_every_97th()
    t0, n_bins = fitted(nf, fi, c, width)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, width)
    if width == 300:
        assert len(cells) == 24_909
    else:   # one cell past what 160 KiB of LDS hold: the radix select
        assert cells == {(0, 0): 40_000} and 40_000 > 20_480 > TIER_EDGES[-1]
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_one_flow_windows_of_a_second(torch, eng):
    nf, fi, c = D.one_flow_max_first()
    t0, n_bins = fitted(nf, fi, c, 1_000_000)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, 1_000_000)
    assert len(cells) == 9 and max(cells.values()) == 5071
    check(run(torch, eng, nf, n_bins, fi, c, t0, 1_000_000), want)


def test_one_dominant_flow(torch, eng, skew):
    """Both placements of 250 ms windows: the one of test_gpu_flow_series.py (both ends of the
    capture outside) and the fitted one."""
    nf, fi, c, t0, width, n_bins = skew
    assert int((fi == D.NONE).sum()) == 616
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, width)
    assert len(cells) == 152 and max(cells.values()) == 7520
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)
    t0, n_bins = fitted(nf, fi, c, width)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, width)
    assert len(cells) == 176 and max(cells.values()) == 7916
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_receive_times_shuffled_within_a_flow(torch, eng):
    nf, fi, c = S.shuffled_rx()
    t0, n_bins = fitted(nf, fi, c, 10_000)
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, 10_000)
    assert len(cells) == 636 and max(cells.values()) == 25
    check(run(torch, eng, nf, n_bins, fi, c, t0, 10_000), want)


# ---- 2. the size ladder ---------------------------------------------------------------------
def test_size_ladder_over_every_tier_edge(torch, eng, ladder):
    nf, fi, c, t0, width, n_bins, sizes, cells, want = ladder
    assert len(fi) == sum(sizes) == 265_795 and nf == len(sizes) == len(cells)
    assert all(cells[(f, f % 7)] == s for f, s in enumerate(sizes))
    for e in TIER_EDGES + [20_480]:
        assert {e - 1, e, e + 1} <= set(sizes)
    assert set(range(1, 131)) <= set(sizes) and max(sizes) == 32_769
    # interleaved: no flow's records are contiguous in the input
    assert int((np.diff(fi.astype(np.int64)) != 0).sum()) > len(fi) // 2
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


# ---- 3. the value domain --------------------------------------------------------------------
def test_value_domain(torch, eng):
    nf, fi, c, t0, width, n_bins, what = Q.value_domain()
    assert n_bins == 3907 and width == 2**40 and (2**32 * 10**6 - 1) // width == n_bins - 1
    assert (c["tx_usec"] >= 10**6).any()
    want, cells = model_and_sizes(nf, n_bins, fi, c, t0, width)
    row = {name: want[f][[b for (g, b) in cells if g == f][0]] for name, f in what.items()}
    assert len(cells) == nf      # every flow in one window
    assert {b for _, b in cells} == {0, Q.SEC_MID * 10**6 // width, Q.SEC_HIGH * 10**6 // width}
    live = want[want != I64_MIN]
    assert live.min() < -2**51 and live.max() > 2**51
    assert row["wild_low"][0] < -2**51 and row["wild_high"][-1] > 2**51
    hb = row["high_bits"]
    assert len(set(hb.tolist())) >= 5 and set((hb & 0xFFFFFFFF).tolist()) == {123}
    lb = row["low_byte"]
    assert len(set(lb.tolist())) >= 5 and set((lb >> 8).tolist()) == {0x12345}
    assert cells[(what["equal"], Q.SEC_MID * 10**6 // width)] == 5000
    assert set(row["equal"].tolist()) == {777}
    assert set(row["two"].tolist()) == {-5, 2**33 + 1}
    lat = {}
    for name in ("ascending", "descending"):
        sel = fi == what[name]
        k = {n: v[sel].astype(np.int64) for n, v in c.items()}
        lat[name] = (k["rx_sec"] - k["tx_sec"]) * 10**6 + k["rx_usec"] - k["tx_usec"]
    assert (np.diff(lat["ascending"]) >= 0).all() and (np.diff(lat["descending"]) <= 0).all()
    assert lat["ascending"][0] < lat["ascending"][-1]
    assert np.array_equal(row["ascending"], row["descending"])
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


# ---- 4. the rank rule at its edges ----------------------------------------------------------
def test_every_permille_on_cells_of_1_2_999_1000_1001_2001(torch, eng):
    rng = np.random.default_rng(73)
    sizes = [1, 2, 999, 1000, 1001, 2001]
    fi, c = Q.weave(rng, [Q.wild_cols(rng, s, Q.SEC_MID) for s in sizes])
    nf, t0, width = len(sizes), 0, 2**62
    d = [dev(torch, a) for a in (fi, c["tx_sec"], c["tx_usec"], c["rx_sec"], c["rx_usec"])]
    every = list(range(1, 1001))
    want, cells = model_and_sizes(nf, 1, fi, c, t0, width, every)
    assert [cells[(f, 0)] for f in range(nf)] == sizes
    got = []
    for a in range(0, 1000, 32):            # MGENX_FLOW_SERIES_MAX_Q at a time
        got.append(eng.flow_series_quantiles(nf, 1, t0, width, every[a:a + 32], *d))
    torch.cuda.synchronize()
    check(np.concatenate([g.cpu().numpy() for g in got], axis=2), want)


# ---- 5. cross-checks against the existing calls ---------------------------------------------
def series_bins(torch, eng, nf, n_bins, fi, c, t0, width):
    from mgen_amd import FLOW_SERIES_BIN_DTYPE
    state, bins = eng.flow_series_init(nf, n_bins)
    k = {name: dev(torch, c[name]) for name in D.COLS}
    eng.flow_series(state, bins, nf, n_bins, t0, width, dev(torch, fi), k["seq"], k["tx_sec"],
                    k["tx_usec"], k["msg_len"], k["rx_sec"], k["rx_usec"])
    torch.cuda.synchronize()
    return bins.cpu().numpy().view(FLOW_SERIES_BIN_DTYPE).reshape(nf, n_bins)


def test_permille_1000_is_flow_series_lat_max(torch, eng, skew):
    nf, fi, c, t0, width, n_bins = skew
    bins = series_bins(torch, eng, nf, n_bins, fi, c, t0, width)
    assert int((bins["n"] == 0).sum()) == nf * n_bins - 152 > 0     # empty cells: INT64_MIN both
    check(run(torch, eng, nf, n_bins, fi, c, t0, width, [1000])[:, :, 0],
          np.ascontiguousarray(bins["lat_max"]))


def test_permille_1_is_flow_series_lat_min_up_to_1000_records(torch, eng, skew):
    nf, fi, c, t0, width, n_bins = skew
    bins = series_bins(torch, eng, nf, n_bins, fi, c, t0, width)
    small = (bins["n"] > 0) & (bins["n"] <= 1000)
    assert int(small.sum()) == 147 and int((bins["n"] > 0).sum()) == 152
    got = run(torch, eng, nf, n_bins, fi, c, t0, width, [1])[:, :, 0]
    check(got[small], bins["lat_min"][small])
    assert (got[bins["n"] > 1000] >= bins["lat_min"][bins["n"] > 1000]).all()
    check(got[bins["n"] == 0], np.full(int((bins["n"] == 0).sum()), I64_MIN, np.int64))


@pytest.mark.parametrize("name", ["skew", "hand_case"])
def test_one_bin_brackets_flow_dist_quantiles(torch, eng, name):
    """mgenx_flow_dist_quantiles gives the inclusive upper edge of the exact answer's bin."""
    nf, fi, c = getattr(D, name)()
    lo, hi = S.span(nf, fi, c)
    exact = run(torch, eng, nf, 1, fi, c, lo, hi - lo + 1)[:, 0, :]
    dist, hist = eng.flow_dist_init(nf)
    k = {n: dev(torch, c[n]) for n in D.COLS}
    eng.flow_dist(dist, hist, nf, dev(torch, fi), k["seq"], k["tx_sec"], k["tx_usec"],
                  k["msg_len"], k["rx_sec"], k["rx_usec"])
    edges = eng.flow_dist_quantiles(dist, hist, nf, PERMILLE)
    torch.cuda.synchronize()

    def edge(x):
        if x == I64_MIN:
            return I64_MIN
        return -1 if x < 0 else 2**32 if x >= 2**32 else D.bin_lo(D.bin_of(x) + 1) - 1
    want = np.array([[edge(int(x)) for x in r] for r in exact], np.int64)
    assert (exact != I64_MIN).all()
    if name == "hand_case":     # all three branches: negative, inside the bins, past them
        assert (exact < 0).any() and (exact >= 2**32).any() and (exact == 70).any()
    check(edges.cpu().numpy(), want)


# ---- 6. output bounds and purity ------------------------------------------------------------
def test_guards_garbage_and_repeated_calls(torch, eng, skew):
    nf, fi, c, t0, width, n_bins = skew
    want = Q.model(nf, n_bins, fi, c, t0, width, PERMILLE)
    m = nf * n_bins * len(PERMILLE)
    buf = torch.full((m + 128,), FILL, dtype=torch.int64, device="cuda")
    first = run(torch, eng, nf, n_bins, fi, c, t0, width, out=buf[64:64 + m])
    check(first, want)                               # over garbage
    again = run(torch, eng, nf, n_bins, fi, c, t0, width, out=buf[64:64 + m])
    check(again, want)                               # over its own result: nothing accumulates
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)      # a fresh output
    edge = buf.cpu().numpy()
    assert (edge[:64] == FILL).all() and (edge[64 + m:] == FILL).all()
    # no records: every cell is empty, the guards stay
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.flow_series_quantiles(nf, n_bins, t0, width, PERMILLE, z, z, z, z, z, n=0,
                              out=buf[64:64 + m])
    eng.flow_series_quantiles(nf, n_bins, t0, width, PERMILLE, None, None, None, None, None, n=0,
                              out=buf[64:64 + m])
    torch.cuda.synchronize()
    edge = buf.cpu().numpy()
    assert (edge[64:64 + m] == I64_MIN).all()
    assert (edge[:64] == FILL).all() and (edge[64 + m:] == FILL).all()
    # no flows: nothing is touched
    buf.fill_(FILL)
    eng.flow_series_quantiles(0, n_bins, t0, width, PERMILLE, z, z, z, z, z, out=buf)
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


# ---- 7. bad arguments -----------------------------------------------------------------------
def test_bad_arguments_leave_the_output_untouched(torch, eng):
    from mgen_amd import MgenxError
    nf, n_bins = 5, 7
    out = torch.full((nf * n_bins * 32,), FILL, dtype=torch.int64, device="cuda")
    z = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(n_flows=nf, bins=n_bins, width=1000, permille=(500,), cols=(z, z, z, z, z), n=4,
             o=out):
        eng.flow_series_quantiles(n_flows, bins, 0, width, permille, *cols, n=n, out=o)

    call()                                           # the good call the bad ones differ from
    torch.cuda.synchronize()
    out.fill_(FILL)
    bad = [dict(width=0), dict(bins=0), dict(permille=()), dict(permille=[500] * 33),
           dict(permille=[0]), dict(permille=[500, 1001]), dict(permille=[2**32 - 1]),
           dict(n_flows=2**16, bins=2**15), dict(n_flows=2**31 - 1, bins=2)]
    bad += [dict(cols=tuple(None if i == k else z for i in range(5))) for k in range(5)]
    for kw in bad:
        with pytest.raises(MgenxError):
            call(**kw)
    # a null output or permille array, a null context: the C entry itself
    q = (ctypes.c_uint32 * 1)(500)
    p = [ctypes.c_void_p(z.data_ptr())] * 5
    lib, EINVAL = eng.lib, -1
    assert lib.mgenx_flow_series_quantiles(eng.ctx, *p, 4, 0, 1000, n_bins, nf, q, 1, None,
                                           None) == EINVAL
    assert lib.mgenx_flow_series_quantiles(eng.ctx, *p, 4, 0, 1000, n_bins, nf, None, 1,
                                           ctypes.c_void_p(out.data_ptr()), None) == EINVAL
    assert lib.mgenx_flow_series_quantiles(None, *p, 4, 0, 1000, n_bins, nf, q, 1,
                                           ctypes.c_void_p(out.data_ptr()), None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    call(permille=list(range(1, 33)))                # 32 values are allowed
    torch.cuda.synchronize()
    assert bool((out[:nf * n_bins * 32] != FILL).all())


# ---- 8. workspace growth --------------------------------------------------------------------
def test_workspace_grows_and_is_reused(torch, ladder):
    from mgen_amd import Engine
    nf, fi, c, t0, width, n_bins, sizes, cells, want = ladder
    hf, hfi, hc = D.hand_case()
    hwant = Q.model(hf, 2000, hfi, hc, 1_000_000_420, 500, PERMILLE)
    e = Engine(0)                                    # a context whose workspace is still empty
    try:
        check(run(torch, e, hf, 2000, hfi, hc, 1_000_000_420, 500), hwant)
        check(run(torch, e, nf, n_bins, fi, c, t0, width), want)
        check(run(torch, e, hf, 2000, hfi, hc, 1_000_000_420, 500), hwant)
    finally:
        e.close()


# ---- 9. permutation invariance --------------------------------------------------------------
def test_record_order_plays_no_part(torch, eng, skew):
    nf, fi, c, t0, width, n_bins = skew
    base = run(torch, eng, nf, n_bins, fi, c, t0, width)
    p = np.random.default_rng(74).permutation(len(fi))
    check(run(torch, eng, nf, n_bins, fi[p], {k: v[p] for k, v in c.items()}, t0, width), base)
    check(base, Q.model(nf, n_bins, fi, c, t0, width, PERMILLE))


# ---- 10. end to end -------------------------------------------------------------------------
def test_analyze_text_log_series_with_permille(skew):
    from mgen_amd import analyze_text_log_series
    nf, fi, c = skew[:3]
    m = 20_000
    fi = fi[:m]
    lines, keep = [], []
    for i in range(m):
        if i % 3000 == 7:
            lines += ["1700000000.000001 START Mgen Version 5.1.1\n", "no such event\n"]
        if fi[i] == D.NONE:
            continue
        f = int(fi[i])
        lines.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                     "sent>%d.%06d size>%d \n" % (
                         c["rx_sec"][i], c["rx_usec"][i], f + 1, c["seq"][i], 1 + f % 2,
                         c["tx_sec"][i], c["tx_usec"][i], c["msg_len"][i]))
        keep.append(i)
    keep = np.array(keep)
    log = "".join(lines).encode()
    width = 50_000
    res = analyze_text_log_series(log, width, permille=[500, 990])
    assert len(res) == 7
    keys, state, bins, t0, n_lines, n_bad, quant = res
    assert n_lines == len(lines) and quant.dtype == np.int64
    assert quant.shape == bins.shape + (2,) and bins.shape[1] > 8
    kept = {k: v[:m][keep] for k, v in c.items()}
    mine = keys["flow_id"].astype(np.int64) - 1      # the returned order -> this test's flow index
    want = Q.model(nf, bins.shape[1], fi[keep], kept, t0, width, [500, 990])
    check(quant, want[mine])
    assert np.array_equal(quant[:, :, 0] == I64_MIN, bins["n"] == 0)
    # without the keyword: the six elements, the same bytes
    plain = analyze_text_log_series(log, width)
    assert len(plain) == 6 and plain[3:] == res[3:6]
    for a, b in zip(plain[:3], res[:3]):
        assert a.tobytes() == b.tobytes()


def test_series_main_with_and_without_q(tmp_path, capsys):
    from mgen_amd import analyze_text_log_series, series
    log = tmp_path / "recv.log"
    rows = []
    for i in range(300):                             # two flows, 1 ms apart
        f, seq = i % 2, i // 2
        rx = 1_700_000_000_000_000 + i * 1000
        lat = 250 + (i * 37) % 101
        rows.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                    "sent>%d.%06d size>100 \n" % (rx // 10**6, rx % 10**6, f + 1, seq, f + 1,
                                                   (rx - lat) // 10**6, (rx - lat) % 10**6))
    log.write_text("".join(rows))
    out = tmp_path / "series.txt"
    assert series.main(["-q", "500,990", str(log), "0.05", str(out)]) == 0
    text = out.read_text()
    head = "# " + " ".join(series.COLUMNS)
    table = [ln.split() for ln in text.split("\n")]
    assert [ln for ln in text.split("\n") if ln.startswith("# bin")] == [
        head + " lat_p500 lat_p990"] * 2
    data = [[int(v) for v in r] for r in table if r and r[0] != "#"]
    assert len(data) == 12 and all(len(r) == 12 for r in data)
    for k, r in enumerate(data):                     # the model on the rows of this window
        f, b = k // 6, k % 6
        lat = sorted(250 + (i * 37) % 101 for i in range(b * 50, b * 50 + 50) if i % 2 == f)
        assert r[1] == len(lat) == 25 and r[6] == lat[0] and r[7] == lat[-1]
        assert r[10:] == [lat[Q.rank(500, 25) - 1], lat[Q.rank(990, 25) - 1]]
    capsys.readouterr()
    assert series.main([str(log), "0.05", "-q", "500,990"]) == 0    # the option last
    assert capsys.readouterr().out == text
    # without -q: the table as it was before the option existed
    assert series.main([str(log), "0.05", str(out)]) == 0
    plain = out.read_text()
    assert [ln for ln in plain.split("\n") if ln.startswith("# bin")] == [head] * 2
    stripped = "\n".join(" ".join(r[:10]) if r and r[0] != "#" else
                         ln.replace(" lat_p500 lat_p990", "")
                         for r, ln in zip(table, text.split("\n")))
    assert plain == stripped
    keys, _s, bins, t0, _n, _b = analyze_text_log_series(log.read_bytes(), 50_000)
    assert plain == series.format_series(keys, bins, t0, 50_000)
