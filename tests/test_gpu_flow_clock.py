"""GPU: mgenx_flow_clock (per-flow clock offset and skew: the lower-hull edge over the mean send
time, and the latencies above it) against the serial model of tests/flow_clock_ref.py.  Every
comparison is exact equality of whole arrays, and every output sits between guard regions."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_clock_ref as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sizes at which the product takes another path (kClockEdges in mgenx_flowclock.hpp): the
# lanes of a wave and four times that (its loop takes four chunks at a time), the lanes of a
# workgroup, the largest flow a wave serves, and four times a workgroup's lanes
CLOCK_EDGES = [64, 256, 1024, 2048, 4096]
FILL = 0x5A
GUARD = 256     # bytes on either side of every output


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
def grid():
    nf, fi, c = C.grid_corpus()
    want = C.model(nf, fi, c)
    for w in want:
        w.setflags(write=False)
    return nf, fi, c, want


@pytest.fixture(scope="module")
def dominant():
    """The dominant-flow data in send order, with its model: computed once."""
    nf, fi, c = C.dominant(False)
    want = C.model(nf, fi, c)
    for w in want:
        w.setflags(write=False)
    return nf, fi, c, want


def dev(torch, a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(signed).copy()).cuda()


class Out:
    """The four outputs inside guarded byte buffers filled with FILL."""

    def __init__(self, torch, nf, n, resid=True, stamps=True):
        self.torch, self.nf, self.n = torch, nf, n
        self.sizes = {"clock": nf * 64, "resid": n * 8 if resid else None,
                      "sec": n * 4 if stamps else None, "usec": n * 4 if stamps else None}
        self.buf = {k: torch.full((GUARD + s + GUARD,), FILL, dtype=torch.uint8, device="cuda")
                    for k, s in self.sizes.items() if s is not None}

    def ptr(self, k):
        return ctypes.c_void_p(self.buf[k].data_ptr() + GUARD) if k in self.buf else None

    def get(self, k, dtype):
        raw = self.buf[k].cpu().numpy()
        s = self.sizes[k]
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + s:] == FILL).all(), k + " guard"
        return raw[GUARD:GUARD + s].copy().view(dtype)


def call(torch, eng, nf, fi, c, out, opts=0, n=None):
    from mgen_amd import _stream
    n = len(fi) if n is None else n
    d = [dev(torch, np.asarray(a)) for a in (fi, c["tx_sec"], c["tx_usec"], c["rx_sec"], c["rx_usec"])]
    rc = eng.lib.mgenx_flow_clock(eng.ctx, *[ctypes.c_void_p(t.data_ptr()) for t in d], n, nf, opts,
                                  out.ptr("clock"), out.ptr("resid"), out.ptr("sec"),
                                  out.ptr("usec"), _stream(eng.device))
    torch.cuda.synchronize()
    return rc


def check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        assert False, (what, len(bad), bad[:8].tolist(), got[bad[:4]].tolist(),
                       want[bad[:4]].tolist())


def run_and_check(torch, eng, nf, fi, c, want=None, opts=0, resid=True, stamps=True):
    want = C.model(nf, fi, c, offset_only=bool(opts & 1)) if want is None else want
    out = Out(torch, nf, len(fi), resid, stamps)
    assert call(torch, eng, nf, fi, c, out, opts) == 0
    check(out.get("clock", C.CLOCK_DTYPE), want[0], "clock")
    if resid:
        check(out.get("resid", np.int64), want[1], "resid")
    if stamps:
        check(out.get("sec", np.uint32), want[2], "rx_sec_out")
        check(out.get("usec", np.uint32), want[3], "rx_usec_out")
    return want


# ---- 1. the small data sets -----------------------------------------------------------------
def test_hand_case(torch, eng):
    nf, fi, c = C.hand_case()
    want = run_and_check(torch, eng, nf, fi, c)
    assert want[0][0].tolist() == (8, 10**9 + 4, 2, 10**9 + 8, 4, 25, 10, 1, 9)


def test_grid_corpus(torch, eng, grid):
    nf, fi, c, want = grid
    assert int((np.asarray(fi) >= nf).sum()) == 1000
    run_and_check(torch, eng, nf, fi, c, want)


def test_many_flows_of_0_to_5_records(torch, eng):
    nf, fi, c = C.tiny_flows()
    want = run_and_check(torch, eng, nf, fi, c)
    assert int((want[0]["n"] == 0).sum()) > 300


# ---- 2. the size ladder ---------------------------------------------------------------------
def test_size_ladder_over_every_edge(torch, eng):
    nf, fi, c, sizes = C.ladder(CLOCK_EDGES)
    for e in CLOCK_EDGES:
        assert {e - 1, e, e + 1} <= set(sizes)
    assert sizes[1::2] == [1] * (len(sizes) // 2)
    want = run_and_check(torch, eng, nf, fi, c)
    assert want[0]["n"].tolist() == sizes


# ---- 3. large flows -------------------------------------------------------------------------
def test_one_dominant_flow_in_send_order(torch, eng, dominant):
    nf, fi, c, want = dominant
    assert want[0][0]["n"] == 200_000 and nf == 501
    # the fitted slope is the drift the data were made with: 50 ppm within 2
    a = want[0][0]
    assert 48 <= 10**6 * int(a["db"] - a["da"]) // int(a["xb"] - a["xa"]) <= 52
    run_and_check(torch, eng, nf, fi, c, want)


def test_one_dominant_flow_shuffled(torch, eng, dominant):
    nf, fi, c = C.dominant(True)
    want = run_and_check(torch, eng, nf, fi, c)
    # the same points: the same fit and sums; ia / ib follow the model
    for k in ("n", "xa", "da", "xb", "db", "resid_sum", "resid_max"):
        assert np.array_equal(want[0][k], dominant[3][0][k]), k
    assert not np.array_equal(want[0]["ia"], dominant[3][0]["ia"])


@pytest.mark.parametrize("k_tenths", [1, 9])
def test_parabola(torch, eng, k_tenths):
    nf, fi, c = C.parabola(k_tenths)
    want = run_and_check(torch, eng, nf, fi, c)
    a = want[0][0]
    assert a["n"] == 50_000 and a["xb"] - a["xa"] == 1 and (a["db"] > a["da"]) == (k_tenths == 1)


# ---- 4. the value domain --------------------------------------------------------------------
def test_value_domain(torch, eng):
    nf, fi, c, names = C.value_domain()
    want = run_and_check(torch, eng, nf, fi, c)
    run_and_check(torch, eng, nf, fi, c, opts=1)
    step = want[0][names["step"]]
    assert step["xb"] - step["xa"] == 1 and step["db"] - step["da"] > 2**51
    far = want[1][np.asarray(fi) == names["step_far"]]
    assert int((far != 0).sum()) == 1       # the residual kept modulo 2^64


# ---- 5. order, options, outputs -------------------------------------------------------------
def test_record_order_plays_no_part(torch, eng, grid):
    nf, fi, c, base = grid
    p = np.random.default_rng(75).permutation(len(fi))
    want = run_and_check(torch, eng, nf, fi[p], {k: v[p] for k, v in c.items()})
    for k in ("n", "xa", "da", "xb", "db", "resid_sum", "resid_max"):
        assert np.array_equal(want[0][k], base[0][k]), k
    check(want[1], base[1][p], "resid permuted")


def test_offset_only(torch, eng, grid, dominant):
    nf, fi, c, _ = grid
    want = run_and_check(torch, eng, nf, fi, c, opts=1)
    assert np.array_equal(want[0]["xa"], want[0]["xb"]) and np.array_equal(want[0]["ia"], want[0]["ib"])
    nf, fi, c, _ = dominant
    run_and_check(torch, eng, nf, fi, c, opts=1)


@pytest.mark.parametrize("resid,stamps", [(False, False), (True, False), (False, True)])
def test_every_combination_of_optional_outputs(torch, eng, grid, resid, stamps):
    nf, fi, c, want = grid
    run_and_check(torch, eng, nf, fi, c, want, resid=resid, stamps=stamps)


def test_garbage_repeated_calls_and_no_records(torch, eng, grid):
    nf, fi, c, want = grid
    out = Out(torch, nf, len(fi))
    for _ in range(2):              # over garbage, then over its own result
        assert call(torch, eng, nf, fi, c, out) == 0
        check(out.get("clock", C.CLOCK_DTYPE), want[0], "clock")
        check(out.get("resid", np.int64), want[1], "resid")
        check(out.get("sec", np.uint32), want[2], "sec")
        check(out.get("usec", np.uint32), want[3], "usec")
    # no records: the empty structs, nothing else
    empty = C.model(nf, fi[:0], {k: v[:0] for k, v in c.items()})[0]
    assert call(torch, eng, nf, fi, c, out, n=0) == 0
    check(out.get("clock", C.CLOCK_DTYPE), empty, "empty clock")
    check(out.get("resid", np.int64), want[1], "resid left alone")
    # no flows: nothing is touched
    for b in out.buf.values():
        b.fill_(FILL)
    assert call(torch, eng, 0, fi, c, out) == 0
    assert all(bool((b == FILL).all()) for b in out.buf.values())


def test_bad_arguments_leave_the_outputs_untouched(torch, eng):
    from mgen_amd import MgenxError, _stream
    nf, fi, c = C.hand_case()
    out = Out(torch, nf, len(fi))
    keep = [dev(torch, np.asarray(fi))]
    z = [ctypes.c_void_p(keep[0].data_ptr())] * 5       # (the values do not matter)
    lib, EINVAL, n = eng.lib, -1, len(fi)
    o = [out.ptr(k) for k in ("clock", "resid", "sec", "usec")]
    st = _stream(eng.device)
    assert lib.mgenx_flow_clock(None, *z, n, nf, 0, *o, st) == EINVAL
    assert lib.mgenx_flow_clock(eng.ctx, *z, n, nf, 0, None, o[1], o[2], o[3], st) == EINVAL
    for k in range(5):
        cols = [None if i == k else z[i] for i in range(5)]
        assert lib.mgenx_flow_clock(eng.ctx, *cols, n, nf, 0, *o, st) == EINVAL
    assert lib.mgenx_flow_clock(eng.ctx, *z, n, nf, 0, o[0], o[1], o[2], None, st) == EINVAL
    assert lib.mgenx_flow_clock(eng.ctx, *z, n, nf, 0, o[0], o[1], None, o[3], st) == EINVAL
    for opts in (2, 3, 0x80000000):
        assert lib.mgenx_flow_clock(eng.ctx, *z, n, nf, opts, *o, st) == EINVAL
    assert lib.mgenx_flow_clock(eng.ctx, *z, 2**31, nf, 0, *o, st) == EINVAL
    assert lib.mgenx_flow_clock(eng.ctx, *z, n, 2**31, 0, *o, st) == EINVAL
    with pytest.raises(MgenxError):
        eng.flow_clock(nf, keep[0], keep[0], keep[0], keep[0], keep[0], opts=4)
    torch.cuda.synchronize()
    assert all(bool((b == FILL).all()) for b in out.buf.values())


def test_workspace_grows_and_is_reused(torch, dominant):
    from mgen_amd import Engine
    nf, fi, c, want = dominant
    hf, hfi, hc = C.hand_case()
    e = Engine(0)                                    # a context whose workspace is still empty
    try:
        run_and_check(torch, e, hf, hfi, hc)
        run_and_check(torch, e, nf, fi, c, want)
        run_and_check(torch, e, hf, hfi, hc)
    finally:
        e.close()


# ---- 6. invariants against the existing kernels ---------------------------------------------
@pytest.mark.parametrize("name", ["grid", "dominant"])
def test_flow_dist_on_the_corrected_stamps(torch, eng, grid, dominant, name):
    from mgen_amd import FLOW_CLOCK_DTYPE, FLOW_DIST_DTYPE
    nf, fi, c, want = grid if name == "grid" else dominant
    n = len(fi)
    d = {k: dev(torch, np.asarray(v)) for k, v in c.items()}
    idx = dev(torch, np.asarray(fi))
    clock, resid, rs, ru = eng.flow_clock(nf, idx, d["tx_sec"], d["tx_usec"], d["rx_sec"],
                                          d["rx_usec"], resid=True, stamps=True)
    seq = torch.zeros(n, dtype=torch.int32, device="cuda")
    ln = torch.ones(n, dtype=torch.int16, device="cuda")
    dist, _ = eng.flow_dist_init(nf, hist=False)
    eng.flow_dist(dist, None, nf, idx, seq, d["tx_sec"], d["tx_usec"], ln, rs, ru)
    torch.cuda.synchronize()
    clock = clock.cpu().numpy().view(FLOW_CLOCK_DTYPE)
    check(clock, want[0], "clock")
    dist = dist.cpu().numpy().view(FLOW_DIST_DTYPE)
    full = clock["n"] > 0
    assert np.array_equal(dist["n"], clock["n"]) and int(full.sum()) > nf // 2
    assert (dist["lat_min"][full] == 0).all() and (dist["lat_neg"] == 0).all()
    assert np.array_equal(dist["lat_sum"][full], clock["resid_sum"][full])
    assert np.array_equal(dist["lat_max"][full], clock["resid_max"][full])
    # dev_resid equals the latency recomputed from the corrected columns
    live = np.asarray(fi) < nf
    rs, ru = rs.cpu().numpy().view(np.uint32), ru.cpu().numpy().view(np.uint32)
    lat = (rs.astype(np.int64) - c["tx_sec"].astype(np.int64)) * 10**6 + ru.astype(np.int64) \
        - c["tx_usec"].astype(np.int64)
    resid = resid.cpu().numpy()
    assert np.array_equal(lat[live], resid[live]) and (resid[~live] == C.I64_MIN).all()


# ---- 7. end to end --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drift():
    log, nf, fi, c = C.drift_log()
    return log, nf, fi, c, C.model(nf, fi, c)


def test_analyze_text_log_clock(drift):
    from mgen_amd import analyze_text_log_clock
    log, nf, fi, c, want = drift
    keys, clock, n_lines, n_bad = analyze_text_log_clock(log)
    assert n_lines == log.count(b"\n") and n_bad == 0
    assert keys["flow_id"].tolist() == [2, 1]        # flows in the order of their first line
    mine = keys["flow_id"].astype(np.int64) - 1
    # the model on the parsed columns: record indices count the log's lines, START lines included
    line_of = np.flatnonzero([b"RECV" in ln for ln in log.split(b"\n")[:-1]])
    w = want[0][mine].copy()
    w["ia"], w["ib"] = line_of[w["ia"]], line_of[w["ib"]]
    check(clock, w, "clock of the log")
    for e in clock:          # +40 ppm and 2.5 s, as the log was made
        assert 39_000 <= 10**9 * int(e["db"] - e["da"]) // int(e["xb"] - e["xa"]) <= 41_000
        assert 2_500_000 <= e["da"] <= 2_500_000 + 600
    off = analyze_text_log_clock(log, offset_only=True)[1]
    w = C.model(nf, fi, c, offset_only=True)[0][mine]
    for k in ("n", "xa", "da", "xb", "db", "resid_sum", "resid_max"):
        assert np.array_equal(off[k], w[k]), k
    assert np.array_equal(off["ia"], line_of[w["ia"]]) and np.array_equal(off["ia"], off["ib"])


def test_analyze_text_log_series_and_dist_with_clock(torch, eng, drift):
    from mgen_amd import (FLOW_DIST_DTYPE, FLOW_SERIES_BIN_DTYPE, analyze_text_log_dist,
                          analyze_text_log_series)
    log, nf, fi, c, want = drift
    width = 100_000
    res = analyze_text_log_series(log, width, clock="fit", permille=[500, 990])
    keys, state, bins, t0, n_lines, n_bad, quant = res
    mine = keys["flow_id"].astype(np.int64) - 1
    # the plain calls fed the model's corrected stamps
    n_bins = bins.shape[1]
    d = {k: dev(torch, np.asarray(v)) for k, v in c.items()}
    rs, ru = dev(torch, want[2]), dev(torch, want[3])
    idx = dev(torch, fi)
    lo = int((want[2].astype(np.int64) * 10**6 + want[3]).min())
    assert t0 == lo
    st, bn = eng.flow_series_init(nf, n_bins)
    eng.flow_series(st, bn, nf, n_bins, t0, width, idx, d["seq"], d["tx_sec"], d["tx_usec"],
                    d["msg_len"], rs, ru)
    q = eng.flow_series_quantiles(nf, n_bins, t0, width, [500, 990], idx, d["tx_sec"],
                                  d["tx_usec"], rs, ru)
    torch.cuda.synchronize()
    bn = bn.cpu().numpy().view(FLOW_SERIES_BIN_DTYPE).reshape(nf, n_bins)
    assert bins.tobytes() == bn[mine].tobytes() and np.array_equal(quant, q.cpu().numpy()[mine])
    live = bins["n"] > 0
    # the 2.5 s are gone: what is left is the delay above the floor, far below 0.1 s
    assert (bins["lat_min"][live] >= 0).all() and (bins["lat_max"][live] < 100_000).all()
    # clock=None: today's result, byte for byte
    plain = analyze_text_log_series(log, width)
    none = analyze_text_log_series(log, width, clock=None)
    assert plain[3:] == none[3:] and all(a.tobytes() == b.tobytes() for a, b in zip(plain[:3], none[:3]))
    assert (plain[2]["lat_min"][plain[2]["n"] > 0] > 2_000_000).all()
    # the distribution: latencies above the line
    dist = analyze_text_log_dist(log, clock="fit")[1]
    assert dist.dtype == FLOW_DIST_DTYPE and (dist["lat_min"] == 0).all()
    assert np.array_equal(dist["lat_sum"], want[0]["resid_sum"][mine])
    assert (analyze_text_log_dist(log)[1]["lat_min"] > 2_000_000).all()
    assert (analyze_text_log_dist(log, clock="offset")[1]["lat_min"] == 0).all()


def test_clock_and_series_command_lines(tmp_path, drift):
    log, nf, fi, c, want = drift
    path = tmp_path / "recv.log"
    path.write_bytes(log)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "mgen_amd.clock", str(path)], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split("\n")
    assert rows[0] == "# flow src dst n t_a_us lat_a_us t_b_us lat_b_us skew_ppb resid_mean resid_max"
    assert len(rows) == 4 and rows[3] == ""
    for row, f in zip(rows[1:3], (1, 0)):
        e = want[0][f]
        skew = 10**9 * int(e["db"] - e["da"]) // int(e["xb"] - e["xa"])
        assert row.split() == [str(f + 1), "10.0.0.%d/5001" % (f + 1), "10.0.0.9/5000"] + [
            str(int(v)) for v in (e["n"], e["xa"], e["da"], e["xb"], e["db"], skew,
                                  int(e["resid_sum"]) // int(e["n"]), e["resid_max"])]
    from mgen_amd import series
    out = tmp_path / "series.txt"
    assert series.main(["-c", "fit", str(path), "0.1", str(out)]) == 0
    fitted = out.read_text()
    assert series.main([str(path), "0.1", str(out), "-c", "fit"]) == 0      # the option last
    assert out.read_text() == fitted
    data = [[int(v) for v in ln.split()] for ln in fitted.split("\n") if ln and ln[0] != "#"]
    assert len(data) > 20 and all(0 <= r[6] <= r[7] < 100_000 for r in data)    # above the line
    assert series.main([str(path), "0.1", str(out)]) == 0
    raw = [[int(v) for v in ln.split()] for ln in out.read_text().split("\n") if ln and ln[0] != "#"]
    assert all(r[6] > 2_000_000 for r in raw)
