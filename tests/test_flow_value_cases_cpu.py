"""CPU: the preconditions of every case of test_gpu_flow_values.py (flow_value_cases), asserted
from the oracle alone: a GPU case cannot go green on an input that missed its edge.  Also
V4's independent pin (a one-record window reports that record's NumPy latency) against the
oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_value_cases as C  # noqa: E402

M = C.M


def _kept(name, f=None):
    """the kept reports of the case (of flow f), from the shared oracle run"""
    c = C.by_name(name)
    _, orep, ocnt = C.oracle_run(name)
    fl = range(c["n_flows"]) if f is None else [f]
    return np.concatenate([orep[g, :min(int(ocnt[g]), c["per_flow"])] for g in fl])


def test_cases_are_well_formed():
    for small in (False, True):
        assert C.names(small) == [c["name"] for fam in C.FAMILIES for c in C.cases(fam, small)]
        for name in C.names(small):
            c = C.by_name(name, small)
            assert set(c["cols"]) == set(C.COLS)
            assert all(c["cols"][k].dtype == C.DT[k] and len(c["cols"][k]) == c["n"] for k in C.COLS)
            assert int(c["cols"]["idx"].max()) == c["n_flows"] - 1
            assert small or name.startswith("V7-long") or c["n"] <= 62_000, (name, c["n"])
            assert any(len(sp) > 1 and sp[1] == 1 for sp in c["splits"])
            assert all(sp[-1] < c["n"] for sp in c["splits"])
    assert len(C.names(True, C.FAMILIES[:6])) >= 6


def test_v1_latency_signs():
    c = C.by_name("V1")
    d = c["cols"]
    assert ((d["tx_sec"] == d["rx_sec"]) & (d["tx_usec"] == d["rx_usec"])).any()
    of, _, ocnt = C.oracle_run("V1")
    assert int(ocnt.min()) > 8 and sum(a.dup_msg_count for a in of) > 0
    r0 = _kept("V1", 0)
    assert len(r0) > 8 and (r0["latency_max"] < 0).all() and (r0["latency_max"] < -3599).all()
    r = _kept("V1")
    assert ((r["latency_min"] < 0) & (r["latency_max"] > 0)).any()
    assert ((r["latency_max"] == 0.0) & (r["latency_min"] < 0)).any()
    assert (_kept("V1", 7)["latency_min"] > 3599).all()


def test_v2_unnormalised_tx_usec():
    c = C.by_name("V2")
    d = c["cols"]
    for f, comp in ((0, True), (1, True), (2, False), (3, False)):
        i = C.flow_records(c, f)
        for v in C.V2_USEC:
            assert (d["tx_usec"][i] == v).sum() > 10, (f, v)
        r = _kept("V2", f)
        r = r[r["msg_count"] > 0]
        assert len(r) > 8
        if comp:
            assert (np.abs(r["latency_min"]) < 1.001).all() and (r["latency_max"] < 1.001).all()
        else:
            assert (r["latency_min"] < -4294).any() and (r["latency_min"] < -2147).any()
    # Delta widens first: the oracle's extreme equals the int64 arithmetic, not a u32 wrap
    i = np.flatnonzero((d["tx_usec"] == (1 << 32) - 1) & (d["idx"] >= 2))
    assert C.numpy_latency(d, i).max() < -4290


@pytest.mark.parametrize("w", C.V3_WINDOWS)
def test_v3_window_end_ties(w):
    name = f"V3-w{w}"
    c = C.by_name(name)
    add = c["meta"]["add"]
    assert add == {0.001: 963, 0.05: 47894, 1.0: M + 11211, 600.0: 599 * M + M}[w]
    r = _kept(name)
    gap = (r["rx_sec"] - r["start_sec"]) * M + (r["rx_usec"] - r["start_usec"])
    need = 40 if w == 600.0 else 100
    assert int((gap == add).sum()) >= need and int((gap == add + 1).sum()) >= need
    assert (gap >= add).all()
    d = c["cols"]
    assert any(int(d["rx_usec"][C.flow_records(c, f)[0]]) == u
               for f in range(3) for u in (999_999,))
    assert int(d["rx_usec"][C.flow_records(c, 1)[0]]) == 999_037
    # runs of equal stamps, and records one microsecond before an end
    rx = d["rx_sec"].astype(np.int64) * M + d["rx_usec"]
    r0 = rx[C.flow_records(c, 0)]
    assert int((np.diff(r0) == 0).sum()) > 50
    ends = (r["start_sec"] * M + r["start_usec"] + add)[r["flow"] == 0]
    assert np.isin(ends - 1, r0).sum() > 50


@pytest.mark.parametrize("w", C.V4_WINDOWS)
def test_v4_degenerate_windows(w):
    from oracle import oracle as O
    name = f"V4-w{w}"
    c = C.by_name(name)
    assert O.quantized_window(w) == (1e-6 if w == 5e-7 else 0.0)
    of, orep, ocnt = C.oracle_run(name)
    d = c["cols"]
    rx = d["rx_sec"].astype(np.int64) * M + d["rx_usec"]
    for f in range(c["n_flows"]):
        i = C.flow_records(c, f)
        assert (np.diff(rx[i]) > 0).all()
        assert int(ocnt[f]) == len(i) - 1 > c["per_flow"]       # every record closes
        assert (orep[f, :c["per_flow"]]["duration"] > 0).all()
    # the crossings: per_flow is reached inside a call of the last split, and before its last
    sp = c["splits"][-1]
    for f in range(c["n_flows"]):
        cross = C.flow_records(c, f)[c["per_flow"] + 1]          # closes report per_flow
        assert sp[1] < cross < sp[-1]
    pins = C.v4_pins(c, ocnt)
    assert len(pins) > 100
    for f, k, lat in pins:
        r = orep[f, k]
        assert r["msg_count"] == 1
        assert r["latency_ave"] == r["latency_min"] == r["latency_max"] == lat, (f, k)
    assert len({lat for _, _, lat in pins}) > 50 and min(lat for _, _, lat in pins) < 0


def test_v4_zero_duration_gives_inf_and_nan():
    _, orep, ocnt = C.oracle_run("V4-zero-duration")
    assert int(ocnt[0]) == 9
    r = orep[0, :9]
    assert (r["duration"] == 0.0).all()
    assert np.isposinf(r["rate"]).any()
    nan = np.isnan(r["rate"])
    assert nan.any() and np.signbit(r["rate"][nan]).all()       # x86's 0 / 0
    assert C.reports_equal(r, r)
    other = r.copy()
    other["rate"][nan] = np.nan                                  # another NaN passes ...
    assert C.reports_equal(other, r)
    other["rate"][nan] = 0.0                                     # ... a number does not
    assert not C.reports_equal(other, r)


def test_v5_receive_clock():
    c = C.by_name("V5")
    d = c["cols"]
    of, orep, ocnt = C.oracle_run("V5")
    rx = d["rx_sec"].astype(np.int64) * M + d["rx_usec"]
    step = np.diff(rx[C.flow_records(c, 0)])
    assert ((step < -0.9 * M) & (step > -1.1 * M)).any() and (step < -3599 * M).any()
    n0 = int(ocnt[0])
    assert n0 > 20
    # thousands of records under one stamp: the first closed, the rest are in the open window
    k = c["meta"]["same_stamp"]
    i1 = C.flow_records(c, 1)
    assert k == 5000 and (rx[i1[-k:]] == rx[i1[-1]]).all() and rx[i1[-k - 1]] < rx[i1[-1]]
    last = orep[1, int(ocnt[1]) - 1]
    assert (int(last["rx_sec"]) * M + int(last["rx_usec"])) == rx[i1[-1]]
    assert (of[1].window_start.sec * M + of[1].window_start.usec) == rx[i1[-1]]
    assert of[1].msg_count > 0.9 * k
    # rx_usec >= 10^6 on closing records: the report keeps it, the next one starts from it
    r2 = orep[2, :int(ocnt[2])]
    big = np.flatnonzero(r2["rx_usec"] >= M)
    assert len(big) >= 8 and int(r2["rx_usec"].max()) >= 4293 * M
    big = big[big + 1 < len(r2)]
    assert (r2["start_usec"][big + 1] == r2["rx_usec"][big]).all()
    assert (d["rx_usec"] >= M).sum() >= 8
    assert of[2].window_end.usec < M


def test_v6_high_rx_sec():
    c = C.by_name("V6-2^31")
    d = c["cols"]
    assert int(d["rx_sec"].min()) < (1 << 31) <= int(d["rx_sec"].max())
    _, orep, ocnt = C.oracle_run("V6-2^31")
    r = _kept("V6-2^31")
    assert (r["start_sec"] < (1 << 31)).any() and (r["start_sec"] >= (1 << 31)).any()
    assert (r["duration"] > 0).all() and int(ocnt.min()) > 8
    for w in (1.0, 600.0):
        name = f"V6-2^32-w{w}"
        c = C.by_name(name)
        d = c["cols"]
        assert int(d["rx_sec"].min()) >= (1 << 32) - 700 and int(d["rx_sec"].max()) == (1 << 32) - 1
        of, orep, ocnt = C.oracle_run(name)
        assert int(ocnt.min()) > 0
        assert all(a.window_end.sec > 0xFFFFFFFF for a in of)
        # a call of the last split starts after a flow's end went past 2^32 s
        assert _prefix_past_2_32(c, c["splits"][-1][-1])


def _prefix_past_2_32(c, n):
    """the oracle over the first n records: whether some flow's window end is past 2^32 s"""
    from oracle import oracle as O
    d = {k: v[:n] for k, v in c["cols"].items()}
    of, _, _ = O.flow_reduce_batch(c["n_flows"], d["idx"], d["seq"], d["tx_sec"], d["tx_usec"],
                                   d["msg_len"], d["rx_sec"], d["rx_usec"], window=c["window"],
                                   per_flow=1)
    return any(a.window_end.sec > 0xFFFFFFFF for a in of)


def test_v7_sizes():
    c = C.by_name("V7-short")
    assert set(np.unique(c["cols"]["msg_len"])) == {0, 1, 65535}
    _, _, ocnt = C.oracle_run("V7-short")
    assert int(ocnt.min()) > 8
    for w in (600.0, 1.0):
        name = f"V7-long-w{w}"
        c = C.by_name(name)
        assert (0,) in c["splits"]                              # the long flow in a single call
        assert int((c["cols"]["idx"] == 0).sum()) == C.V7_LONG > 1_048_576 + 256
        of, _, ocnt = C.oracle_run(name)
        if w == 600.0:
            assert int(ocnt[0]) == 0 and of[0].msg_count == C.V7_LONG
            assert of[0].byte_count == 78_641_934_465 > 1 << 32
        else:
            assert 300 < int(ocnt[0]) < c["per_flow"]
            per = C.V7_LONG / int(ocnt[0])
            assert 2000 < per < 5000                            # a close every few thousand
        assert all(a.msg_count > 100 for a in of[1:])          # the short flows beside it
