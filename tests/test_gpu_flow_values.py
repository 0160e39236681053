"""GPU: mgenx_flow_reduce over the value domain its other tests leave out (flow_value_cases:
latencies of any sign and size, unnormalised microseconds, records exactly at a window end,
windows of 0 and 1 us, a receive clock that steps back or stands still, seconds across 2^31
and up to 2^32, sizes 0 / 1 / 65535 and a flow of 1.2M records in one call) against the
oracle.  Every comparison is exact -- state, counts, kept reports byte for byte -- except that
where the oracle's double is NaN the GPU's must be NaN; report slots past the kept ones must
stay untouched.  One call equals the same records in several calls; the row form equals the
column form; the resident worker's Update, one record per call, equals both.  The inputs'
preconditions are asserted from the oracle alone in test_flow_value_cases_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_value_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run_gpu(torch, eng, c, splits=(0,), rows=False, rrec=False):
    """The case through Engine.flow_reduce (or flow_reduce_rows) in the calls `splits` starts,
    report buffers pre-filled with C.FILL: (state, reports, counts, report_rec or None) and
    the raw bytes of all four."""
    from mgen_amd import FLOW_REPORT_DTYPE, FLOW_STATE_DTYPE, REC_DTYPE
    d, n_flows, per_flow = c["cols"], c["n_flows"], c["per_flow"]
    flows = eng.flow_init(n_flows, c["window"])
    reports = torch.full((n_flows * per_flow * 96,), C.FILL, dtype=torch.uint8, device="cuda")
    count = torch.zeros(n_flows, dtype=torch.int32, device="cuda")
    rr = torch.full((n_flows * per_flow * 4,), C.FILL, dtype=torch.uint8, device="cuda") \
        if rrec else None
    bounds = list(splits) + [c["n"]]
    for a, b in zip(bounds[:-1], bounds[1:]):
        t = {k: dev(torch, d[k][a:b]) for k in C.COLS}
        kw = dict(reports=reports, per_flow=per_flow, report_count=count, report_rec=rr)
        if rows:
            r = np.zeros(b - a, REC_DTYPE)
            r["flow_id"], r["seq_num"] = d["idx"][a:b] + 1, d["seq"][a:b]
            r["tx_sec"], r["tx_usec"] = d["tx_sec"][a:b], d["tx_usec"][a:b]
            r["msg_len"] = d["msg_len"][a:b]
            r["dst_len"], r["payload_len"] = 4, 7    # fields the reduction does not read
            eng.flow_reduce_rows(flows, n_flows, t["idx"], dev(torch, r.view(np.uint8)),
                                 t["rx_sec"], t["rx_usec"], **kw)
        else:
            eng.flow_reduce(flows, n_flows, t["idx"], t["seq"], t["tx_sec"], t["tx_usec"],
                            t["msg_len"], t["rx_sec"], t["rx_usec"], **kw)
    torch.cuda.synchronize()
    raw = [x.cpu().numpy() for x in (flows, reports, count)] + \
          [rr.cpu().numpy() if rrec else None]
    st = raw[0].view(FLOW_STATE_DTYPE)
    rep = raw[1].view(FLOW_REPORT_DTYPE).reshape(n_flows, per_flow)
    rv = raw[3].view(np.uint32).reshape(n_flows, per_flow) if rrec else None
    return (st, rep, raw[2].view(np.uint32), rv), raw


@pytest.mark.parametrize("name", C.names())
def test_flow_values_vs_oracle(torch, eng, name):
    """One call and every split of the case (one of them after record 1) against the oracle."""
    c = C.by_name(name)
    of, orep, ocnt = C.oracle_run(name)
    for sp in c["splits"]:
        (st, rep, cnt, _), _ = run_gpu(torch, eng, c, sp)
        C.compare(st, rep, cnt, of, orep, ocnt, c["per_flow"])


@pytest.mark.parametrize("w", C.V4_WINDOWS)
def test_flow_values_one_record_windows_pin(torch, eng, w):
    """V4's pin, independent of the oracle: a window opened by a counted record and closed by
    one that is not reports msg_count 1 and that record's latency as ave, min and max -- the
    NumPy value of (rx_sec - tx_sec) + 1e-6 * (rx_usec - tx_usec)."""
    c = C.by_name(f"V4-w{w}")
    _, _, ocnt = C.oracle_run(c["name"])
    (_, rep, cnt, _), _ = run_gpu(torch, eng, c, c["splits"][-1])
    assert np.array_equal(cnt, ocnt)
    pins = C.v4_pins(c, ocnt)
    assert len(pins) > 100
    for f, k, lat in pins:
        r = rep[f, k]
        assert r["msg_count"] == 1, (f, k)
        assert r["latency_ave"] == r["latency_min"] == r["latency_max"] == lat, (f, k)


@pytest.mark.parametrize("name", ["V1", "V3-w0.001", "V3-w0.05", "V3-w1.0", "V3-w600.0",
                                  "V7-short"])
def test_flow_values_rows_equal_columns(torch, eng, name):
    """The row form with report_rec: byte for byte the column form's state, reports, counts
    and report_rec, which equal the oracle's; report_rec names the record that closed each
    kept report, and is untouched past the kept ones."""
    c = C.by_name(name)
    of, orep, ocnt = C.oracle_run(name)
    (st, rep, cnt, rrec), raw_c = run_gpu(torch, eng, c, rrec=True)
    _, raw_r = run_gpu(torch, eng, c, rows=True, rrec=True)
    for a, b in zip(raw_c, raw_r):
        assert np.array_equal(a, b)
    C.compare(st, rep, cnt, of, orep, ocnt, c["per_flow"], rrec)
    d = c["cols"]
    for f in range(c["n_flows"]):
        k = min(int(cnt[f]), c["per_flow"])
        i = rrec[f, :k].astype(np.int64)
        assert (d["idx"][i] == f).all() and (np.diff(i) > 0).all()
        assert np.array_equal(d["rx_sec"][i], rep[f, :k]["rx_sec"])
        assert np.array_equal(d["rx_usec"][i], rep[f, :k]["rx_usec"])


@pytest.mark.parametrize("name", C.names(True, C.FAMILIES[:6]))
def test_worker_flow_update_values(torch, eng, name):
    """Reduced copies of V1-V6 through mgenx_worker_flow_update, one record per call (the
    worker's FlowSM::exact, code apart from the batch kernel's): every returned report and the
    final state against the oracle."""
    from mgen_amd import FLOW_STATE_DTYPE
    c = C.by_name(name, True)
    d = c["cols"]
    of, orep, ocnt = C.oracle_run(name, True, 1024)
    assert int(ocnt.sum()) > 0 and int(ocnt.max()) <= 1024
    flows = eng.flow_init(c["n_flows"], c["window"])
    torch.cuda.synchronize()
    reps = [[] for _ in range(c["n_flows"])]
    w = eng.worker()
    try:
        for i in range(c["n"]):
            f = int(d["idx"][i])
            rep = w.flow_update(flows, f, int(d["seq"][i]), int(d["rx_sec"][i]),
                                int(d["rx_usec"][i]), int(d["msg_len"][i]), int(d["tx_sec"][i]),
                                int(d["tx_usec"][i]))
            if rep is not None:
                reps[f].append(rep)
    finally:
        w.close()
    st = flows.cpu().numpy().view(FLOW_STATE_DTYPE)
    for f, a in enumerate(of):
        s = st[f]
        assert s["msg_count"] == a.msg_count and s["byte_count"] == a.byte_count, f
        assert s["dup_count"] == a.dup_msg_count and s["n_reports"] == a.n_reports, f
        assert s["seq_start"] == a.seq_start and s["window_valid"] == a.window_valid, f
        assert s["latency_sum"] == a.latency_sum, (f, s["latency_sum"], a.latency_sum)
        assert s["latency_min"] == a.latency_min and s["latency_max"] == a.latency_max, f
        assert (s["win_start_sec"], s["win_start_usec"]) == (a.window_start.sec,
                                                             a.window_start.usec), f
        assert (s["win_end_sec"], s["win_end_usec"]) == (a.window_end.sec, a.window_end.usec), f
        assert s["mask_n"] == a.nset, f
        if a.nset:
            assert s["mask_first"] == a.first, f
            assert s["mask"].tobytes() == bytes(a.bits), f
        assert len(reps[f]) == int(ocnt[f]), f
        for k, r in enumerate(reps[f]):
            o = orep[f, k]
            for nm in ("start_sec", "start_usec", "duration", "msg_count", "rate", "loss",
                       "latency_ave", "latency_min", "latency_max", "rx_sec", "rx_usec"):
                assert r[nm] == o[nm] or (nm in C.F8 and np.isnan(o[nm]) and np.isnan(r[nm])), \
                    (f, k, nm, r[nm], o[nm])
