"""GPU: a context's workspaces grow under calls that have already carved them.

flow_reduce, flow_dist, flow_series and msg_match each keep one device buffer on the context that
is reallocated when a call needs more than it holds and is carved into the call's arrays.  Each
case makes a small call, a call that forces the reallocation and the small call again on ONE
Engine, and compares every output array of every call, byte for byte, with the same call on a
fresh Engine (whose buffer was sized by that call alone).  flow_reduce has a second case whose
calls all take the single-pass scan: its epoch-tagged words live in their own allocation and must
survive the growth of the main workspace and then be reused.  Correctness against the oracle and
the serial models is the other tests' job."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_FLOWS = 8          # the counting-sort path of flow_reduce (n_flows + 1 <= 1536 bins)
PER_FLOW = 4
N_BINS = 16
SIZES = (64, 20_000, 64)
SCAN1_SIZES = (5_000, 300_000, 5_000, 5_000)   # at most 74 tiles: the single-pass scan each time


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def data():
    """The records of every size used, generated once."""
    from mgen_amd.workloads import poisson_flows
    out = {}
    for n in sorted(set(SIZES + SCAN1_SIZES)):
        d = poisson_flows(n, N_FLOWS, seed=n, loss=0.0, dup=0.0, mean_gap_us=20_000)
        assert len(d["seq"]) == n
        out[n] = d
    return out


def dev(torch, a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else a.astype(dtype))
    return torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32).copy()).cuda()


def cols(torch, d):
    k = {name: dev(torch, d[name]) for name in ("seq", "tx_sec", "tx_usec", "msg_len", "rx_sec",
                                                "rx_usec")}
    k["flow_idx"] = dev(torch, d["flow_id"] - 1, np.uint32)
    return k


def host(torch, *tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def flow_reduce(torch, eng, d):
    k = cols(torch, d)
    n = len(d["seq"])
    flows = eng.flow_init(N_FLOWS, 0.05)
    reports = torch.zeros(N_FLOWS * PER_FLOW * 96, dtype=torch.uint8, device="cuda")
    count = torch.zeros(N_FLOWS, dtype=torch.int32, device="cuda")
    rec = torch.zeros(N_FLOWS * PER_FLOW, dtype=torch.int32, device="cuda")
    eng.flow_reduce(flows, N_FLOWS, k["flow_idx"], k["seq"], k["tx_sec"], k["tx_usec"],
                    k["msg_len"], k["rx_sec"], k["rx_usec"], n=n, reports=reports,
                    per_flow=PER_FLOW, report_count=count, report_rec=rec)
    return host(torch, flows, reports, count, rec)


def flow_dist(torch, eng, d):
    k = cols(torch, d)
    dist, hist = eng.flow_dist_init(N_FLOWS)
    eng.flow_dist(dist, hist, N_FLOWS, k["flow_idx"], k["seq"], k["tx_sec"], k["tx_usec"],
                  k["msg_len"], k["rx_sec"], k["rx_usec"])
    return host(torch, dist, hist)


def flow_series(torch, eng, d):
    k = cols(torch, d)
    rx = d["rx_sec"].astype(np.int64) * 1_000_000 + d["rx_usec"]
    t0 = int(rx.min())
    width = max(1, int(rx.max() - t0) // (N_BINS - 2) + 1)
    state, bins = eng.flow_series_init(N_FLOWS, N_BINS)
    eng.flow_series(state, bins, N_FLOWS, N_BINS, t0, width, k["flow_idx"], k["seq"], k["tx_sec"],
                    k["tx_usec"], k["msg_len"], k["rx_sec"], k["rx_usec"])
    return host(torch, state, bins)


def msg_match(torch, eng, d):
    """The sender logged every record; the receiver lost every 17th and saw every 29th twice."""
    n = len(d["seq"])
    fi = (d["flow_id"] - 1).astype(np.uint32)
    send = {"flow_idx": fi, "seq": d["seq"], "t_sec": d["tx_sec"], "t_usec": d["tx_usec"],
            "len": d["msg_len"].astype(np.uint32)}
    i = np.arange(n)
    pick = np.sort(np.concatenate([i[i % 17 != 16], i[i % 29 == 28]]), kind="stable")
    recv = {"flow_idx": fi[pick], "seq": d["seq"][pick], "tx_sec": d["tx_sec"][pick],
            "tx_usec": d["tx_usec"][pick], "rx_sec": d["rx_sec"][pick],
            "rx_usec": d["rx_usec"][pick]}
    s = {name: dev(torch, v) for name, v in send.items()}
    r = {name: dev(torch, v) for name, v in recv.items()}
    return host(torch, *eng.msg_match(N_FLOWS, s, r))


def grow_and_compare(torch, data, call, sizes):
    from mgen_amd import Engine
    eng = Engine(0)
    try:
        got = [call(torch, eng, data[n]) for n in sizes]
    finally:
        eng.close()
    for j, n in enumerate(sizes):
        fresh = Engine(0)
        try:
            want = call(torch, fresh, data[n])
        finally:
            fresh.close()
        assert len(got[j]) == len(want)
        for a, (g, w) in enumerate(zip(got[j], want)):
            assert g == w, f"call {j} ({n} records), output {a} differs from a fresh engine's"


@pytest.mark.parametrize("call", [flow_reduce, flow_dist, flow_series, msg_match])
def test_workspace_grows_between_calls(torch, data, call):
    grow_and_compare(torch, data, call, SIZES)


def test_flow_reduce_scan_words_survive_workspace_growth(torch, data):
    grow_and_compare(torch, data, flow_reduce, SCAN1_SIZES)
