"""GPU: mgenx_flow_dist (latency histogram, jitter, gaps, reordering per flow) against the
serial model of tests/flow_dist_ref.py.  Integer arithmetic: every comparison is byte equality
of the state and the histogram."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as R  # noqa: E402

PERMILLE = (1, 500, 900, 990, 999, 1000)


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
    """Data set 5 with its model, computed once."""
    nf, fi, c = R.skew()
    return nf, fi, c, R.model(nf, fi, c)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run(torch, eng, nf, fi, c, cuts=(), hist=True):
    """One call, or one call per batch cut at `cuts`; returns (dist, hist) as numpy."""
    from mgen_amd import FLOW_DIST_DTYPE
    dist, h = eng.flow_dist_init(nf, hist=hist)
    edges = [0] + list(cuts) + [len(fi)]
    for a, b in zip(edges[:-1], edges[1:]):
        k = {name: dev(torch, c[name][a:b]) for name in R.COLS}
        eng.flow_dist(dist, h, nf, dev(torch, fi[a:b]), k["seq"], k["tx_sec"], k["tx_usec"],
                      k["msg_len"], k["rx_sec"], k["rx_usec"])
    torch.cuda.synchronize()
    return (dist.cpu().numpy().view(FLOW_DIST_DTYPE),
            h.cpu().numpy().view(np.uint64) if hist else None)


def check(got, want):
    (d, h), (wd, wh) = got, want
    if d.tobytes() != wd.tobytes():
        for f in range(len(wd)):
            for name in wd.dtype.names:
                assert np.array_equal(d[f][name], wd[f][name]), (f, name, d[f][name], wd[f][name])
    assert h.tobytes() == wh.tobytes(), np.argwhere(h != wh)[:8]


def test_hand_case(torch, eng):
    nf, fi, c = R.hand_case()
    check(run(torch, eng, nf, fi, c), R.model(nf, fi, c))


def test_many_tiny_flows(torch, eng):
    nf, fi, c = R.tiny_flows()
    assert 5000 < len(fi) < 7000
    check(run(torch, eng, nf, fi, c), R.model(nf, fi, c))


@pytest.mark.parametrize("data", [R.one_flow_max_first, R.one_flow_every_97th])
def test_one_long_flow_carries_its_maximum_across_chunks(torch, eng, data):
    nf, fi, c = data()
    want = R.model(nf, fi, c)
    if data is R.one_flow_max_first:
        assert int(want[0][0]["reordered"]) >= len(fi) - 18     # every record after the 18th
    else:
        assert int(want[0][0]["reordered"]) == len(fi) // 97
    check(run(torch, eng, nf, fi, c), want)


def test_maximum_carried_past_the_carry_kernels_first_round(torch, eng):
    """One flow of 2^20 + 1025 + 3 records (1026 chunks: flow_dist_carry_kernel walks a second
    round of 1024 chunks with the flow still open).  The largest seq is at input position 0 and
    the later ones rise below it, so a maximum that is not carried leaves a record unreordered.
    The expectation is closed-form; the model (vectorised over one flow) checks the rest."""
    n = 2**20 + 1025 + 3
    seq = np.concatenate([[n - 1], np.arange(n - 1)])
    nf, fi, c = (1,) + R._synth(np.zeros(n, np.int64), seq, 23)
    d, h = run(torch, eng, nf, fi, c)
    assert int(d[0]["n"]) == n and int(d[0]["reordered"]) == n - 1
    assert (int(d[0]["seq_min"]), int(d[0]["seq_max"])) == (0, n - 1)
    assert int(d[0]["reorder_max"]) == n - 1 and int(d[0]["reorder_sum"]) == n * (n - 1) // 2
    check((d, h), R.model(nf, fi, c))


def test_flow_edges_at_every_chunk_offset(torch, eng):
    nf, fi, c = R.boundary_sweep()
    assert len(fi) == 80_200
    check(run(torch, eng, nf, fi, c), R.model(nf, fi, c))


def test_one_dominant_flow(torch, eng, skew):
    nf, fi, c, want = skew
    assert int(want[0][0]["n"]) > len(fi) // 2 - 2000 and int((fi == R.NONE).sum()) > 300
    assert int(want[0]["reordered"].sum()) > 1000 and int(want[0]["lat_neg"].sum()) == 0
    check(run(torch, eng, nf, fi, c), want)


def test_streaming_batches_equal_one_call(torch, eng, skew):
    nf, fi, c, want = skew
    n = len(fi)
    one = run(torch, eng, nf, fi, c)
    cut = run(torch, eng, nf, fi, c, cuts=(1, 777, 20_000, n - 1))
    assert cut[0].tobytes() == one[0].tobytes() and cut[1].tobytes() == one[1].tobytes()
    check(cut, want)


def test_without_histogram_and_empty_batch(torch, eng, skew):
    from mgen_amd import FLOW_DIST_DTYPE
    nf, fi, c, want = skew
    d, h = run(torch, eng, nf, fi, c, hist=False)
    assert h is None and d.tobytes() == want[0].tobytes()
    # n == 0 leaves both arrays as they are
    dist, hist = eng.flow_dist_init(nf)
    dist.view(torch.uint8).fill_(0x5A)
    hist.fill_(77)
    z32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    z16 = torch.zeros(1, dtype=torch.int16, device="cuda")
    eng.flow_dist(dist, hist, nf, z32, z32, z32, z32, z16, z32, z32, n=0)
    torch.cuda.synchronize()
    assert bool((dist == 0x5A).all()) and bool((hist == 77).all())
    assert dist.numel() == nf * FLOW_DIST_DTYPE.itemsize


def test_quantiles(torch, eng, skew):
    from mgen_amd import FLOW_DIST_DTYPE, flow_dist_bin, flow_dist_bin_lo
    for nf, fi, c in (R.hand_case(), skew[:3]):
        nf += 2                                    # flows past the data: the last one stays empty
        wd, wh = R.model(nf, fi, c)
        dist, hist = eng.flow_dist_init(nf)
        k = {name: dev(torch, c[name]) for name in R.COLS}
        eng.flow_dist(dist, hist, nf, dev(torch, fi), k["seq"], k["tx_sec"], k["tx_usec"],
                      k["msg_len"], k["rx_sec"], k["rx_usec"])
        q = eng.flow_dist_quantiles(dist, hist, nf, PERMILLE).cpu().numpy()
        assert dist.cpu().numpy().view(FLOW_DIST_DTYPE).tobytes() == wd.tobytes()
        want = R.quantiles(wd, wh, PERMILLE)
        assert np.array_equal(q, want)
        assert (q[nf - 1] == -2**63).all()         # the empty flow
        for f in range(nf - 1):
            lat = np.sort(R.latencies(fi, c, f))
            if len(lat) == 0:
                assert (q[f] == -2**63).all()
                continue
            for j, pm in enumerate(PERMILLE):
                x = int(lat[R.rank(pm, len(lat)) - 1])
                if x < 0:
                    assert q[f, j] == -1
                elif x >= 2**32:
                    assert q[f, j] == 2**32
                else:
                    assert flow_dist_bin_lo(flow_dist_bin(x)) <= x <= q[f, j]
                    assert q[f, j] == flow_dist_bin_lo(flow_dist_bin(x) + 1) - 1


def test_analyze_text_log_dist(skew):
    from mgen_amd import analyze_text_log_dist
    nf, fi, c = skew[:3]
    m = 20_000
    fi = fi[:m]
    lines, keep = [], []
    for i in range(m):
        if i % 3000 == 7:
            lines += ["1700000000.000001 START Mgen Version 5.1.1\n",
                      "1700000000.000002 LISTEN proto>UDP port>5000\n",
                      "1700000000.000003 RECV proto>UDP flow>x seq>1 src>10.0.0.1/5001 "
                      "dst>10.0.0.9/5000 sent>1700000000.000000 size>64 \n",
                      "no such event\n"]
        if fi[i] == R.NONE:
            continue
        f = int(fi[i])
        lines.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                     "sent>%d.%06d size>%d \n" % (
                         c["rx_sec"][i], c["rx_usec"][i], f + 1, c["seq"][i], 1 + f % 2,
                         c["tx_sec"][i], c["tx_usec"][i], c["msg_len"][i]))
        keep.append(i)
    keep = np.array(keep)
    keys, dist, quant, hist, n_lines, n_bad = analyze_text_log_dist(
        "".join(lines).encode(), permille=PERMILLE)
    assert n_lines == len(lines) and n_bad == 2 * ((m - 8) // 3000 + 1)
    wd, wh = R.model(nf, fi[keep], {k: v[:m][keep] for k, v in c.items()})
    live = np.nonzero(wd["n"])[0]
    assert len(keys) == len(live) == len(dist)
    mine = keys["flow_id"].astype(np.int64) - 1    # the returned order -> this test's flow index
    assert sorted(mine.tolist()) == live.tolist()
    assert np.array_equal(keys["src"]["addr"][:, 3], 1 + mine % 2)
    assert dist.tobytes() == wd[mine].tobytes()
    assert hist.tobytes() == wh[mine].tobytes()
    assert np.array_equal(quant, R.quantiles(wd[mine], wh[mine], PERMILLE))
