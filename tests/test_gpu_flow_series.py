"""GPU: mgenx_flow_series (records, bytes, latency, jitter and sequence movement per flow and
window of receive time) against the serial model of tests/flow_series_ref.py.  Integer
arithmetic: every comparison is byte equality of the state and the bins."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_dist_ref as D  # noqa: E402
import flow_series_ref as S  # noqa: E402


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
    """flow_dist_ref's data set 5, windows of 250 ms placed so that the first and the last tenth
    of the capture time fall outside them, and its model: computed once."""
    nf, fi, c = D.skew()
    lo, hi = S.span(nf, fi, c)
    t0 = lo + (hi - lo) // 10
    width = 250_000
    n_bins = (hi - (hi - lo) // 10 - t0) // width
    assert n_bins >= 4
    return nf, fi, c, t0, width, n_bins, S.model(nf, n_bins, fi, c, t0, width)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run(torch, eng, nf, n_bins, fi, c, t0, width, cuts=()):
    """One call, or one call per batch cut at `cuts`; returns (state, bins) as numpy."""
    from mgen_amd import FLOW_SERIES_BIN_DTYPE, FLOW_SERIES_STATE_DTYPE
    state, bins = eng.flow_series_init(nf, n_bins)
    edges = [0] + list(cuts) + [len(fi)]
    for a, b in zip(edges[:-1], edges[1:]):
        k = {name: dev(torch, c[name][a:b]) for name in D.COLS}
        eng.flow_series(state, bins, nf, n_bins, t0, width, dev(torch, fi[a:b]), k["seq"],
                        k["tx_sec"], k["tx_usec"], k["msg_len"], k["rx_sec"], k["rx_usec"])
    torch.cuda.synchronize()
    return (state.cpu().numpy().view(FLOW_SERIES_STATE_DTYPE),
            bins.cpu().numpy().view(FLOW_SERIES_BIN_DTYPE).reshape(nf, n_bins))


def check(got, want):
    (s, b), (ws, wb) = got, want
    assert s.dtype == ws.dtype and b.dtype == wb.dtype and b.shape == wb.shape
    if s.tobytes() != ws.tobytes():
        for name in ws.dtype.names:
            bad = np.nonzero(s[name] != ws[name])[0]
            assert len(bad) == 0, ("state", name, bad[:8], s[name][bad[:8]], ws[name][bad[:8]])
    if b.tobytes() != wb.tobytes():
        for name in wb.dtype.names:
            bad = np.argwhere(b[name] != wb[name])
            assert len(bad) == 0, ("bins", name, bad[:8], b[name][tuple(bad[0])],
                                   wb[name][tuple(bad[0])])
    assert s.tobytes() == ws.tobytes() and b.tobytes() == wb.tobytes()


def fitted(nf, fi, c, width):
    """(t0, n_bins): windows of `width` from the lowest receive time, just enough for the highest."""
    lo, hi = S.span(nf, fi, c)
    return lo, (hi - lo) // width + 1


def test_hand_case_with_records_outside_the_bins(torch, eng):
    nf, fi, c = D.hand_case()
    t0, width, n_bins = 1_000_000_420, 500, 2000
    want = S.model(nf, n_bins, fi, c, t0, width)
    assert want[0]["outside"].tolist() == [1, 2, 1]
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_many_tiny_flows(torch, eng):
    nf, fi, c = D.tiny_flows()
    t0, n_bins = fitted(nf, fi, c, 100_000)
    assert nf == 3000 and 5 < n_bins < 40
    check(run(torch, eng, nf, n_bins, fi, c, t0, 100_000), S.model(nf, n_bins, fi, c, t0, 100_000))


def test_flow_and_bin_edges_at_every_chunk_offset(torch, eng):
    nf, fi, c = D.boundary_sweep()
    t0, n_bins = fitted(nf, fi, c, 50_000)
    assert len(fi) == 80_200 and nf == 400 and 300 < n_bins < 360
    check(run(torch, eng, nf, n_bins, fi, c, t0, 50_000), S.model(nf, n_bins, fi, c, t0, 50_000))


@pytest.mark.parametrize("width", [300, 2**40])
def test_one_flow_short_runs_and_one_run_per_chunk(torch, eng, width):
    nf, fi, c = D.one_flow_every_97th()
    t0, n_bins = fitted(nf, fi, c, width)
    if width == 300:
        assert 25_000 < n_bins < 29_000           # nearly a record per run
    else:
        assert n_bins == 1 and len(fi) >= 39 * 1024   # the carry of M across 40 chunks
    want = S.model(nf, n_bins, fi, c, t0, width)
    assert int(want[1]["late"].sum()) == len(fi) // 97
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_one_flow_whose_maximum_comes_first(torch, eng):
    nf, fi, c = D.one_flow_max_first()
    t0, n_bins = fitted(nf, fi, c, 1_000_000)
    want = S.model(nf, n_bins, fi, c, t0, 1_000_000)
    assert int(want[1]["late"].sum()) >= len(fi) - 18     # every record after the 18th
    assert int(want[1]["fresh"][0, 1:].sum()) == 0
    check(run(torch, eng, nf, n_bins, fi, c, t0, 1_000_000), want)


def test_one_dominant_flow_with_both_ends_outside(torch, eng, skew):
    nf, fi, c, t0, width, n_bins, want = skew
    assert int(want[0]["outside"][0]) > 0 and int(want[0]["n"][0]) > len(fi) // 2 - 2000
    assert int(want[1]["n"].sum()) + int(want[0]["outside"].sum()) == int(want[0]["n"].sum())
    check(run(torch, eng, nf, n_bins, fi, c, t0, width), want)


def test_receive_times_shuffled_within_a_flow(torch, eng):
    nf, fi, c = S.shuffled_rx()
    t0, n_bins = fitted(nf, fi, c, 10_000)
    check(run(torch, eng, nf, n_bins, fi, c, t0, 10_000), S.model(nf, n_bins, fi, c, t0, 10_000))


def test_streaming_batches_equal_one_call(torch, eng, skew):
    nf, fi, c, t0, width, n_bins, want = skew
    cut = run(torch, eng, nf, n_bins, fi, c, t0, width, cuts=(1, 777, 20_000, len(fi) - 1))
    check(cut, want)


def test_empty_batch_and_bad_arguments(torch, eng):
    from mgen_amd import MgenxError
    nf, n_bins = 5, 7
    state, bins = eng.flow_series_init(nf, n_bins)
    state.fill_(0x5A)
    bins.fill_(0x5A)
    z32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    z16 = torch.zeros(1, dtype=torch.int16, device="cuda")
    eng.flow_series(state, bins, nf, n_bins, 0, 1000, z32, z32, z32, z32, z16, z32, z32, n=0)
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all()) and bool((bins == 0x5A).all())
    with pytest.raises(MgenxError):
        eng.flow_series(state, bins, nf, n_bins, 0, 0, z32, z32, z32, z32, z16, z32, z32)
    with pytest.raises(MgenxError):
        eng.flow_series(state, bins, nf, 0, 0, 1000, z32, z32, z32, z32, z16, z32, z32)
    with pytest.raises(MgenxError):
        eng.flow_series_init(nf, 0)
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all()) and bool((bins == 0x5A).all())


def test_one_bin_equals_flow_dist(torch, eng, skew):
    """The existing kernel as the cross-check: one all-covering bin per flow."""
    from mgen_amd import FLOW_DIST_DTYPE
    nf, fi, c = skew[:3]
    lo, hi = S.span(nf, fi, c)
    state, bins = run(torch, eng, nf, 1, fi, c, lo, hi - lo + 1)
    dist, _ = eng.flow_dist_init(nf, hist=False)
    k = {name: dev(torch, c[name]) for name in D.COLS}
    eng.flow_dist(dist, None, nf, dev(torch, fi), k["seq"], k["tx_sec"], k["tx_usec"],
                  k["msg_len"], k["rx_sec"], k["rx_usec"])
    torch.cuda.synchronize()
    dist = dist.cpu().numpy().view(FLOW_DIST_DTYPE)
    assert int(dist["n"].sum()) > 59_000 and not state["outside"].any()
    for name in ("n", "bytes", "lat_sum", "lat_min", "lat_max", "jitter_sum"):
        assert np.array_equal(bins[:, 0][name], dist[name]), name
    assert np.array_equal(bins[:, 0]["late"], dist["reordered"])
    assert np.array_equal(state["seq_max"], dist["seq_max"])


def test_analyze_text_log_series(skew):
    from mgen_amd import analyze_text_log_series
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
        if fi[i] == D.NONE:
            continue
        f = int(fi[i])
        lines.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                     "sent>%d.%06d size>%d \n" % (
                         c["rx_sec"][i], c["rx_usec"][i], f + 1, c["seq"][i], 1 + f % 2,
                         c["tx_sec"][i], c["tx_usec"][i], c["msg_len"][i]))
        keep.append(i)
    keep = np.array(keep)
    width = 50_000
    keys, state, bins, t0, n_lines, n_bad = analyze_text_log_series("".join(lines).encode(), width)
    assert n_lines == len(lines) and n_bad == 2 * ((m - 8) // 3000 + 1)
    kept = {k: v[:m][keep] for k, v in c.items()}
    lo, hi = S.span(nf, fi[keep], kept)
    assert t0 == lo and bins.shape[1] == (hi - lo) // width + 1 > 8
    ws, wb = S.model(nf, bins.shape[1], fi[keep], kept, t0, width)
    live = np.nonzero(ws["n"])[0]
    assert len(keys) == len(live) == len(state) == len(bins)
    mine = keys["flow_id"].astype(np.int64) - 1    # the returned order -> this test's flow index
    assert sorted(mine.tolist()) == live.tolist()
    assert np.array_equal(keys["src"]["addr"][:, 3], 1 + mine % 2)
    check((state, bins), (ws[mine], wb[mine]))
    assert not state["outside"].any() and int(bins["n"].sum()) == len(keep)
    # given t0 and n_bins are taken as they are
    k2, s2, b2, t2, _, _ = analyze_text_log_series("".join(lines).encode(), width,
                                                   t0_us=lo + 3 * width, n_bins=5)
    ws2, wb2 = S.model(nf, 5, fi[keep], kept, lo + 3 * width, width)
    assert t2 == lo + 3 * width and b2.shape == (len(live), 5)
    check((s2, b2), (ws2[mine], wb2[mine]))


def test_series_main_writes_the_table(tmp_path, capsys):
    from mgen_amd import series
    log = tmp_path / "recv.log"
    rows = []
    for i in range(300):                           # two flows, 1 ms apart, seq 7 of flow 1 lost
        f, seq = i % 2, i // 2
        if (f, seq) == (0, 7):
            continue
        rx = 1_700_000_000_000_000 + i * 1000
        rows.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                    "sent>%d.%06d size>100 \n" % (rx // 10**6, rx % 10**6, f + 1, seq, f + 1,
                                                   (rx - 250) // 10**6, (rx - 250) % 10**6))
    log.write_text("".join(rows))
    out = tmp_path / "series.txt"
    assert series.main([str(log), "0.05", str(out)]) == 0
    text = out.read_text()
    sets = text.split("\n\n\n")
    assert len(sets) == 2 and sets[0].startswith("# flow>1 src>10.0.0.1/5001 dst>10.0.0.9/5000\n")
    data = [[int(v) for v in ln.split()] for ln in sets[0].split("\n") if ln and ln[0] != "#"]
    assert len(data) == 6 and [r[0] for r in data] == [
        1_700_000_000_000_000 + b * 50_000 for b in range(6)]
    # bin_start n bytes fresh late advance lat_min lat_max lat_sum jitter_sum
    assert data[0] == [1_700_000_000_000_000, 24, 2400, 24, 0, 25, 250, 250, 6000, 0]
    assert sum(r[1] for r in data) == 149 and sum(r[5] for r in data) == 150
    assert series.main([str(log), "0.05"]) == 0 and capsys.readouterr().out == text
    assert series.main([str(log)]) == 2
