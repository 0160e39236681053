"""GPU: mgenx_msg_match_multi_ex (the loss runs per receiver, their list, and the loss that pairs
of receivers share) against the serial model of tests/msg_match_multi_ex_ref.py.  Integer
arithmetic: every output is compared byte for byte, and every call runs with guard regions around
its outputs.  The shapes sit on the edges of the passes: a wave is 64 owners, a workgroup of the
run pass 1024 (kChunk), a wave of the pair pass 4096."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msg_match_multi_ex_ref as MX  # noqa: E402
import msg_match_multi_ref as MM  # noqa: E402

NONE = MM.NONE
T0 = 1_700_000_000
GUARD = 256          # bytes on either side of every output
PAT = 0xA5
EINVAL = -1
BASE_NAMES = ("send_mask", "recv_send", "recv_first", "cells", "fanout", "stats")
BASE_DTYPES = (np.uint64, np.uint32, np.uint8, MM.CELL, MM.FANOUT, MM.STATS)
ALL = "slp"          # the parts: s = run statistics, l = run list, p = pair matrix


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
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def call(torch, eng, nf, n_rcv, send, recv, opts=0, parts=ALL, min_run=1, run_cap=0, expect=0,
         lx="struct", null_runs=False):
    """One mgenx_msg_match_multi_ex call with GUARD bytes of PAT before and after every output.
    lx: "struct" (the parts named in `parts`), "null" (lx == NULL) or "plain"
    (mgenx_msg_match_multi itself).  Returns the outputs as a dict of numpy arrays; `runs` is
    None when the list did not fit, after the check that not one byte of it changed.  With
    expect != 0 the call must return that code and leave every output byte as it was."""
    from mgen_amd import MultiLoss, _ptr, _stream
    ns, nr = len(send["flow_idx"]), len(recv["flow_idx"])
    s = [dev(torch, send[k]) for k in MM.SEND_COLS]
    r = [dev(torch, recv[k]) for k in MM.RECV_COLS]
    n_cells = nf * n_rcv
    sizes = dict(send_mask=8 * ns, recv_send=4 * nr, recv_first=nr, cells=n_cells * 80,
                 fanout=nf * 560, stats=32, rcv_runs=n_cells * 160, runs=run_cap * 40, n_runs=8,
                 pairs=n_cells * n_rcv * 32)
    if expect:       # a refused call never reaches the outputs: any size will do
        sizes = {k: min(b, 4096) for k, b in sizes.items()}
    bufs = {k: torch.full((GUARD + b + GUARD,), PAT, dtype=torch.uint8, device="cuda")
            for k, b in sizes.items()}
    at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    cols = [_ptr(t) if t.numel() else None for t in s] + [ns] + \
        [_ptr(t) if t.numel() else None for t in r] + [nr, n_rcv, nf, opts] + \
        [ctypes.c_void_p(at[k]) for k in BASE_NAMES] + [None]
    if lx == "plain":
        rc = eng.lib.mgenx_msg_match_multi(eng.ctx, *cols, _stream(0))
    else:
        st = MultiLoss(min_run=min_run, run_cap=run_cap)
        if "s" in parts:
            st.dev_rcv_runs = at["rcv_runs"]
        if "l" in parts:
            st.dev_n_runs = at["n_runs"]
            st.dev_runs = None if null_runs else at["runs"]
        if "p" in parts:
            st.dev_pairs = at["pairs"]
        rc = eng.lib.mgenx_msg_match_multi_ex(
            eng.ctx, *cols, None if lx == "null" else ctypes.byref(st), _stream(0))
    assert rc == expect, (rc, eng.lib.mgenx_last_error(eng.ctx))
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    if expect:
        for k, h in host.items():
            assert (h == PAT).all(), k           # a refused call writes nothing
        return {}
    written = set(BASE_NAMES)
    if lx == "struct":
        written |= {k for p, k in (("s", "rcv_runs"), ("l", "n_runs"), ("p", "pairs")) if p in parts}
    got = {}
    for k, h in host.items():
        if k not in written and k != "runs":
            assert (h == PAT).all(), k           # a part that is off
            continue
        assert (h[:GUARD] == PAT).all() and (h[GUARD + sizes[k]:] == PAT).all(), "write outside"
        got[k] = h[GUARD:GUARD + sizes[k]].copy()
    for k, dt in zip(BASE_NAMES, BASE_DTYPES):
        got[k] = got[k].view(dt)
    got["cells"] = got["cells"].reshape(nf, n_rcv)
    if "rcv_runs" in got:
        got["rcv_runs"] = got["rcv_runs"].view(MX.RUNS).reshape(nf, n_rcv)
    if "pairs" in got:
        got["pairs"] = got["pairs"].view(MX.PAIR).reshape(nf, n_rcv, n_rcv)
    runs = got.pop("runs")
    if "n_runs" in got:
        got["n_runs"] = int(got["n_runs"].view(np.uint64)[0])
        if got["n_runs"] <= run_cap:
            got["runs"] = runs.view(MX.RUN)[:got["n_runs"]]
            assert (runs[got["n_runs"] * 40:] == PAT).all(), "the list's spare entries"
        else:
            assert (runs == PAT).all(), "a list that does not fit stays untouched"
            got["runs"] = None
    else:
        assert (runs == PAT).all()
    return got


def same(g, w, name):
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, name
    if g.tobytes() == w.tobytes():
        return
    if w.dtype.names:
        for fld in w.dtype.names:
            bad = np.argwhere(g[fld] != w[fld])
            assert len(bad) == 0, (name, fld, bad[:8].tolist(), g[fld][tuple(bad[0])],
                                   w[fld][tuple(bad[0])])
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]])


def check(got, want, parts=ALL):
    for k in BASE_NAMES:
        same(got[k], want["base"][k], k)
    if "s" in parts:
        same(got["rcv_runs"], want["rcv_runs"], "rcv_runs")
    if "l" in parts:
        assert got["n_runs"] == len(want["runs"])
        if got["runs"] is not None:
            same(got["runs"], want["runs"], "runs")
    if "p" in parts:
        same(got["pairs"], want["pairs"], "pairs")
    return got


def both(torch, eng, nf, n_rcv, send, recv, opts=0, min_run=1, want=None):
    """All three parts against the model: the two passes of the run list."""
    if want is None:
        want = MX.model(nf, n_rcv, send, recv, no_time=bool(opts & 1), min_run=min_run)
    n = len(want["runs"])
    if n:
        first = check(call(torch, eng, nf, n_rcv, send, recv, opts, min_run=min_run), want)
        assert first["runs"] is None
    got = check(call(torch, eng, nf, n_rcv, send, recv, opts, min_run=min_run, run_cap=n), want)
    assert got["runs"] is not None
    return got, want


def make_send(flow, seq=None, size=100):
    """Send columns from the flows (seq: the record's number within its flow unless given); the
    stamp is i ms after T0."""
    flow = np.asarray(flow, np.uint32)
    n = len(flow)
    if seq is None:
        seq = np.zeros(n, np.uint32)
        for f in np.unique(flow):
            seq[flow == f] = np.arange((flow == f).sum())
    t = T0 * 10**6 + np.arange(n, dtype=np.int64) * 1000
    return dict(flow_idx=flow, seq=np.asarray(seq, np.uint32), t_sec=(t // 10**6).astype(np.uint32),
                t_usec=(t % 10**6).astype(np.uint32),
                len=np.broadcast_to(np.asarray(size, np.uint32), (n,)).copy())


def logs(send, per_rcv, lat=300):
    """The receivers' logs one after the other: per_rcv = [(receiver, send indices), ...]."""
    parts = []
    for rcv, idx in per_rcv:
        idx = np.asarray(idx, np.int64)
        rx = send["t_sec"][idx].astype(np.int64) * 10**6 + send["t_usec"][idx] + lat + rcv
        parts.append(dict(flow_idx=send["flow_idx"][idx], seq=send["seq"][idx],
                          tx_sec=send["t_sec"][idx], tx_usec=send["t_usec"][idx],
                          rx_sec=(rx // 10**6).astype(np.uint32),
                          rx_usec=(rx % 10**6).astype(np.uint32),
                          rcv=np.full(len(idx), rcv, np.uint32)))
    if not parts:
        return MM.cols(MM.RECV_COLS, [])
    return {k: np.concatenate([p[k] for p in parts]) for k in MM.RECV_COLS}


def without(n, lost):
    """The indices 0 .. n - 1 that are not in `lost`."""
    keep = np.ones(n, bool)
    keep[np.asarray(lost, np.int64)] = False
    return np.nonzero(keep)[0]


# ------------------------------------------------------------------ the shapes of one flow
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_one_flow_none_all_and_every_other_lost(torch, eng, n):
    send = make_send(np.zeros(n))
    ix = np.arange(n)
    # receiver 0 loses nothing, 1 everything, 2 the odd ranks, 3 the even ones
    recv = logs(send, [(0, ix), (2, ix[::2]), (3, ix[1::2])])
    got, _ = both(torch, eng, 1, 4, send, recv)
    rr = got["rcv_runs"][0]
    assert rr["loss_runs"].tolist() == [0, 1, n // 2, (n + 1) // 2]
    assert rr["loss_run_max"].tolist() == [0, n, 1 if n > 1 else 0, 1]
    assert int(got["pairs"][0, 0, 0]["span"]) == n
    assert got["pairs"][0, 1].tobytes() == bytes(4 * 32)       # receiver 1 has no span


def test_the_hand_case_and_the_engine_method(torch, eng):
    nf, n_rcv, send, recv = MM.hand_case()
    got, want = both(torch, eng, nf, n_rcv, send, recv)
    assert got["rcv_runs"]["loss_runs"].tolist() == [[2, 3, 1], [1, 2, 1]]
    assert tuple(int(v) for v in got["pairs"][0, 0, 1]) == (6, 3, 2, 2)
    out = eng.msg_match_multi_loss(nf, n_rcv, {k: dev(torch, v) for k, v in send.items()},
                                   {k: dev(torch, v) for k, v in recv.items()})
    torch.cuda.synchronize()
    assert len(out) == 9
    for name, t in zip(BASE_NAMES + ("rcv_runs", "runs", "pairs"), out):
        assert t.cpu().numpy().tobytes() == got[name].tobytes(), name
    out = eng.msg_match_multi_loss(nf, n_rcv, {k: dev(torch, v) for k, v in send.items()},
                                   {k: dev(torch, v) for k, v in recv.items()}, run_stats=False,
                                   min_run=None, timeline=(2000 * 10**6 + 300, 300, 2))
    assert len(out) == 11 and out[8] is None and out[9] is None
    assert out[10].cpu().numpy().tobytes() == got["pairs"].tobytes()


@pytest.mark.parametrize("n,first,last", [(2100, 10, 2090), (3300, 500, 3200)])
def test_a_run_through_whole_chunks(torch, eng, n, first, last):
    # the carry passes through one chunk (two for 3300) untouched; receiver 1 loses nothing
    send = make_send(np.zeros(n))
    recv = logs(send, [(0, without(n, np.arange(first, last + 1))), (1, np.arange(n))])
    got, _ = both(torch, eng, 1, 2, send, recv)
    assert [tuple(int(v) for v in r)[:6] for r in got["runs"]] == \
        [(0, last - first + 1, first, last, 0, 0)]


def test_runs_at_the_chunk_edges(torch, eng):
    n = 2300
    send = make_send(np.zeros(n))
    recv = logs(send, [
        (0, without(n, np.arange(1000, 1024))),               # ends on chunk 0's last position
        (1, without(n, np.arange(1024, 1030))),               # starts on chunk 1's first
        (2, without(n, np.r_[1023, 2047, 2048])),             # one owner each side of an edge
        (3, without(n, np.r_[0:64, 2240:2300])),              # head and tail: whole tiles
        (4, without(n, np.r_[63, 64, 127, 1087, 1088]))])     # the edges of waves
    got, _ = both(torch, eng, 1, 5, send, recv)
    assert got["rcv_runs"][0]["loss_runs"].tolist() == [1, 1, 2, 2, 3]
    assert got["rcv_runs"][0]["loss_run_max"].tolist() == [24, 6, 2, 64, 2]


@pytest.mark.parametrize("n_rcv", [1, 2, 63, 64])
def test_the_receiver_counts(torch, eng, n_rcv):
    n = 200
    send = make_send(np.arange(n) % 2)
    rng = np.random.default_rng(n_rcv)
    per = [(r, np.nonzero(rng.integers(0, 4, n) > 0)[0]) for r in range(n_rcv)]
    got, _ = both(torch, eng, 2, n_rcv, send, logs(send, per))
    assert int(got["rcv_runs"]["loss_runs"].min()) > 0


@pytest.mark.parametrize("lossy", [True, False])
def test_receiver_63(torch, eng, lossy):
    # the lossy one among 64, and the only one anything was delivered to
    n = 1100
    send = make_send(np.zeros(n))
    hears = without(n, np.r_[5:9, 500:700, 1099])
    per = [(r, np.arange(n)) for r in range(63)] if lossy else []
    got, _ = both(torch, eng, 1, 64, send, logs(send, per + [(63, hears)]))
    assert int(got["rcv_runs"][0, 63]["loss_runs"]) == 3
    assert int(got["rcv_runs"][0, 0]["loss_runs"]) == (0 if lossy else 1)
    assert tuple(int(v) for v in got["pairs"][0, 63, 63]) == (1099, 204, 204, 204)
    assert int(got["send_mask"][0]) == (2**64 - 1 if lossy else 2**63)


def test_64_flows_of_one_owner(torch, eng):
    send = make_send(np.arange(64))
    recv = logs(send, [(0, np.arange(0, 64, 2)), (1, np.arange(64)), (2, [63])])
    got, _ = both(torch, eng, 64, 3, send, recv)
    assert got["rcv_runs"]["loss_runs"][:, 0].tolist() == [0, 1] * 32
    assert got["n_runs"] == 32 + 63


def test_flows_of_three_owners_over_the_edges(torch, eng):
    # 700 flows in 2100 owners: 64 and 1024 are no multiples of 3
    nf = 700
    send = make_send(np.repeat(np.arange(nf), 3))
    rng = np.random.default_rng(3)
    per = [(r, np.nonzero(rng.integers(0, 3, 3 * nf) > 0)[0]) for r in range(3)]
    both(torch, eng, nf, 3, send, logs(send, per))
    # the same flows interleaved in the log: the sort brings them together
    send = make_send(np.tile(np.arange(nf), 3))
    both(torch, eng, nf, 3, send, logs(send, per))


def test_flows_without_owners_and_cells_never_delivered(torch, eng):
    # flow 1 is receiver-only (orphans), flow 2 reaches receiver 0 only, flow 3 nobody
    flow = np.r_[np.zeros(70), np.full(130, 2), np.full(90, 3), np.zeros(10)]
    send = make_send(flow)
    recv = logs(send, [(0, np.r_[0:60, 70:180]), (1, np.r_[3:50, 295:300])])
    ghost = {k: v[:4].copy() for k, v in recv.items()}
    ghost["flow_idx"][:] = 1
    recv = {k: np.concatenate([recv[k], ghost[k]]) for k in recv}
    got, _ = both(torch, eng, 4, 2, send, recv)
    assert got["rcv_runs"]["loss_runs"].tolist() == [[1, 2], [0, 0], [1, 1], [1, 1]]
    assert got["rcv_runs"]["loss_run_max"].tolist() == [[20, 25], [0, 0], [20, 130], [90, 90]]
    flags = {(int(r["flow_idx"]), int(r["rcv"])): int(r["flags"]) for r in got["runs"]
             if r["flow_idx"] >= 2}
    assert flags == {(2, 0): 2, (2, 1): 3, (3, 0): 3, (3, 1): 3}
    assert got["pairs"][1].tobytes() == bytes(4 * 32) and got["pairs"][3].tobytes() == bytes(4 * 32)


@pytest.mark.parametrize("opts", [0, 1])
def test_duplicates_skipped_records_and_strangers(torch, eng, opts):
    n = 1500
    flow = np.zeros(n, np.uint32)
    seq = np.arange(n, dtype=np.uint32)
    dups = [64, 127, 128, 300, 301, 1023, 1024, 1400]     # each repeats the record 40 before it
    seq[dups] = seq[np.asarray(dups) - 40]
    flow[np.r_[5:1500:97]] = NONE                          # skipped records in between
    flow[np.r_[11:1500:131]] = 7                           # flow_idx >= n_flows
    send = make_send(flow, seq)
    if not opts:                                           # a duplicate repeats the stamp too
        for k in ("t_sec", "t_usec"):
            send[k][dups] = send[k][np.asarray(dups) - 40]
    lost0 = np.r_[60:70, 120:135, 290:310, 1015:1030, 1390:1410]
    recv = logs(send, [(0, without(n, lost0)), (1, without(n, np.r_[0:128, 1024:1500])),
                       (2, np.arange(n)), (3, np.arange(100)), (9, np.arange(50))])
    got, _ = both(torch, eng, 1, 3, send, recv, opts=opts)
    assert int(got["stats"][0]["send_dup"]) == len(dups)
    assert int(got["stats"][0]["send_skipped"]) > 20
    assert int(got["stats"][0]["recv_skipped"]) > 150      # receivers 3 and 9, and the strangers
    assert int(got["rcv_runs"][0, 0]["loss_runs"]) == 5
    assert not np.isin(got["runs"]["first_send"], dups).any()
    assert not np.isin(got["runs"]["last_send"], dups).any()


def test_pairs_that_do_not_overlap_or_touch_in_one_owner(torch, eng):
    n = 4300                                               # past one wave of the pair pass
    send = make_send(np.zeros(n))
    third = n // 3
    recv = logs(send, [
        (0, np.arange(0, third, 2)),                       # hears the first third only
        (1, np.arange(2 * third, n, 3)),                   # the last third only
        (2, np.r_[third - 1:2 * third:5, 2 * third]),      # touches 0 in one owner, 1 in one
        (3, np.arange(0, n, 7))])
    got, _ = both(torch, eng, 1, 4, send, recv)
    p = got["pairs"][0]
    assert p[0, 1].tobytes() == bytes(32) and p[1, 0].tobytes() == bytes(32)
    assert tuple(int(v) for v in p[0, 2]) == (1, 0, 0, 0)
    assert tuple(int(v) for v in p[2, 1]) == (1, 0, 0, 0)
    assert tuple(int(v) for v in p[3, 3]) == (4299, 3684, 3684, 3684)


def test_spans_that_touch_in_exactly_one_owner(torch, eng):
    n = 130
    send = make_send(np.zeros(n))
    recv = logs(send, [(0, np.r_[0:64:3, 64]), (1, np.r_[64, 70:130:2]), (2, [64])])
    got, _ = both(torch, eng, 1, 3, send, recv)
    p = got["pairs"][0]
    assert tuple(int(v) for v in p[0, 1]) == (1, 0, 0, 0)
    assert tuple(int(v) for v in p[2, 2]) == (1, 0, 0, 0)
    assert tuple(int(v) for v in p[1, 1]) == (65, 34, 34, 34)


def burst_case():
    n = 2500
    send = make_send(np.arange(n) % 2)
    recv = logs(send, [(0, without(n, np.r_[10:14, 100:130, 1000:1003, 2400:2500])),
                       (1, without(n, np.r_[0:40, 101:131, 700, 1500:1520])),
                       (2, without(n, np.r_[100:130]))])
    return send, recv


@pytest.fixture(scope="module")
def burst():
    send, recv = burst_case()
    return send, recv, MX.model(2, 3, send, recv)


def test_min_run(torch, eng, burst):
    send, recv, m = burst
    longest = int(m["rcv_runs"]["loss_run_max"].max())
    assert longest == 50
    counts = []
    for min_run in (0, 1, 2, longest + 1):
        want = MX.model(2, 3, send, recv, min_run=min_run, base=m["base"])
        got, _ = both(torch, eng, 2, 3, send, recv, min_run=min_run, want=want)
        counts.append(got["n_runs"])
    assert counts[0] == counts[1] == int(m["rcv_runs"]["loss_runs"].sum())
    assert counts[1] > counts[2] > counts[3] == 0


def test_a_list_one_entry_too_small_stays_untouched(torch, eng, burst):
    send, recv, m = burst
    n = len(m["runs"])
    short = check(call(torch, eng, 2, 3, send, recv, run_cap=n - 1), m)
    assert short["runs"] is None and short["n_runs"] == n
    full = check(call(torch, eng, 2, 3, send, recv, run_cap=n), m)
    assert len(full["runs"]) == n
    wide = check(call(torch, eng, 2, 3, send, recv, run_cap=n + 3), m)   # spare entries untouched
    assert len(wide["runs"]) == n


@pytest.mark.parametrize("parts", ["s", "l", "p", "sl", "sp", "lp", "slp"])
def test_each_part_alone_and_together(torch, eng, burst, parts):
    send, recv, m = burst
    check(call(torch, eng, 2, 3, send, recv, parts=parts, run_cap=len(m["runs"])), m, parts)


@pytest.fixture(scope="module")
def rand():
    send, recv = MX.random_case(2024, 5000, 7, 5)
    return send, recv, MX.model(7, 5, send, recv, min_run=2)


def test_random_against_the_model_and_twice_the_same_bytes(torch, eng, rand):
    send, recv, m = rand
    a, _ = both(torch, eng, 7, 5, send, recv, min_run=2, want=m)
    b = call(torch, eng, 7, 5, send, recv, min_run=2, run_cap=len(m["runs"]))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    # the case is what it claims to be
    assert len(m["runs"]) > 50 and int(m["rcv_runs"]["loss_run_max"].max()) > 30
    assert int(m["base"]["stats"][0]["send_dup"]) > 20
    assert int(m["base"]["cells"]["lost_head"][:, 1].min()) > 100


def test_random_against_msg_match_ex_per_receiver(torch, eng, rand):
    send, recv, m = rand
    from mgen_amd import FLOW_MATCH_DTYPE
    got = call(torch, eng, 7, 5, send, recv, min_run=2, run_cap=len(m["runs"]))
    d_send = {k: dev(torch, v) for k, v in send.items()}
    for r in range(5):
        one = {k: dev(torch, v) for k, v in MX.one_receiver(recv, r).items()}
        out = eng.msg_match_timeline(7, d_send, one, 0, 1, 0, min_run=2)
        torch.cuda.synchronize()
        flows = out[3].cpu().numpy().view(FLOW_MATCH_DTYPE)
        for fld in ("loss_runs", "loss_run_max", "loss_run_hist"):
            assert got["rcv_runs"][:, r][fld].tolist() == flows[fld].tolist(), (r, fld)
        mine = got["runs"][got["runs"]["rcv"] == r].copy()
        mine["rcv"] = 0
        assert mine.tobytes() == out[7].cpu().numpy().tobytes(), r


# ------------------------------------------------------------------ the empty sides
def test_no_send_records_no_recv_records_no_flows(torch, eng):
    send = make_send(np.arange(10) % 2)
    recv = logs(send, [(0, np.arange(10)), (2, np.arange(4))])
    none_s, none_r = MM.cols(MM.SEND_COLS, []), MM.cols(MM.RECV_COLS, [])
    got, _ = both(torch, eng, 2, 3, none_s, recv)
    assert got["rcv_runs"].tobytes() == bytes(6 * 160) and got["pairs"].tobytes() == bytes(18 * 32)
    assert got["n_runs"] == 0
    got, _ = both(torch, eng, 2, 3, send, none_r)
    assert got["rcv_runs"]["loss_run_max"].tolist() == [[5] * 3] * 2 and got["n_runs"] == 6
    assert (got["runs"]["flags"] == 3).all()
    got, _ = both(torch, eng, 0, 3, send, recv)
    assert got["n_runs"] == 0 and got["rcv_runs"].size == 0 and got["pairs"].size == 0
    both(torch, eng, 2, 3, none_s, none_r)


def test_no_flows_and_null_arrays(torch, eng):
    from mgen_amd import MultiLoss, _ptr, _stream
    send = make_send(np.zeros(5))
    s = [dev(torch, send[k]) for k in MM.SEND_COLS]
    mask = torch.zeros(5, dtype=torch.int64, device="cuda")
    stats = torch.zeros(32, dtype=torch.uint8, device="cuda")
    n_runs = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    lx = MultiLoss(dev_n_runs=n_runs.data_ptr())
    rc = eng.lib.mgenx_msg_match_multi_ex(
        eng.ctx, *[_ptr(t) for t in s], 5, None, None, None, None, None, None, None, 0, 3, 0, 0,
        _ptr(mask), None, None, None, None, _ptr(stats), None, ctypes.byref(lx), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(n_runs.item()) == 0


# ------------------------------------------------------------------ refused calls
def test_einval_leaves_every_byte(torch, eng, burst):
    send, recv, _m = burst
    # whatever mgenx_msg_match_multi refuses
    call(torch, eng, 2, 0, send, recv, expect=EINVAL)
    call(torch, eng, 2, 65, send, recv, expect=EINVAL)
    call(torch, eng, 2**26, 32, send, recv, expect=EINVAL)         # n_flows * n_rcv = 2^31
    # the pair matrix too large: n_flows * n_rcv^2 = 2^31, the cells still legal
    call(torch, eng, 2**19, 64, send, recv, parts="p", expect=EINVAL)
    call(torch, eng, 2**19, 64, send, recv, parts="slp", expect=EINVAL)
    # a list asked for with room but without a place
    call(torch, eng, 2, 3, send, recv, parts="l", run_cap=4, null_runs=True, expect=EINVAL)
    # a null list with no room is the first pass of two
    got = call(torch, eng, 2, 3, send, recv, parts="l", run_cap=0, null_runs=True)
    assert got["n_runs"] > 0


# ------------------------------------------------------------------ nothing asked for
@pytest.mark.parametrize("lx", ["null", "struct"])
def test_without_parts_it_is_msg_match_multi(torch, eng, rand, lx):
    send, recv, _m = rand
    plain = call(torch, eng, 7, 5, send, recv, lx="plain")
    off = call(torch, eng, 7, 5, send, recv, lx=lx, parts="")
    for k in BASE_NAMES:
        assert plain[k].tobytes() == off[k].tobytes(), k
    # the series too (outputs seven and eight) through the engine: the same bytes either way
    tl = (T0 * 10**6, 50_000, 16)
    d_send = {k: dev(torch, v) for k, v in send.items()}
    d_recv = {k: dev(torch, v) for k, v in recv.items()}
    a = eng.msg_match_multi(7, 5, d_send, d_recv, timeline=tl)
    b = eng.msg_match_multi_loss(7, 5, d_send, d_recv, timeline=tl, run_stats=False, min_run=None,
                                 pairs=False)
    torch.cuda.synchronize()
    assert len(a) == 8 and len(b) == 11
    for k in range(8):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
