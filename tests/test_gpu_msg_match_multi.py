"""GPU: mgenx_msg_match_multi (one sender's log joined with many receivers' logs: the delivery
matrix) against the serial model of tests/msg_match_multi_ref.py.  Integer arithmetic: every
output array and struct is compared byte for byte, and every call runs with guard regions around
its outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msg_match_multi_ref as MM  # noqa: E402

NONE = MM.NONE
T0 = 1_700_000_000
GUARD = 256          # bytes on either side of every output
PAT = 0xA5
OUT_NAMES = ("send_mask", "recv_send", "recv_first", "cells", "fanout", "stats", "bins", "outside")
OUT_DTYPES = (np.uint64, np.uint32, np.uint8, MM.CELL, MM.FANOUT, MM.STATS, MM.BIN, np.uint64)


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


def call(torch, eng, nf, n_rcv, send, recv, opts=0, timeline=None, expect=0, ns=None, nr=None):
    """One mgenx_msg_match_multi call with GUARD bytes of PAT before and after every output.
    Returns the outputs as a dict of numpy arrays in the model's dtypes; with expect != 0 the
    call must return that code and leave every output byte as it was."""
    from mgen_amd import MultiTimeline, _ptr, _stream
    ns = len(send["flow_idx"]) if ns is None else ns
    nr = len(recv["flow_idx"]) if nr is None else nr
    s = [dev(torch, send[k]) for k in MM.SEND_COLS]
    r = [dev(torch, recv[k]) for k in MM.RECV_COLS]
    n_bins = timeline[2] if timeline else 0
    small = expect != 0          # a refused call never reaches the outputs: any size will do
    sizes = [8 * ns, 4 * nr, nr, nf * n_rcv * 80, nf * 560, 32, nf * n_bins * 64,
             nf * 8 if timeline else 0]
    if small:
        sizes = [min(b, 4096) for b in sizes]
    bufs = [torch.full((GUARD + b + GUARD,), PAT, dtype=torch.uint8, device="cuda") for b in sizes]
    outs = [ctypes.c_void_p(b.data_ptr() + GUARD) for b in bufs]
    tl = None
    if timeline:
        tl = ctypes.byref(MultiTimeline(t0_us=timeline[0], width_us=timeline[1], n_bins=n_bins,
                                        dev_bins=outs[6].value, dev_outside=outs[7].value))
    rc = eng.lib.mgenx_msg_match_multi(
        eng.ctx, *[_ptr(t) if t.numel() else None for t in s], ns,
        *[_ptr(t) if t.numel() else None for t in r], nr, n_rcv, nf, opts, *outs[:6], tl,
        _stream(0))
    assert rc == expect, (rc, eng.lib.mgenx_last_error(eng.ctx))
    torch.cuda.synchronize()
    got = {}
    for name, b, size, dt in zip(OUT_NAMES, bufs, sizes, OUT_DTYPES):
        h = b.cpu().numpy()
        if expect:
            assert (h == PAT).all(), name
            continue
        assert (h[:GUARD] == PAT).all() and (h[GUARD + size:] == PAT).all(), "write outside"
        got[name] = h[GUARD:GUARD + size].copy().view(dt)
    if not expect:
        got["cells"] = got["cells"].reshape(nf, n_rcv)
        if timeline:
            got["bins"] = got["bins"].reshape(nf, n_bins)
        else:
            del got["bins"], got["outside"]
    return got


def check(got, want):
    assert sorted(got) == sorted(want)
    for name in OUT_NAMES:
        if name not in want:
            continue
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, name
        if g.tobytes() == w.tobytes():
            continue
        if w.dtype.names:
            for fld in w.dtype.names:
                bad = np.argwhere(g[fld] != w[fld])
                assert len(bad) == 0, (name, fld, bad[:8].tolist(), g[fld][tuple(bad[0])],
                                       w[fld][tuple(bad[0])])
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]])
    return got


def both(torch, eng, nf, n_rcv, send, recv, opts=0, timeline=None):
    want = MM.model(nf, n_rcv, send, recv, no_time=bool(opts & 1), timeline=timeline)
    return check(call(torch, eng, nf, n_rcv, send, recv, opts, timeline), want)


def make_send(flow, seq, t_us=None, size=100):
    """Send columns from flow / seq; the stamp is i ms after T0 unless given."""
    flow = np.asarray(flow, np.uint32)
    n = len(flow)
    t = T0 * 10**6 + (np.arange(n, dtype=np.int64) * 1000 if t_us is None else np.asarray(t_us))
    return dict(flow_idx=flow, seq=np.asarray(seq, np.uint32), t_sec=(t // 10**6).astype(np.uint32),
                t_usec=(t % 10**6).astype(np.uint32),
                len=np.broadcast_to(np.asarray(size, np.uint32), (n,)).copy())


def recv_of(send, idx, rcv, lat=300):
    """The recv records of send records idx at receivers rcv (an array or one number)."""
    idx = np.asarray(idx, np.int64)
    rcv = np.broadcast_to(np.asarray(rcv, np.uint32), idx.shape).copy()
    rx = send["t_sec"][idx].astype(np.int64) * 10**6 + send["t_usec"][idx] + lat + rcv
    return dict(flow_idx=send["flow_idx"][idx], seq=send["seq"][idx], tx_sec=send["t_sec"][idx],
                tx_usec=send["t_usec"][idx], rx_sec=(rx // 10**6).astype(np.uint32),
                rx_usec=(rx % 10**6).astype(np.uint32), rcv=rcv)


def logs(send, per_rcv):
    """The receivers' logs one after the other: per_rcv = [(receiver, send indices), ...]."""
    parts = [recv_of(send, idx, r) for r, idx in per_rcv]
    if not parts:
        return MM.cols(MM.RECV_COLS, [])
    return {k: np.concatenate([p[k] for p in parts]) for k in MM.RECV_COLS}


# ------------------------------------------------------------------ the small cases
def test_the_hand_case_and_the_engine_method(torch, eng):
    nf, n_rcv, send, recv = MM.hand_case()
    tl = (2000 * 10**6 + 300, 300, 2)
    got = both(torch, eng, nf, n_rcv, send, recv, timeline=tl)
    assert got["send_mask"].tolist() == [5, 5, 1, 7, 0, 0, 0, 0, 3, 3, 2, 3, 0, 1]
    assert got["cells"]["lost_head"].tolist() == [[0, 2, 0], [0, 1, 3]]
    assert got["cells"]["lost_tail"].tolist() == [[0, 1, 6], [1, 1, 0]]
    assert got["outside"].tolist() == [3, 1]
    # the same through Engine.msg_match_multi
    out = eng.msg_match_multi(nf, n_rcv, {k: dev(torch, v) for k, v in send.items()},
                              {k: dev(torch, v) for k, v in recv.items()}, timeline=tl)
    torch.cuda.synchronize()
    assert len(out) == 8
    for name, t in zip(OUT_NAMES, out):
        assert t.cpu().numpy().tobytes() == got[name].tobytes(), name
    assert len(eng.msg_match_multi(nf, n_rcv, {k: dev(torch, v) for k, v in send.items()},
                                   {k: dev(torch, v) for k, v in recv.items()})) == 6


def test_no_send_records(torch, eng):
    send = make_send(np.arange(10) % 2, np.arange(10) // 2)
    recv = logs(send, [(0, np.arange(10)), (2, np.arange(4))])
    got = both(torch, eng, 2, 3, MM.cols(MM.SEND_COLS, []), recv)
    assert (got["recv_send"] == NONE).all() and not got["recv_first"].any()
    assert got["cells"]["rx_orphan"].tolist() == [[5, 0, 2], [5, 0, 2]]
    assert int(got["stats"][0]["recv_unmatched"]) == 14


def test_no_recv_records(torch, eng):
    send = make_send(np.arange(2100) % 3, np.arange(2100) // 3)
    none = MM.cols(MM.RECV_COLS, [])
    got = both(torch, eng, 4, 2, send, none)
    assert got["cells"]["lost_head"].tolist() == [[700, 700]] * 3 + [[0, 0]]
    assert not got["cells"]["lost_tail"].any() and (got["cells"]["first_send"] == NONE).all()
    assert got["fanout"]["reach_hist"][:, 0].tolist() == [700, 700, 700, 0]
    # nr == 0 with the series on
    got = both(torch, eng, 4, 2, send, none, timeline=(T0 * 10**6, 500_000, 5))
    assert got["bins"]["sent"].sum() == 2100 and not got["outside"].any()
    assert int(got["bins"][0, 0]["reach_min"]) == 0 == int(got["bins"][0, 0]["reach_max"])
    assert int(got["bins"][3, 0]["reach_min"]) == 2**64 - 1


def test_no_flows(torch, eng):
    send = make_send([NONE] * 5, range(5))
    got = both(torch, eng, 0, 3, send, logs(send, [(1, np.arange(5))]))
    assert int(got["stats"][0]["send_skipped"]) == 5 == int(got["stats"][0]["recv_skipped"])
    both(torch, eng, 0, 3, send, logs(send, [(1, np.arange(5))]), timeline=(0, 1000, 4))


def test_one_receiver_equals_msg_match(torch, eng):
    """n_rcv == 1: the cells are mgenx_msg_match's per-flow fields, on the same context."""
    from mgen_amd import FLOW_MATCH_DTYPE
    rng = np.random.default_rng(11)
    n = 5000
    send = make_send(rng.integers(0, 4, n), rng.integers(0, 3000, n))
    idx = np.sort(rng.choice(n, 3500, replace=False))[200:-300]
    recv = logs(send, [(0, np.concatenate([idx, idx[:50]]))])
    recv["seq"][:10] ^= 0x40000000          # orphans
    got = both(torch, eng, 4, 1, send, recv)
    one = {k: dev(torch, v) for k, v in recv.items() if k != "rcv"}
    out = eng.msg_match(4, {k: dev(torch, v) for k, v in send.items()}, one)
    torch.cuda.synchronize()
    flows = out[3].cpu().numpy().view(FLOW_MATCH_DTYPE)
    for k in ("delivered", "delivered_bytes", "rx_dup", "rx_orphan", "lost_head", "lost_tail",
              "lat_sum", "lat_min", "lat_max"):
        assert got["cells"][:, 0][k].tolist() == flows[k].tolist(), k
    for k in ("sent", "sent_bytes", "send_dup"):
        assert got["fanout"][k].tolist() == flows[k].tolist(), k
    assert got["recv_send"].tobytes() == out[2].cpu().numpy().tobytes()


@pytest.mark.parametrize("n_rcv,where", [(64, (0, 31, 32, 63)), (33, (0, 31, 32))])
def test_high_receiver_bits(torch, eng, n_rcv, where):
    """Traffic on both sides of bit 31 and on bit 63: a 32-bit shift or a sign would show."""
    n = 300
    send = make_send(np.arange(n) % 2, np.arange(n) // 2)
    per = [(r, np.arange(k * 7, n - k * 11)) for k, r in enumerate(where)]
    got = both(torch, eng, 2, n_rcv, send, logs(send, per), timeline=(T0 * 10**6, 50_000, 7))
    full = sum(1 << r for r in where)
    assert int(got["send_mask"][100]) == full and int(got["send_mask"][0]) == 1
    assert int(got["fanout"][0]["reach_hist"][len(where)]) > 0
    assert int(got["cells"][0, where[-1]]["delivered"]) > 0
    assert not got["cells"][:, 1]["delivered"].any()


def test_every_receiver_has_all(torch, eng):
    """n_rcv == 64, every message at every receiver: reach_hist[64] and reached_all."""
    n = 70
    send = make_send(np.zeros(n), np.arange(n))
    got = both(torch, eng, 1, 64, send, logs(send, [(r, np.arange(n)) for r in range(64)]),
               timeline=(T0 * 10**6, 10_000, 7))
    assert (got["send_mask"] == np.uint64(2**64 - 1)).all()
    assert int(got["fanout"][0]["reach_hist"][64]) == n == int(got["fanout"][0]["reached_all"])
    assert got["bins"][0]["reach_min"].tolist() == [64] * 7


# ------------------------------------------------------------------ chunk and flow edges
def test_flow_edges_around_the_chunk_edge(torch, eng):
    """A flow edge at every offset 1020..1028 of the sorted send positions, send duplicates on
    both sides of it, and the first and the last delivered owner of a receiver right there."""
    for edge in range(1020, 1029):
        flow = np.concatenate([np.zeros(edge), np.ones(40)])
        seq = np.concatenate([np.arange(edge), np.arange(40)])
        # duplicates of earlier records at sorted positions edge - 2 and edge + 1
        seq[edge - 2], seq[edge + 1] = 5, 0
        # the send log interleaves the flows: the sorted order puts the edge at `edge`
        order = np.argsort(np.concatenate([np.arange(edge) * 2, np.arange(40) * 50 + 1]),
                           kind="stable")
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        # (the duplicates' stamps differ from their owners': the identity goes without the time)
        send = make_send(flow[order], seq[order])
        per = [(0, inv[[edge - 1]]),                       # last owner of flow 0 only
               (1, inv[[edge]]),                            # first owner of flow 1 only
               (2, inv[np.arange(edge - 4, edge + 4)]),     # across the edge, the duplicates too
               (3, inv[[3, edge + 2, edge + 39]])]
        got = both(torch, eng, 2, 5, send, logs(send, per), opts=1)
        c = got["cells"]
        assert got["fanout"]["send_dup"].tolist() == [1, 1], edge
        assert (int(c[0, 0]["lost_head"]), int(c[0, 0]["lost_tail"])) == (edge - 2, 0), edge
        assert (int(c[1, 1]["lost_head"]), int(c[1, 1]["lost_tail"])) == (0, 38), edge
        assert int(c[0, 2]["lost_tail"]) == 0 and int(c[1, 2]["lost_head"]) == 0, edge
        assert int(c[0, 4]["lost_head"]) == edge - 1 and int(c[1, 4]["lost_head"]) == 39, edge


def test_rank_carry_over_three_chunks(torch, eng):
    """One flow over three chunks (another before it shifts the edges); receiver 1's only
    delivery is in the middle chunk, receiver 2's first in the first and last in the third."""
    n0, n1 = 700, 3000
    flow = np.concatenate([np.zeros(n0), np.ones(n1)])
    send = make_send(flow, np.arange(n0 + n1))
    dup = n0 + 900                                # a send duplicate before the delivery: no rank
    send["seq"][dup], send["t_usec"][dup], send["t_sec"][dup] = (
        send["seq"][n0 + 3], send["t_usec"][n0 + 3], send["t_sec"][n0 + 3])
    per = [(0, np.arange(n0 + n1)), (1, [n0 + 1500]), (2, [n0 + 10, n0 + 2990])]
    got = both(torch, eng, 2, 3, send, logs(send, per))
    c = got["cells"][1]
    assert (int(c[1]["lost_head"]), int(c[1]["lost_tail"])) == (1499, n1 - 1 - 1 - 1499)
    assert (int(c[1]["first_send"]), int(c[1]["last_send"])) == (n0 + 1500, n0 + 1500)
    assert (int(c[2]["lost_head"]), int(c[2]["lost_tail"])) == (10, 9)
    assert int(got["fanout"][1]["sent"]) == n1 - 1


def test_one_owner_at_all_receivers_and_many_copies_at_one(torch, eng):
    send = make_send(np.zeros(8), np.arange(8))
    recv = logs(send, [(r, [3]) for r in range(64)] + [(5, [6] * 200)])   # one wave, then 200
    recv["rx_usec"][64:] = np.arange(200, 0, -1) + 7000   # the lowest index is not the earliest
    got = both(torch, eng, 1, 64, send, recv)
    assert int(got["send_mask"][3]) == 2**64 - 1 and int(got["send_mask"][6]) == 1 << 5
    assert int(got["cells"][0, 5]["rx_dup"]) == 199 and int(got["cells"][0, 5]["delivered"]) == 2
    assert got["recv_first"].tolist() == [1] * 65 + [0] * 199
    assert int(got["cells"][0, 5]["lat_max"]) == 200 + 7000 - 6000


def test_a_silent_receiver_and_what_is_skipped(torch, eng):
    """Receiver 1 has no record; flow 2 is seen by the receivers alone; rcv out of range and
    MGENX_FLOW_NONE are skipped."""
    n = 1500
    send = make_send(np.arange(n) % 2, np.arange(n) // 2)
    recv = logs(send, [(0, np.arange(0, n, 3)), (2, np.arange(50, n - 50))])
    extra = MM.cols(MM.RECV_COLS, [(2, k, T0, k, T0, k + 9, k % 3) for k in range(30)] +
                    [(0, 1, T0, 2000, T0, 2300, 3), (0, 1, T0, 2000, T0, 2300, NONE),
                     (NONE, 1, T0, 2000, T0, 2300, 0)])
    recv = {k: np.concatenate([recv[k], extra[k]]) for k in MM.RECV_COLS}
    got = both(torch, eng, 3, 3, send, recv)
    c = got["cells"]
    assert c[:2, 1]["lost_head"].tolist() == [750, 750] and not c[:, 1]["lost_tail"].any()
    assert (c[:, 1]["first_send"] == NONE).all() and (c[:, 1]["last_send"] == NONE).all()
    assert (c[:, 1]["lat_min"] == 2**63 - 1).all() and (c[:, 1]["lat_max"] == -2**63).all()
    assert c[2]["rx_orphan"].tolist() == [10, 10, 10]
    assert int(got["stats"][0]["recv_skipped"]) == 3


def test_identity_with_and_without_the_stamp(torch, eng):
    """The same seq resent with another stamp: two messages with the time, one without."""
    send = make_send([0, 0, 0, 0], [1, 2, 2, 3])
    recv = logs(send, [(0, [0, 1, 2, 3]), (1, [2])])
    got = both(torch, eng, 1, 2, send, recv)
    assert int(got["fanout"][0]["sent"]) == 4 and got["send_mask"].tolist() == [1, 1, 3, 1]
    got = both(torch, eng, 1, 2, send, recv, opts=1)
    assert int(got["fanout"][0]["sent"]) == 3 and got["send_mask"].tolist() == [1, 3, 0, 1]
    assert int(got["fanout"][0]["send_dup"]) == 1 and int(got["cells"][0, 0]["rx_dup"]) == 1


# ------------------------------------------------------------------ size
@pytest.mark.parametrize("ns,nr", [(131_071, 1_048_575), (131_073, 1_048_577),
                                   (150_000, 960_000)])
def test_table_pressure_and_slot_rounding(torch, eng, ns, nr):
    """2 ns and 2 nr just below and just above a power of two (both tables at their fullest and
    their emptiest), and 150,000 sends with 8 x 120,000 recv records."""
    rng = np.random.default_rng(ns)
    send = make_send(rng.integers(0, 6, ns), rng.integers(0, 2**32, ns, dtype=np.uint64),
                     size=rng.integers(20, 1400, ns))
    if nr == 960_000:
        per = [(r, np.sort(rng.choice(ns, 120_000, replace=False))) for r in range(8)]
    else:       # the receivers' logs with copies: nr records of at most nr (owner, rcv) pairs
        cut = np.sort(rng.integers(0, nr + 1, 7))
        per = [(r, np.sort(rng.integers(0, ns, k)))
               for r, k in enumerate(np.diff(np.concatenate([[0], cut, [nr]])))]
    recv = logs(send, per)
    assert len(recv["seq"]) == nr
    recv["seq"][::5000] ^= 0x80000000          # orphans
    got = both(torch, eng, 6, 8, send, recv)
    assert int(got["fanout"]["deliveries"].sum()) == int(got["cells"]["delivered"].sum()) > ns


# ------------------------------------------------------------------ the series
def test_series_window_edges_and_outside(torch, eng):
    t0, width, n_bins = T0 * 10**6 + 5000, 1000, 6
    t_us = np.array([4999, 5000, 5999, 6000, 6001, 10_999, 11_000, 0, 7000, 7000, 2**31],
                    np.int64)
    send = make_send(np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0]), np.arange(11), t_us=t_us)
    recv = logs(send, [(0, np.arange(11)), (1, [1, 3, 5, 8]), (2, [1, 8])])
    got = both(torch, eng, 2, 3, send, recv, timeline=(t0, width, n_bins))
    assert got["outside"].tolist() == [2, 2]
    assert got["bins"]["sent"].tolist() == [[2, 1, 1, 0, 0, 0], [0, 1, 1, 0, 0, 1]]
    assert got["bins"]["reached_all"].tolist() == [[1, 0, 1, 0, 0, 0], [0] * 6]
    # a t0 far below and far above every stamp, and the widest legal ones
    for t0x in (-2**62, 2**62, 0):
        both(torch, eng, 2, 3, send, recv, timeline=(t0x, 2**40, 3))


def test_series_sums_to_the_fanout(torch, eng):
    rng = np.random.default_rng(3)
    n = 6000
    send = make_send(rng.integers(0, 3, n), np.arange(n), size=rng.integers(20, 1400, n))
    per = [(r, np.sort(rng.choice(n, 4000 + 300 * r, replace=False))) for r in range(4)]
    got = both(torch, eng, 3, 4, send, logs(send, per), timeline=(T0 * 10**6, 250_000, 24))
    assert not got["outside"].any()
    for k in ("sent", "sent_bytes", "deliveries", "reached_all"):
        assert got["bins"][k].sum(axis=1).tolist() == got["fanout"][k].tolist(), k
    assert got["bins"]["reached_any"].sum(axis=1).tolist() == (
        got["fanout"]["sent"] - got["fanout"]["reach_hist"][:, 0]).tolist()
    # a log out of time order: every wave mixes many windows
    send2 = make_send(send["flow_idx"], np.arange(n), t_us=rng.integers(0, 6_000_000, n))
    both(torch, eng, 3, 4, send2, logs(send2, per), timeline=(T0 * 10**6 + 1000, 250_000, 20))
    # and receivers mixed record by record: every wave mixes many cells
    recv = logs(send, per)
    mix = rng.permutation(len(recv["seq"]))
    both(torch, eng, 3, 4, send, {k: v[mix] for k, v in recv.items()})


# ------------------------------------------------------------------ the context's workspace
def test_workspace_reuse_and_msg_match_after(torch, eng):
    from mgen_amd import FLOW_MATCH_DTYPE
    rng = np.random.default_rng(8)
    send = make_send(rng.integers(0, 3, 9000), np.arange(9000))
    one = recv_of(send, np.sort(rng.choice(9000, 7000, replace=False)), 0)
    one.pop("rcv")
    ds, dr = {k: dev(torch, v) for k, v in send.items()}, {k: dev(torch, v) for k, v in one.items()}
    before = [t.cpu().numpy().tobytes() for t in eng.msg_match(3, ds, dr)]
    big = make_send(rng.integers(0, 5, 40_000), np.arange(40_000))
    both(torch, eng, 5, 6, big, logs(big, [(r, np.arange(r, 40_000, r + 1)) for r in range(6)]))
    small = make_send(rng.integers(0, 2, 90), np.arange(90))
    both(torch, eng, 2, 2, small, logs(small, [(1, np.arange(0, 90, 2))]))
    after = [t.cpu().numpy().tobytes() for t in eng.msg_match(3, ds, dr)]
    assert before == after
    assert after[3] != bytes(3 * FLOW_MATCH_DTYPE.itemsize)


# ------------------------------------------------------------------ refused calls
def test_bad_arguments_change_no_byte(torch, eng):
    from mgen_amd import _ptr, _stream
    send = make_send(np.zeros(8), np.arange(8))
    recv = logs(send, [(0, np.arange(8))])
    ok = (T0 * 10**6, 1000, 4)
    for n_rcv in (0, 65, 2**32 - 1):
        call(torch, eng, 1, n_rcv, send, recv, expect=-1)
    call(torch, eng, 1, 2, send, recv, expect=-1, ns=2**30 + 1)
    call(torch, eng, 1, 2, send, recv, expect=-1, nr=2**30 + 1)
    call(torch, eng, 2**25, 64, send, recv, expect=-1)               # n_flows * n_rcv == 2^31
    call(torch, eng, 2**20, 1, send, recv, expect=-1, timeline=(0, 1000, 2**11))
    call(torch, eng, 1, 2, send, recv, expect=-1, timeline=(ok[0], 0, 4))
    call(torch, eng, 1, 2, send, recv, expect=-1, timeline=(2**62 + 1, 1000, 4))
    call(torch, eng, 1, 2, send, recv, expect=-1, timeline=(-2**62 - 1, 1000, 4))
    # a null required pointer, one at a time
    s = [dev(torch, send[k]) for k in MM.SEND_COLS]
    r = [dev(torch, recv[k]) for k in MM.RECV_COLS]
    outs = [torch.full((4096,), PAT, dtype=torch.uint8, device="cuda") for _ in range(6)]
    args = [_ptr(t) for t in s] + [8] + [_ptr(t) for t in r] + [8, 1, 1, 0] + \
        [_ptr(t) for t in outs] + [None, _stream(0)]
    required = list(range(5)) + list(range(6, 13)) + list(range(17, 23))
    for k in required:
        bad = list(args)
        bad[k] = None
        assert eng.lib.mgenx_msg_match_multi(eng.ctx, *bad) == -1, k
    assert eng.lib.mgenx_msg_match_multi(None, *args) == -1
    torch.cuda.synchronize()
    for t in outs:
        assert (t.cpu().numpy() == PAT).all()
    # the columns of an empty side may be null: the call itself is fine
    call(torch, eng, 1, 2, MM.cols(MM.SEND_COLS, []), MM.cols(MM.RECV_COLS, []))


# ------------------------------------------------------------------ end to end
def _insert(text, at, line):
    lines = text.split(b"\n")
    assert lines[-1] == b""
    lines.insert(at, line)
    return b"\n".join(lines)


def _host_flow_numbering(parsed, table):
    """Flow indices from the parsed columns, on the host: key = dst address, dst port, source
    port, flow id; numbered by first OK line, continuing `table`."""
    n = len(parsed["err"])
    idx = np.full(n, NONE, np.uint32)
    for k in range(n):
        if parsed["err"][k]:
            continue
        key = (bytes(parsed["dst_addr"][16 * k:16 * k + 16]), int(parsed["dst_len"][k]),
               int(parsed["dst_port"][k]), int(parsed["src_port"][k]), int(parsed["flow_id"][k]))
        idx[k] = table.setdefault(key, len(table))
    return idx


def test_text_logs_end_to_end(torch, eng, tmp_path, capsys):
    """A sender's log and three receivers' logs: flow 1 to an IPv4 multicast group, flow 11 to an
    IPv6 destination, flow 12 in receiver 2's log alone; receiver 1's log starts late."""
    from mgen_amd import (ADDR_DTYPE, EVENT_RECV, EVENT_SEND, LOG_EPOCH, PACK_CHECKSUM, PARSE_OK,
                          match_text_logs_multi, to_device)
    from mgen_amd._abi import DESC_DTYPE
    from mgen_amd.workloads import make_templates
    t4, pool = make_templates(1, dst=(224, 225, 1, 2))
    t6, _ = make_templates(2, ipv6=True)
    t6["flow_id"] += 10                    # flow ids 11 and 12; 12 is seen by receiver 2 alone
    tmpl = np.concatenate([t4, t6])
    n_tmpl, per, msg_len = len(tmpl), 60, 96
    n = 2 * per                            # the sender's messages
    extra = 5                              # the receiver-only flow's
    d = np.zeros(n + extra, DESC_DTYPE)
    d["tmpl"][:n] = np.arange(n) % 2
    d["tmpl"][n:] = 2
    d["seq_num"][:n] = np.arange(n) // 2
    d["seq_num"][n:] = np.arange(extra)
    t_us = T0 * 10**6 + 999_000 + np.arange(n + extra, dtype=np.int64) * 700
    d["tx_sec"], d["tx_usec"], d["msg_len"] = t_us // 10**6, t_us % 10**6, msg_len
    src_port = (40_000 + np.arange(n_tmpl)).astype(np.uint16)
    dt, dp, dd = to_device(tmpl), to_device(pool), to_device(d)
    crc = torch.empty(n_tmpl, dtype=torch.int32, device="cuda")
    eng.pack_prepare(dt, n_tmpl, dp, crc)
    slab = torch.zeros((n + extra) * msg_len, dtype=torch.uint8, device="cuda")
    out_len = eng.pack(dt, crc, dd, n + extra, dp, slab, stride=msg_len, opts=PACK_CHECKSUM)
    assert int((out_len == 0).sum().item()) == 0
    text, _ = eng.log_send(dt, dd, n, src_port=to_device(src_port), out_len=out_len,
                           protocol=1, opts=LOG_EPOCH)
    send_log = text.cpu().numpy().tobytes()
    assert send_log.count(b"\n") == n
    send_log = _insert(send_log, 0, b"%d.000000 START Mgen Version 5.02b" % T0)

    rng = np.random.default_rng(5)
    sels = [np.setdiff1d(np.arange(n), rng.choice(n, 9, replace=False)),       # some loss
            np.arange(41, n),                                                  # starts late
            np.concatenate([np.arange(0, n - 30), [7, 7], np.arange(n, n + extra)])]
    recv_logs = []
    for r, sel in enumerate(sels):
        m = len(sel)
        rslab = slab.view(n + extra, msg_len)[torch.from_numpy(sel).cuda()].contiguous().view(-1)
        cols = eng.unpack(rslab, m, stride=msg_len, fixed_len=msg_len, ext=True)
        assert int(cols["err"].sum().item()) == 0
        src = np.zeros(m, ADDR_DTYPE)
        src["type"], src["len"] = 1, 4
        src["port"] = src_port[d["tmpl"][sel]]
        src["addr"][:, :4] = [192, 168, 7, 1]
        rx_us = t_us[sel] + rng.integers(100, 5000, m)
        rtext, _ = eng.log_recv_text(rslab, m, cols, to_device(src.view(np.uint8)),
                                     to_device((rx_us // 10**6).astype(np.uint32)),
                                     to_device((rx_us % 10**6).astype(np.uint32)), stride=msg_len,
                                     opts=LOG_EPOCH)
        log = rtext.cpu().numpy().tobytes()
        assert log.count(b"\n") == m
        recv_logs.append(_insert(log, 0, b"%d.000000 JOIN group>224.225.1.2" % T0))

    width = 20_000
    res = match_text_logs_multi(send_log, recv_logs, width_us=width)
    keys, cells, fanout, stats, mask, n_send_flows, bins, outside, t0_us = res
    assert n_send_flows == 2 and keys["flow_id"].tolist() == [1, 11, 12]
    assert keys["dst"]["len"].tolist() == [4, 16, 16]
    assert keys["dst"]["addr"][0][:4].tolist() == [224, 225, 1, 2]
    assert cells.shape == (3, 3) and len(mask) == n + 1
    assert fanout["sent"].tolist() == [per, per, 0]
    assert cells["lost_head"][:2, 1].tolist() == [21, 20] and not cells["lost_head"][:2, 2].any()
    assert cells["lost_tail"][:2, 2].tolist() == [15, 15]
    assert cells["rx_orphan"][2].tolist() == [0, 0, extra] and int(stats["recv_unmatched"]) == extra
    assert int(cells["rx_dup"].sum()) == 2 and int(stats["recv_skipped"]) == 3
    assert not outside.any() and int(bins[:2]["sent"].sum()) == n

    # the whole result against the model over the parsed columns
    def parse(log, want):
        t = torch.from_numpy(np.frombuffer(log, np.uint8).copy()).cuda()
        line_off, k = eng.text_index(t)
        p = eng.log_parse_text(t, line_off, k)
        h = {name: p[name].cpu().numpy() for name in (
            "event", "status", "flow_id", "seq_num", "tx_sec", "tx_usec", "rx_sec", "rx_usec",
            "size", "dst_addr", "dst_len", "dst_port")}
        h["src_port"] = p["src"].cpu().numpy().view(ADDR_DTYPE)["port"]
        h["err"] = ~((h["event"] == want) & (h["status"] == PARSE_OK))
        return h
    u = lambda a: a.view(np.uint32)  # noqa: E731
    table = {}
    ps = parse(send_log, EVENT_SEND)
    send = dict(flow_idx=_host_flow_numbering(ps, table), seq=u(ps["seq_num"]),
                t_sec=u(ps["rx_sec"]), t_usec=u(ps["rx_usec"]), len=u(ps["size"]))
    parts = []
    for r, log in enumerate(recv_logs):
        pr = parse(log, EVENT_RECV)
        parts.append(dict(flow_idx=_host_flow_numbering(pr, table), seq=u(pr["seq_num"]),
                          tx_sec=u(pr["tx_sec"]), tx_usec=u(pr["tx_usec"]), rx_sec=u(pr["rx_sec"]),
                          rx_usec=u(pr["rx_usec"]),
                          rcv=np.full(len(pr["err"]), r, np.uint32)))
    recv = {k: np.concatenate([p[k] for p in parts]) for k in MM.RECV_COLS}
    want = MM.model(3, 3, send, recv, timeline=(t0_us, width, bins.shape[1]))
    got = dict(send_mask=mask, cells=cells.view(MM.CELL), fanout=fanout.view(MM.FANOUT),
               stats=np.array([stats]).view(MM.STATS), bins=bins.view(MM.BIN), outside=outside)
    check(got, {k: want[k] for k in got})

    # the command-line tool prints the rows per receiver and the reach histogram
    from mgen_amd.match_multi import main
    paths = []
    for name, log in zip(("send", "r0", "r1", "r2"), [send_log] + recv_logs):
        (tmp_path / name).write_bytes(log)
        paths.append(str(tmp_path / name))
    capsys.readouterr()
    assert main(["-w", "0.02"] + paths) == 0
    out = capsys.readouterr().out.split("\n")
    assert out[0].startswith("# flow dst rcv sent delivered lost lost_head")
    assert out[1].split()[:5] == ["1", "224.225.1.2/5000", "0", str(per),
                                  str(int(cells[0, 0]["delivered"]))]
    assert out[2].split()[:7] == ["1", "224.225.1.2/5000", "1", str(per), str(per - 21), "21", "21"]
    at = out.index("# flow dst sent reached_all all_ratio reach_0 reach_1 reach_2 reach_3")
    assert at == 1 + 9 + 1
    assert out[at + 1].split()[:4] == ["1", "224.225.1.2/5000", str(per),
                                       str(int(fanout[0]["reached_all"]))]
    assert any(line.startswith("# bin_start_us sent reached_any") for line in out[at:])
    assert main(paths[:1]) == 2
