"""GPU: the timeline of mgenx_msg_match_ex (the series per send-time window, the run list, the
owner column) against the serial model of tests/match_timeline_ref.py.  Integer arithmetic: every
output is compared byte for byte, and every call runs with guard regions around its outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_timeline_ref as TL  # noqa: E402
import msg_match_ref as M  # noqa: E402

NONE = M.NONE
T0 = 1_700_000_000
T0US = T0 * 10**6
GUARD = 256          # bytes on either side of every output
PAT = 0xA5
BASE = ("send_rx_count", "send_first_rx", "recv_send", "flows", "stats")


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


class Out:
    """A device buffer of `size` bytes with GUARD bytes of PAT on either side."""

    def __init__(self, torch, size):
        self.size = size
        self.buf = torch.full((GUARD + size + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def get(self, dtype):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == PAT).all() and (h[GUARD + self.size:] == PAT).all(), "write outside"
        return h[GUARD:GUARD + self.size].copy().view(dtype)


def run_tl(torch, eng, nf, send, recv, t0=0, width=1, n_bins=0, min_run=1, opts=0, run_cap=None,
           runs=True, owner=True, tl=True, plain=False):
    """One mgenx_msg_match_ex call (two when run_cap is None: the list is sized by the first).
    Returns a dict of numpy arrays in the model's dtypes; "runs" is the whole list buffer of
    run_cap entries, written or not.  plain: mgenx_msg_match itself."""
    from mgen_amd import FLOW_MATCH_DTYPE, MATCH_STATS_DTYPE, MatchTimeline, _ptr, _stream
    ns, nr = len(send["flow_idx"]), len(recv["flow_idx"])
    s = [dev(torch, send[k]) for k in M.SEND_COLS]
    r = [dev(torch, recv[k]) for k in M.RECV_COLS]
    sizes = (ns * 4, ns * 4, nr * 4, nf * FLOW_MATCH_DTYPE.itemsize, MATCH_STATS_DTYPE.itemsize)
    base = [Out(torch, b) for b in sizes]
    o_bins = Out(torch, nf * n_bins * 64)
    o_out = Out(torch, nf * 8 if n_bins else 0)
    o_n = Out(torch, 8)
    o_own = Out(torch, ns * 4)
    args = ([eng.ctx] + [_ptr(t) if t.numel() else None for t in s] + [ns] +
            [_ptr(t) if t.numel() else None for t in r] + [nr, nf, opts] +
            [ctypes.c_void_p(b.ptr) for b in base])
    if plain:
        rc = eng.lib.mgenx_msg_match(*args, _stream(0))
        assert rc == 0, eng.lib.mgenx_last_error(eng.ctx)
        torch.cuda.synchronize()
        return {k: b.get(dt) for k, b, dt in zip(BASE, base, (np.uint32, np.uint32, np.uint32,
                                                               M.FLOW, M.STATS))}
    o_runs = Out(torch, 0)
    t = MatchTimeline(t0_us=t0, width_us=width, n_bins=n_bins, min_run=min_run,
                      dev_bins=o_bins.ptr if n_bins else None,
                      dev_outside=o_out.ptr if n_bins else None, dev_runs=None, run_cap=0,
                      dev_n_runs=o_n.ptr if runs else None,
                      dev_send_owner=o_own.ptr if owner else None)
    passes = [0] if run_cap is None else [run_cap]
    for k, cap in enumerate(passes):
        if cap:
            o_runs = Out(torch, cap * 40)
            t.dev_runs, t.run_cap = o_runs.ptr, cap
        rc = eng.lib.mgenx_msg_match_ex(*args, ctypes.byref(t) if tl else None, _stream(0))
        assert rc == 0, eng.lib.mgenx_last_error(eng.ctx)
        torch.cuda.synchronize()
        if run_cap is None and k == 0 and runs and tl:
            count = int(o_n.get(np.uint64)[0])
            if count:
                passes.append(count)
    got = {k: b.get(dt) for k, b, dt in zip(BASE, base, (np.uint32, np.uint32, np.uint32,
                                                         M.FLOW, M.STATS))}
    got["bins"] = o_bins.get(TL.BIN).reshape(nf, n_bins)
    got["outside"] = o_out.get(np.uint64)
    got["n_runs"] = o_n.get(np.uint64)
    got["runs"] = o_runs.get(TL.RUN)
    got["owner"] = o_own.get(np.uint32)
    return got


def same(name, g, w):
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (name, g.shape, w.shape)
    if g.tobytes() == w.tobytes():
        return
    if w.dtype.names:
        for fld in w.dtype.names:
            bad = np.argwhere(g[fld] != w[fld])
            assert len(bad) == 0, (name, fld, bad[:8].tolist(), g[fld][tuple(bad[0])],
                                   w[fld][tuple(bad[0])])
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]])


def both(torch, eng, nf, send, recv, t0, width, n_bins, min_run=1, opts=0, want=None):
    """The product against the model, every output; then the sums the header promises, on the
    product's own numbers."""
    if want is None:
        want = TL.model(nf, send, recv, t0, width, n_bins, min_run, no_time=bool(opts & 1))
    base, owner, bins, outside, runs = want
    got = run_tl(torch, eng, nf, send, recv, t0, width, n_bins, min_run, opts)
    for name, w in zip(BASE, base):
        same(name, got[name], w)
    same("owner", got["owner"], owner)
    same("bins", got["bins"], bins)
    same("outside", got["outside"], outside if n_bins else outside[:0])
    assert int(got["n_runs"][0]) == len(runs)
    same("runs", got["runs"], runs)
    flows = got["flows"]
    if max(min_run, 1) == 1:
        assert int(got["n_runs"][0]) == int(flows["loss_runs"].sum())
    for f in range(nf if n_bins else 0):
        if int(got["outside"][f]):
            continue
        b = got["bins"][f]
        for k in ("sent", "sent_bytes", "delivered", "delivered_bytes", "rx_dup", "lat_sum"):
            assert b[k].sum(dtype=b[k].dtype) == flows[f][k], (f, k)
        assert b["lat_min"].min() == flows[f]["lat_min"], f
        assert b["lat_max"].max() == flows[f]["lat_max"], f
    return got


def stamps(t):
    t = np.asarray(t, np.int64)
    return (t // 10**6).astype(np.uint32), (t % 10**6).astype(np.uint32)


def make(flow, seq, lost=(), t_us=None, size=100, lat=300):
    """Send columns from flow / seq (stamp i ms after T0 unless given) and the recv side: every
    send not in `lost`, in send order, received `lat` us later."""
    flow = np.asarray(flow, np.uint32)
    n = len(flow)
    t = T0US + (np.arange(n, dtype=np.int64) * 1000 if t_us is None else np.asarray(t_us))
    sec, usec = stamps(t)
    send = dict(flow_idx=flow, seq=np.asarray(seq, np.uint32), t_sec=sec, t_usec=usec,
                len=np.broadcast_to(np.asarray(size, np.uint32), (n,)).copy())
    keep = np.ones(n, bool)
    keep[np.asarray(list(lost), np.int64)] = False
    return send, recv_of(send, np.nonzero(keep)[0], lat)


def recv_of(send, idx, lat=300):
    idx = np.asarray(idx, np.int64)
    rx = send["t_sec"][idx].astype(np.int64) * 10**6 + send["t_usec"][idx] + lat
    sec, usec = stamps(rx)
    return dict(flow_idx=send["flow_idx"][idx], seq=send["seq"][idx], tx_sec=send["t_sec"][idx],
                tx_usec=send["t_usec"][idx], rx_sec=sec, rx_usec=usec)


def copy_row(send, dst, src):
    for k in M.SEND_COLS:
        send[k][dst] = send[k][src]


def tuples(runs):
    return [(int(r["flow_idx"]), int(r["length"]), int(r["first_send"]), int(r["last_send"]),
             int(r["flags"])) for r in runs]


# ------------------------------------------------------------------ the small cases
def test_hand_case(torch, eng):
    nf, send, recv = M.hand_case()
    got = both(torch, eng, nf, send, recv, 1_000_000_100, 250, 3)
    assert got["owner"].tolist() == [0, 1, 2, 3, 4, NONE, 6, 1, 8, 9, 10, 11]
    assert tuples(got["runs"]) == [(0, 1, 0, 0, 1), (0, 3, 3, 6, 0), (0, 2, 10, 11, 2),
                                   (1, 1, 9, 9, 2)]
    assert got["bins"]["sent"].tolist() == [[3, 2, 3], [1, 0, 1]]
    got = both(torch, eng, nf, send, recv, 1_000_000_100, 250, 2, min_run=2)
    assert got["outside"].tolist() == [3, 1]
    assert tuples(got["runs"]) == [(0, 3, 3, 6, 0), (0, 2, 10, 11, 2)]
    both(torch, eng, nf, send, recv, 0, 1, 0, min_run=0)      # no series; 0 is taken as 1


def test_engine_method(torch, eng):
    from mgen_amd import LOSS_RUN_DTYPE, MATCH_BIN_DTYPE
    nf, send, recv = M.hand_case()
    base, owner, bins, outside, runs = TL.model(nf, send, recv, 1_000_000_100, 250, 3, 1)
    out = eng.msg_match_timeline(nf, {k: dev(torch, v) for k, v in send.items()},
                                 {k: dev(torch, v) for k, v in recv.items()},
                                 1_000_000_100, 250, 3)
    torch.cuda.synchronize()
    assert len(out) == 9
    assert out[3].cpu().numpy().view(M.FLOW).tobytes() == base[3].tobytes()
    assert out[5].cpu().numpy().view(MATCH_BIN_DTYPE).tobytes() == bins.tobytes()
    assert out[6].cpu().numpy().view(np.uint64).tolist() == outside.tolist()
    assert out[7].cpu().numpy().view(LOSS_RUN_DTYPE).tobytes() == runs.tobytes()
    assert out[8].cpu().numpy().view(np.uint32).tolist() == owner.tolist()


def test_null_and_all_off_timeline_are_msg_match(torch, eng):
    n = 5000
    send, recv = make(np.arange(n) % 3, np.arange(n) // 3, lost=range(7, n, 11))
    want = run_tl(torch, eng, 3, send, recv, plain=True)
    for kw in (dict(tl=False), dict(runs=False, owner=False)):
        got = run_tl(torch, eng, 3, send, recv, **kw)
        for name in BASE:
            assert got[name].tobytes() == want[name].tobytes(), (kw, name)
        # nothing of the timeline was touched
        assert (got["n_runs"].view(np.uint8) == PAT).all()
        assert (got["owner"].view(np.uint8) == PAT).all()


def test_empty_sides_and_no_flows(torch, eng):
    send, recv = make(np.arange(2100) % 3, np.arange(2100) // 3)
    got = both(torch, eng, 4, send, M.cols(M.RECV_COLS, []), T0US, 500_000, 5)
    assert tuples(got["runs"]) == [(f, 700, f, 2097 + f, 3) for f in range(3)]
    assert got["bins"]["sent"].sum() == 2100 and not got["bins"]["delivered"].any()
    got = both(torch, eng, 2, M.cols(M.SEND_COLS, []), recv, T0US, 1000, 4)
    assert got["bins"]["lat_min"].tolist() == [[2**63 - 1] * 4] * 2
    assert int(got["n_runs"][0]) == 0 and len(got["owner"]) == 0
    send, recv = make([NONE] * 5, range(5))
    got = both(torch, eng, 0, send, recv, T0US, 1000, 4)
    assert got["owner"].tolist() == [NONE] * 5 and int(got["n_runs"][0]) == 0
    both(torch, eng, 0, M.cols(M.SEND_COLS, []), M.cols(M.RECV_COLS, []), 0, 1, 1)


# ------------------------------------------------------------------ the run list
def test_one_run_across_three_chunk_edges_with_duplicates(torch, eng):
    """One flow: records 11..3298 are lost, across the edges at 1024, 2048 and 3072.  Send
    duplicates of the delivered record 9 lie directly after it (10), on both sides of two chunk
    edges (1023, 1024, 2047, 2048) and directly before the delivered record that ends the run
    (3299): first_send / last_send are 11 and 3298, not their neighbours."""
    n = 3500
    dups = [10, 1023, 1024, 2047, 2048, 3299]
    send, _ = make(np.zeros(n), np.arange(n))
    for d in dups:
        copy_row(send, d, 9)
    recv = recv_of(send, [i for i in range(n) if i < 10 or i >= 3300])
    got = both(torch, eng, 1, send, recv, T0US, 10**6, 4)
    assert tuples(got["runs"]) == [(0, 3288 - 4, 11, 3298, 0)]
    assert int(got["runs"][0]["t_first_us"]) == T0US + 11_000
    assert int(got["runs"][0]["t_last_us"]) == T0US + 3_298_000
    assert got["owner"][dups].tolist() == [9] * 6
    # a run from the first position after an edge's duplicates to the last before the next's
    recv = recv_of(send, [i for i in range(n) if i < 1025 or i >= 2047])
    got = both(torch, eng, 1, send, recv, T0US, 10**6, 4)
    assert tuples(got["runs"]) == [(0, 1022, 1025, 2046, 0)]


@pytest.mark.parametrize("whole", [False, True])
def test_runs_do_not_merge_across_flow_edges(torch, eng, whole):
    """A flow edge at every offset 1020..1028 of a chunk, a tail run before it (the first flow's
    last five records, or the whole flow) and a head run after it: two runs, never one."""
    for edge in range(1020, 1029):
        flow = np.concatenate([np.zeros(edge), np.ones(40)])
        order = np.argsort(np.concatenate([np.arange(edge) * 2, np.arange(40) * 50 + 1]),
                           kind="stable")
        seq = np.concatenate([np.arange(edge), np.arange(40)])
        lost_sorted = list(range(0 if whole else edge - 5, edge + 5))
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        send, recv = make(flow[order], seq[order], lost=inv[lost_sorted])
        got = both(torch, eng, 2, send, recv, T0US, 100_000, 12)
        r = got["runs"]
        assert len(r) == 2 and r["flow_idx"].tolist() == [0, 1], edge
        assert r["length"].tolist() == [edge if whole else 5, 5], edge
        assert r["flags"].tolist() == [3 if whole else 2, 1], edge
        assert r["first_send"].tolist() == [inv[lost_sorted[0]], inv[edge]], edge
        assert r["last_send"].tolist() == [inv[edge - 1], inv[edge + 4]], edge


def test_flow_never_delivered(torch, eng):
    n = 2600
    flow = np.arange(n) % 2
    send, recv = make(flow, np.arange(n) // 2, lost=np.nonzero(flow == 1)[0])
    got = both(torch, eng, 3, send, recv, T0US, 10**6, 3)
    assert tuples(got["runs"]) == [(1, 1300, 1, n - 1, 3)]


@pytest.fixture(scope="module")
def short_runs():
    """Flow 0: 40,000 messages, every second one lost (20,000 runs of 1).  Flow 1: 3,000 with
    runs of 2 and 3."""
    n, m = 40_000, 3000
    flow = np.concatenate([np.zeros(n), np.ones(m)])
    seq = np.concatenate([np.arange(n), np.arange(m)])
    lost = list(range(1, n, 2)) + [n + i for i in range(m) if i % 10 in (3, 4, 7, 8, 9)]
    send, recv = make(flow, seq, lost=lost)
    return send, recv, {k: TL.model(2, send, recv, T0US, 10**6, 44, k) for k in (1, 2)}


@pytest.mark.parametrize("min_run", [1, 2])
def test_many_runs_of_one(torch, eng, short_runs, min_run):
    send, recv, models = short_runs
    want = models[min_run]
    got = both(torch, eng, 2, send, recv, T0US, 10**6, 44, min_run, want=want)
    count = int(got["n_runs"][0])
    assert count == (20_600 if min_run == 1 else 600)
    # the list's capacity: exact, one short (not one byte is written), none
    exact = run_tl(torch, eng, 2, send, recv, min_run=min_run, run_cap=count)
    assert exact["runs"].tobytes() == want[4].tobytes()
    short = run_tl(torch, eng, 2, send, recv, min_run=min_run, run_cap=count - 1)
    assert int(short["n_runs"][0]) == count and (short["runs"].view(np.uint8) == PAT).all()
    more = run_tl(torch, eng, 2, send, recv, min_run=min_run, run_cap=count + 3)
    assert more["runs"][:count].tobytes() == want[4].tobytes()
    assert (more["runs"][count:].view(np.uint8) == PAT).all()
    none = run_tl(torch, eng, 2, send, recv, min_run=min_run, run_cap=0)
    assert int(none["n_runs"][0]) == count and len(none["runs"]) == 0


def test_mixed_run_lengths_and_a_threshold(torch, eng):
    """Runs of every length 1..40, in a shuffled order, each followed by 1..3 delivered messages,
    over 4 interleaved flows: min_run = 8 keeps the runs of 8 and more."""
    rng = np.random.default_rng(40)
    lost, at = [], 0
    for rep in range(6):
        for length in rng.permutation(40) + 1:
            lost += range(at, at + length)
            at += length + int(rng.integers(1, 4))
    n = at
    flow = rng.integers(0, 4, n)
    seq = np.arange(n)
    # `lost` is per sorted position: map to send indices
    order = np.argsort(flow, kind="stable")
    send, recv = make(flow, seq, lost=order[np.asarray(lost)])
    got = both(torch, eng, 4, send, recv, T0US, 250_000, 30, min_run=8)
    assert got["runs"]["length"].min() >= 8 and len(got["runs"]) > 100
    both(torch, eng, 4, send, recv, T0US, 250_000, 30, min_run=1)
    got = both(torch, eng, 4, send, recv, T0US, 250_000, 30, min_run=41)
    assert len(got["runs"]) == 0


# ------------------------------------------------------------------ the series
def test_window_edges(torch, eng):
    t0, width, nb = T0US + 123, 777, 5
    t = [t0, t0 - 1, t0 + nb * width - 1, t0 + nb * width, t0 + width - 1, t0 + width]
    send, recv = make([0, 0, 1, 1, 0, 1], range(6), t_us=np.array(t) - T0US, lost=[2])
    got = both(torch, eng, 2, send, recv, t0, width, nb)
    assert got["bins"]["sent"].tolist() == [[2, 0, 0, 0, 0], [0, 1, 0, 0, 1]]
    assert got["outside"].tolist() == [1, 1]


def test_time_axis_extremes(torch, eng):
    n = 3000
    rng = np.random.default_rng(11)
    flow = rng.integers(0, 3, n)
    send, recv = make(flow, np.arange(n), lost=rng.choice(n, 300, replace=False))
    # a t_usec of 10^6 and more is taken as it is (the recv side carries the same stamp)
    bump = rng.choice(n, 500, replace=False)
    send["t_usec"][bump] += 3_000_000
    recv = recv_of(send, np.nonzero(np.isin(np.arange(n), recv["seq"]))[0])
    # every stamp lies before t0: negative floors, all outside
    got = both(torch, eng, 3, send, recv, T0US + 10**9, 1000, 4)
    assert got["outside"].sum() == n and not got["bins"]["sent"].any()
    assert got["runs"]["t_first_us"].max() > T0US + 3_000_000
    both(torch, eng, 3, send, recv, 2**62, 1, 4)
    both(torch, eng, 3, send, recv, -2**62, 2**63, 2)
    # width 1: a window per microsecond
    both(torch, eng, 3, send, recv, T0US + 5000, 1, 2000)
    # a width above 2^32 us: one window takes everything from t0 on
    got = both(torch, eng, 3, send, recv, T0US + 1_500_000, 2**32 + 12345, 2)
    assert not got["bins"]["sent"][:, 1].any() and got["outside"].sum() > 0
    # stamps near the top of the u32 seconds
    send["t_sec"][:] = 2**32 - 1
    recv = recv_of(send, np.nonzero(np.isin(np.arange(n), recv["seq"]))[0])
    recv["rx_sec"][:] = 2**32 - 1
    both(torch, eng, 3, send, recv, (2**32 - 1) * 10**6, 400_000, 12)


def test_key_changes_inside_and_across_chunks(torch, eng):
    # 1,024 flows x 3 windows, round robin: every position has another key than its neighbours
    n = 1024 * 9
    flow = np.arange(n) % 1024
    rng = np.random.default_rng(3)
    send, recv = make(flow, np.arange(n) // 1024, lost=rng.choice(n, 900, replace=False),
                      size=rng.integers(20, 9000, n))
    both(torch, eng, 1024, send, recv, T0US, 3_072_000, 3)
    # 3 flows x 700 windows
    n = 6300
    send, recv = make(np.arange(n) % 3, np.arange(n) // 3, lost=rng.choice(n, 600, replace=False))
    got = both(torch, eng, 3, send, recv, T0US, 9000, 700)
    assert got["bins"]["sent"].min() == 3 and not got["outside"].any()


def test_log_out_of_time_order(torch, eng):
    """The stamps are a shuffle of the send order: a cell comes up again from positions that do
    not follow each other and from several chunks."""
    n = 9000
    rng = np.random.default_rng(8)
    t = rng.permutation(n).astype(np.int64) * 1000
    send, recv = make(np.arange(n) % 2, np.arange(n) // 2, t_us=t,
                      lost=rng.choice(n, 800, replace=False),
                      lat=rng.integers(-500, 90_000, n - 800))
    got = both(torch, eng, 2, send, recv, T0US, 10**6, 9)
    assert got["bins"]["sent"].sum(axis=0).tolist() == [1000] * 9 and not got["outside"].any()


def test_one_cell_and_a_wrapping_sum(torch, eng):
    n = 50_000
    send, recv = make(np.zeros(n), np.arange(n), t_us=np.arange(n) - T0US + 5 * 10**6)
    recv["rx_sec"][:] = 4_000_000_000         # 4 * 10^15 us each: the sum passes 2^63 many times
    got = both(torch, eng, 1, send, recv, 0, 10**9, 2)
    assert int(got["bins"][0][0]["delivered"]) == n
    assert int(got["bins"][0][0]["lat_min"]) > 3 * 10**15
    exact = sum(4 * 10**15 + (5_000_300 + i) % 10**6 - (5_000_000 + i) for i in range(n))
    assert exact > 2**64 and int(got["bins"][0][0]["lat_sum"]) == M._wrap_i64(exact)


def test_no_time_duplicates_carry_other_stamps(torch, eng):
    """Under MGENX_MATCH_NO_TIME equal (flow, seq) are one message whatever the stamps: only the
    owner's stamp places it, the duplicates' windows stay empty."""
    from mgen_amd import MATCH_NO_TIME
    n = 2400
    seq = np.arange(n) // 2
    t = np.arange(n, dtype=np.int64) * 1000
    dup = np.arange(300, n, 7)
    seq[dup] = seq[dup - 250]                 # the same flow (even distance), another stamp
    t[dup] += 50_000_000                      # ... in windows of their own
    send, _ = make(np.arange(n) % 2, seq, t_us=t)
    idx = [i for i in range(n) if i % 5 and i not in set(dup.tolist())]
    recv = recv_of(send, idx)
    got = both(torch, eng, 2, send, recv, T0US, 100_000, 600, opts=MATCH_NO_TIME)
    assert int(got["stats"][0]["send_dup"]) == len(dup)
    assert not got["bins"]["sent"][:, 400:].any() and not got["outside"].any()
    both(torch, eng, 2, send, recv, T0US, 100_000, 600)      # with the stamps: owners of their own


def test_two_runs_leave_identical_bytes(torch, eng):
    n = 60_000
    rng = np.random.default_rng(77)
    send, _ = make(rng.integers(0, 50, n), np.arange(n), t_us=rng.integers(0, 10**8, n),
                   size=rng.integers(28, 70_000, n))
    keep = np.nonzero(rng.random(n) >= 0.1)[0]
    idx = np.concatenate([keep, keep[rng.random(len(keep)) < 0.02]])
    rng.shuffle(idx)
    recv = recv_of(send, idx, lat=rng.integers(-2000, 900_000, len(idx)))
    a = run_tl(torch, eng, 50, send, recv, T0US, 10**6, 100, 2)
    b = run_tl(torch, eng, 50, send, recv, T0US, 10**6, 100, 2)
    assert int(a["n_runs"][0]) > 100 and a["bins"]["rx_dup"].sum() > 500
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_einval(torch, eng):
    from mgen_amd import MatchTimeline, _ptr, _stream
    nf, send, recv = M.hand_case()
    s = [dev(torch, send[k]) for k in M.SEND_COLS]
    r = [dev(torch, recv[k]) for k in M.RECV_COLS]
    outs = [Out(torch, 4096) for _ in range(5)]
    buf = Out(torch, 4096)
    good = dict(t0_us=0, width_us=1, n_bins=2, min_run=1, dev_bins=buf.ptr, dev_outside=buf.ptr,
                dev_runs=buf.ptr, run_cap=4, dev_n_runs=buf.ptr, dev_send_owner=buf.ptr)

    def call(n_flows=nf, **kw):
        t = MatchTimeline(**{**good, **kw})
        return eng.lib.mgenx_msg_match_ex(
            eng.ctx, *[_ptr(x) for x in s], 12, *[_ptr(x) for x in r], 8, n_flows, 0,
            *[ctypes.c_void_p(o.ptr) for o in outs], ctypes.byref(t), _stream(0))

    assert call(width_us=0) == -1
    assert call(t0_us=2**62 + 1) == -1 and call(t0_us=-2**62 - 1) == -1
    assert call(n_bins=2**30) == -1                       # 2 flows x 2^30 windows = 2^31 cells
    assert call(dev_bins=None) == -1 and call(dev_outside=None) == -1
    assert call(dev_runs=None) == -1
    torch.cuda.synchronize()
    for o in outs + [buf]:
        assert (o.get(np.uint8) == PAT).all()             # found before anything ran
    # the same values with the part off, or nothing to write, are fine
    assert call(width_us=0, n_bins=0) == 0
    assert call(dev_runs=None, run_cap=0) == 0
    assert call(dev_bins=None, dev_outside=None, n_flows=0) == 0
    assert call(t0_us=2**62) == 0 and call(t0_us=-2**62) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
def _insert(text, at, line):
    lines = text.split(b"\n")
    assert lines[-1] == b""
    lines.insert(at, line)
    return b"\n".join(lines)


def test_text_logs_end_to_end(torch, eng, tmp_path, capsys):
    from mgen_amd import (ADDR_DTYPE, LOG_EPOCH, PACK_CHECKSUM, match_text_logs,
                          match_text_logs_timeline, to_device)
    from mgen_amd._abi import DESC_DTYPE
    from mgen_amd.workloads import make_templates
    t4, pool = make_templates(3, dst=(10, 1, 2, 3))
    t6, _ = make_templates(4, ipv6=True)
    t6["flow_id"] += 10                    # flow ids 11..14; 14 is seen by the receiver alone
    tmpl = np.concatenate([t4, t6])
    n_tmpl, per, msg_len = len(tmpl), 40, 96
    n = 6 * per                            # the sender's messages
    extra = 7                              # the receiver-only flow's
    d = np.zeros(n + extra, DESC_DTYPE)
    d["tmpl"][:n] = np.arange(n) % 6
    d["tmpl"][n:] = 6
    d["seq_num"][:n] = np.arange(n) // 6
    d["seq_num"][n:] = np.arange(extra)
    t_us = T0US + 999_000 + np.arange(n + extra, dtype=np.int64) * 700
    d["tx_sec"], d["tx_usec"], d["msg_len"] = t_us // 10**6, t_us % 10**6, msg_len
    src_port = (40_000 + np.arange(n_tmpl)).astype(np.uint16)
    dt, dp, dd = to_device(tmpl), to_device(pool), to_device(d)
    crc = torch.empty(n_tmpl, dtype=torch.int32, device="cuda")
    eng.pack_prepare(dt, n_tmpl, dp, crc)
    slab = torch.zeros((n + extra) * msg_len, dtype=torch.uint8, device="cuda")
    out_len = eng.pack(dt, crc, dd, n + extra, dp, slab, stride=msg_len, opts=PACK_CHECKSUM)
    text, _ = eng.log_send(dt, dd, n, src_port=to_device(src_port), out_len=out_len,
                           protocol=1, opts=LOG_EPOCH)
    send_log = text.cpu().numpy().tobytes()
    assert send_log.count(b"\n") == n

    # on the way: the messages 60..89 (five of every flow) and a few more dropped
    dropped = np.unique(np.concatenate([np.arange(60, 90), [0, 6, 133, n - 1]]))
    keep = np.setdiff1d(np.arange(n + extra), dropped)
    rng = np.random.default_rng(5)
    sel = np.concatenate([keep, rng.choice(keep[keep < n], 12, replace=False)])
    sel = sel[np.argsort(sel + rng.uniform(-8, 8, len(sel)), kind="stable")]
    m = len(sel)
    rslab = slab.view(n + extra, msg_len)[torch.from_numpy(sel).cuda()].contiguous().view(-1)
    cols = eng.unpack(rslab, m, stride=msg_len, fixed_len=msg_len, ext=True)
    src = np.zeros(m, ADDR_DTYPE)
    src["type"], src["len"] = 1, 4
    src["port"] = src_port[d["tmpl"][sel]]
    src["addr"][:, :4] = [192, 168, 7, 1]
    rx_us = t_us[sel] + rng.integers(100, 5000, m)
    rtext, _ = eng.log_recv_text(rslab, m, cols, to_device(src.view(np.uint8)),
                                 to_device((rx_us // 10**6).astype(np.uint32)),
                                 to_device((rx_us % 10**6).astype(np.uint32)), stride=msg_len,
                                 opts=LOG_EPOCH)
    recv_log = rtext.cpu().numpy().tobytes()
    send_log = _insert(send_log, 0, b"%d.000000 START Mgen Version 5.02b" % T0)
    recv_log = _insert(recv_log, 33, b"not a log line")

    width = 50_000
    keys, flows, stats, bins, outside, runs, t0_us, n_send_flows = match_text_logs_timeline(
        send_log, recv_log, width)
    plain = match_text_logs(send_log, recv_log)
    assert flows.tobytes() == plain[1].tobytes() and keys.tobytes() == plain[0].tobytes()
    assert n_send_flows == 6 and len(keys) == 7 and keys["flow_id"].tolist()[-1] == 14
    assert t0_us == int(t_us[0]) and bins.shape == (7, (int(t_us[n - 1]) - t0_us) // width + 1)
    assert not outside.any() and not bins[6]["sent"].any()

    # the model over the send log's own columns: line k + 1 of the log is message k
    line = np.arange(n) + 1
    sec, usec = stamps(t_us[:n])
    send = dict(flow_idx=np.r_[NONE, d["tmpl"][:n]].astype(np.uint32),
                seq=np.r_[0, d["seq_num"][:n]].astype(np.uint32), t_sec=np.r_[0, sec],
                t_usec=np.r_[0, usec], len=np.r_[0, np.full(n, msg_len)].astype(np.uint32))
    rsec, rusec = stamps(rx_us)
    recv = dict(flow_idx=d["tmpl"][sel].astype(np.uint32), seq=d["seq_num"][sel].astype(np.uint32),
                tx_sec=stamps(t_us[sel])[0], tx_usec=stamps(t_us[sel])[1], rx_sec=rsec,
                rx_usec=rusec)
    _, _, wbins, wout, wruns = TL.model(7, send, recv, t0_us, width, bins.shape[1], 1)
    same("bins", bins.view(TL.BIN), wbins)
    same("runs", runs.view(TL.RUN), wruns)
    assert line[0] == 1 and int(runs[0]["first_send"]) == 1       # message 0 is line 2

    # the command line: the series, then the runs of at least 3
    from mgen_amd.match_series import main
    (tmp_path / "send.log").write_bytes(send_log)
    (tmp_path / "recv.log").write_bytes(recv_log)
    capsys.readouterr()
    assert main([str(tmp_path / "send.log"), str(tmp_path / "recv.log"), "0.05"]) == 0
    out = capsys.readouterr().out
    blocks = out.split("\n\n\n")
    assert len(blocks) == 7
    assert blocks[0].startswith("# flow>1 src>-/40000 dst>10.1.2.3/5000\n# bin_start_us sent ")
    assert blocks[3].startswith("# flow>11 src>-/40003 dst>::1/5000\n")
    assert blocks[6].count("\n") == 2                              # the receiver-only flow: no rows
    rows = [x.split() for x in blocks[0].split("\n")[2:] if x]
    assert [int(x[0]) for x in rows] == [t0_us + b * width for b in range(bins.shape[1])
                                         if bins[0][b]["sent"]]
    assert sum(int(x[1]) for x in rows) == per
    assert sum(int(x[5]) for x in rows) == int(flows[0]["sent"] - flows[0]["delivered"])
    assert all((x[7] == "-") == (x[3] == "0") for x in rows)
    assert main(["-r", "3", str(tmp_path / "send.log"), str(tmp_path / "recv.log"), "0.05"]) == 0
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "# flow dst length first_send_us last_send_us first_line last_line head tail"
    long_runs = [r for r in wruns if r["length"] >= 3]
    assert len(out) == 1 + len(long_runs) + 1 and len(long_runs) == 6
    want = long_runs[3]
    assert out[4].split() == ["11", "::1/5000", str(int(want["length"])),
                              str(int(want["t_first_us"])), str(int(want["t_last_us"])),
                              str(int(want["first_send"]) + 1), str(int(want["last_send"]) + 1),
                              "0", "0"]
    assert main(["-r", "0", "a", "b", "1"]) == 2 and main(["a", "b"]) == 2
