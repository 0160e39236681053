"""GPU: mgenx_msg_match (a sender's log joined with a receiver's: per-message delivery, loss
runs, latency) against the serial model of tests/msg_match_ref.py.  Integer arithmetic: every
output array and struct is compared byte for byte, and every call runs with guard regions around
its outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msg_match_ref as M  # noqa: E402

NONE = M.NONE
T0 = 1_700_000_000
GUARD = 256          # bytes on either side of every output
PAT = 0xA5


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


def run(torch, eng, nf, send, recv, opts=0):
    """One mgenx_msg_match call with GUARD bytes of PAT before and after every output; returns
    (send_rx_count, send_first_rx, recv_send, flows, stats) as numpy, in the model's dtypes."""
    from mgen_amd import FLOW_MATCH_DTYPE, MATCH_STATS_DTYPE, _ptr, _stream
    ns, nr = len(send["flow_idx"]), len(recv["flow_idx"])
    s = [dev(torch, send[k]) for k in M.SEND_COLS]
    r = [dev(torch, recv[k]) for k in M.RECV_COLS]
    sizes = (ns * 4, ns * 4, nr * 4, nf * FLOW_MATCH_DTYPE.itemsize, MATCH_STATS_DTYPE.itemsize)
    bufs = [torch.full((GUARD + b + GUARD,), PAT, dtype=torch.uint8, device="cuda") for b in sizes]
    outs = [ctypes.c_void_p(b.data_ptr() + GUARD) for b in bufs]
    rc = eng.lib.mgenx_msg_match(eng.ctx, *[_ptr(t) if t.numel() else None for t in s], ns,
                                 *[_ptr(t) if t.numel() else None for t in r], nr, nf, opts,
                                 *outs, _stream(0))
    assert rc == 0, eng.lib.mgenx_last_error(eng.ctx)
    torch.cuda.synchronize()
    got = []
    for b, size, dt in zip(bufs, sizes, (np.uint32, np.uint32, np.uint32, FLOW_MATCH_DTYPE,
                                         MATCH_STATS_DTYPE)):
        h = b.cpu().numpy()
        assert (h[:GUARD] == PAT).all() and (h[GUARD + size:] == PAT).all(), "write outside"
        got.append(h[GUARD:GUARD + size].copy().view(dt))
    return tuple(got)


def check(got, want):
    names = ("send_rx_count", "send_first_rx", "recv_send", "flows", "stats")
    for name, g, w in zip(names, got, want):
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


def make(flow, seq, lost=(), t_us=None, size=100, lat=300):
    """Send columns from flow / seq (stamp i ms after T0 unless given) and the recv side: every
    send not in `lost`, in send order, received `lat` us later."""
    flow = np.asarray(flow, np.uint32)
    n = len(flow)
    t = T0 * 10**6 + (np.arange(n, dtype=np.int64) * 1000 if t_us is None else np.asarray(t_us))
    send = dict(flow_idx=flow, seq=np.asarray(seq, np.uint32), t_sec=(t // 10**6).astype(np.uint32),
                t_usec=(t % 10**6).astype(np.uint32),
                len=np.broadcast_to(np.asarray(size, np.uint32), (n,)).copy())
    keep = np.ones(n, bool)
    keep[np.asarray(list(lost), np.int64)] = False
    return send, recv_of(send, np.nonzero(keep)[0], lat)


def recv_of(send, idx, lat=300):
    idx = np.asarray(idx, np.int64)
    rx = send["t_sec"][idx].astype(np.int64) * 10**6 + send["t_usec"][idx] + lat
    return dict(flow_idx=send["flow_idx"][idx], seq=send["seq"][idx], tx_sec=send["t_sec"][idx],
                tx_usec=send["t_usec"][idx], rx_sec=(rx // 10**6).astype(np.uint32),
                rx_usec=(rx % 10**6).astype(np.uint32))


def both(torch, eng, nf, send, recv, opts=0):
    want = M.model(nf, send, recv, no_time=bool(opts & 1))
    return check(run(torch, eng, nf, send, recv, opts), want)


# ------------------------------------------------------------------ the small cases
def test_tiny_nothing_lost(torch, eng):
    send, recv = make(np.arange(15) % 3, np.arange(15) // 3)
    cnt, first, rs, flows, stats = both(torch, eng, 3, send, recv)
    assert cnt.tolist() == [1] * 15 and rs.tolist() == list(range(15))
    assert flows["sent"].tolist() == flows["delivered"].tolist() == [5, 5, 5]
    assert not flows["loss_runs"].any() and flows["lat_min"].tolist() == [300] * 3
    # the same through Engine.msg_match
    from mgen_amd import FLOW_MATCH_DTYPE
    out = eng.msg_match(3, {k: dev(torch, v) for k, v in send.items()},
                        {k: dev(torch, v) for k, v in recv.items()})
    torch.cuda.synchronize()
    assert out[3].cpu().numpy().view(FLOW_MATCH_DTYPE).tobytes() == flows.tobytes()
    assert out[2].cpu().numpy().view(np.uint32).tolist() == list(range(15))


def test_no_send_records(torch, eng):
    _, recv = make(np.arange(10) % 2, np.arange(10) // 2)
    cnt, first, rs, flows, stats = both(torch, eng, 2, M.cols(M.SEND_COLS, []), recv)
    assert (rs == NONE).all() and flows["rx_orphan"].tolist() == [5, 5]
    assert int(stats[0]["recv_unmatched"]) == 10


def test_no_recv_records(torch, eng):
    send, _ = make(np.arange(2100) % 3, np.arange(2100) // 3)
    cnt, first, rs, flows, stats = both(torch, eng, 4, send, M.cols(M.RECV_COLS, []))
    assert flows["lost_head"].tolist() == flows["sent"].tolist() == [700, 700, 700, 0]
    assert flows["loss_runs"].tolist() == [1, 1, 1, 0] and not flows["lost_tail"].any()
    assert int(flows[3]["lat_min"]) == 2**63 - 1 and int(flows[3]["lat_max"]) == -2**63


def test_no_flows(torch, eng):
    send, recv = make([NONE] * 5, range(5))
    cnt, first, rs, flows, stats = both(torch, eng, 0, send, recv)
    assert int(stats[0]["send_skipped"]) == 5 == int(stats[0]["recv_skipped"])


# ------------------------------------------------------------------ chunk and flow edges
def test_one_run_across_two_chunk_edges(torch, eng):
    """Positions 1000..3100 of one flow are lost: the run crosses the edges at 1024, 2048 and
    3072, with two whole chunks undelivered."""
    n = 4000
    send, recv = make(np.zeros(n), np.arange(n), lost=range(1000, 3101))
    _, _, _, flows, _ = both(torch, eng, 1, send, recv)
    assert int(flows[0]["loss_runs"]) == 1 and int(flows[0]["loss_run_max"]) == 2101
    assert int(flows[0]["lost_head"]) == 0 == int(flows[0]["lost_tail"])
    assert flows[0]["loss_run_hist"].tolist() == [0] * 11 + [1] + [0] * 6


@pytest.mark.parametrize("whole", [False, True])
def test_runs_do_not_merge_across_flow_edges(torch, eng, whole):
    """A flow edge at every offset 1020..1028 of a chunk, loss runs on both sides of it (the
    whole first flow lost, or its last five records)."""
    for edge in range(1020, 1029):
        flow = np.concatenate([np.zeros(edge), np.ones(40)])
        # the send log interleaves the flows: the sorted order puts the edge at `edge`
        order = np.argsort(np.concatenate([np.arange(edge) * 2, np.arange(40) * 50 + 1]),
                           kind="stable")
        seq = np.concatenate([np.arange(edge), np.arange(40)])
        lost_sorted = list(range(0 if whole else edge - 5, edge + 5))
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        send, recv = make(flow[order], seq[order], lost=inv[lost_sorted])
        _, _, _, flows, _ = both(torch, eng, 2, send, recv)
        assert int(flows[1]["lost_head"]) == 5 and int(flows[1]["lost_tail"]) == 0, edge
        if whole:
            assert int(flows[0]["lost_head"]) == edge and int(flows[0]["lost_tail"]) == 0, edge
        else:
            assert int(flows[0]["lost_head"]) == 0 and int(flows[0]["lost_tail"]) == 5, edge
        assert flows["loss_runs"].tolist() == [1, 1], edge


def test_many_short_runs_and_one_delivered(torch, eng):
    """Flow 0: 40,000 messages, every second one lost (20,000 runs of 1).  Flow 1: 40,000 with a
    single delivered message in the middle."""
    n = 40_000
    flow = np.concatenate([np.zeros(n), np.ones(n)])
    seq = np.concatenate([np.arange(n), np.arange(n)])
    lost = list(range(1, n, 2)) + [n + i for i in range(n) if i != 20_001]
    send, recv = make(flow, seq, lost=lost)
    _, _, _, flows, _ = both(torch, eng, 2, send, recv)
    assert int(flows[0]["loss_runs"]) == 20_000 == int(flows[0]["loss_run_hist"][0])
    assert int(flows[0]["lost_tail"]) == 1 and int(flows[0]["lost_head"]) == 0
    assert (int(flows[1]["lost_head"]), int(flows[1]["lost_tail"])) == (20_001, 19_998)
    assert int(flows[1]["delivered"]) == 1 and int(flows[1]["loss_runs"]) == 2


def test_one_run_past_the_carry_kernels_first_round(torch, eng):
    """One flow of 2^20 + 1025 + 3 messages of which only the first and the last arrive: 1026
    chunks, so the one-workgroup carry kernels (match_carry_kernel; for the run list also
    match_carry_fl_kernel and match_run_base_kernel) walk a second round of 1024 chunks with the
    run still open.  The expectation is closed-form."""
    from mgen_amd import LOSS_RUN_DTYPE
    ns = 2**20 + 1025 + 3
    send, _ = make(np.zeros(ns), np.arange(ns))
    recv = recv_of(send, [0, ns - 1])
    cnt, first, rs, flows, stats = run(torch, eng, 1, send, recv)
    f = flows[0]
    assert rs.tolist() == [0, ns - 1] and int(cnt.sum()) == 2
    assert (int(f["sent"]), int(f["delivered"])) == (ns, 2)
    assert (int(f["loss_runs"]), int(f["loss_run_max"])) == (1, ns - 2)
    want_hist = [0] * 18
    want_hist[min((ns - 2).bit_length() - 1, 17)] = 1
    assert f["loss_run_hist"].tolist() == want_hist
    assert int(f["lost_head"]) == 0 == int(f["lost_tail"])
    # the run list at min_run = 1
    out = eng.msg_match_timeline(1, {k: dev(torch, v) for k, v in send.items()},
                                 {k: dev(torch, v) for k, v in recv.items()},
                                 T0 * 10**6, 2**40, 1, min_run=1)
    torch.cuda.synchronize()
    assert out[3].cpu().numpy().tobytes() == flows.tobytes()
    runs = out[7].cpu().numpy().view(LOSS_RUN_DTYPE)
    assert len(runs) == 1
    assert (int(runs[0]["flow_idx"]), int(runs[0]["length"])) == (0, ns - 2)
    assert (int(runs[0]["first_send"]), int(runs[0]["last_send"])) == (1, ns - 2)


# ------------------------------------------------------------------ identity and duplicates
def test_identity(torch, eng):
    """Equal (flow, seq) with different stamps: distinct messages, duplicates under NO_TIME.
    Equal seq and stamp in different flows never match each other."""
    from mgen_amd import MATCH_NO_TIME
    t = np.array([0, 1000, 2000, 2000, 5000, 6000], np.int64)
    send, _ = make([0, 0, 0, 1, 1, 2], [7, 7, 8, 8, 9, 9], t_us=t)
    # recvs: flow 0 seq 7 second stamp; flow 1 seq 8 (stamp of send 2 and 3); flow 2 seq 9 with
    # the stamp of flow 1's seq 9 (send 4): an orphan by default
    recv = recv_of(send, [1, 3, 4])
    recv["flow_idx"][2] = 2
    cnt, first, rs, flows, stats = both(torch, eng, 3, send, recv)
    assert rs.tolist() == [1, 3, NONE] and cnt.tolist() == [0, 1, 0, 1, 0, 0]
    assert int(stats[0]["send_dup"]) == 0 and int(flows[2]["rx_orphan"]) == 1
    cnt, first, rs, flows, stats = both(torch, eng, 3, send, recv, MATCH_NO_TIME)
    assert rs.tolist() == [0, 3, 5] and cnt.tolist() == [1, 0, 0, 1, 0, 1]
    assert int(stats[0]["send_dup"]) == 1 == int(flows[0]["send_dup"])


def test_send_duplicates_far_apart(torch, eng):
    n = 20_000
    flow, seq = np.arange(n) % 7, np.arange(n) // 7
    t = np.arange(n, dtype=np.int64) * 1000
    for a, b in ((7000, 5), (19_000, 5), (19_001, 18_000)):   # three of one identity, two of one
        flow[a], seq[a], t[a] = flow[b], seq[b], t[b]
    send, _ = make(flow, seq, t_us=t)
    recv = recv_of(send, [19_000, 7000, 5, 18_000, 19_001, 100])
    cnt, first, rs, flows, stats = both(torch, eng, 7, send, recv)
    assert rs.tolist() == [5, 5, 5, 18_000, 18_000, 100]
    assert cnt[5] == 3 and cnt[7000] == 0 == cnt[19_000] and first[5] == 0
    assert first[7000] == NONE and int(stats[0]["send_dup"]) == 3


def test_rx_duplicates_first_is_the_lowest_index(torch, eng):
    send, _ = make(np.zeros(300), np.arange(300))
    recv = recv_of(send, [10, 20, 10, 10, 30])
    recv["rx_usec"][0] += 5000          # the later copies arrived earlier by the clock
    cnt, first, rs, flows, stats = both(torch, eng, 1, send, recv)
    assert first[10] == 0 and cnt[10] == 3 and int(flows[0]["rx_dup"]) == 2
    assert int(flows[0]["lat_max"]) == 5300 and int(flows[0]["lat_min"]) == 300


# ------------------------------------------------------------------ table pressure
@pytest.fixture(scope="module")
def pressure():
    """150,000 sends (seq = index, 64 flows, a few skipped), recvs shuffled with 5 % dropped and
    1 % duplicated, and the model: computed once."""
    n, nf = 150_000, 64
    rng = np.random.default_rng(20261020)
    flow = rng.integers(0, nf, n).astype(np.uint32)
    flow[rng.integers(0, n, 40)] = NONE
    flow[rng.integers(0, n, 40)] = nf            # the first index that does not count
    send, _ = make(flow, np.arange(n), size=rng.integers(28, 70_000, n))
    keep = np.nonzero(rng.random(n) >= 0.05)[0]
    idx = np.concatenate([keep, keep[rng.random(len(keep)) < 0.01]])
    rng.shuffle(idx)
    recv = recv_of(send, idx, lat=rng.integers(-2000, 900_000, len(idx)))
    return nf, send, recv, M.model(nf, send, recv)


def test_table_pressure(torch, eng, pressure):
    nf, send, recv, want = pressure
    got = check(run(torch, eng, nf, send, recv), want)
    flows, stats = got[3], got[4]
    assert int(stats[0]["send_skipped"]) > 40 and int(stats[0]["recv_skipped"]) > 40
    assert int(flows["rx_dup"].sum()) > 1000 and int(flows["loss_runs"].sum()) > 5000


def test_two_runs_leave_identical_bytes(torch, eng, pressure):
    nf, send, recv, _ = pressure
    a = run(torch, eng, nf, send, recv)
    b = run(torch, eng, nf, send, recv)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("ns", [4096, 4097])
def test_slot_rounding(torch, eng, ns):
    rng = np.random.default_rng(ns)
    send, _ = make(rng.integers(0, 5, ns), rng.integers(0, 2**32, ns, dtype=np.uint64))
    idx = rng.permutation(ns)[: ns - 300]
    recv = recv_of(send, idx)
    recv["seq"][:20] ^= 0x80000000          # orphans
    both(torch, eng, 5, send, recv)


# ------------------------------------------------------------------ end to end
def _insert(text, at, line):
    lines = text.split(b"\n")
    assert lines[-1] == b""
    lines.insert(at, line)
    return b"\n".join(lines)


def _host_flow_numbering(parsed, nf_before, table):
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
    from mgen_amd import (ADDR_DTYPE, EVENT_RECV, EVENT_SEND, LOG_EPOCH, PACK_CHECKSUM, PARSE_OK,
                          match_text_logs, to_device)
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

    # on the way: 30 messages dropped, 12 duplicated, the order disturbed
    rng = np.random.default_rng(5)
    dropped = rng.choice(n, 30, replace=False)
    dropped = np.unique(np.concatenate([dropped, [0, 6, n - 1]]))   # head and tail for certain
    keep = np.setdiff1d(np.arange(n + extra), dropped)
    sel = np.concatenate([keep, rng.choice(keep[keep < n], 12, replace=False)])
    sel = sel[np.argsort(sel + rng.uniform(-8, 8, len(sel)), kind="stable")]
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
    recv_log = rtext.cpu().numpy().tobytes()
    assert recv_log.count(b"\n") == m

    send_log = _insert(send_log, 0, b"%d.000000 START Mgen Version 5.02b" % T0)
    send_log = _insert(send_log, 17, b"%d.100000 SEND proto>UDP flow>x seq>1" % T0)
    recv_log = _insert(recv_log, 0, b"%d.000000 LISTEN proto>UDP port>5000" % T0)
    recv_log = _insert(recv_log, 33, b"not a log line")

    keys, flows, stats, cnt, first, rs, n_send_flows = match_text_logs(send_log, recv_log)
    assert n_send_flows == 6 and len(keys) == 7 == len(flows)
    assert keys["flow_id"].tolist() == [1, 2, 3, 11, 12, 13, 14]
    assert keys["dst"]["len"].tolist() == [4, 4, 4, 16, 16, 16, 16]
    assert len(cnt) == n + 2 == len(first) and len(rs) == m + 2
    lost = np.bincount(d["tmpl"][dropped], minlength=7)[:6]
    assert (flows["sent"][:6] - flows["delivered"][:6]).tolist() == lost.tolist()
    assert flows["sent"][:6].tolist() == [per] * 6 and int(flows[6]["sent"]) == 0
    assert int(flows[6]["rx_orphan"]) == extra == int(stats["recv_unmatched"])
    assert int(flows["rx_dup"].sum()) == 12 and int(flows[0]["lost_head"]) >= 2
    assert int(stats["send_skipped"]) == 2 == int(stats["recv_skipped"])

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
    ps, pr = parse(send_log, EVENT_SEND), parse(recv_log, EVENT_RECV)
    table = {}
    s_idx = _host_flow_numbering(ps, 0, table)
    r_idx = _host_flow_numbering(pr, len(table), table)
    u = lambda a: a.view(np.uint32)  # noqa: E731
    send = dict(flow_idx=s_idx, seq=u(ps["seq_num"]), t_sec=u(ps["rx_sec"]),
                t_usec=u(ps["rx_usec"]), len=u(ps["size"]))
    recv = dict(flow_idx=r_idx, seq=u(pr["seq_num"]), tx_sec=u(pr["tx_sec"]),
                tx_usec=u(pr["tx_usec"]), rx_sec=u(pr["rx_sec"]), rx_usec=u(pr["rx_usec"]))
    want = M.model(7, send, recv)
    check((cnt, first, rs, flows.view(M.FLOW), np.array([stats]).view(M.STATS)), want)

    # the command-line tool prints one row per flow
    from mgen_amd.match import main
    (tmp_path / "send.log").write_bytes(send_log)
    (tmp_path / "recv.log").write_bytes(recv_log)
    capsys.readouterr()
    assert main([str(tmp_path / "send.log"), str(tmp_path / "recv.log")]) == 0
    out = capsys.readouterr().out.split("\n")
    assert out[0].startswith("# flow dst sent delivered lost") and len(out) == 1 + 7 + 1
    assert out[1].split()[:5] == ["1", "10.1.2.3/5000", str(per), str(per - lost[0]), str(lost[0])]
    assert out[7].split()[:4] == ["14", "::1/5000", "0", "0"]
