"""Binary logs through the analysis helpers (mgen_amd.analyze_text_log*, match_text_logs*): a
binary receiver log gives what its epoch-converted text gives, a binary sender's log joins
with a text or a binary receiver's log on a scenario whose losses are known by construction,
and a truncated binary log is an error, not a prefix."""
import numpy as np
import pytest

import binlog_util as B

pytestmark = pytest.mark.gpu
LOG_EPOCH = 0x1


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def recv_log(oracle):
    """(binary receiver log, its epoch text, records, REPORT lines of the text)."""
    rng = np.random.default_rng(41)
    import binlog_parse_ref as M
    parts = (B.recv_records(oracle, n=600) + B.events(rng) + B.data_recv_records(oracle, n=40))
    # the golden matrix holds a few messages whose tx_usec is 10^6 or more: the contract keeps
    # them (status OK) where the text grammar refuses the converted line, so the two routes
    # differ there by design (test_binlog_parse_cpu.test_model_exceptions); they stay out here
    agree = [r for r in parts if M.parse_record(r)["tx_usec"] < 1_000_000]
    assert len(parts) - 5 < len(agree) < len(parts)
    parts = agree
    log = B.binlog(parts)
    text, st, n = oracle.convert_binary_log(log, opts=LOG_EPOCH)
    assert st == 0 and n == len(parts)
    reports = text.count(b" REPORT ")
    assert reports >= 40 and text.count(b"\n") == n + reports
    return log, text, n, reports


def _same_arrays(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def test_analyze_text_log(torch, recv_log):
    import mgen_amd
    log, text, n, reports = recv_log
    bk, bc, bn, bbad = mgen_amd.analyze_text_log(log)
    tk, tc, tn, tbad = mgen_amd.analyze_text_log(text)
    assert (bn, tn) == (n, n + reports) and bbad == tbad and len(bk) > 10
    _same_arrays(bk, tk)
    _same_arrays(bc, tc)


def test_analyze_text_log_dist(torch, recv_log):
    import mgen_amd
    log, text, n, reports = recv_log
    b = mgen_amd.analyze_text_log_dist(log)
    t = mgen_amd.analyze_text_log_dist(text)
    assert (b[4], t[4]) == (n, n + reports) and b[5] == t[5]
    for x, y in zip(b[:4], t[:4]):
        _same_arrays(x, y)


def test_analyze_text_log_series(torch, recv_log):
    import mgen_amd
    log, text, n, reports = recv_log
    b = mgen_amd.analyze_text_log_series(log, 10_000_000, n_bins=32, permille=(500, 990))
    t = mgen_amd.analyze_text_log_series(text, 10_000_000, n_bins=32, permille=(500, 990))
    assert (b[4], t[4]) == (n, n + reports) and b[5] == t[5] and b[3] == t[3]
    for k in (0, 1, 2, 6):
        _same_arrays(b[k], t[k])


def test_analyze_text_log_clock(torch, recv_log):
    import mgen_amd
    log, text, n, reports = recv_log
    bk, bc, bn, bbad = mgen_amd.analyze_text_log_clock(log)
    tk, tc, tn, tbad = mgen_amd.analyze_text_log_clock(text)
    assert (bn, tn) == (n, n + reports) and bbad == tbad
    _same_arrays(bk, tk)
    # ia / ib are indices into the log's own elements: record k of the binary log is the k-th
    # line of the text that is not a REPORT line, so they are compared through that map
    line_of = np.array([j for j, ln in enumerate(text.split(b"\n")[:-1])
                        if b" REPORT " not in ln], np.uint32)
    assert len(line_of) == n
    mapped = bc.copy()
    for name in ("ia", "ib"):
        some = bc[name] != mgen_amd.CLOCK_NONE
        assert some.any()
        mapped[name][some] = line_of[bc[name][some]]
    _same_arrays(mapped, tc)


@pytest.fixture(scope="module")
def scenario(oracle):
    """Two flows of 50 messages from one sender, written with the oracle's binary writers.
    Flow 1 loses seq 0-2 (head), 10, 20-21 and 48-49 (tail); flow 2 loses 5-7.  Returns (binary
    send log, binary recv log, {flow id: expected counts})."""
    from mgen_amd.workloads import make_templates
    from mgen_amd._abi import DESC_DTYPE
    per, size = 50, 128
    tmpl, pool = make_templates(2)
    n = 2 * per
    i = np.arange(n)
    d = np.zeros(n, DESC_DTYPE)
    d["tmpl"], d["seq_num"] = i % 2, i // 2
    d["tx_sec"], d["tx_usec"] = 1_700_000_000 + i // 10, (i % 10) * 1000
    d["msg_len"] = size
    offs = (i * size).astype(np.uint64)
    sizes = np.full(n, size, np.uint32)
    slab, _ = oracle.udp_pack_batch(tmpl, d, pool, n * size + 16, rec_off=offs, checksum=True)
    f = oracle.udp_recv_batch(slab, n, rec_off=offs, rec_len=sizes)
    assert (f["err"] == 0).all()
    ports = np.array([40001, 40002], np.uint16)
    send_log = B.binlog([B.start(1_699_999_999, 0),
                         oracle.log_send_batch(tmpl, d, pool, ports, protocol=1, binary=True)])
    lost = {1: {0, 1, 2, 10, 20, 21, 48, 49}, 2: {5, 6, 7}}
    keep = np.array([int(d["seq_num"][k]) not in lost[int(d["tmpl"][k]) + 1] for k in range(n)])
    src = np.zeros(n, oracle.ADDR_DTYPE)
    src["type"], src["len"] = 1, 4
    src["addr"][:, :4] = [10, 0, 0, 1]
    src["port"] = ports[d["tmpl"]]
    rx_s = d["tx_sec"].astype(np.uint32)
    rx_u = (d["tx_usec"] + 250).astype(np.uint32)
    idx = np.nonzero(keep)[0]
    recv_log = B.binlog([B.listen(1_699_999_999, 5, 1, 5000),
                         oracle.log_recv_binary(f[idx], slab, offs[idx], src[idx], rx_s[idx],
                                                rx_u[idx], protocol=1)])
    want = {1: dict(sent=50, delivered=42, lost_head=3, lost_tail=2, loss_runs=4),
            2: dict(sent=50, delivered=47, lost_head=0, lost_tail=0, loss_runs=1)}
    return send_log, recv_log, want


@pytest.mark.parametrize("recv_as", ["binary", "text"])
def test_match_binary_send_log(torch, oracle, scenario, recv_as):
    import mgen_amd
    send_log, recv_log, want = scenario
    if recv_as == "text":
        recv_log, st, _ = oracle.convert_binary_log(recv_log, opts=LOG_EPOCH)
        assert st == 0
    keys, flows, stats, cnt, first, rs, n_send = mgen_amd.match_text_logs(send_log, recv_log)
    assert n_send == len(keys) == 2 and len(cnt) == 101 and len(rs) == 90
    for k in range(2):
        w = want[int(keys["flow_id"][k])]
        got = {name: int(flows[name][k]) for name in w}
        assert got == w, (k, got)
        assert int(flows["lat_min"][k]) == int(flows["lat_max"][k]) == 250
        assert int(keys["src"]["port"][k]) == 0
    assert int(stats["recv_unmatched"]) == 0
    # the timeline and the multi-receiver forms run over the same ingest
    out = mgen_amd.match_text_logs_timeline(send_log, recv_log, 1_000_000)
    assert sorted(int(x) for x in out[5]["length"]) == [1, 2, 2, 3, 3]
    m = mgen_amd.match_text_logs_multi(send_log, [recv_log])
    assert m[1]["delivered"].reshape(-1).tolist() == [42, 47]


def test_truncated_binary_log_raises(torch, recv_log):
    import mgen_amd
    log = recv_log[0]
    with pytest.raises(mgen_amd.MgenxError, match="SHORT"):
        mgen_amd.analyze_text_log(log[:-5])
    with pytest.raises(mgen_amd.MgenxError, match="SHORT"):
        mgen_amd.match_text_logs(log[:-5], log)
