"""Binary log ingest on the GPU (mgenx_binlog_parse): every column of a shuffled mixed log
against the plain-Python model (binlog_parse_ref) and against the text route the project
already trusts (mgenx_convert_binary_log -> mgenx_text_index -> mgenx_log_parse_text), the
payload bytes with the two-pass convention, rejected stored messages, and guard words after
every output array."""
import ctypes

import numpy as np
import pytest

import binlog_parse_ref as M
import binlog_util as B
import logparse_ref as R
from test_binlog_parse_cpu import rejected_records, tcp_send_cuts
from test_gpu_logparse import _rows

pytestmark = pytest.mark.gpu
GUARD = 64
LOG_EPOCH = 0x1


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
def mixed(oracle):
    """(log image, its records): 1500 RECV, 300 SEND (UDP / SINK) and the TCP SEND cuts, every
    other event, 80 MGEN_DATA records, shuffled."""
    rng = np.random.default_rng(31)
    parts = (B.recv_records(oracle, n=1500) + B.send_records(oracle, n=300) + B.events(rng) +
             B.data_recv_records(oracle, n=80) + tcp_send_cuts(oracle))
    parts = [parts[i] for i in rng.permutation(len(parts))]
    return B.binlog(parts), parts


def _device_log(torch, log):
    import mgen_amd
    offs, info = mgen_amd.binlog_index(log)
    assert info.status == 0
    buf = torch.from_numpy(np.frombuffer(bytes(log), np.uint8).copy()).cuda()
    ro = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    return buf, ro, int(info.n_records)


def _expect(got, want, k):
    """status and event always; every field of an OK record."""
    assert (got["status"], got["event"]) == (want["status"], want["event"]), k
    if want["status"] != R.OK:
        return
    diff = {f: (got[f], want[f]) for f in want if f in got and got[f] != want[f]}
    assert not diff, (k, diff)
    assert got["msg_len"] == min(want["size"], 65535) and got["payload_type"] == 0
    assert got["dst_addr4"] == int.from_bytes(want["dst"][3][:4], "little")
    assert got["payload_len"] == len(want["data"])


def test_mixed_log_matches_model_and_text_route(torch, eng, mixed):
    log, parts = mixed
    buf, ro, n = _device_log(torch, log)
    assert n == len(parts)
    got = _rows(eng.binlog_parse(buf, ro, n, payload=True), n)
    want = [M.parse_record(r) for r in parts]
    for k in range(n):
        w = dict(want[k])
        del w["kind"]
        _expect(got[k], w, k)
    assert {w["event"] for w in want} == set(range(1, 17)) - {2}
    # the text route: convert (epoch stamps), index, parse; REPORT lines are not records
    text, _ = eng.convert_binary_log(buf, ro, n, 0, LOG_EPOCH)
    line_off, n_lines = eng.text_index(text)
    tp = eng.log_parse_text(text, line_off, n_lines, payload=True)
    keep = np.nonzero(tp["event"].cpu().numpy() != 17)[0]
    assert len(keep) == n and n_lines > n
    trows = _rows(tp, n_lines)
    rejected = refused = 0
    for k, j in enumerate(keep):
        t, g = trows[j], dict(got[k])
        assert t["event"] == g["event"], k
        if want[k]["status"] != R.OK:      # a rejected stored message: the converter logs a
            rejected += 1                  # fresh MgenMsg there, the ingest says MALFORMED
            assert g["status"] == R.MALFORMED and g["err"] == R.ERROR_NOT_RECV
            continue
        if t["status"] != R.OK:
            # the contract's other exception: a value the text grammar refuses is kept, status
            # OK (the golden matrix holds a few messages with tx_usec >= 10^6); the model check
            # above has compared every field of the record
            refused += 1
            assert want[k]["tx_usec"] >= 1_000_000 and g["status"] == R.OK, k
            continue
        if t["event"] == R.RECV:
            assert t["ttl"] == 0 and t["present"] & R.HAS_TTL
            t["ttl"], t["present"] = -1, t["present"] & ~R.HAS_TTL
        assert t == g, (k, {f: (t[f], g[f]) for f in t if t[f] != g[f]})
    assert rejected < n // 20 and refused < 10


def test_payload_two_passes_and_empty_batch(torch, eng, mixed):
    from mgen_amd import LOGPARSE_COLS, LogparseOut, _ptr, _stream
    log, parts = mixed
    buf, ro, n = _device_log(torch, log)
    want = [M.parse_record(r) for r in parts]
    data = [w["data"] if w["status"] == R.OK else b"" for w in want]
    total = sum(map(len, data))
    assert total > 1000
    ev = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    s = LogparseOut()
    s.event, s.status, s.payload_off = ev.data_ptr(), st.data_ptr(), off.data_ptr()

    def run(cap):
        pay = torch.full((max(cap, 1) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        s.payload, s.payload_cap = pay.data_ptr(), cap
        rc = eng.lib.mgenx_binlog_parse(eng.ctx, _ptr(buf), buf.numel(), _ptr(ro), n, 0,
                                        ctypes.byref(s), _stream(0))
        assert rc == 0
        torch.cuda.synchronize()
        return pay.cpu().numpy()
    small = run(total - 1)                       # too small: the offsets only
    offs = off.cpu().numpy()
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum([len(d) for d in data])]))
    assert (small == 0xA5).all()
    full = run(total)
    assert bytes(full[:total]) == b"".join(data) and (full[total:] == 0xA5).all()
    # n == 0: only payload_off[0] is written
    off.fill_(-7)
    rc = eng.lib.mgenx_binlog_parse(eng.ctx, None, 0, None, 0, 0, ctypes.byref(s), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist()[:2] == [0, -7]
    p = eng.binlog_parse(buf[:0], ro[:0], 0, payload=True)
    assert all(p[name].numel() == 0 for name, _, _ in LOGPARSE_COLS) and p["payload"].numel() == 0


def test_rejected_stored_messages(torch, eng, oracle):
    """test_convert_logs_rejected_stored_messages' corpus between good records: MALFORMED with
    the event still right, the neighbours unaffected."""
    recs, n_recv = rejected_records(oracle)
    rng = np.random.default_rng(9)
    good = B.recv_records(oracle, n=40) + B.events(rng)
    good = [g for g in good if M.parse_record(g)["status"] == R.OK]
    parts, bad_at = [], []
    for k, g in enumerate(good):
        parts.append(g)
        if k < len(recs):
            bad_at.append(len(parts))
            parts.append(recs[k])
    assert len(bad_at) == len(recs)
    buf, ro, n = _device_log(torch, B.binlog(parts))
    assert n == len(parts)
    got = _rows(eng.binlog_parse(buf, ro, n, payload=True), n)
    for k in range(n):
        w = M.parse_record(parts[k])
        del w["kind"]
        assert (w["status"] != R.OK) == (k in bad_at)
        _expect(got[k], w, k)
        if k in bad_at:
            assert got[k]["err"] == R.ERROR_NOT_RECV
            assert got[k]["event"] == (1 if bad_at.index(k) < n_recv else 3)


def test_guard_words_after_every_array(torch, eng, mixed):
    from mgen_amd import LOGPARSE_COLS, LogparseOut, _ptr, _stream
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    log, parts = mixed
    buf, ro, n = _device_log(torch, log)
    n = 1000                         # not a multiple of the workgroup's 256 records
    total = sum(len(w["data"]) for w in map(M.parse_record, parts[:n]) if w["status"] == R.OK)
    arrs = {}
    for name, dt, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT:
        t = torch.empty((n + GUARD) * w, dtype=getattr(torch, dt), device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        arrs[name] = t
    arrs["payload_off"] = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    arrs["payload"] = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    s = LogparseOut()
    for name, _, _ in LOGPARSE_COLS:
        setattr(s, name, arrs[name].data_ptr())
    s.cols = eng._cols_struct({k: arrs[k] for k, _, _ in COLS_CORE + COLS_EXT})
    s.payload, s.payload_cap = arrs["payload"].data_ptr(), total
    s.payload_off = arrs["payload_off"].data_ptr()
    rc = eng.lib.mgenx_binlog_parse(eng.ctx, _ptr(buf), buf.numel(), _ptr(ro), n, 0,
                                    ctypes.byref(s), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    widths = {name: w for name, _, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT}
    widths.update(payload_off=1, payload=1)
    used = {name: n * w for name, w in widths.items()}
    used["payload_off"], used["payload"] = n + 1, total
    for name, t in arrs.items():
        tail = t[used[name]:]
        assert tail.numel() == GUARD * widths[name]
        if name == "payload_off":
            assert bool((tail == -7).all()), name
        else:
            assert bool((tail.view(torch.uint8) == 0xA5).all()), name
    assert int(arrs["payload_off"][n].item()) == total
    assert bool((arrs["event"][:n] != 0).all())
