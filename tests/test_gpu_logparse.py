"""GPU: text log ingest (mgenx_text_index + mgenx_log_parse_text, Engine.text_index /
log_parse_text, mgen_amd.analyze_text_log).  The emitters' output is pinned byte for byte to
the oracle (tests/test_gpu_log.py), so parsing it back must return every field that went in;
status and the fields no emitter input defines are checked against the plain-Python grammar
checker (tests/logparse_ref.py, itself proven on the CPU in tests/test_logparse_cpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logparse_corpus as C   # noqa: E402
import logparse_ref as R      # noqa: E402

DAY = 1_699_920_000            # a UTC midnight


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
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "udp_matrix.npz"),
                        allow_pickle=False))


def _text(torch, buf):
    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda()


def _rows(p, n):
    """The parse outputs as per-line dicts in logparse_ref.parse_line's terms."""
    h = {k: v.cpu().numpy() for k, v in p.items()}
    src = h["src"].reshape(n, 20)
    dst_addr, host_addr = h["dst_addr"].reshape(n, 16), h["host_addr"].reshape(n, 16)
    u16 = lambda a: a.view(np.uint16)   # noqa: E731
    u32 = lambda a: a.view(np.uint32)   # noqa: E731
    off = h["payload_off"] if "payload_off" in h else None
    out = []
    for i in range(n):
        d = dict(event=int(h["event"][i]), status=int(h["status"][i]),
                 protocol=int(h["protocol"][i]), present=int(u16(h["present"])[i]),
                 rx_sec=int(u32(h["rx_sec"])[i]), rx_usec=int(u32(h["rx_usec"])[i]),
                 tx_sec=int(u32(h["tx_sec"])[i]), tx_usec=int(u32(h["tx_usec"])[i]),
                 flow=int(u32(h["flow_id"])[i]), seq=int(u32(h["seq_num"])[i]),
                 size=int(u32(h["size"])[i]), ttl=int(h["ttl"][i]), flags=int(h["flags"][i]),
                 err=int(h["err"][i]), gps=int(h["gps_status"][i]),
                 lat_raw=int(u32(h["lat_raw"])[i]), lon_raw=int(u32(h["lon_raw"])[i]),
                 alt=int(h["alt"][i]),
                 src=(int(src[i, 0]), int(src[i, 1]), int(src[i, 2]) | int(src[i, 3]) << 8,
                      bytes(src[i, 4:])),
                 dst=(int(h["dst_type"][i]), int(h["dst_len"][i]), int(u16(h["dst_port"])[i]),
                      bytes(dst_addr[i])),
                 host=(int(h["host_type"][i]), int(h["host_len"][i]),
                       int(u16(h["host_port"])[i]), bytes(host_addr[i])),
                 msg_len=int(u16(h["msg_len"])[i]), payload_len=int(u16(h["payload_len"])[i]),
                 payload_type=int(h["payload_type"][i]),
                 dst_addr4=int(u32(h["dst_addr4"])[i]))
        if off is not None:
            d["data"] = bytes(h["payload"][int(off[i]):int(off[i + 1])])
        out.append(d)
    return out


def _check(got, want, i, line=b""):
    """status (and event) always; every field of an OK line."""
    assert got["status"] == want["status"], (i, line[:200], got["status"])
    if want["status"] != R.OK:
        assert got["err"] == R.ERROR_NOT_RECV, (i, line[:200])
        return
    diff = {k: (got[k], want[k]) for k in want if k in got and got[k] != want[k]}
    assert not diff, (i, line[:200], diff)
    assert got["msg_len"] == min(want["size"], 65535)
    assert got["dst_addr4"] == int.from_bytes(want["dst"][3][:4], "little")
    assert got["payload_type"] == 0
    if "data" in want:
        assert got["payload_len"] == len(want["data"])


# ------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("mode,opts,proto", C.MATRIX_ROWS)
def test_round_trip_golden_matrix(torch, eng, gold, oracle, mode, opts, proto):
    from mgen_amd import OPT_CHECKSUM_FORCE, OPT_TCP, PARSE_NO_DAYS, to_device
    uopts = {"udp": 0, "udp_force": OPT_CHECKSUM_FORCE, "tcp_force": OPT_TCP | OPT_CHECKSUM_FORCE}
    n = len(gold["unpack_lens"])
    slab = to_device(gold["unpack_slab"]).view(torch.uint8)
    offs = to_device(gold["unpack_offs"]).view(torch.int64)
    lens = to_device(gold["unpack_lens"]).view(torch.int32)
    cols = eng.unpack(slab, n, rec_off=offs, rec_len=lens, opts=uopts[mode], ext=True)
    src, rx_sec, rx_usec, ttl = C.matrix_inputs(oracle, gold, opts)
    text, emit_off = eng.log_recv_text(
        slab, n, cols, to_device(src.view(np.uint8)), to_device(rx_sec), to_device(rx_usec),
        rec_off=offs, ttl=to_device(ttl), protocol=proto, opts=opts)
    line_off, n_lines = eng.text_index(text)
    assert n_lines == n
    assert np.array_equal(line_off.cpu().numpy(), emit_off.cpu().numpy())
    p = eng.log_parse_text(text, line_off, n, opts=PARSE_NO_DAYS, payload=True)
    torch.cuda.synchronize()
    want = C.expect_from_fields(gold[f"unpack_fields_{mode}"], gold["unpack_slab"],
                                gold["unpack_offs"], src, rx_sec, rx_usec, ttl, proto, opts)
    got = _rows(p, n)
    lines = R.split_lines(text.cpu().numpy().tobytes())
    for i in range(n):
        _check(got[i], want[i], i, lines[i])
    ok = np.array([w["status"] == R.OK for w in want])
    assert ok.sum() > n // 2
    assert sum(w["event"] == 2 for w in want) > 100          # RERR lines give their code
    # re-emit from the parsed columns and the decoded payload: the identical text.  The one
    # thing a line does not carry is WHY it has no gps> (an out-of-range status ends the line
    # early): such lines get an out-of-range status back.
    c2 = {k: v for k, v in p.items()}
    c2["payload_off"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    c2["hdr_len"] = torch.zeros(n, dtype=torch.int16, device="cuda")
    if not opts & 4:
        no_gps = (p["event"] == 1) & (p["status"] == 0) & ((p["present"] & 4) == 0)
        c2["gps_status"] = torch.where(no_gps, torch.full_like(p["gps_status"], 3),
                                       p["gps_status"])
    pay = torch.cat([p["payload"], torch.zeros(16, dtype=torch.uint8, device="cuda")])
    text2, _ = eng.log_recv_text(pay, n, c2, p["src"], p["rx_sec"], p["rx_usec"],
                                 rec_off=p["payload_off"][:n].contiguous(), ttl=p["ttl"],
                                 protocol=proto, opts=opts)
    lines2 = R.split_lines(text2.cpu().numpy().tobytes())
    assert len(lines2) == n
    bad = [(lines[i], lines2[i]) for i in range(n) if ok[i] and lines[i] != lines2[i]]
    assert not bad, bad[:3]


# ------------------------------------------------------------------ 2. line index
def _random_text(seed, total=300_000):
    rng = np.random.default_rng(seed)
    parts, size = [], 0
    while size < total:
        ln = int(rng.integers(0, 601))
        body = rng.integers(0, 256, ln, dtype=np.uint8)
        body[body == 10] = 32
        parts.append(body.tobytes() + b"\n")
        size += ln + 1
    return b"".join(parts)


@pytest.mark.parametrize("variant", ["final_lf", "no_final_lf", "empty", "only_lf"])
def test_text_index_matches_numpy(torch, eng, variant):
    buf = {"final_lf": _random_text(1), "no_final_lf": _random_text(2) + b"tail without lf",
           "empty": b"", "only_lf": b"\n" * 70_001}[variant]
    a = np.frombuffer(buf, np.uint8)
    ends = np.nonzero(a == 10)[0].astype(np.int64) + 1
    want = np.concatenate([[0], ends, [len(buf)] if len(buf) and buf[-1:] != b"\n" else []])
    text = _text(torch, buf) if buf else torch.zeros(1, dtype=torch.uint8, device="cuda")
    line_off, n = eng.text_index(text, nbytes=len(buf))
    assert n == len(want) - 1
    assert np.array_equal(line_off.cpu().numpy(), want.astype(np.int64))
    if n > 4:   # the too-small-cap pass: the count comes back, no offset is written
        cap = n - 1
        off = torch.full((cap + 1 + 64,), -7, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        from mgen_amd import _ptr, _stream
        rc = eng.lib.mgenx_text_index(eng.ctx, _ptr(text), len(buf), _ptr(off), cap, _ptr(cnt),
                                      _stream(0))
        assert rc == 0
        assert int(cnt.item()) == n and bool((off == -7).all())
        # an exact cap: cap + 1 offsets, nothing after them
        off2 = torch.full((n + 1 + 64,), -7, dtype=torch.int64, device="cuda")
        rc = eng.lib.mgenx_text_index(eng.ctx, _ptr(text), len(buf), _ptr(off2), n, _ptr(cnt),
                                      _stream(0))
        assert rc == 0
        h = off2.cpu().numpy()
        assert np.array_equal(h[:n + 1], want) and (h[n + 1:] == -7).all()


# ------------------------------------------------------------------ shared: packed records
def _emit(torch, eng, flow_id, seq, tx_sec, tx_usec, rx_sec, rx_usec, src, n_flows, opts,
          msg_len=64):
    """Pack -> unpack -> RECV lines of records (flow ids 1..n_flows) in the given order.
    Returns (text tensor, unpack columns, device src / rx_sec / rx_usec)."""
    from mgen_amd import PACK_CHECKSUM, to_device
    from mgen_amd._abi import DESC_DTYPE
    from mgen_amd.workloads import make_templates
    n = len(seq)
    tmpl, pool = make_templates(n_flows)
    d = np.zeros(n, DESC_DTYPE)
    d["tmpl"] = np.asarray(flow_id) - 1
    d["seq_num"], d["tx_sec"], d["tx_usec"], d["msg_len"] = seq, tx_sec, tx_usec, msg_len
    dt, dp = to_device(tmpl), to_device(pool)
    crc = torch.empty(n_flows, dtype=torch.int32, device="cuda")
    eng.pack_prepare(dt, n_flows, dp, crc)
    slab = torch.zeros(n * msg_len, dtype=torch.uint8, device="cuda")
    eng.pack(dt, crc, to_device(d), n, dp, slab, stride=msg_len, opts=PACK_CHECKSUM)
    cols = eng.unpack(slab, n, stride=msg_len, fixed_len=msg_len, ext=True)
    assert int(cols["err"].sum().item()) == 0
    d_src = to_device(src.view(np.uint8))
    d_rs, d_ru = to_device(np.asarray(rx_sec, np.uint32)), to_device(np.asarray(rx_usec, np.uint32))
    text, _ = eng.log_recv_text(slab, n, cols, d_src, d_rs, d_ru, stride=msg_len, opts=opts)
    return text, cols, d_src, d_rs, d_ru


def _flow_sources(oracle, flow_id):
    src = np.zeros(len(flow_id), oracle.ADDR_DTYPE)
    src["type"], src["len"] = 1, 4
    src["port"] = 7000 + np.asarray(flow_id)
    src["addr"][:, :4] = [10, 0, 0, 9]
    src["addr"][:, 3] = np.asarray(flow_id) & 255
    return src


# ------------------------------------------------------------------ 3. days
def test_legacy_stamps_across_two_midnights(torch, eng, oracle):
    n = 4096
    rng = np.random.default_rng(31)
    rx_us = (DAY + 86400 - 2) * 10**6 + 123456 + np.cumsum(
        rng.integers(0, 90_000_000, n, dtype=np.int64))
    rx_us[0] = (DAY + 86400 - 2) * 10**6 + 123456          # 23:59:58 of the first day
    tx_us = rx_us - rng.integers(-3_000_000, 3_000_001, n, dtype=np.int64)
    assert (rx_us[-1] - rx_us[0]) // 10**6 > 2 * 86400      # crosses two midnights
    flow = np.ones(n, np.uint32)
    text, _, _, _, _ = _emit(torch, eng, flow, np.arange(n), tx_us // 10**6, tx_us % 10**6,
                             rx_us // 10**6, rx_us % 10**6, _flow_sources(oracle, flow), 1, 0)
    line_off, n_lines = eng.text_index(text)
    assert n_lines == n
    p = eng.log_parse_text(text, line_off, n, day_base=DAY)
    assert int(p["status"].sum().item()) == 0
    got_rx = p["rx_sec"].cpu().numpy().view(np.uint32).astype(np.int64)
    got_tx = p["tx_sec"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got_rx, rx_us // 10**6)
    assert np.array_equal(got_tx, tx_us // 10**6)
    assert np.array_equal(p["rx_usec"].cpu().numpy().view(np.uint32), rx_us % 10**6)
    assert np.array_equal(p["tx_usec"].cpu().numpy().view(np.uint32), tx_us % 10**6)
    # MGENX_PARSE_NO_DAYS: both stay times of day
    from mgen_amd import PARSE_NO_DAYS
    q = eng.log_parse_text(text, line_off, n, opts=PARSE_NO_DAYS, day_base=DAY)
    assert np.array_equal(q["rx_sec"].cpu().numpy().view(np.uint32), (rx_us // 10**6) % 86400)
    assert np.array_equal(q["tx_sec"].cpu().numpy().view(np.uint32), (tx_us // 10**6) % 86400)


# ------------------------------------------------------------------ 4. analytics end to end
def test_analytics_from_text_equals_unpack_path(torch, eng, oracle):
    from mgen_amd import (FLOW_COUNTERS_DTYPE, LOG_EPOCH, REPORT_KEY_DTYPE, analyze_text_log)
    from mgen_amd.workloads import poisson_flows
    n_flows, window = 64, 0.05
    d = poisson_flows(n_flows * 512, n_flows, seed=77, loss=0.05, dup=0.02, reorder=6,
                      msg_len=64)
    n = len(d["seq"])
    src = _flow_sources(oracle, d["flow_id"])
    text, cols, d_src, d_rs, d_ru = _emit(torch, eng, d["flow_id"], d["seq"], d["tx_sec"],
                                          d["tx_usec"], d["rx_sec"], d["rx_usec"], src, n_flows,
                                          LOG_EPOCH)

    def reduce(c, s, rs, ru, m):
        table = eng.flow_table(1024)
        idx, nf = eng.flow_lookup(table, c, s, m)
        nf = int(nf.item())
        flows = eng.flow_init(nf, window)
        eng.flow_reduce(flows, nf, idx, c["seq_num"], c["tx_sec"], c["tx_usec"], c["msg_len"],
                        rs, ru, n=m)
        keys = eng.flow_keys(table, nf, protocol=1).cpu().numpy()
        cnt = eng.flow_export(flows, nf).cpu().numpy()
        idx = idx.cpu().numpy().view(np.uint32)
        eng.flow_table_destroy(table)
        return keys, cnt, nf, idx

    keys0, cnt0, nf0, idx0 = reduce(cols, d_src, d_rs, d_ru, n)
    assert nf0 == n_flows
    # the oracle on the same records
    of, _, _ = oracle.flow_reduce_batch(nf0, idx0, d["seq"], d["tx_sec"], d["tx_usec"],
                                        d["msg_len"], d["rx_sec"], d["rx_usec"], window=window,
                                        per_flow=0)
    c0 = cnt0.view(FLOW_COUNTERS_DTYPE)
    assert sum(a.dup_msg_count for a in of) > 0 and sum(a.n_reports for a in of) > n_flows
    for f, a in enumerate(of):
        assert (c0["msg_count"][f], c0["byte_count"][f], c0["dup_count"][f]) == (
            a.msg_count, a.byte_count, a.dup_msg_count), f
        assert c0["n_reports"][f] == a.n_reports and c0["seq_start"][f] == a.seq_start, f
        assert (c0["latency_sum"][f], c0["latency_min"][f], c0["latency_max"][f]) == (
            a.latency_sum, a.latency_min, a.latency_max), f
    # the same text with other events between the RECV lines
    lines = R.split_lines(text.cpu().numpy().tobytes())
    extra = [b"1700000000.000001 START Mgen Version 5.1.1\n",
             b"1700000000.000002 LISTEN proto>UDP port>5000\n",
             b"1700000000.000003 SEND proto>UDP flow>3 seq>9 srcPort>7003 dst>127.0.0.1/5000 "
             b"size>64\n",
             b"1700000000.000004 ON flow>1 srcPort>59275 dst>127.0.0.1/5000 \n"]
    mixed = []
    for i, ln in enumerate(lines):
        if i % 1000 == 0:
            mixed += extra
        mixed.append(ln)
    for buf, n_extra in ((b"".join(lines), 0), (b"".join(mixed), len(mixed) - n)):
        t = _text(torch, buf)
        line_off, m = eng.text_index(t)
        assert m == n + n_extra
        p = eng.log_parse_text(t, line_off, m)
        assert int(p["status"].sum().item()) == 0
        assert int((p["err"] == 0).sum().item()) == n
        keys1, cnt1, nf1, idx1 = reduce(p, p["src"], p["rx_sec"], p["rx_usec"], m)
        assert nf1 == nf0
        assert cnt1.tobytes() == cnt0.tobytes() and keys1.tobytes() == keys0.tobytes()
        assert int((idx1 == 0xFFFFFFFF).sum()) == n_extra
        k2, c2, m2, bad2 = analyze_text_log(buf, window=window)
        assert (m2, bad2) == (m, 0)
        assert c2.tobytes() == cnt0.tobytes()
        assert k2.tobytes() == keys0.view(REPORT_KEY_DTYPE)[:nf0].tobytes()


# ------------------------------------------------------------------ 5. malformed input
GUARD = 64


def _parse_guarded(torch, eng, text, line_off, n, payload_cap):
    """mgenx_log_parse_text into arrays that each end in a GUARD-element pattern region."""
    from mgen_amd import LOGPARSE_COLS, LogparseOut, _ptr, _stream
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    arrs = {}
    for name, dt, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT:
        t = torch.empty((n + GUARD) * w, dtype=getattr(torch, dt), device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        arrs[name] = t
    arrs["payload_off"] = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    arrs["payload"] = torch.full((payload_cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    s = LogparseOut()
    for name, _, _ in LOGPARSE_COLS:
        setattr(s, name, arrs[name].data_ptr())
    s.cols = eng._cols_struct({k: arrs[k] for k, _, _ in COLS_CORE + COLS_EXT})
    s.payload, s.payload_cap = arrs["payload"].data_ptr(), payload_cap
    s.payload_off = arrs["payload_off"].data_ptr()
    rc = eng.lib.mgenx_log_parse_text(eng.ctx, _ptr(text), text.numel(), _ptr(line_off), n, 0, 0,
                                      ctypes.byref(s), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    widths = {name: w for name, _, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT}
    widths.update(payload_off=1, payload=1)
    used = {name: n * w for name, w in widths.items()}
    used["payload_off"], used["payload"] = n + 1, payload_cap
    for name, t in arrs.items():
        tail = t[used[name]:]
        assert tail.numel() == GUARD * widths[name]
        if name == "payload_off":
            assert bool((tail == -7).all()), name
        else:
            assert bool((tail.view(torch.uint8) == 0xA5).all()), name
    return {name: t[:used[name]] for name, t in arrs.items()}


def test_malformed_and_hostile_lines(torch, eng):
    buf = C.hostile_corpus()
    want = R.parse_log(buf)
    lines = R.split_lines(buf)
    t = _text(torch, buf)
    line_off, n = eng.text_index(t)
    assert n == len(want)
    total = sum(len(w["data"]) for w in want if w["status"] == R.OK)
    p = _parse_guarded(torch, eng, t, line_off, n, total)
    assert int(p["payload_off"][n].item()) == total
    got = _rows(p, n)
    for i in range(n):
        assert got[i]["event"] == want[i]["event"], (i, lines[i][:200])
        w = dict(want[i])
        del w["kind"]
        if w["status"] != R.OK:
            w.pop("data")
        _check(got[i], w, i, lines[i])
    ok = sum(w["status"] == R.OK for w in want)
    assert ok > 100 and n - ok > 500
    assert max(len(w["data"]) for w in want) == 8192 and max(map(len, lines)) > 65536
    # the payload pass with a capacity that is too small writes the offsets only
    q = _parse_guarded(torch, eng, t, line_off, n, total - 1)
    assert int(q["payload_off"][n].item()) == total
    assert bool((q["payload"] == 0xA5).all())


# ------------------------------------------------------------------ 6. the manual's lines
def test_doc_lines_on_the_gpu(torch, eng):
    from mgen_amd import PARSE_NO_DAYS
    buf = C.doc_lines()
    t = _text(torch, buf)
    line_off, n = eng.text_index(t)
    assert n == 5
    p = eng.log_parse_text(t, line_off, n, opts=PARSE_NO_DAYS, payload=True)
    got = _rows(p, n)
    for i, (g, w) in enumerate(zip(got, C.DOC_EXPECT)):
        assert g["status"] == R.OK
        diff = {k: (g[k], w[k]) for k in w if g[k] != w[k]}
        assert not diff, (i, diff)
    assert [g["msg_len"] for g in got] == [1024, 1024, 65535, 1024, 65535]
    assert [g["err"] for g in got] == [0, 0, 0, 0, R.ERROR_NOT_RECV]
    assert got[0]["alt"] == got[2]["alt"] == -999 and got[0]["lat_raw"] == 70740000
