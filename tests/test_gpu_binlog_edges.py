"""The edges of binary log ingest on the GPU (mgenx_binlog_parse): the crafted records of
binlog_cases -- fields on both sides of the 128 staged bytes, record lengths around the 16-byte
staging chunks, cut and rejected messages -- at every start alignment, a "record" at every byte
offset of a log, buffers that end inside a record, batch sizes around the workgroup's 256
records and every optional output pointer alone.  Every comparison is against
binlog_parse_ref.parse_record over the bytes the contract says a record owns,
buf[at : min(at + 4 + recordLength, buf_bytes)]: every column and the payload bytes of an OK
record, status and event of a MALFORMED one.  Each case runs once."""
import ctypes

import numpy as np
import pytest

import binlog_cases as C
import binlog_parse_ref as M
import logparse_ref as R
from test_gpu_binlog_parse import GUARD, _expect
from test_gpu_logparse import _rows

pytestmark = pytest.mark.gpu
SLACK = 2048


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


def _dev(torch, data, slack=0, fill=0):
    a = np.full(len(data) + slack, fill, np.uint8)
    a[:len(data)] = np.frombuffer(bytes(data), np.uint8)
    return torch.from_numpy(a).cuda()


def _offsets(torch, offs):
    """Offsets as the int64 bit patterns of the API's uint64."""
    return torch.from_numpy(np.array(offs, np.uint64).view(np.int64).copy()).cuda()


def _want(buf, at, nbytes=None):
    w = M.parse_record(C.owned(buf, at, nbytes))
    del w["kind"]
    return w


def _compare(p, n, wants):
    """The parsed columns against the model's dicts; the payload offsets against the model's
    cumulative data lengths (a MALFORMED record has no data)."""
    lens = [len(w["data"]) if w["status"] == R.OK else 0 for w in wants]
    off = p["payload_off"].cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
    assert p["payload"].numel() == sum(lens)
    got = _rows(p, n)
    for k in range(n):
        _expect(got[k], wants[k], k)
    return got


@pytest.fixture(scope="module")
def crafted():
    """(names, records, the model's answers)."""
    names, recs = zip(*C.crafted())
    wants = []
    for rec in recs:
        w = M.parse_record(rec)
        del w["kind"]
        wants.append(w)
    return names, recs, wants


@pytest.fixture(scope="module")
def edge(torch):
    """The every-offset log: (bytes, true record offsets, every offset 0 .. nbytes and the
    offsets outside the buffer, the model's answer for each)."""
    buf, offs, _ = C.edge_log()
    n = len(buf)
    every = list(range(n + 1)) + [n + 1, 2 ** 40, 2 ** 63, 2 ** 64 - 1]
    every += [offs[3], offs[3], 0, n, 2 ** 64 - 1] + list(range(offs[9], offs[7], -1))
    blank = R.blank()
    del blank["kind"]
    wants = [_want(buf, at) if at < n else dict(blank) for at in every]
    return buf, offs, every, wants


def test_crafted_corpus_shuffled(torch, eng, crafted):
    names, recs, wants = crafted
    order = np.random.default_rng(41).permutation(len(recs))
    buf, offs = C.pack([recs[i] for i in order])
    p = eng.binlog_parse(_dev(torch, buf), _offsets(torch, offs), len(offs), payload=True)
    got = _compare(p, len(offs), [wants[i] for i in order])
    ok = [g for g in got if g["status"] == R.OK]
    assert len(ok) > 300 and any(len(g["data"]) == 1028 - C.RECV_FULL for g in ok)
    assert any(w["status"] == R.OK and w["present"] & R.HAS_DATA and "byte128" in name
               for name, w in zip(names, wants))


def test_every_start_alignment(torch, eng, crafted):
    """Sixteen copies of every record in one buffer with 0 .. 15 bytes of 0xEE before each, so
    that each record starts at all sixteen alignments of the 16-byte loads; explicit offsets.
    The answers are those of the packed records."""
    names, recs, wants = crafted
    buf, offs, which = bytearray(), [], []
    for c in range(16):
        for k, rec in enumerate(recs):
            buf += b"\xEE" * ((k + c - len(buf)) % 16)
            offs.append(len(buf))
            which.append(k)
            buf += rec
    seen = {k: set() for k in range(len(recs))}
    for k, at in zip(which, offs):
        seen[k].add(at % 16)
    assert all(s == set(range(16)) for s in seen.values())
    p = eng.binlog_parse(_dev(torch, buf), _offsets(torch, offs), len(offs), payload=True)
    _compare(p, len(offs), [wants[k] for k in which])


def test_a_record_at_every_byte_offset(torch, eng, edge):
    """rec_off = 0, 1, ..., nbytes, then offsets outside the buffer, duplicates and a
    descending stretch: the header-outside-the-buffer branches, the clip to the buffer's end,
    thousands of garbage headers and overlapping records in one call."""
    buf, offs, every, wants = edge
    n = len(every)
    p = eng.binlog_parse(_dev(torch, buf), _offsets(torch, every), n, payload=True)
    got = _compare(p, n, wants)
    nb = len(buf)
    for k in range(nb - 3, n):
        if every[k] > nb - 4:             # fewer than 4 bytes left, or outside: blank
            assert (got[k]["event"], got[k]["status"]) == (0, R.MALFORMED), k
    ok = sum(w["status"] == R.OK for w in wants)
    true_ok = sum(wants[at]["status"] == R.OK for at in set(offs))
    assert ok > true_ok > 100            # garbage forms some records too


def _same_columns(torch, a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_nothing_past_buf_bytes_is_read(torch, eng, edge):
    """The log at the front of a tensor 2 KiB longer, nbytes = the log's length: the answers
    with the slack zeroed and with the slack 0xFF are the same, and the model's."""
    buf, offs, every, wants = edge
    n = len(every)
    ro = _offsets(torch, every)
    zero = eng.binlog_parse(_dev(torch, buf, SLACK, 0x00), ro, n, payload=True, nbytes=len(buf))
    ones = eng.binlog_parse(_dev(torch, buf, SLACK, 0xFF), ro, n, payload=True, nbytes=len(buf))
    _same_columns(torch, zero, ones)
    _compare(ones, n, wants)


@pytest.mark.parametrize("beyond", ["the record's own bytes", "0xFF"])
def test_buffer_ends_inside_a_record(torch, eng, edge, beyond):
    """nbytes cut back by 1 .. 160 bytes: the log ends with a 1028-byte record, a 129-byte RECV
    and a START, so a whole short record, every cut of the RECV and the long record's tail go.
    A cut record is MALFORMED with its event kept while 4 bytes of it remain; what lies beyond
    nbytes -- the record's true bytes, or 0xFF -- changes nothing."""
    buf, offs, _, _ = edge
    tail = offs[-6:]
    assert [len(buf) - at for at in tail[-3:]] == [12 + 129 + 1028, 12 + 129, 12]
    ro = _offsets(torch, tail)
    base = _dev(torch, buf, SLACK, 0xFF)
    cut_kept = blank = 0
    for k in range(1, 161):
        nb = len(buf) - k
        dev = base
        if beyond == "0xFF":
            dev = base.clone()
            dev[nb:] = 0xFF
        p = eng.binlog_parse(dev, ro, len(tail), payload=True, nbytes=nb)
        wants = [_want(buf, at, nb) for at in tail]
        got = _compare(p, len(tail), wants)
        for at, g in zip(tail, got):
            whole = at + len(C.owned(buf, at)) <= nb
            assert (g["status"] == R.OK) == whole, (k, at)
            if not whole and nb - at >= 4:
                assert g["event"] == buf[at], (k, at)
                cut_kept += 1
            elif not whole:
                assert g["event"] == 0, (k, at)
                blank += 1
    assert cut_kept > 140 and blank > 150


def _guarded_arrays(torch, n, total):
    from mgen_amd import LOGPARSE_COLS
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    arrs = {}
    for name, dt, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT:
        t = torch.empty((n + GUARD) * w, dtype=getattr(torch, dt), device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        arrs[name] = t
    arrs["payload_off64"] = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    arrs["payload"] = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return arrs


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513])
def test_batch_sizes_with_guard_words(torch, eng, crafted, n):
    """Batch sizes around one and two workgroups of 256 records: every output array and the
    payload are written up to their n-th element and not a byte further."""
    from mgen_amd import LOGPARSE_COLS, LogparseOut, _ptr, _stream
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    _, recs, wants = crafted
    pick = [(7 * k) % len(recs) for k in range(n)]      # 7 and the corpus size are coprime
    buf, offs = C.pack([recs[i] for i in pick])
    want = [wants[i] for i in pick]
    total = sum(len(w["data"]) for w in want if w["status"] == R.OK)
    arrs = _guarded_arrays(torch, n, total)
    s = LogparseOut()
    for name, _, _ in LOGPARSE_COLS:
        setattr(s, name, arrs[name].data_ptr())
    s.cols = eng._cols_struct({k: arrs[k] for k, _, _ in COLS_CORE + COLS_EXT})
    s.payload, s.payload_cap = arrs["payload"].data_ptr(), total
    s.payload_off = arrs["payload_off64"].data_ptr()
    dbuf, ro = _dev(torch, buf), _offsets(torch, offs)
    rc = eng.lib.mgenx_binlog_parse(eng.ctx, _ptr(dbuf), dbuf.numel(), _ptr(ro), n, 0,
                                    ctypes.byref(s), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    widths = {name: w for name, _, w in LOGPARSE_COLS + COLS_CORE + COLS_EXT}

    def untouched(x):
        return bool((x.view(torch.uint8) == 0xA5).all())
    p = {}
    for name, t in arrs.items():
        if name == "payload_off64":
            assert t[n + 1:].numel() == GUARD and bool((t[n + 1:] == -7).all())
            p[name] = t[:n + 1]
            continue
        used = total if name == "payload" else n * widths[name]
        assert t[used:].numel() == GUARD * widths.get(name, 1) and untouched(t[used:]), name
        p[name] = t[:used]
    # members the parser ignores stay as they were
    assert untouched(p.pop("hdr_len")) and untouched(p.pop("payload_off"))
    p["payload_off"] = p.pop("payload_off64")
    got = _compare(p, n, want)
    assert got[0]["event"] == recs[pick[0]][0] and got[n - 1]["event"] == recs[pick[-1]][0]


@pytest.fixture(scope="module")
def full_run(torch, eng, crafted):
    _, recs, wants = crafted
    buf, offs = C.pack(recs)
    dbuf, ro = _dev(torch, buf), _offsets(torch, offs)
    p = eng.binlog_parse(dbuf, ro, len(offs), payload=True)
    _compare(p, len(offs), wants)
    return dbuf, ro, len(offs), p


def _call(torch, eng, dbuf, ro, n, **ptrs):
    from mgen_amd import LogparseOut, _ptr, _stream
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    s = LogparseOut()
    cols = {}
    for name, t in ptrs.items():
        if name == "payload_cap":
            s.payload_cap = t
        elif name.startswith("cols_"):
            cols[name[5:]] = t
        else:
            setattr(s, name, t.data_ptr())
    assert set(cols) <= {k for k, _, _ in COLS_CORE + COLS_EXT}
    s.cols = eng._cols_struct(cols)
    rc = eng.lib.mgenx_binlog_parse(eng.ctx, _ptr(dbuf), dbuf.numel(), _ptr(ro), n, 0,
                                    ctypes.byref(s), _stream(0))
    assert rc == 0
    torch.cuda.synchronize()


def test_optional_pointers(torch, eng, full_run):
    """Every pointer but event and status is optional: each given alone gets the full run's
    values; an array bound to no pointer, and a member the parser ignores, stay untouched."""
    from mgen_amd import LOGPARSE_COLS
    from mgen_amd._abi import COLS_CORE, COLS_EXT
    dbuf, ro, n, full = full_run
    sentinel = torch.full((n * 20 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")

    def fresh(dt="uint8", w=1):
        t = torch.empty(n * w + GUARD, dtype=getattr(torch, dt), device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        return t

    def untouched(t):
        return bool((t.view(torch.uint8) == 0xA5).all())
    ev, st = fresh(), fresh()
    _call(torch, eng, dbuf, ro, n, event=ev, status=st)
    assert torch.equal(ev[:n], full["event"]) and torch.equal(st[:n], full["status"])
    assert untouched(ev[n:]) and untouched(st[n:])
    members = [(name, name, dt, w) for name, dt, w in LOGPARSE_COLS[2:]]
    members += [("cols_" + name, name, dt, w) for name, dt, w in COLS_CORE + COLS_EXT]
    assert len(members) == 7 + 14 + 10
    for arg, name, dt, w in members:
        one, ev, st = fresh(dt, w), fresh(), fresh()
        _call(torch, eng, dbuf, ro, n, event=ev, status=st, **{arg: one})
        assert torch.equal(ev[:n], full["event"]) and torch.equal(st[:n], full["status"]), arg
        assert untouched(one[n * w:]), arg
        if arg in ("cols_hdr_len", "cols_payload_off"):
            assert untouched(one), arg                   # ignored members
        else:
            assert torch.equal(one[:n * w], full[name]), arg
    # payload_off without payload; payload with room for all, one byte short, none
    total = full["payload"].numel()
    assert total > 1000
    for cap in (None, total, total - 1, 0):
        ev, st = fresh(), fresh()
        off = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
        args = dict(event=ev, status=st, payload_off=off)
        pay = None
        if cap is not None:
            pay = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            args.update(payload=pay, payload_cap=cap)
        _call(torch, eng, dbuf, ro, n, **args)
        assert torch.equal(off[:n + 1], full["payload_off"]) and bool((off[n + 1:] == -7).all())
        if cap == total:
            assert torch.equal(pay[:total], full["payload"]) and untouched(pay[total:])
        elif cap is not None:
            assert untouched(pay), cap
    assert bool((sentinel == 0x5A).all())
