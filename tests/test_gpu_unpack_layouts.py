"""Crafted header layouts through every unpack kernel family, field for field against the
oracle (which test_wire_model_cpu.py holds to a second, plain-Python statement of
MgenMsg::Unpack on the same records).

A record that a sender packed has dstAddrLen 4 or 16 and hostAddrLen 0, 4 or 16, so the
register-only decode (fast_layout) takes nearly every record of the other corpora.  Unpack
(mgenMsg.cpp:315-500) bounds neither length, accepts any host type, stops at six places and
floors the payload pointer to a word; the kernels decode all that on a second path
(parse_header), chosen and handed over to separately in the general / header-only, the var,
the long and the two fixed-length kernels.  wire_cases.py drives that path on purpose: every
(dst, host) length pair of a 17 x 12 lattice with invalid host types, gpsStatus >= 3 and
payload lengths that fit exactly or miss by one, a truncation ladder over every received
length, and the lattice interleaved with ordinary records for the kernels that parse in quad
lane 0 and broadcast.  Every case asserts which kernel the dispatch launched."""
import os
import re
import socket

import numpy as np
import pytest

import wire_cases as C
from test_gpu_parity import COLMAP, compare_cols, host_cols, rows_to_cols

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ("udp", "udp_force", "tcp_force")


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


def _opts(rule):
    from mgen_amd import OPT_CHECKSUM_FORCE, OPT_TCP
    return {"udp": 0, "udp_force": OPT_CHECKSUM_FORCE, "tcp_force": OPT_TCP | OPT_CHECKSUM_FORCE}[rule]


def _want(oracle, slab, n, rule, **where):
    return oracle.udp_recv_batch(slab, n, force=rule != "udp", tcp=rule == "tcp_force", **where)


def check_core(c, f, n, what):
    """the 13 core columns and dst_addr4 of n records == the oracle's fields"""
    for gname, oname, dt in COLMAP[:13]:
        got = np.asarray(c[gname]).view(dt)[:n]
        want = f[oname][:n].astype(dt)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, gname, bad.size, bad[:8], got[bad[:4]], want[bad[:4]])
    got4 = np.asarray(c["dst_addr4"]).view(np.uint8).reshape(-1, 4)[:n]
    bad = np.nonzero((got4 != f["dst_addr"][:n, :4]).any(axis=1))[0]
    assert bad.size == 0, (what, "dst_addr4", bad[:8])


class Batch:
    """records placed by rec_off / rec_len, on the host and on the device"""

    def __init__(self, torch, records):
        from mgen_amd import to_device
        self.records = list(records)
        self.n = len(self.records)
        self.slab, self.offs, self.lens = C.place(self.records, "offsets")
        self.d_slab = to_device(self.slab).view(torch.uint8)
        self.d_offs = to_device(self.offs).view(torch.int64)
        self.d_lens = to_device(self.lens).view(torch.int32)
        self.where = dict(rec_off=self.d_offs, rec_len=self.d_lens)
        self._want = {}

    def want(self, oracle, rule):
        if rule not in self._want:
            self._want[rule] = _want(oracle, self.slab, self.n, rule, rec_off=self.offs,
                                     rec_len=self.lens)
        return self._want[rule]


@pytest.fixture(scope="module")
def general(torch):
    """the lattices of 65, 128, 301 and 512 bytes, the ladder and the plain errors: ~1,300
    records at unaligned offsets"""
    return Batch(torch, C.general_batch())


def _cols_then_rows(torch, eng, b, f, opts, kernel, what):
    cols = eng.unpack(b.d_slab, b.n, opts=opts, ext=True, **b.where)
    assert eng.last_unpack_kernel() == kernel
    torch.cuda.synchronize()
    compare_cols(cols, f, b.n, (what, "cols"))
    core = eng.unpack(b.d_slab, b.n, opts=opts, **b.where)      # core columns alone
    assert eng.last_unpack_kernel() == kernel
    check_core(host_cols(core, b.n), f, b.n, (what, "core cols"))
    rows = eng.alloc_rows(b.n)
    eng.unpack(b.d_slab, b.n, opts=opts, cols={"rows": rows}, **b.where)
    assert eng.last_unpack_kernel() == kernel
    torch.cuda.synchronize()
    check_core(rows_to_cols(rows, b.n), f, b.n, (what, "rows"))
    return cols


@pytest.mark.parametrize("rule", RULES)
def test_general_kernel(torch, eng, oracle, general, rule):
    from mgen_amd import UNPACK_K_GENERAL
    _cols_then_rows(torch, eng, general, general.want(oracle, rule), _opts(rule),
                    UNPACK_K_GENERAL, ("general", rule))


def test_header_only_kernel(torch, eng, oracle, general):
    """OPT_SKIP_CRC is Unpack alone: the UDP rule's fields without its checksum verdict"""
    from mgen_amd import OPT_SKIP_CRC, UNPACK_K_HEADER
    f = general.want(oracle, "udp").copy()
    assert int((f["err"] == 2).sum()) > 100
    f["err"][f["err"] == 2] = 0
    _cols_then_rows(torch, eng, general, f, OPT_SKIP_CRC, UNPACK_K_HEADER, "header")


# ---------------------------------------------------------------- fixed-length kernels
@pytest.fixture(scope="module")
def interleaved(torch, oracle, gold):
    """{L: (records [n, L], device slab)}: the lattice among ordinary packed records"""
    from mgen_amd import to_device
    cache = {}

    def get(L):
        if L not in cache:
            n, _ = C.interleaved_index()
            recs = C.interleaved(L, C.fillers(oracle, gold, n, L))
            slab, stride = C.place([r.tobytes() for r in recs], "stride")
            assert stride == L
            cache[L] = (slab, n, to_device(slab).view(torch.uint8), {})
        return cache[L]
    return get


def _fixed_want(oracle, entry, L, rule):
    slab, n, _, want = entry
    if rule not in want:
        want[rule] = _want(oracle, slab, n, rule, stride=L, fixed_len=L)
    return want[rule]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("L,out", [(65, "cols"), (301, "cols"), (1024, "cols"), (301, "rows")])
def test_fixed_pipelined_kernel(torch, eng, oracle, interleaved, L, out, rule):
    """quad lane 0 parses a general layout and broadcasts it over the fast decode's registers:
    general layouts at every position of a 16-record group beside fast neighbours, a whole
    group of them, a whole group without, and a partial last group"""
    from mgen_amd import UNPACK_K_FIXED
    entry = interleaved(L)
    _, n, d_slab, _ = entry
    f = _fixed_want(oracle, entry, L, rule)
    if out == "rows":
        rows = eng.alloc_rows(n)
        eng.unpack(d_slab, n, stride=L, fixed_len=L, opts=_opts(rule), cols={"rows": rows})
        assert eng.last_unpack_kernel() == UNPACK_K_FIXED
        torch.cuda.synchronize()
        c = rows_to_cols(rows, n)
    else:
        cols = eng.unpack(d_slab, n, stride=L, fixed_len=L, opts=_opts(rule))
        assert eng.last_unpack_kernel() == UNPACK_K_FIXED
        c = host_cols(cols, n)
    check_core(c, f, n, ("fixed", L, out, rule))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("L", [512, 1024])
def test_fixed_ring_kernel(torch, eng, oracle, interleaved, L, rule):
    from mgen_amd import UNPACK_K_FIXED_RING
    entry = interleaved(L)
    _, n, d_slab, _ = entry
    rows = eng.alloc_rows(n)
    eng.unpack(d_slab, n, stride=L, fixed_len=L, opts=_opts(rule), cols={"rows": rows})
    assert eng.last_unpack_kernel() == UNPACK_K_FIXED_RING
    torch.cuda.synchronize()
    check_core(rows_to_cols(rows, n), _fixed_want(oracle, entry, L, rule), n, ("ring", L, rule))


# ---------------------------------------------------------------- var kernel
VAR_SLAB_LIMIT = 150 << 20


@pytest.fixture(scope="module")
def var_batch(torch, oracle):
    """The GENERAL batch repeated to the smallest n that gives every wave two 64-record
    tiles (one 16-wave block per CU: 524,288 records on 256 CUs).  The unique batch has an
    odd record count, so a record's place in a tile moves from one repeat to the next; the
    expected fields are computed once on the unique batch and tiled."""
    from mgen_amd import to_device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 16 * 64
    recs = list(C.general_batch())
    if len(recs) % 2 == 0:
        recs.append(C.ladder()[0][-1])
    slab, offs, lens = C.place(recs, "offsets")
    reps = -(-n // len(recs))
    if reps * len(slab) > VAR_SLAB_LIMIT:       # lattices up to 128 bytes and the ladder
        recs = list(C.general_batch((65, 128)))
        if len(recs) % 2 == 0:
            recs.append(C.ladder()[0][-1])
        slab, offs, lens = C.place(recs, "offsets")
        reps = -(-n // len(recs))
    assert reps * len(slab) <= VAR_SLAB_LIMIT and len(recs) % 2 == 1
    big = np.tile(slab, reps)
    base = (np.arange(reps, dtype=np.uint64) * np.uint64(len(slab)))[:, None]
    all_offs = (base + offs[None, :]).reshape(-1)[:n]
    all_lens = np.tile(lens, reps)[:n]
    want = {rule: np.tile(_want(oracle, slab, len(recs), rule, rec_off=offs, rec_len=lens),
                          reps)[:n] for rule in ("udp", "tcp_force")}
    return dict(n=n, slab=to_device(big).view(torch.uint8),
                offs=to_device(all_offs).view(torch.int64),
                lens=to_device(all_lens).view(torch.int32), want=want)


@pytest.mark.parametrize("rule", ["udp", "tcp_force"])
def test_var_kernel(torch, eng, var_batch, rule):
    from mgen_amd import UNPACK_K_VAR
    v, n = var_batch, var_batch["n"]
    f = v["want"][rule]
    rows = eng.alloc_rows(n)
    eng.unpack(v["slab"], n, rec_off=v["offs"], rec_len=v["lens"], opts=_opts(rule),
               cols={"rows": rows})
    assert eng.last_unpack_kernel() == UNPACK_K_VAR
    torch.cuda.synchronize()
    check_core(rows_to_cols(rows, n), f, n, ("var", rule, "rows"))
    del rows
    cols = eng.unpack(v["slab"], n, rec_off=v["offs"], rec_len=v["lens"], opts=_opts(rule),
                      ext=True)
    assert eng.last_unpack_kernel() == UNPACK_K_VAR
    torch.cuda.synchronize()
    compare_cols(cols, f, n, ("var", rule, "cols"))


# ---------------------------------------------------------------- long kernel
@pytest.mark.parametrize("rule", RULES)
def test_long_kernel_rec_len(torch, eng, oracle, rule):
    """lattice(4099) and the 8,200-byte record whose payload fits the received bytes but not
    the 8,192 a TCP receiver unpacks, by rec_off / rec_len"""
    from mgen_amd import UNPACK_K_LONG
    b = Batch(torch, C.lattice(4099) + (C.long_extra(),))
    f = b.want(oracle, rule)
    assert f["hdr_len"][-1] == 48 and f["err"][-1] == 0
    assert f["payload_len"][-1] == (0 if rule == "tcp_force" else 8152)
    cols = _cols_then_rows(torch, eng, b, f, _opts(rule), UNPACK_K_LONG, ("long", rule))
    assert int(cols["payload_off"][-1].item()) == (0 if rule == "tcp_force" else 48)


@pytest.mark.parametrize("rule", RULES)
def test_long_kernel_fixed_stride(torch, eng, oracle, rule):
    from mgen_amd import UNPACK_K_LONG, to_device
    L = 4099
    slab, stride = C.place(list(C.lattice(L)), "stride")
    n = C.LATTICE_N
    d_slab = to_device(slab).view(torch.uint8)
    f = _want(oracle, slab, n, rule, stride=L, fixed_len=L)
    cols = eng.unpack(d_slab, n, stride=L, fixed_len=L, opts=_opts(rule), ext=True)
    assert eng.last_unpack_kernel() == UNPACK_K_LONG
    torch.cuda.synchronize()
    compare_cols(cols, f, n, ("long stride", rule, "cols"))
    rows = eng.alloc_rows(n)
    eng.unpack(d_slab, n, stride=L, fixed_len=L, opts=_opts(rule), cols={"rows": rows})
    assert eng.last_unpack_kernel() == UNPACK_K_LONG
    torch.cuda.synchronize()
    check_core(rows_to_cols(rows, n), f, n, ("long stride", rule, "rows"))


# ---------------------------------------------------------------- downstream of the decode
def _log_inputs(oracle, n):
    """sources (every IPv6 zero-group pattern and the special forms first, IPv4 and random
    IPv6 after), receive times and TTLs of n records"""
    rng = np.random.default_rng(0x106)
    v6 = C.ipv6_sources()
    src = np.zeros(n, oracle.ADDR_DTYPE)
    six = rng.random(n) < 0.3
    six[:len(v6)] = True
    src["type"] = np.where(six, 2, 1)
    src["len"] = np.where(six, 16, 4)
    src["port"] = rng.integers(0, 65536, n)
    src["addr"] = rng.integers(0, 256, (n, 16))
    src["addr"][:len(v6)] = np.frombuffer(b"".join(v6), np.uint8).reshape(-1, 16)
    src["addr"][~six, 4:] = 0
    rx_sec = rng.integers(1_600_000_000, 1_800_000_000, n, dtype=np.int64).astype(np.uint32)
    rx_usec = rng.integers(0, 1_000_000, n).astype(np.uint32)
    ttl = rng.integers(-1, 256, n).astype(np.int32)
    return src, rx_sec, rx_usec, ttl


def test_log_lines_of_crafted_layouts(torch, eng, oracle, general):
    """The text and binary RECV / RERR logs of the GENERAL batch's decode: the data> hex
    comes from the floored payload offset, an address whose length does not match its type
    prints (invalid), and the src> token of every IPv6 source equals inet_ntop's."""
    from mgen_amd import UNPACK_K_GENERAL, to_device
    b, n = general, general.n
    f = b.want(oracle, "udp")
    assert np.any((f["payload_len"] != 0) & (f["payload_off"] != f["hdr_len"]) &
                  (f["payload_type"] == 0) & (f["err"] == 0) & (f["gps_status"] < 3))
    assert np.any((f["err"] == 0) & (f["dst_len"] != 4) & (f["dst_len"] != 16))
    cols = eng.unpack(b.d_slab, n, ext=True, **b.where)
    assert eng.last_unpack_kernel() == UNPACK_K_GENERAL
    src, rx_sec, rx_usec, ttl = _log_inputs(oracle, n)
    d_src = to_device(src.view(np.uint8))
    text, line_off = eng.log_recv_text(b.d_slab, n, cols, d_src, to_device(rx_sec),
                                       to_device(rx_usec), rec_off=b.d_offs, ttl=to_device(ttl))
    got = text.cpu().numpy().tobytes()
    want = oracle.log_recv_text(f, b.slab, b.offs, src, rx_sec, rx_usec, ttl=ttl)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]][:3]
        raise AssertionError([(i, g[i], w[i]) for i in bad] or (len(got), len(want)))
    lines = got.decode().splitlines()
    assert len(lines) == n and int(line_off[n].item()) == len(want)
    assert sum("(invalid)" in ln for ln in lines) > 100
    assert sum(" data>" in ln for ln in lines) > 30
    checked = 0
    for i in np.nonzero(src["type"] == 2)[0]:
        m = re.search(r" src>(\S+)/(\d+)", lines[i])
        assert m, lines[i]
        assert m.group(1) == socket.inet_ntop(socket.AF_INET6, src["addr"][i].tobytes()), i
        assert int(m.group(2)) == src["port"][i]
        checked += 1
    assert checked >= len(C.ipv6_sources())
    out, pos = eng.log_recv_binary(b.d_slab, n, cols, d_src, to_device(rx_sec),
                                   to_device(rx_usec), rec_off=b.d_offs, rec_len=b.d_lens)
    got = out.cpu().numpy().tobytes()
    want = oracle.log_recv_binary(f, b.slab, b.offs, src, rx_sec, rx_usec, rec_len=b.lens)
    if got != want:
        p = pos.cpu().numpy()
        bad = [i for i in range(n) if got[p[i]:p[i + 1]] != want[p[i]:p[i + 1]]][:3]
        raise AssertionError((len(got), len(want), bad))


# ---------------------------------------------------------------- the doc's sizes, no oracle
def test_doc_sizes_on_the_gpu_alone(torch, eng):
    """doc/mgen.xml:4734-4737, 4743-4745, 4834-4844 on eng.pack -> eng.unpack: nothing is
    packed below 28 (IPv4 dst) / 40 (IPv6 dst) bytes; 28 / 40 decode with that header length;
    with a host address and GPS, 52 / 76 is the first size whose header is complete, one
    byte fewer loses payload_len, four fewer the GPS block, a cut host address the host."""
    from mgen_amd import to_device
    from mgen_amd._abi import DESC_DTYPE, TMPL_DTYPE
    t = np.zeros(4, TMPL_DTYPE)
    t["flow_id"] = [1, 2, 3, 4]
    t["dst_type"], t["dst_len"], t["dst_port"] = [1, 1, 2, 2], [4, 4, 16, 16], 5000
    t["dst_addr"] = np.arange(1, 17, dtype=np.uint8)
    t["host_type"], t["host_len"], t["host_port"] = [0, 1, 0, 2], [0, 4, 0, 16], [0, 4000, 0, 4001]
    t["host_addr"] = np.arange(33, 49, dtype=np.uint8)
    t["host_addr"][[0, 2]] = 0
    t["host_addr"][1, 4:] = 0
    t["dst_addr"][:2, 4:] = 0
    lat = (10 + 180) * 60000
    t["lat_raw"], t["lon_raw"], t["alt"], t["gps_status"], t["payload_type"] = lat, lat, 7, 2, 1
    cases = [(0, 27), (0, 28), (1, 52), (1, 51), (1, 48), (1, 35),
             (2, 39), (2, 40), (3, 76), (3, 75), (3, 72), (3, 59)]
    n = len(cases)
    d = np.zeros(n, DESC_DTYPE)
    d["tmpl"] = [c[0] for c in cases]
    d["msg_len"] = [c[1] for c in cases]
    d["seq_num"] = np.arange(n)
    pool = np.zeros(16, np.uint8)
    dt, dp, dd = to_device(t), to_device(pool), to_device(d)
    crc = torch.empty(len(t), dtype=torch.int32, device="cuda")
    eng.pack_prepare(dt, len(t), dp, crc)
    stride = 128
    slab = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    out_len = eng.pack(dt, crc, dd, n, dp, slab, stride=stride).cpu().numpy().view(np.uint32)
    assert out_len.tolist() == [0 if s in (27, 39) else s for _, s in cases]
    offs = to_device((np.arange(n) * stride).astype(np.uint64)).view(torch.int64)
    lens = to_device(np.array([s for _, s in cases], np.uint32)).view(torch.int32)
    c = host_cols(eng.unpack(slab, n, rec_off=offs, rec_len=lens, ext=True), n)
    col = lambda name, dtype: c[name].view(dtype)[:n]
    err, hdr = col("err", np.uint8), col("hdr_len", np.uint16)
    dlen, hlen, htype = col("dst_len", np.uint8), col("host_len", np.uint8), col("host_type", np.uint8)
    gps, ptype, lat_raw = col("gps_status", np.uint8), col("payload_type", np.uint8), col("lat_raw", np.uint32)
    by = {case: i for i, case in enumerate(cases)}
    assert err[by[0, 27]] == 3                                   # ERROR_LENGTH
    for tm, size, a in ((0, 28, 4), (2, 40, 16)):
        i = by[tm, size]
        assert (err[i], hdr[i], dlen[i], htype[i], gps[i]) == (0, size, a, 0, 0)
    for tm, full, a in ((1, 52, 4), (3, 76, 16)):
        i = by[tm, full]
        assert (err[i], hdr[i], dlen[i], hlen[i], gps[i], ptype[i]) == (0, full, a, a, 2, 1)
        assert lat_raw[i] == lat
        i = by[tm, full - 1]                                     # payload_len lost
        assert (err[i], hdr[i], hlen[i], gps[i], ptype[i], lat_raw[i]) == (0, 0, a, 2, 1, lat)
        i = by[tm, full - 4]                                     # GPS lost
        assert (err[i], hdr[i], hlen[i], htype[i], gps[i]) == (0, 28 + 2 * a, a, 1 if a == 4 else 2, 0)
        assert lat_raw[i] == 10800000
        i = by[tm, 28 + 2 * a - 1]                               # host lost
        assert (err[i], hlen[i], htype[i], dlen[i]) == (0, 0, 0, a)
