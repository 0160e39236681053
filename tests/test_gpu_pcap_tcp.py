"""GPU tests of MGEN-over-TCP in pcap2mgen (mgenx_pcap_tcp / mgenx_pcapng_tcp, mgenx_tcp_frame
and the `tcp` option of every layer above them).

Expected values never come from the code under test: whole logs come from the oracle (its
pcap2mgen lines for the UDP packets, its proto>TCP lines over its TCP receive of each original
stream), per-packet arrays, stream tables, scratch bytes, pieces and counts from the serial
model of the contract in tests/pcap_tcp_util.py (itself pinned by tests/test_pcap_tcp_cpu.py),
records from the oracle's TCP framing over the model's streams.  What the contract leaves
untouched is compared with the parse's own output before the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pcap_frag_util as F
import pcap_tcp_util as T
import pcap_util as P
import pcapng_util as G

pytestmark = pytest.mark.gpu
GUARD = 256
U64_MAX = 2**64 - 1
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                   "pcap2mgen")


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


def _diff(got: bytes, want: bytes):
    gl, wl = got.split(b"\n"), want.split(b"\n")
    for k, (a, b) in enumerate(zip(gl, wl)):
        if a != b:
            return f"line {k}:\n got  {a!r}\n want {b!r}"
    return f"line counts {len(gl)} vs {len(wl)}"


def _host(p):
    import mgen_amd
    o = {k: v.cpu().numpy().copy() for k, v in p.items()}
    o["src"] = o["src"].view(mgen_amd.ADDR_DTYPE)
    return o


class Run:
    """Parse + pcap_tcp of one capture: the sizing call on an empty window with no stream
    table, then the exact window and table (`short` bytes / `cap_short` rows less), with guard
    regions behind the window, the table and the pieces."""

    def __init__(self, eng, torch, file, link=1, ng=False, short=0, cap_short=0):
        import mgen_amd
        self.eng, self.torch = eng, torch
        self.soff = soff = (len(file) + 15) & ~15
        img = np.zeros(soff, np.uint8)
        img[:len(file)] = np.frombuffer(file, np.uint8)
        if ng:
            offs, pif, ifaces, info = mgen_amd.pcapng_index(file)
        else:
            offs, info = mgen_amd.pcap_index(file)
        self.n = n = len(offs)
        assert info.link_type == link
        po = torch.from_numpy(offs.view(np.int64).copy()).cuda()

        def parse(buf):
            if not ng:
                return eng.pcap_parse(buf, po, n, link, info.flags)
            return eng.pcapng_parse(buf, po, torch.from_numpy(pif.view(np.int32).copy()).cuda(),
                                    n, torch.from_numpy(ifaces.view(np.uint8).copy()).cuda(),
                                    len(ifaces), link, info.flags)
        small = torch.from_numpy(img).cuda()
        p = parse(small)
        self.base = _host(p)
        self.fits0, st, _, _, _ = eng.pcap_tcp(small, soff, po, n, link, info.flags, p,
                                               stream_cap=0)
        self.stats0 = st.as_dict()
        self.after0 = _host(p)
        need, ns = self.stats0["scratch_bytes"], self.stats0["n_streams"]
        self.big = big = torch.full((soff + need + GUARD,), 0xA5, dtype=torch.uint8,
                                    device="cuda")
        big[:soff] = small
        self.p = p = parse(big[:soff])
        table = torch.full(((ns + 1) * 80,), 0xA5, dtype=torch.uint8, device="cuda")
        pe = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
        pp = torch.full((n + 1,), -2, dtype=torch.int32, device="cuda")
        self.cap = cap = ns - cap_short
        self.fits, st, _, _, _ = eng.pcap_tcp(big[:soff + need - short], soff, po, n, link,
                                              info.flags, p,
                                              out=(table[:cap * 80], pe[:n], pp[:n]))
        self.stats = st.as_dict()
        torch.cuda.synchronize()
        self.table, self.piece_end, self.piece_pkt = table, pe, pp
        self.out = _host(p)
        h = big.cpu().numpy()
        self.scratch, self.guard = h[soff:soff + need].tobytes(), h[soff + need:]
        self.image_intact = np.array_equal(h[:soff], img)
        self.streams = table.cpu().numpy()[:ns * 80].view(mgen_amd.TCP_STREAM_DTYPE)
        self.table_guard = table.cpu().numpy()[ns * 80:]
        self.h_end, self.h_pkt = pe.cpu().numpy(), pp.cpu().numpy()

    def frame(self, long_bytes=0, cap=None):
        s = self.stats
        recs, status, k = self.eng.tcp_frame(
            self.big, self.table, s["n_streams"], self.piece_end, self.piece_pkt, s["n_pieces"],
            self.p["rx_sec"], self.p["rx_usec"], long_bytes=long_bytes, cap=cap)
        self.torch.cuda.synchronize()
        if recs is not None:
            recs = {name: t.cpu().numpy() for name, t in recs.items()}
        return recs, status.cpu().numpy(), k


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


def _addr(raw, port):
    a = np.zeros((), T.F_ADDR)
    a["type"], a["len"], a["port"] = (1 if len(raw) == 4 else 2), len(raw), port
    a["addr"][:len(raw)] = np.frombuffer(raw, np.uint8)
    return a


def _check_against_model(r: Run, recs, link):
    """Everything the contract fixes, against the model; the rest against the parse."""
    b, o = r.base, r.out
    ref = T.tcp_ref(recs, link, examined=[s != 6 for s in b["status"]])
    need, ns, npc = (ref.stats[k] for k in ("scratch_bytes", "n_streams", "n_pieces"))
    # the sizing call: no space unless nothing is needed, exact stats, nothing changed
    assert r.stats0 == ref.stats and r.fits0 == (need == 0 and ns == 0)
    if not r.fits0:
        assert _same(r.after0, b)
    assert r.fits and r.stats == ref.stats
    want = [bs if s is None else s for bs, s in zip(b["status"], ref.status)]
    assert o["status"].tolist() == want
    assert _same(o, b, [k for k in b if k != "status"])
    assert r.scratch == ref.scratch
    assert (r.guard == 0xA5).all() and r.image_intact and (r.table_guard == 0xA5).all()
    got = r.streams
    for s, t in enumerate(ref.streams):
        ver, src, dst, sport, dport = t["key"]
        assert got["src"][s] == _addr(src, sport) and got["dst"][s] == _addr(dst, dport), s
        row = tuple(int(got[k][s]) for k in ("off", "len", "dropped", "first_pkt", "n_segments",
                                             "flags", "rsv"))
        assert row == (r.soff + t["off"], t["len"], t["dropped"], t["first_pkt"],
                       t["n_segments"], t["flags"], 0), (s, row, t["off"])
    assert r.h_end[:npc].tolist() == [r.soff + e for e, _ in ref.pieces]
    assert r.h_pkt[:npc].tolist() == [p for _, p in ref.pieces]
    assert (r.h_end[npc:] == -2).all() and (r.h_pkt[npc:] == -2).all()
    return ref


def _check_frames(r: Run, oracle, ref, recs):
    """tcp_frame through both paths against the oracle's framing of the model's streams."""
    want, status = T.frame_ref(oracle, ref)
    out = []
    for long_bytes in (1, U64_MAX):
        got, st, k = r.frame(long_bytes)
        assert k == len(want) and st.tolist() == status, (long_bytes, k, len(want))
        assert got["rec_off"].tolist() == [r.soff + w[0] for w in want], long_bytes
        assert got["rec_len"].tolist() == [w[1] for w in want]
        assert got["rec_stream"].tolist() == [w[2] for w in want]
        assert got["rec_pkt"].tolist() == [w[3] for w in want]
        assert got["rx_sec"].view(np.uint32).tolist() == [recs[w[3]][0] for w in want]
        assert got["rx_usec"].view(np.uint32).tolist() == [recs[w[3]][1] for w in want]
        src = got["rec_src"].view(T.F_ADDR)
        assert all(src[j] == r.streams["src"][w[2]] for j, w in enumerate(want))
        out.append(got)
    assert _same(out[0], out[1])
    return want


# ---------------------------------------------------------------- whole logs
LOG_CASES = {
    "v4-eth": dict(),
    "v4-vlan": dict(vlan=77),
    "v4-sll": dict(link=113),
    "v6": dict(v6=True),
    "v4-pcapng": dict(ng=True),
    "v4-reassemble": dict(frag_mtu=1500, reassemble=True),
}


@pytest.fixture(scope="module")
def log_captures(oracle):
    out = {}
    for k, (name, c) in enumerate(LOG_CASES.items()):
        c = dict(c)
        ng, reassemble = c.pop("ng", False), c.pop("reassemble", False)
        f, conns, whole = T.capture(oracle, seed=60 + k, **c)
        link = c.get("link", 1)
        log, n_tcp, ref = T.expected_log(oracle, f, link, conns, whole)
        given = G.from_pcap(f, seed=k, epb_options=True).file if ng else f
        out[name] = dict(pcap=f, given=given, log=log, n_tcp=n_tcp, ref=ref,
                         reassemble=reassemble)
    return out


@pytest.mark.parametrize("case", list(LOG_CASES))
def test_tcp_log_equals_oracle(eng, log_captures, case):
    from mgen_amd.pcap import Pcap2Mgen
    c = log_captures[case]
    assert c["n_tcp"] >= 30 and c["ref"].stats["n_gap_streams"] == 0
    assert c["ref"].stats["n_streams"] >= 8
    run = Pcap2Mgen(eng, tcp=True, reassemble=c["reassemble"])
    got = run.run(c["given"])
    assert got == c["log"], _diff(got, c["log"])
    assert got.count(b"proto>TCP") == c["n_tcp"]
    assert run.last_tcp_stats.as_dict() == c["ref"].stats
    assert run.last_tcp_records == c["n_tcp"]
    if c["reassemble"]:
        assert run.last_defrag_stats.n_datagrams > 10


@pytest.mark.parametrize("case", list(LOG_CASES))
def test_default_is_unchanged(eng, oracle, log_captures, case):
    from mgen_amd.pcap import Pcap2Mgen
    c = log_captures[case]
    want, _ = oracle.pcap2mgen(c["pcap"], analytics=True, window=0.05)
    run = Pcap2Mgen(eng, analytics=True, window=0.05)
    got = run.run(c["given"])
    assert got == want, _diff(got, want)
    assert run.last_tcp_stats is None and b"proto>TCP" not in got


def test_whole_capture_against_model(eng, torch, oracle, log_captures):
    for case, link, ng in (("v4-eth", 1, False), ("v4-sll", 113, False), ("v4-pcapng", 1, True)):
        c = log_captures[case]
        recs = F.records(c["pcap"])
        r = Run(eng, torch, c["given"], link=link, ng=ng)
        ref = _check_against_model(r, recs, link)
        _check_frames(r, oracle, ref, recs)


def test_rerr_line_for_a_corrupted_record(eng, oracle):
    """A record whose checksum fails logs RERR (MgenTcpTransport::OnRecvMsg), not nothing."""
    from mgen_amd.pcap import Pcap2Mgen
    rng = np.random.default_rng(2)
    stream = bytearray(T.mgen_stream(oracle, rng, [200, 300, 150], 3, 1_700_000_000_000_000))
    stream[320] ^= 0x55                       # inside the second record's payload
    c = T.Conn()
    f = T.pcap_of([c.ip(s[0], s[2], s[1]) for s in T.segment(bytes(stream), 256, 77)])
    offs, lens, fld, _, _ = oracle.tcp_scan(bytes(stream))
    assert list(lens) == [200, 300, 150] and fld["err"][1] != 0
    recs = F.records(f)
    done = [1, 2, 3]                          # SYN, then [0,256) [256,512) [512,650)
    want = oracle.log_recv_text(fld, np.frombuffer(bytes(stream), np.uint8), offs,
                                np.stack([c.addr("src")] * 3), [recs[p][0] for p in done],
                                [recs[p][1] for p in done], protocol=2, ttl=None,
                                opts=oracle.LOG_NO_DATA)
    assert want.count(b"RERR") == 1 and want.count(b"RECV") == 2
    got = Pcap2Mgen(eng, tcp=True).run(f)
    assert got == want, _diff(got, want)


# ---------------------------------------------------------------- the state machine
def _bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _records(rng, sizes):
    """A stream of well-framed records: big-endian length, version byte 2, random bytes."""
    return b"".join(struct.pack(">HB", n, 2) + _bytes(rng, n - 3) for n in sizes)


def _ips(c, segs):
    return [c.ip(seq, pay, flags) for seq, flags, pay in segs]


def case_one_byte_segments(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [28, 30]), 1))


def case_segment_with_20_records(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [28 + k for k in range(20)]), 1448))


def case_record_over_40_segments(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [8000]), 200))


def case_exact_duplicate(rng):
    s = T.segment(_records(rng, [300, 300]), 250)
    return _ips(T.Conn(), [s[0], s[1], s[2], s[2], s[1], s[3]])


def case_partial_overlap_from_both_sides(rng):
    d = _records(rng, [30])
    c = T.Conn()
    return [c.ip(100, flags=T.SYN), c.ip(101, d[0:10]), c.ip(121, d[20:30]), c.ip(106, d[5:25])]


def case_segment_inside_covered_bytes(rng):
    d = _records(rng, [30])
    c = T.Conn()
    return [c.ip(100, flags=T.SYN), c.ip(101, d), c.ip(111, d[10:20])]


def case_reversed_order(rng):
    s = T.segment(_records(rng, [700, 29, 400]), 100)
    return _ips(T.Conn(), s[:1] + s[:0:-1])


def case_hole_in_the_middle(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [500, 500, 500]), 128, lose=(4,)))


def case_hole_at_offset_0(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [500]), 128, lose=(0,)))


def case_no_syn(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [100, 64]), 60, syn=False))


def case_syn_repeated(rng):
    s = T.segment(_records(rng, [100, 64]), 60)
    return _ips(T.Conn(), [s[0], s[0], s[1], s[0]] + s[2:])


def case_tuple_reuse_with_a_new_syn(rng):
    c = T.Conn()
    return (_ips(c, T.segment(_records(rng, [100]), 60, isn=5000)) +
            _ips(c, T.segment(_records(rng, [90, 40]), 70, isn=900000)) +
            _ips(c, T.segment(_records(rng, [33]), 70, isn=5000)))


def case_data_ahead_of_its_syn(rng):
    s = T.segment(_records(rng, [100, 64]), 60)
    return _ips(T.Conn(), [s[1], s[0]] + s[2:])


def case_seq_wraps(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [400, 400]), 90, isn=0xFFFFFF00 - 1))


def case_stale_segment(rng):
    c = T.Conn()
    s = T.segment(_records(rng, [100]), 60, isn=1000)
    return _ips(c, s) + [c.ip(900, b"before the base"), c.ip(1001 + 2**31 - 4, b"past 2 GiB")]


def case_pure_acks_fin_rst(rng):
    c = T.Conn()
    b = c.reverse()
    s = T.segment(_records(rng, [100]), 60, isn=1000)
    return ([b.ip(1, flags=T.ACK)] + _ips(c, s[:2]) + [b.ip(1, flags=T.ACK)] + _ips(c, s[2:]) +
            [c.ip(1101, flags=T.FIN | T.ACK), b.ip(1, flags=T.RST), c.ip(1101, b"after the FIN")])


def case_short_segment_with_ethernet_padding(rng):
    return _ips(T.Conn(), T.segment(_records(rng, [5]), 2))


def case_header_options(rng):
    c = T.Conn()
    d = _records(rng, [64])
    return [c.ip(1, flags=T.SYN, doff=24), c.ip(2, d[:30], doff=24), c.ip(32, d[30:], doff=32)]


def case_data_offset_16(rng):
    c = T.Conn()
    d = _records(rng, [64])
    return [c.ip(1, flags=T.SYN), c.ip(2, d[:30]), c.ip(32, d[30:], doff=16)]


def case_snap_cut_payload(rng):
    c = T.Conn()
    d = _records(rng, [64, 64])
    cut = c.ip(34, d[32:96])
    return [c.ip(1, flags=T.SYN), c.ip(2, d[:32]), (cut, 14 + len(cut) - 1), c.ip(98, d[96:])]


def case_9000_byte_segment(rng):
    d = _records(rng, [4000, 5000, 36])
    c = T.Conn()
    return [c.ip(1, flags=T.SYN), c.ip(2, d[:36]), c.ip(38, d[36:9036 - 36]), c.ip(9002, d[9000:])]


def case_both_directions(rng):
    c = T.Conn()
    a = _ips(c, T.segment(_records(rng, [300, 300]), 100, isn=10))
    b = _ips(c.reverse(), T.segment(_records(rng, [200, 250]), 100, isn=10))
    return [x for pair in zip(a, b) for x in pair] + a[len(b):]


def case_stream_lengths_15_16_17(rng):
    out = []
    for k, n in enumerate((15, 16, 17)):
        out += _ips(T.Conn(sport=100 + k), T.segment(_records(rng, [n]), 9))
    return out


def case_alignments(rng):
    """Sixteen streams; a filler record before each puts its first payload at file alignment
    0..15 (_place_alignments).  After 32 bytes, sixteen segments of 20 bytes each start three
    bytes early: trimmed to 17, their pieces start at scratch alignments 0..15 in turn."""
    out = []
    for k in range(16):
        c = T.Conn(sport=2000 + k)
        d = _records(rng, [32 + 16 * 17])
        out.append(("fill", k))
        out.append(c.ip(1, d[:32]))
        for j in range(16):
            lo = 32 + 17 * j
            out.append(c.ip(1 + lo - 3, d[lo - 3:lo + 17]))
    return out


def case_one_key_300_segments(rng):
    s = T.segment(_records(rng, [28] * 100 + [3000, 2204]), 27, rng=rng, retx=0.1, reorder=4)
    assert len(s) >= 300
    return _ips(T.Conn(), s)


def case_mixed_ipv6_ipv4(rng):
    a = _ips(T.Conn(T.A6, T.B6, 9, 10), T.segment(_records(rng, [300, 31]), 100))
    b = _ips(T.Conn(sport=9, dport=10), T.segment(_records(rng, [200, 64]), 100))
    return [x for pair in zip(a, b) for x in pair]


CASES = {f[5:]: g for f, g in sorted(globals().items()) if f.startswith("case_")}
EXPECT = {          # (streams, streams with a gap, stale segments, dropped bytes) by hand
    "one_byte_segments": (1, 0, 0, 0), "segment_with_20_records": (1, 0, 0, 0),
    "record_over_40_segments": (1, 0, 0, 0), "exact_duplicate": (1, 0, 0, 0),
    "partial_overlap_from_both_sides": (1, 0, 0, 0), "segment_inside_covered_bytes": (1, 0, 0, 0),
    "reversed_order": (1, 0, 0, 0), "hole_in_the_middle": (1, 1, 0, 1500 - 5 * 128),
    "hole_at_offset_0": (1, 1, 0, 500 - 128), "no_syn": (1, 0, 0, 0), "syn_repeated": (1, 0, 0, 0),
    "tuple_reuse_with_a_new_syn": (3, 0, 0, 0), "data_ahead_of_its_syn": (2, 1, 0, 104),
    "seq_wraps": (1, 0, 0, 0), "stale_segment": (1, 0, 2, 0), "pure_acks_fin_rst": (2, 0, 0, 0),
    "short_segment_with_ethernet_padding": (1, 0, 0, 0), "header_options": (1, 0, 0, 0),
    "data_offset_16": (1, 0, 0, 0), "snap_cut_payload": (1, 1, 0, 32),
    "9000_byte_segment": (1, 0, 0, 0), "both_directions": (2, 0, 0, 0),
    "stream_lengths_15_16_17": (3, 0, 0, 0), "alignments": (16, 0, 0, 0),
    "one_key_300_segments": (1, 0, 0, 0), "mixed_ipv6_ipv4": (2, 0, 0, 0),
}


def _place_alignments(items):
    out, off = [], 24
    for f in items:
        if isinstance(f, tuple) and f[0] == "fill":
            # an ARP-sized record, 60..75 bytes: the next record's TCP payload (its offset +
            # 16 + 14 + 20 + 20) lands on alignment f[1]
            extra = (f[1] - (off + 16 + 60 + 16 + 54)) % 16
            fr = P.eth(bytes(46 + extra), etype=0x0806)
            out.append(("raw", fr))
            off += 16 + len(fr)
        else:
            out.append(f)
            off += 16 + len(F.link_frame(f, 1))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_state_machine_against_model(eng, torch, oracle, case):
    rng = np.random.default_rng(len(case))
    items = CASES[case](rng)
    if case == "alignments":
        items = _place_alignments(items)
    f = T.pcap_of(items)
    recs = F.records(f)
    r = Run(eng, torch, f)
    ref = _check_against_model(r, recs, 1)
    s = ref.stats
    assert (s["n_streams"], s["n_gap_streams"], s["n_stale"], s["dropped_bytes"]) == \
        EXPECT[case], s
    want = _check_frames(r, oracle, ref, recs)
    if case == "alignments":
        src, at = [], 24
        for _, _, d, _ in recs:
            c = T.classify(d, len(d), 1)
            if c and c["seq"] == 1:
                src.append((at + 16 + 54) % 16)
            at += 16 + len(d)
        assert src == list(range(16))
        assert all(t["len"] == 32 + 16 * 17 for t in ref.streams)
        ends = sorted({e % 16 for e, _ in ref.pieces})
        assert ends == list(range(16))
    if case == "segment_with_20_records":
        assert len(want) == 20 and len({w[3] for w in want}) == 1
    if case == "record_over_40_segments":
        assert len(want) == 1 and want[0][3] == 40
    if case == "9000_byte_segment":
        assert r.base["status"].tolist() == [4, 4, 1, 4] and r.out["status"].tolist() == [9] * 4
    if case == "snap_cut_payload":
        assert r.out["status"].tolist() == [9, 9, 5, 9]
    if case == "data_offset_16":
        assert r.out["status"].tolist() == [9, 9, 4]
    if case == "stream_lengths_15_16_17":
        assert [t["len"] for t in ref.streams] == [15, 16, 17]
        assert [t["off"] for t in ref.streams] == [0, 16, 32] and s["scratch_bytes"] == 64


def test_pcapng_sll_ipv6_against_model(eng, torch, oracle):
    a = _ips(T.Conn(T.A6, T.B6, 9, 10), T.segment(_records(np.random.default_rng(1), [300, 31]),
                                                  100, isn=0xFFFFFFF0))
    f = T.pcap_of(a + [a[2]], link=113)
    ng = G.from_pcap(f, swapped=True, seed=4, epb_options=True, unknown_blocks=True,
                     kind=lambda i: "opb" if i % 3 == 0 else "epb")
    recs = G.expected_records(ng.file, ng.walk)
    r = Run(eng, torch, ng.file, link=113, ng=True)
    ref = _check_against_model(r, recs, 113)
    assert ref.stats["n_streams"] == 1 and ref.streams[0]["len"] == 331
    _check_frames(r, oracle, ref, recs)


# ---------------------------------------------------------------- sizing
@pytest.mark.parametrize("short,cap_short", [(1, 0), (0, 1)], ids=["window", "stream_cap"])
def test_one_short_changes_nothing(eng, torch, short, cap_short):
    rng = np.random.default_rng(8)
    f = T.pcap_of(case_both_directions(rng) + case_stream_lengths_15_16_17(rng))
    recs = F.records(f)
    ref = T.tcp_ref(recs, 1)
    assert ref.stats["n_streams"] == 5 and ref.stats["scratch_bytes"] == 608 + 464 + 64
    r = Run(eng, torch, f, short=short, cap_short=cap_short)
    # the empty window, and the window / table one short: ENOSPC, exact stats, nothing changed
    assert not r.fits0 and not r.fits and r.stats0 == r.stats == ref.stats
    assert _same(r.after0, r.base) and _same(r.out, r.base)
    assert (np.frombuffer(r.scratch, np.uint8) == 0xA5).all() and (r.guard == 0xA5).all()
    assert (r.table.cpu().numpy() == 0xA5).all()
    assert (r.h_end == -2).all() and (r.h_pkt == -2).all() and r.image_intact
    _check_against_model(Run(eng, torch, f), recs, 1)       # exact: fits


# ---------------------------------------------------------------- framing
def test_frame_cut_record_bad_length_and_cap(eng, torch, oracle):
    rng = np.random.default_rng(11)
    cut = _records(rng, [40, 50, 60])[:-7]                   # the last record is cut
    bad = _records(rng, [33, 44]) + b"\0\3" + _bytes(rng, 40)  # msg_len 3 after two records
    tail = _records(rng, [30])[:1]                           # one byte: no length to read
    items = []
    for k, d in enumerate((cut, bad, tail)):
        items += _ips(T.Conn(sport=700 + k), T.segment(d, 48))
    f = T.pcap_of(items)
    recs = F.records(f)
    r = Run(eng, torch, f)
    ref = _check_against_model(r, recs, 1)
    want = _check_frames(r, oracle, ref, recs)
    assert [(w[1], w[2]) for w in want] == [(40, 0), (50, 0), (33, 1), (44, 1)]
    assert T.frame_ref(oracle, ref)[1] == [0, 1, 0]
    for long_bytes in (1, U64_MAX):
        got, st, k = r.frame(long_bytes, cap=3)              # cap too small: the count alone
        assert got is None and k == 4 and st.tolist() == [0, 1, 0]
        got, st, k = r.frame(long_bytes, cap=4)
        assert k == 4 and got["rec_len"].tolist() == [40, 50, 33, 44]


# ---------------------------------------------------------------- the command line
def test_pcap2mgen_cli(oracle, tmp_path, log_captures):
    c = log_captures["v4-sll"]
    r = subprocess.run([EXE, "tcp"], input=c["given"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == c["log"], _diff(r.stdout, c["log"])
    c = log_captures["v4-pcapng"]
    pin = tmp_path / "x.pcapng"
    pin.write_bytes(c["given"])
    r = subprocess.run([EXE, "infile", str(pin), "tcp"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == c["log"], _diff(r.stdout, c["log"])
    # without the word the output is as before; `t` still means trace, which is refused
    r = subprocess.run([EXE], input=c["given"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == oracle.pcap2mgen(c["pcap"])[0]
    r = subprocess.run([EXE, "t"], input=c["given"], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"trace" in r.stderr and r.stdout == b""
    # a gap and a stale segment: the stats line
    rng = np.random.default_rng(5)
    f = T.pcap_of(case_hole_in_the_middle(rng) + case_stale_segment(rng)[3:])
    r = subprocess.run([EXE, "tcp"], input=f, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stderr == (b"pcap2mgen: tcp: 1 streams, 1 records, 1 cut at a gap (860 bytes "
                        b"dropped), 2 stale segments\n")
