"""GPU tests of IP reassembly in pcap2mgen (mgenx_pcap_defrag / mgenx_pcapng_defrag and the
`reassemble` option of every layer above them).

Expected values never come from the code under test: whole logs come from the oracle over the
same traffic captured unfragmented, per-packet arrays, scratch bytes and counts from the serial
model of the contract in tests/pcap_frag_util.py (itself pinned by tests/test_pcap_frag_cpu.py).
What the contract leaves untouched is compared with the parse's own output before the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pcap_frag_util as F
import pcap_util as P
import pcapng_util as G

pytestmark = pytest.mark.gpu
GUARD = 256
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
    o["udp_len"] = o["udp_len"].view(np.uint32)
    return o


class Run:
    """Parse + defrag of one capture: the sizing call on an empty window, then the exact
    window with a guard region behind it."""

    def __init__(self, eng, torch, file, link=1, timeout_us=30_000_000, ng=False, short=0):
        import mgen_amd
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
        defrag = eng.pcapng_defrag if ng else eng.pcap_defrag
        small = torch.from_numpy(img).cuda()
        p = parse(small)
        self.base = _host(p)
        self.fits0, st = defrag(small, soff, po, n, link, info.flags, p, timeout_us=timeout_us)
        self.stats0 = st.as_dict()
        self.after0 = _host(p)
        need = self.stats0["scratch_bytes"]
        big = torch.full((soff + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        big[:soff] = small
        p = parse(big[:soff])
        self.fits, st = defrag(big[:soff + need - short], soff, po, n, link, info.flags, p,
                               timeout_us=timeout_us)
        self.stats = st.as_dict()
        torch.cuda.synchronize()
        self.out = _host(p)
        h = big.cpu().numpy()
        self.scratch, self.guard = h[soff:soff + need].tobytes(), h[soff + need:]
        self.image_intact = np.array_equal(h[:soff], img)


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


def _check_against_model(r: Run, recs, link, timeout_us=30_000_000):
    """Everything the contract fixes, against the model; the rest against the parse."""
    b, o = r.base, r.out
    ref = F.frag_ref(recs, link, b["status"], b["udp_len"], b["src"]["port"], timeout_us)
    need = ref.stats["scratch_bytes"]
    # the sizing call: no space unless nothing is needed, exact need, nothing changed
    assert r.stats0 == ref.stats and r.fits0 == (need == 0)
    if need:
        assert _same(r.after0, b)
    assert r.fits and r.stats == ref.stats
    assert np.array_equal(o["status"], ref.status), (o["status"], ref.status)
    assert np.array_equal(o["udp_len"], ref.udp_len)
    assert np.array_equal(o["src"]["port"], ref.port)
    for k in ("type", "len", "addr"):
        assert np.array_equal(o["src"][k], b["src"][k]), k
    assert _same(o, b, ("ttl", "rx_sec", "rx_usec"))
    want_off = np.where(ref.udp_rel >= 0, r.soff + ref.udp_rel, b["udp_off"])
    assert np.array_equal(o["udp_off"], want_off)
    assert r.scratch == ref.scratch
    assert (r.guard == 0xA5).all() and r.image_intact
    return ref


# ---------------------------------------------------------------- 1, 2: whole logs
LOG_CASES = {
    "v4-mtu1500": dict(mtu=1500),
    "v4-mtu576-sll": dict(mtu=576, link=113),
    "v6-mtu1280": dict(mtu=1280, v6=True),
    "v4-vlan": dict(mtu=1500, vlan=77),
    "v4-pcapng": dict(mtu=1500, ng=True),
}


@pytest.fixture(scope="module")
def log_captures(oracle):
    out = {}
    for k, (name, c) in enumerate(LOG_CASES.items()):
        c = dict(c)
        ng = c.pop("ng", False)
        whole, cut = F.capture(oracle, seed=20 + k, n=40, **c)
        out[name] = (whole, cut, G.from_pcap(cut, seed=k, epb_options=True).file if ng else cut)
    return out


@pytest.mark.parametrize("analytics", [False, True], ids=["plain", "analytic"])
@pytest.mark.parametrize("case", list(LOG_CASES))
def test_reassembled_log_equals_oracle_on_unfragmented_capture(eng, oracle, log_captures, case,
                                                               analytics):
    from mgen_amd.pcap import Pcap2Mgen
    whole, cut, given = log_captures[case]
    want, st = oracle.pcap2mgen(whole, analytics=analytics, window=0.05)
    assert (st == 0).sum() >= 30 and len(want) > 0
    run = Pcap2Mgen(eng, analytics=analytics, window=0.05, reassemble=True)
    got = run.run(given)
    assert got == want, _diff(got, want)
    s = run.last_defrag_stats
    n_big = len(F.records(cut)) - len(F.records(whole))
    assert s.n_datagrams > 20 and s.n_incomplete == 0 and s.n_not_udp == 0
    assert s.n_fragments == n_big + s.n_datagrams


@pytest.mark.parametrize("case", list(LOG_CASES))
def test_default_is_unchanged(eng, oracle, log_captures, case):
    from mgen_amd.pcap import Pcap2Mgen
    _, cut, given = log_captures[case]
    want, _ = oracle.pcap2mgen(cut, analytics=True, window=0.05)
    run = Pcap2Mgen(eng, analytics=True, window=0.05)
    got = run.run(given)
    assert got == want, _diff(got, want)
    assert run.last_defrag_stats is None


# ---------------------------------------------------------------- 3: past the 4094-byte rule
def test_8192_byte_messages(eng, torch, oracle):
    from mgen_amd.pcap import Pcap2Mgen
    whole, cut = F.capture(oracle, seed=31, n=13, lo=8192, hi=8192, small=False)
    recs = F.records(cut)
    r = Run(eng, torch, cut)
    ref = _check_against_model(r, recs, 1)
    assert ref.stats["n_datagrams"] == 12 and ref.stats["n_fragments"] == 72
    done = [(p, D) for p, L, D, _ in ref.datagrams]
    assert all(len(D) == 8200 for _, D in done)
    # the RECV lines over the model's datagrams
    slab = np.frombuffer(ref.scratch, np.uint8).copy()
    idx = np.array([p for p, _ in done])
    off = ref.udp_rel[idx].astype(np.uint64)
    f = oracle.udp_recv_batch(slab, len(idx), rec_off=off, rec_len=ref.udp_len[idx])
    src = np.zeros(len(idx), oracle.ADDR_DTYPE)
    src["type"], src["len"], src["port"] = 1, 4, ref.port[idx]
    for k, p in enumerate(idx):
        src["addr"][k, :4] = np.frombuffer(recs[p][2][26:30], np.uint8)
    ttl = np.array([recs[p][2][22] for p in idx])
    want = oracle.log_recv_text(f, slab, off, src, [recs[p][0] for p in idx],
                                [recs[p][1] for p in idx], protocol=1, ttl=ttl,
                                opts=oracle.LOG_NO_DATA)
    got = Pcap2Mgen(eng, reassemble=True).run(cut)
    assert want.count(b"\n") == 12 and got == want, _diff(got, want)
    assert Pcap2Mgen(eng).run(cut) == oracle.pcap2mgen(cut)[0]      # the default: as before


# ---------------------------------------------------------------- 4: the state machine
A4, B4, C4 = bytes([10, 0, 0, 5]), bytes([10, 0, 0, 6]), bytes([10, 0, 0, 2])
A6 = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1])
B6 = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [2])


def _udp4(rng, n, src=A4, dst=C4, ul=None, proto=17):
    """An IPv4 datagram whose UDP datagram is n bytes long in all (UDP length field ul)."""
    body = struct.pack(">HHHH", int(rng.integers(1024, 60000)), 5001, n if ul is None else ul, 0)
    body = (body + bytes(rng.integers(0, 256, max(0, n - 8), dtype=np.uint8)))[:n]
    return P.ipv4(body, src, dst, proto=proto, total=None if n <= 65515 else 0)


def _udp6(rng, n, src=A6, dst=B6):
    body = struct.pack(">HHHH", int(rng.integers(1024, 60000)), 6001, n, 0)
    body = (body + bytes(rng.integers(0, 256, max(0, n - 8), dtype=np.uint8)))[:n]
    return P.ipv6(body, src, dst)


def _pcap(frames, link=1, dt=50, times=None):
    """frames: IP packets, (IP packet, caplen) or ("raw", link frame) -> a capture, dt
    microseconds apart."""
    recs = []
    for k, f in enumerate(frames):
        ip, cap = f if isinstance(f, tuple) else (f, None)
        fr, cap = (cap, None) if ip == "raw" else (F.link_frame(ip, link), cap)
        t = 1_700_000_000_000_000 + (times[k] if times else k * dt)
        sec, usec = divmod(t, 1_000_000)
        recs.append((sec, usec, fr) if cap is None else (sec, usec, fr, cap, len(fr)))
    return P.pcap(recs, link=link)


def _hdr4(src=A4, dst=C4, proto=17):
    return P.ipv4(b"", src, dst, proto=proto)


def case_reversed_and_shuffled(rng):
    a = F.fragment(_udp4(rng, 3000), 576, 1)
    b = F.fragment(_udp4(rng, 2999, src=B4), 576, 2)
    c = F.fragment(_udp6(rng, 5000), 1280, 3)
    return a[::-1] + [b[k] for k in rng.permutation(len(b))] + c[::-1]


def case_two_keys_interleaved(rng):
    a = F.fragment(_udp4(rng, 2400), 576, 9)
    b = F.fragment(_udp4(rng, 2400, src=B4), 576, 9)
    # the two directions of one IPv6 address pair, same id: one hash, two keys
    c = F.fragment(_udp6(rng, 4000, A6, B6), 1280, 0x01020304)
    d = F.fragment(_udp6(rng, 4000, B6, A6), 1280, 0x01020304)
    return [x for pair in zip(a, b) for x in pair] + [x for pair in zip(c, d) for x in pair]


def case_key_reused_after_completion(rng):
    return F.fragment(_udp4(rng, 2000), 576, 5) + F.fragment(_udp4(rng, 1800), 576, 5)


def case_lost_middle_then_id_reused(rng):
    a = F.fragment(_udp4(rng, 2400), 576, 5)
    return a[:2] + a[3:] + F.fragment(_udp4(rng, 2300), 576, 5)


def case_exact_duplicate(rng):
    a = F.fragment(_udp4(rng, 1600), 576, 5)
    return [a[0], a[1], a[1], a[2], a[0], a[1]]


def case_partial_overlap(rng):
    d = _udp4(rng, 64)[20:]
    h = _hdr4()
    return [F.frag_v4(h, d[0:32], 0, True, 5), F.frag_v4(h, d[24:48], 24, True, 5),
            F.frag_v4(h, d[48:64], 48, False, 5), F.frag_v4(h, d[0:24], 0, True, 5)]


def case_second_last_fragment(rng):
    d = _udp4(rng, 64)[20:]
    h = _hdr4()
    return [F.frag_v4(h, d[0:16], 0, True, 5), F.frag_v4(h, d[48:64], 48, False, 5),
            F.frag_v4(h, d[32:40], 32, False, 5), F.frag_v4(h, d[0:32], 0, True, 5)]


def case_last_below_a_held_end(rng):
    d = _udp4(rng, 64)[20:]
    h = _hdr4()
    return [F.frag_v4(h, d[16:32], 16, True, 5), F.frag_v4(h, d[8:16], 8, False, 5),
            F.frag_v4(h, d[0:8], 0, True, 5)]


def case_sixty_fifth_fragment(rng):
    d = _udp4(rng, 8 * 70)[20:]
    h = _hdr4()
    return [F.frag_v4(h, d[8 * k:8 * k + 8], 8 * k, k < 69, 5) for k in range(70)]


def case_sixty_four_fragments_complete(rng):
    d = _udp4(rng, 8 * 64)[20:]
    h = _hdr4()
    return [F.frag_v4(h, d[8 * k:8 * k + 8], 8 * k, k < 63, 5) for k in range(64)]


def case_ipv6_atomic(rng):
    d = _udp6(rng, 300)
    return [F.frag_v6(d[:40], d[40:], 0, False, 77), d]


def case_not_udp_on_completion(rng):
    short = _udp6(rng, 5)                                    # L < 8
    big = F.fragment(_udp4(rng, 1600, ul=1601), 576, 5)      # ul > L
    small = F.fragment(_udp4(rng, 1600, src=B4, ul=7), 576, 5)   # ul < 8
    return [F.frag_v6(short[:40], short[40:], 0, False, 1)] + big + small


def case_non_udp_fragments(rng):
    t = F.fragment(_udp4(rng, 1600, proto=6), 576, 5)
    d = _udp6(rng, 64)
    return t + [F.frag_v6(d[:40], d[40:], 0, False, 7, inner=6)]


def case_invalid_payloads(rng):
    a = F.fragment(_udp4(rng, 1200), 576, 5)
    d = _udp4(rng, 64)[20:]
    h = _hdr4(src=B4)
    six = _udp6(rng, 64)
    cut6 = F.frag_v6(six[:40], six[40:], 0, True, 9)
    short6 = bytearray(cut6)
    struct.pack_into(">H", short6, 4, 4)                     # payload length 4 < 8
    return [a[0], (a[1], 300), a[2],                         # cut by the snapshot length
            F.frag_v4(h, b"", 0, True, 6),                   # no payload
            F.frag_v4(h, d[0:20], 0, True, 7),               # MF and 20 % 8
            F.frag_v4(h, d[0:8], 65528, True, 8),            # off + len > 65535
            (cut6, 14 + 44), bytes(short6)]                  # fragment header cut; pl < 8


def case_lengths(rng):
    out = []
    for k, n in enumerate((8, 9, 23, 24)):
        d = _udp4(rng, n)[20:] if n > 8 else None
        if n == 8:
            six = _udp6(rng, 8)
            out.append(F.frag_v6(six[:40], six[40:], 0, False, 50))
        else:
            first = 8 if n == 9 else 16
            out += [F.frag_v4(_hdr4(), d[:first], 0, True, 50 + k),
                    F.frag_v4(_hdr4(), d[first:], first, False, 50 + k)]
    return out + F.fragment(_udp4(rng, 65535), 1500, 60)


def case_one_key_200_packets(rng):
    out = []
    for _ in range(25):
        out += F.fragment(_udp4(rng, 576 * 7 + 100), 576, 5)
    assert len(out) == 200
    return out


def case_source_alignments(rng):
    """Sixteen datagrams; a filler record before each puts its first payload at the next
    alignment 0..15 in the file."""
    frames = []
    for k in range(16):
        frames.append(("fill", k))
        frames += F.fragment(_udp4(rng, 1000 + 8 * k, src=bytes([10, 0, 1, k])), 576, k)
    return frames


CASES = {f[5:]: g for f, g in sorted(globals().items()) if f.startswith("case_")}


@pytest.mark.parametrize("case", list(CASES))
def test_state_machine_against_model(eng, torch, case):
    rng = np.random.default_rng(len(case))
    frames = CASES[case](rng)
    if case == "source_alignments":
        frames = _place_alignments(frames)
    f = _pcap(frames)
    recs = F.records(f)
    ref = _check_against_model(Run(eng, torch, f), recs, 1)
    s = ref.stats
    expect = {                       # (datagrams, not UDP, incomplete) worked by hand
        "reversed_and_shuffled": (3, 0, 0), "two_keys_interleaved": (4, 0, 0),
        "key_reused_after_completion": (2, 0, 0), "lost_middle_then_id_reused": (1, 0, 1),
        "exact_duplicate": (1, 0, 2), "partial_overlap": (1, 0, 1),
        "second_last_fragment": (1, 1, 1), "last_below_a_held_end": (1, 1, 1),
        "sixty_fifth_fragment": (0, 0, 2), "sixty_four_fragments_complete": (1, 0, 0),
        "ipv6_atomic": (1, 0, 0), "not_udp_on_completion": (3, 3, 0),
        "non_udp_fragments": (0, 0, 0), "invalid_payloads": (0, 0, 1),
        "lengths": (5, 0, 0), "one_key_200_packets": (25, 0, 0),
        "source_alignments": (16, 0, 0)}[case]
    assert (s["n_datagrams"], s["n_not_udp"], s["n_incomplete"]) == expect, s
    if case == "source_alignments":
        first = [F.classify(d, o, 1) for _, _, d, o in recs]
        at, off = [], 24
        for (_, _, d, _), c in zip(recs, first):
            if c and c["off"] == 0:
                at.append((off + 16 + c["lo"]) % 16)
            off += 16 + len(d)
        assert at == list(range(16))
    if case == "lengths":
        assert [L for _, L, _, _ in ref.datagrams] == [8, 9, 23, 24, 65535]
    if case == "invalid_payloads":
        assert ref.status.tolist() == [8, 5, 8, 3, 3, 3, 5, 3]


def _place_alignments(frames):
    out, off = [], 24
    for f in frames:
        if isinstance(f, tuple) and f[0] == "fill":
            # an ARP-sized record, 60..75 bytes: the next record's IPv4 payload (its offset +
            # 16 + 14 + 20) lands on alignment f[1]
            extra = (f[1] - (off + 16 + 60 + 16 + 34)) % 16
            fr = P.eth(bytes(46 + extra), etype=0x0806)
            out.append(("raw", fr))
            off += 16 + len(fr)
        else:
            out.append(f)
            off += 16 + len(F.link_frame(f, 1))
    return out


@pytest.mark.parametrize("timeout_us,done", [(100, 0), (101, 1), (0, 1)],
                         ids=["exceeded", "exactly", "disabled"])
def test_timeout(eng, torch, timeout_us, done):
    rng = np.random.default_rng(3)
    a = F.fragment(_udp4(rng, 1400), 576, 5)
    assert len(a) == 3
    f = _pcap(a, times=[0, 100, 101])
    ref = _check_against_model(Run(eng, torch, f, timeout_us=timeout_us), F.records(f), 1,
                               timeout_us)
    assert ref.stats["n_datagrams"] == done and ref.stats["n_incomplete"] == 2 * (1 - done)
    # a receive time that runs backwards does not expire anything
    f = _pcap(a, times=[500, 0, 200])
    ref = _check_against_model(Run(eng, torch, f, timeout_us=100), F.records(f), 1, 100)
    assert ref.stats["n_datagrams"] == 1


def test_pcapng_and_sll_against_model(eng, torch, oracle):
    _, cut = F.capture(oracle, seed=41, n=20, mtu=576, link=113, v6=True)
    ng = G.from_pcap(cut, swapped=True, seed=4, epb_options=True, unknown_blocks=True,
                     kind=lambda i: "opb" if i % 3 == 0 else "epb")
    ref = _check_against_model(Run(eng, torch, ng.file, link=113, ng=True),
                               G.expected_records(ng.file, ng.walk), 113)
    assert ref.stats["n_datagrams"] > 10
    ref = _check_against_model(Run(eng, torch, cut, link=113), F.records(cut), 113)
    assert ref.stats["n_datagrams"] > 10


# ---------------------------------------------------------------- 5: sizing
def test_window_one_byte_short(eng, torch):
    rng = np.random.default_rng(8)
    f = _pcap(case_reversed_and_shuffled(rng))
    r = Run(eng, torch, f, short=1)
    ref = F.frag_ref(F.records(f), 1, r.base["status"], r.base["udp_len"],
                     r.base["src"]["port"])
    assert ref.stats["scratch_bytes"] == 3008 + 3008 + 5008
    assert not r.fits0 and not r.fits and r.stats0 == r.stats == ref.stats
    assert _same(r.after0, r.base) and _same(r.out, r.base)
    assert (np.frombuffer(r.scratch, np.uint8) == 0xA5).all() and (r.guard == 0xA5).all()
    assert Run(eng, torch, f).fits                   # the exact window: _check_against_model


# ---------------------------------------------------------------- 6: the command line
def test_pcap2mgen_cli(oracle, tmp_path, log_captures):
    whole, cut, _ = log_captures["v4-mtu576-sll"]
    pin = tmp_path / "x.pcap"
    pin.write_bytes(cut)
    want, _ = oracle.pcap2mgen(whole, analytics=True, window=0.05)
    r = subprocess.run([EXE, "infile", str(pin), "analytic", "window", "0.05", "reassemble"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want, _diff(r.stdout, want)
    whole, _, given = log_captures["v4-pcapng"]         # the pcapng front end, from stdin
    r = subprocess.run([EXE, "reassemble"], input=given, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == oracle.pcap2mgen(whole)[0], _diff(r.stdout, oracle.pcap2mgen(whole)[0])
    # an incomplete datagram: the stats line; "re" still means report, fragtime takes seconds
    rng = np.random.default_rng(5)
    f = _pcap(case_lost_middle_then_id_reused(rng))
    r = subprocess.run([EXE, "reas", "fragtime", "0"], input=f, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stderr == (b"pcap2mgen: reassembly: 9 fragments, 1 datagrams (0 not UDP), "
                        b"1 incomplete\n")
    r = subprocess.run([EXE, "re"], input=cut, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == oracle.pcap2mgen(cut, analytics=True)[0]
