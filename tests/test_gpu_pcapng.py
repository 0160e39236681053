"""GPU parity of pcap2mgen over pcapng captures: mgenx_pcapng_index (host block walk) ->
mgenx_pcapng_parse (device: packet block layout, 64-bit time stamp, the frame walk shared with
mgenx_pcap_parse) -> mgenx_pcapng_snap -> the pcap2mgen pipeline.

Expected values never come from the code under test: tests/pcapng_util.py re-emits a classic
capture as pcapng and gives back the equivalent classic file (the same frames with the times
the time stamp rule of DESIGN.md 4.10 yields), and that file goes to the oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pcap_util as P
import pcapng_util as G

pytestmark = pytest.mark.gpu


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


def _parse(eng, torch, f, pkt_off=None, pkt_if=None):
    """Index + mgenx_pcapng_parse of a file image: (outputs as numpy arrays, offsets, info);
    pkt_off / pkt_if replace what the index found."""
    import mgen_amd
    offs, pif, ifaces, info = mgen_amd.pcapng_index(f)
    offs = offs if pkt_off is None else pkt_off
    pif = pif if pkt_if is None else pkt_if
    buf = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    po = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    pi = torch.from_numpy(pif.view(np.int32).copy()).cuda()
    it = torch.from_numpy(ifaces.view(np.uint8).copy()).cuda()
    p = eng.pcapng_parse(buf, po, pi, len(offs), it, len(ifaces), info.link_type, info.flags)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in p.items()}
    out["src"] = out["src"].view(mgen_amd.ADDR_DTYPE)
    for k in ("rx_sec", "rx_usec", "udp_len", "cap_len"):
        out[k] = out[k].view(np.uint32)
    return out, offs, info


FRAME_CASES = {
    "eth-native-default": dict(link=1),
    "sll-swapped-ns": dict(link=113, swapped=True, ifaces=({"tsresol": 9},)),
    "eth-mixed": dict(link=1, n=500, ifaces=({"tsresol": 0x8A}, {"tsresol": 3,
                                                                "tsoffset": 1_000_000}),
                      epb_options=True, unknown_blocks=True, second_section_at=310,
                      kind=lambda i: "spb" if i % 13 == 6 else "opb" if i % 5 == 2 else "epb"),
}


@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_frame_walk_matches_oracle(eng, torch, oracle, case):
    """Each packet re-wrapped as a classic record (the rule's sec / usec, caplen, origlen,
    data) goes through the oracle's frame walk."""
    c = dict(FRAME_CASES[case])
    link, n = c.pop("link"), c.pop("n", 400)
    ng = G.from_pcap(P.capture(oracle, seed=50 + link, n=n, link=link), seed=link, **c)
    p, offs, info = _parse(eng, torch, ng.file)
    assert info.status == 0 and len(offs) == n and info.link_type == link
    recs = G.expected_records(ng.file, ng.walk)
    seen = np.zeros(8, int)
    for i, (sec, usec, data, origlen) in enumerate(recs):
        rec = struct.pack("<IIII", sec, usec, len(data), origlen) + data
        st, uo, ul, s, ttl, osec, ousec = oracle.pcap_frame(rec, link, 0)
        seen[st] += 1
        assert (osec, ousec) == (sec, usec)
        assert p["status"][i] == st, i
        assert (p["rx_sec"][i], p["rx_usec"][i]) == (sec, usec), i
        assert (p["data_off"][i], p["cap_len"][i]) == ng.walk.packets[i][:2]
        if st == 0:
            # the oracle counts from its record's 16-byte header
            assert p["udp_off"][i] - p["data_off"][i] == uo - 16 and p["udp_len"][i] == ul
            assert p["ttl"][i] == ttl
            assert p["src"][i]["type"] == s["type"] and p["src"][i]["port"] == s["port"]
            assert bytes(p["src"][i]["addr"][:s["len"]]) == bytes(s["addr"][:s["len"]])
        else:
            assert p["udp_len"][i] == 0
    assert seen[0] > n // 2 and (seen[1:6] > 0).sum() >= 3, seen    # skipped kinds are there
    if case == "eth-mixed":
        assert len(set(ng.walk.pkt_if)) == 4


def test_worked_time_stamps_on_device(eng, torch):
    """The worked values of the time stamp rule, and its wrap-around, through the kernel."""
    e = "<"
    fr = P.eth(P.ipv4(P.udp(bytes(30), 1, 2), bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])))
    rows = [(9, None, 1700000000123456789, (1700000000, 123456)),
            (3, None, 1700000000123, (1700000000, 123000)),
            (0x8A, None, 1700000000 * 1024 + 513, (1700000000, 500976)),
            (None, 1700000000, 5000007, (1700000005, 7)),
            (6, -1, 7, None), (19, None, 10 ** 19 - 1, None), (0x80 | 63, 5, (1 << 63) + 5, None),
            (0, 9, 12345, None), (12, None, (1 << 64) - 1, None), (0x80, None, 77, None)]
    f = G.shb(e) + b"".join(G.idb(e, 1, tsresol=r, tsoffset=o) for r, o, _, _ in rows)
    f += b"".join(G.epb(e, k, t, fr) for k, (_, _, t, _) in enumerate(rows))
    p, offs, info = _parse(eng, torch, f)
    assert len(offs) == len(rows) and (p["status"] == 0).all()
    for k, (r, o, t, want) in enumerate(rows):
        R, binary = G.units(r)
        rule = G.ts_rule(t, R, binary, o or 0)
        assert want is None or rule == want
        assert (p["rx_sec"][k], p["rx_usec"][k]) == rule, (k, rule)


PIPELINE_CASES = [      # the case list of test_gpu_pcap.test_pcap2mgen_matches_oracle
    dict(seed=1), dict(seed=2, analytics=True), dict(seed=3, analytics=True, window=0.05),
    dict(seed=4, link=113, analytics=True), dict(seed=5, nsec=True, swapped=True),
    dict(seed=6, analytics=True, log_rx=False), dict(seed=7, epoch=True, analytics=True,
                                                    window=0.02)]
# how each is wrapped (time stamps stay 10^-6 but for the nanosecond case, which is 10^-9)
PIPELINE_KNOBS = {
    2: dict(ifaces=({}, {"tsresol": 6})),
    3: dict(epb_options=True, unknown_blocks=True),
    4: dict(swapped=True, second_section_at=400),
    6: dict(kind=lambda i: "opb" if i % 3 == 0 else "epb", ifaces=({}, {}, {})),
    7: dict(ifaces=({"tsresol": 6, "tsoffset": 1_600_000_000},), unknown_blocks=True),
}


@pytest.mark.parametrize("case", PIPELINE_CASES, ids=[f"seed{c['seed']}" for c in PIPELINE_CASES])
def test_pcap2mgen_matches_oracle(eng, oracle, case):
    from mgen_amd.pcap import Pcap2Mgen
    c = dict(case)
    seed = c.pop("seed")
    link, nsec, sw = c.pop("link", 1), c.pop("nsec", False), c.pop("swapped", False)
    f = P.capture(oracle, seed=seed, n=700, link=link, nsec=nsec)
    knobs = dict(PIPELINE_KNOBS.get(seed, {}))
    if nsec:
        knobs["ifaces"] = ({"tsresol": 9},)
    sw = knobs.pop("swapped", False) or sw
    ng = G.from_pcap(f, swapped=sw, seed=seed, **knobs)
    an, rx, w, ep = (c.get("analytics", False), c.get("log_rx", True), c.get("window", 1.0),
                     c.get("epoch", False))
    want, _ = oracle.pcap2mgen(ng.equiv, analytics=an, log_rx=rx, window=w,
                               opts=oracle.LOG_EPOCH if ep else 0)
    run = Pcap2Mgen(eng, analytics=an, log_rx=rx, window=w, epoch=ep)
    got = run.run(ng.file)
    assert len(want) > 0
    assert got == want, _diff(got, want)
    if not nsec:    # 10^-6: the same log as the capture it was made from
        assert got == run.run(f)


@pytest.mark.parametrize("snaplen", [128, 70])
def test_snaplen_capture_matches_oracle(eng, torch, oracle, snaplen):
    """A pcapng capture taken with a snapshot length: the same log as the oracle's on the
    snapped classic capture (mgenx_pcapng_snap zero-extends the cut payloads)."""
    from mgen_amd.pcap import Pcap2Mgen
    f = P.snap(P.capture(oracle, seed=40 + snaplen, n=600), snaplen)
    ng = G.from_pcap(f, seed=snaplen, epb_options=True)
    want, st = oracle.pcap2mgen(f, analytics=True, window=0.05)
    assert oracle.pcap2mgen(ng.equiv, analytics=True, window=0.05)[0] == want
    p, _, info = _parse(eng, torch, ng.file)
    assert info.snap_bytes > 0 and (p["status"] == st).all()
    if snaplen == 128:
        assert (p["status"] == 7).sum() > 100, np.bincount(p["status"])
    got = Pcap2Mgen(eng, analytics=True, window=0.05).run(ng.file)
    assert len(want) > 0
    assert got == want, _diff(got, want)


def test_stopped_and_empty_captures(eng, oracle):
    """A walk that stops keeps the packets before the stop; no packets, no log."""
    from mgen_amd.pcap import Pcap2Mgen
    ng = G.from_pcap(P.capture(oracle, seed=61, n=450), ifaces=({"tsresol": 9},))
    cut = ng.file[:len(ng.file) * 3 // 5 + 2]
    w = G.walk(cut)
    assert w.status == G.TRUNCATED and 200 < w.n_records < 450
    want, _ = oracle.pcap2mgen(G.equivalent_pcap(cut, w), analytics=True, window=0.1)
    got = Pcap2Mgen(eng, analytics=True, window=0.1).run(cut)
    assert len(want) > 0 and got == want, _diff(got, want)
    assert Pcap2Mgen(eng, analytics=True).run(G.shb("<") + G.idb("<", 1)) == b""
    assert Pcap2Mgen(eng).run(G.shb(">")) == b""


def test_offsets_the_index_did_not_produce(eng, torch, oracle):
    """Defined behaviour for foreign offsets: a block head or data outside the buffer, an
    interface row outside the table or a block that is no packet block gives MGENX_PCAP_OOB
    (every read is bounded first); the other packets are unchanged."""
    import mgen_amd
    ng = G.from_pcap(P.capture(oracle, seed=71, n=420), ifaces=({}, {"tsresol": 9}))
    base, offs, info = _parse(eng, torch, ng.file)
    _, pif, ifaces, _ = mgen_amd.pcapng_index(ng.file)
    nb = len(ng.file)
    o2, i2 = offs.copy(), pif.copy()
    bad_off = {3: nb - 8, 64: nb - 4, 65: nb, 200: nb + 1000, 255: 1 << 63, 256: (1 << 64) - 1,
               300: int(offs[9]) + 8, 419: int(offs[7]) + 4}     # the last two: no packet block
    bad_if = {10: len(ifaces), 257: 0xFFFFFFFF, 418: 2}
    for k, v in bad_off.items():
        o2[k] = v
    for k, v in bad_if.items():
        i2[k] = v
    p, _, _ = _parse(eng, torch, ng.file, pkt_off=o2, pkt_if=i2)
    bad = sorted(set(bad_off) | set(bad_if))
    keep = np.setdiff1d(np.arange(len(offs)), bad)
    assert (p["status"][bad] == 6).all() and (p["udp_len"][bad] == 0).all()
    assert (p["cap_len"][bad] == 0).all() and (p["ttl"][bad] == -1).all()
    for k in base:
        assert np.array_equal(p[k][keep], base[k][keep]), k
    assert (base["status"][bad] == 0).sum() > len(bad) // 2     # they were good packets


def test_pcap2mgen_cli(oracle, tmp_path):
    """tools/pcap2mgen takes a pcapng capture with no new option."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                       "pcap2mgen")
    ng = G.from_pcap(P.capture(oracle, seed=33, n=600), swapped=True,
                     ifaces=({"tsresol": 9}, {"tsresol": 6}), epb_options=True,
                     unknown_blocks=True, second_section_at=250)
    pin = tmp_path / "x.pcapng"
    pin.write_bytes(ng.file)
    r = subprocess.run([exe, "infile", str(pin), "analytic", "window", "0.1"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, _ = oracle.pcap2mgen(ng.equiv, analytics=True, window=0.1)
    assert len(want) > 0 and r.stdout == want, _diff(r.stdout, want)
    # cut by a snapshot length, from stdin (mgenx_pcapng_snap through the C++ class)
    f = P.snap(P.capture(oracle, seed=34, n=500), 128)
    ng = G.from_pcap(f, ifaces=({}, {"tsresol": 6}))
    r = subprocess.run([exe, "report"], input=ng.file, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, st = oracle.pcap2mgen(ng.equiv, analytics=True)
    assert (st == 7).sum() > 100 and r.stdout == want, _diff(r.stdout, want)
    r = subprocess.run([exe], input=b"\x0a\x0d\x0d\x0a" + bytes(40), capture_output=True,
                       timeout=120)
    assert r.returncode != 0 and b"not a pcap or pcapng file" in r.stderr
