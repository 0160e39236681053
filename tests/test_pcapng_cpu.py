"""CPU: the pcapng block walk (mgenx_pcapng_index, mgen_amd/csrc/mgenx_pcapng.hpp) against a
pure-Python restatement of the walk rules (tests/pcapng_util.py: DESIGN.md 4.10) -- offsets,
interface rows, the interface table, counts, snap_bytes, flags, link type -- one file per stop
rule with its status / n_records / consumed, what is and is not a pcapng file, the worked time
stamps of the rule, and the walk under the address / undefined-behaviour sanitizers
(tests/cpp/pcapng_host: every prefix and single-field mutations of a capture)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pcap_util as P
import pcapng_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "pcapng_host")


def _frames(n, seed=3):
    """n small UDP-in-IPv4 Ethernet frames of lengths that are no multiple of 4, with times."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pay = bytes(rng.integers(0, 256, int(rng.integers(1, 90)), dtype=np.uint8))
        fr = P.eth(P.ipv4(P.udp(pay, 1000 + i, 2000), bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])),
                   pad_to=0)
        out.append((1_700_000_000 + i, 1000 * i + 7, fr))
    return out


def _check(f: bytes):
    """The C index == the Python walk on f; returns (walk, info)."""
    import mgen_amd
    w = G.walk(f)
    assert w is not None
    offs, pkt_if, ifaces, info = mgen_amd.pcapng_index(f)
    assert info.status == w.status
    assert (info.n_records, info.consumed) == (w.n_records, w.consumed)
    assert list(offs) == w.offs and list(pkt_if) == w.pkt_if
    assert (info.n_ifaces, info.n_sections) == (len(w.ifaces), w.n_sections)
    assert [(int(r["ts_units"]), int(r["ts_offset"]), int(r["snaplen"]), bool(r["ts_binary"]))
            for r in ifaces] == w.ifaces
    assert info.snap_bytes == w.snap_bytes
    assert info.flags == mgen_amd.PCAP_NG | (mgen_amd.PCAP_SWAPPED if w.swapped else 0)
    assert (info.link_type, info.snaplen) == (w.link_type, w.snaplen)
    return w, info


def test_symbols_declared_and_exported():
    import mgen_amd
    L = mgen_amd.load()
    for s in ("mgenx_pcapng_index", "mgenx_pcapng_parse", "mgenx_pcapng_snap"):
        assert s in mgen_amd.EXPORTED_SYMBOLS and hasattr(L, s)


@pytest.mark.parametrize("case", [
    dict(),
    dict(swapped=True, ifaces=({"tsresol": 9},)),
    dict(ifaces=({"tsresol": 0x8A}, {"tsresol": 3, "tsoffset": 1_000_000}), epb_options=True,
         unknown_blocks=True, second_section_at=130,
         kind=lambda i: "spb" if i % 11 == 3 else "opb" if i % 7 == 2 else "epb"),
    dict(snap=70, ifaces=({}, {"snaplen": 0}), swapped=True),
])
def test_index_matches_python_walk(oracle, case):
    c = dict(case)
    f = P.capture(oracle, seed=17, n=200)
    if "snap" in c:
        f = P.snap(f, c.pop("snap"))
    ng = G.from_pcap(f, seed=5, **c)
    w, info = _check(ng.file)
    assert info.status == G.OK and info.n_records == 200 and info.consumed == len(ng.file)
    if "second_section_at" in case:
        assert info.n_sections == 2 and info.n_ifaces == 4 and max(w.pkt_if) == 3
    if "snap" in case:
        assert info.snap_bytes > 0 and info.snaplen == 70


def test_index_fills_only_cap_entries():
    import mgen_amd
    e = "<"
    f = G.shb(e) + G.idb(e, 1) + G.idb(e, 1, tsresol=9) + b"".join(
        G.epb(e, i % 2, 5, fr) for i, (_, _, fr) in enumerate(_frames(6)))
    L = mgen_amd.load()
    info = mgen_amd.PcapngInfo()
    offs = np.full(4, 0xAA, np.uint64)
    pif = np.full(4, 0xAA, np.uint32)
    ifs = np.zeros(2, mgen_amd.PCAPNG_IF_DTYPE)
    ifs["snaplen"] = 0xAA
    b = np.frombuffer(f, np.uint8)
    P_ = ctypes.c_void_p
    rc = L.mgenx_pcapng_index(b.ctypes.data_as(P_), b.size, offs.ctypes.data_as(P_),
                              pif.ctypes.data_as(P_), 3, ifs.ctypes.data_as(P_), 1,
                              ctypes.byref(info))
    assert rc == 0 and info.n_records == 6 and info.n_ifaces == 2
    w = G.walk(f)
    assert list(offs[:3]) == w.offs[:3] and offs[3] == 0xAA and pif[3] == 0xAA
    assert ifs["snaplen"][0] == 0 and ifs["snaplen"][1] == 0xAA


def test_worked_time_stamps():
    """The four worked values of the time stamp rule."""
    assert G.ts_rule(1700000000123456789, *G.units(9)) == (1700000000, 123456)
    assert G.ts_rule(1700000000123, *G.units(3)) == (1700000000, 123000)
    assert G.ts_rule(1700000000 * 1024 + 513, *G.units(0x8A)) == (1700000000, 500976)
    assert G.ts_rule(5000007, *G.units(None), offset=1700000000) == (1700000005, 7)
    # the arithmetic is uint64 and wraps; rx_sec is the low 32 bits
    assert G.ts_rule(7, 10 ** 6, False, -1) == (0xFFFFFFFF, 7)
    assert G.ts_rule((1 << 63) + 5, 1 << 63, True) == (1, (5 * 10 ** 6) >> 63)
    assert G.ts_rule(10 ** 19 - 1, 10 ** 19) == (0, 999999)


def _stop_files():
    """(name, file, status, n_records, consumed) per stop rule 2-8."""
    e = "<"
    fr = [x[2] for x in _frames(5)]
    head = G.shb(e) + G.idb(e, 1, snaplen=96)
    pk = [G.epb(e, 0, 1_700_000_000_000_000 + i, fr[i]) for i in range(5)]
    three = head + b"".join(pk[:3])
    out = []

    def add(name, before, bad, status, n, after=None):
        out.append((name, before + bad + (pk[4] if after is None else after), status, n,
                    len(before)))

    other = ">"
    add("2 section of the other byte order", three, G.shb(other) + G.idb(other, 1), G.SECTION, 3)
    add("2 section with a bad magic", three, G.shb(e, magic=0x1A2B3C4E), G.SECTION, 3)
    add("2 section of major version 2", three, G.shb(e, major=2), G.SECTION, 3)
    add("3 another link type", three, G.idb(e, 113), G.LINKTYPE, 3)
    add("4 decimal exponent 20", three, G.idb(e, 1, tsresol=20), G.TSRESOL, 3)
    add("4 binary exponent 64", three, G.idb(e, 1, tsresol=0x80 | 64), G.TSRESOL, 3)
    add("4 if_tsresol of length 2", three,
        G.idb(e, 1, options=G.option(e, 9, b"\x06\x00") + G.end_of_options(e)), G.TSRESOL, 3)
    add("4 if_tsoffset of length 4", three,
        G.idb(e, 1, options=G.option(e, 14, bytes(4)) + G.end_of_options(e)), G.TSRESOL, 3)
    add("4 if_tsresol twice", three,
        G.idb(e, 1, options=G.option(e, 9, b"\x06") * 2 + G.end_of_options(e)), G.TSRESOL, 3)
    add("4 if_tsoffset twice", three,
        G.idb(e, 1, options=G.option(e, 14, bytes(8)) * 2 + G.end_of_options(e)), G.TSRESOL, 3)
    add("5 EPB on interface 1 of 1", three, G.epb(e, 1, 5, fr[3]), G.NO_IFACE, 3)
    add("5 OPB on interface 7", three, G.opb(e, 7, 5, fr[3]), G.NO_IFACE, 3)
    add("5 SPB in a section without interfaces", three + G.shb(e), G.spb(e, fr[3]), G.NO_IFACE, 3)
    room = len(G.pad4(fr[3]))
    add("6 caplen past the block", three, G.epb(e, 0, 5, fr[3], caplen=room + 1), G.CAPLEN, 3)
    add("7 EPB shorter than its head", three, G.block(e, G.EPB, bytes(16)), G.BLOCK, 3)
    add("7 SPB shorter than its head", three, G.block(e, G.SPB, b""), G.BLOCK, 3)
    add("7 total_len 8", three, G.block(e, 0x0BAD, b"", total=8), G.BLOCK, 3)
    add("7 total_len not a multiple of 4", three, G.block(e, 5, bytes(6)), G.BLOCK, 3)
    add("7 trailing length differs", three, G.block(e, G.EPB, G.epb(e, 0, 5, fr[3])[8:-4],
                                                    trailer=4), G.BLOCK, 3)
    add("7 IDB option past its block", three,
        G.idb(e, 1, options=G.option(e, 9, b"\x06", length=64)), G.BLOCK, 3)
    whole = three + pk[3]
    for cut in (1, 7, 8, 11, 27, 28, len(pk[4]) - 1):
        add(f"8 last block cut to {cut} bytes", whole, pk[4][:cut], G.TRUNCATED, 4, after=b"")
    add("8 a second SHB cut before its magic", whole, G.shb(e)[:10], G.TRUNCATED, 4, after=b"")
    return out


@pytest.mark.parametrize("name,f,status,n,consumed", _stop_files(),
                         ids=[x[0] for x in _stop_files()])
def test_stop_rules(name, f, status, n, consumed):
    """Rules 2-8: each stops the walk at the offending block and keeps the packets before."""
    w, info = _check(f)
    assert (info.status, info.n_records, info.consumed) == (status, n, consumed)


def test_accepted_variants():
    """What does not stop the walk: differing snaplens, an SPB's caplen cut to the snaplen of
    interface 0 and to the block, exponents at the limits, options without an end marker."""
    e = ">"
    fr = [x[2] for x in _frames(4, seed=9)]
    f = (G.shb(e) + G.idb(e, 1, snaplen=40, tsresol=19) + G.idb(e, 1, snaplen=0, tsresol=0x80 | 63)
         + G.idb(e, 1, options=G.option(e, 9, b"\x00")) + G.spb(e, fr[0])
         + G.spb(e, fr[1][:21], origlen=len(fr[1])) + G.epb(e, 2, 9, fr[2]) + G.epb(e, 1, 9, fr[3]))
    w, info = _check(f)
    assert info.status == G.OK and info.n_records == 4 and info.snaplen == 40
    assert [x[0] for x in w.ifaces] == [10 ** 19, 1 << 63, 1]
    assert w.packets[0][1] == 40 and w.packets[1][1] == 24     # snaplen; the padded block room


def test_not_pcapng():
    import mgen_amd
    e = "<"
    classic = P.pcap([(1, 2, _frames(1)[0][2])])
    for f in (classic, bytes(40), b"\x0a\x0d\x0d\x0a" + bytes(6), G.shb(e, major=2) + G.idb(e, 1),
              b"\x0a\x0d\x0d\x0a" + bytes(36), b""):
        assert G.walk(f) is None
        with pytest.raises(mgen_amd.MgenxError):
            mgen_amd.pcapng_index(f if f else np.zeros(0, np.uint8))
    assert mgen_amd.is_pcapng(G.shb(e)) and not mgen_amd.is_pcapng(classic)
    # the classic index still refuses a pcapng file (and zeros)
    with pytest.raises(mgen_amd.MgenxError):
        mgen_amd.pcap_index(G.shb(e) + G.idb(e, 1) + G.epb(e, 0, 5, _frames(1)[0][2]))
    with pytest.raises(mgen_amd.MgenxError):
        mgen_amd.pcap_index(b"\0" * 40)
    # a first SHB the file cuts short is a truncated pcapng file, not something else
    w, info = _check(G.shb(e)[:20])
    assert (info.status, info.n_records, info.consumed) == (G.TRUNCATED, 0, 0)


def test_walk_under_sanitizers(oracle, tmp_path):
    """tests/cpp/pcapng_host (address + undefined-behaviour sanitizers): the index over every
    prefix and over single-field mutations of a 40-packet capture with both byte orders'
    worth of block kinds; a sanitizer report exits non-zero."""
    if not os.path.exists(HOST):      # as the other tests/cpp programs: built on demand
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/pcapng_host"], check=True)
    assert os.path.exists(HOST), "tests/cpp/pcapng_host not built (make all)"
    f = P.snap(P.capture(oracle, seed=23, n=40), 200)
    for k, swapped in enumerate((False, True)):
        ng = G.from_pcap(f, swapped=swapped, ifaces=({"tsresol": 9}, {"tsoffset": 3}),
                         epb_options=True, unknown_blocks=True, second_section_at=25,
                         kind=lambda i: "spb" if i % 9 == 4 else "opb" if i % 5 == 1 else "epb")
        p = tmp_path / f"c{k}.pcapng"
        p.write_bytes(ng.file)
        r = subprocess.run([HOST, str(p)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        hist = dict(x.split() for x in r.stdout.splitlines()[1:])
        assert r.stdout.startswith(f"prefixes {len(ng.file) + 1} ")
        # the mutations reached the stop rules they aim at
        for s in ("ok", "truncated", "block", "no_iface", "caplen", "einval"):
            assert int(hist[s]) > 0, r.stdout
