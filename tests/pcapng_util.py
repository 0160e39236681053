"""pcapng captures for the pcap2mgen tests (test infrastructure).

A writer built byte by byte from the block layouts (Section Header, Interface Description,
Enhanced / obsolete / Simple Packet blocks, options), `from_pcap`, which re-emits a classic
capture of pcap_util as pcapng under a set of knobs, and `walk`, a pure-Python restatement of
the walk rules that the C index is compared with.

`from_pcap` also returns the equivalent classic file: the same frames with the (sec, usec)
the time stamp rule yields for each packet, as a native microsecond pcap.  That file is what
goes to the oracle, so an expected log never comes from the code under test.
"""
import struct
from collections import namedtuple

import numpy as np

import pcap_util as P

SHB, IDB, OPB, SPB, EPB = 0x0A0D0D0A, 1, 2, 3, 6
MAGIC = 0x1A2B3C4D
(OK, TRUNCATED, BLOCK, SECTION, LINKTYPE, NO_IFACE, TSRESOL, CAPLEN) = range(8)
M64 = 1 << 64


# ---------------------------------------------------------------- writer
def pad4(b: bytes) -> bytes:
    return b + bytes(-len(b) % 4)


def block(e, btype, body, total=None, trailer=None) -> bytes:
    """One block; total / trailer override the two length fields (malformed files)."""
    n = 12 + len(body)
    total = n if total is None else total
    trailer = total if trailer is None else trailer
    return struct.pack(e + "II", btype, total) + body + struct.pack(e + "I", trailer)


def option(e, code, value: bytes, length=None) -> bytes:
    return struct.pack(e + "HH", code, len(value) if length is None else length) + pad4(value)


def end_of_options(e) -> bytes:
    return struct.pack(e + "HH", 0, 0)


def shb(e, major=1, minor=0, options=b"", magic=MAGIC) -> bytes:
    return block(e, SHB, struct.pack(e + "IHHq", magic, major, minor, -1) + options)


def idb(e, link, snaplen=0, tsresol=None, tsoffset=None, options=None) -> bytes:
    """tsresol: the if_tsresol byte (9 = 10^-9, 0x8A = 2^-10); options: raw bytes instead."""
    if options is None:
        options = b""
        if tsresol is not None:
            options += option(e, 9, bytes([tsresol]))
        if tsoffset is not None:
            options += option(e, 14, struct.pack(e + "q", tsoffset))
        if options:
            options += end_of_options(e)
    return block(e, IDB, struct.pack(e + "HHI", link, 0, snaplen) + options)


def epb(e, iface, t, data, origlen=None, options=b"", caplen=None) -> bytes:
    origlen = len(data) if origlen is None else origlen
    caplen = len(data) if caplen is None else caplen
    return block(e, EPB, struct.pack(e + "IIIII", iface, t >> 32, t & 0xFFFFFFFF, caplen,
                                     origlen) + pad4(data) + options)


def opb(e, iface, t, data, origlen=None, options=b"") -> bytes:
    origlen = len(data) if origlen is None else origlen
    return block(e, OPB, struct.pack(e + "HHIIII", iface, 0, t >> 32, t & 0xFFFFFFFF, len(data),
                                     origlen) + pad4(data) + options)


def spb(e, data, origlen=None) -> bytes:
    origlen = len(data) if origlen is None else origlen
    return block(e, SPB, struct.pack(e + "I", origlen) + pad4(data))


# ---------------------------------------------------------------- the time stamp rule
def units(tsresol):
    """(units per second, binary) of an if_tsresol byte (None: the default 10^-6)."""
    if tsresol is None:
        return 10 ** 6, False
    return (1 << (tsresol & 0x7F), True) if tsresol & 0x80 else (10 ** tsresol, False)


def ts_rule(t, R, binary=False, offset=0):
    """A 64-bit time stamp of t units on an interface of R units per second -> (rx_sec,
    usec); uint64 arithmetic that wraps."""
    frac = t % R
    if R == 10 ** 6:
        usec = frac
    elif binary:
        usec = (frac * 10 ** 6 % M64) // R
    elif R > 10 ** 6:
        usec = frac // (R // 10 ** 6)
    else:
        usec = frac * (10 ** 6 // R) % M64
    return (t // R + offset) % M64 & 0xFFFFFFFF, usec & 0xFFFFFFFF


# ---------------------------------------------------------------- the walk rules in Python
Walk = namedtuple("Walk", "status n_records consumed offs pkt_if ifaces snap_bytes swapped "
                          "link_type snaplen n_sections packets")
# ifaces: (units, offset, snaplen, binary) per row; packets: (data_off, caplen, origlen, t)


def _idb_options(f, at, end, e):
    R, binary, offset, seen = 10 ** 6, False, 0, set()
    while end - at >= 4:
        code, ln = struct.unpack_from(e + "HH", f, at)
        if code == 0:
            break
        at += 4
        if end - at < ln:
            return BLOCK, None
        if code in (9, 14):
            if code in seen or ln != (1 if code == 9 else 8):
                return TSRESOL, None
            seen.add(code)
            if code == 9:
                v = f[at]
                if v & 0x80:
                    if v & 0x7F > 63:
                        return TSRESOL, None
                    R, binary = 1 << (v & 0x7F), True
                else:
                    if v > 19:
                        return TSRESOL, None
                    R, binary = 10 ** v, False
            else:
                offset = struct.unpack_from(e + "q", f, at)[0]
        at += (ln + 3) & ~3
    return OK, (R, offset, binary)


def walk(f: bytes):
    """The contract's walk over a file image; None where the C index returns MGENX_EINVAL."""
    nb = len(f)
    if nb < 12 or f[:4] != b"\x0a\x0d\x0d\x0a":
        return None
    magic = f[8:12]
    if magic == struct.pack("<I", MAGIC):
        e = "<"
    elif magic == struct.pack(">I", MAGIC):
        e = ">"
    else:
        return None
    minimum = {SHB: 28, IDB: 20, EPB: 32, OPB: 32, SPB: 16}
    off, status = 0, OK
    offs, pkt_if, ifaces, packets = [], [], [], []
    sec_base, n_sections, snap_bytes = 0, 0, 0
    link = snaplen = None
    while off < nb:
        left = nb - off
        if left < 8:
            status = TRUNCATED
            break
        btype, ln = struct.unpack_from(e + "II", f, off)
        if btype == SHB:
            if left < 12:
                status = TRUNCATED
                break
            if f[off + 8:off + 12] != magic:
                status = SECTION
                break
        if ln < minimum.get(btype, 12) or ln % 4:
            status = BLOCK
            break
        if left < ln:
            status = TRUNCATED
            break
        if struct.unpack_from(e + "I", f, off + ln - 4)[0] != ln:
            status = BLOCK
            break
        if btype == SHB:
            if struct.unpack_from(e + "H", f, off + 12)[0] != 1:
                if off == 0:
                    return None
                status = SECTION
                break
            n_sections += 1
            sec_base = len(ifaces)
        elif btype == IDB:
            lt, _, sl = struct.unpack_from(e + "HHI", f, off + 8)
            status, o = _idb_options(f, off + 16, off + ln - 4, e)
            if status != OK:
                break
            if link is not None and lt != link:
                status = LINKTYPE
                break
            if link is None:
                link, snaplen = lt, sl
            ifaces.append((o[0], o[1], sl, o[2]))
        elif btype in (EPB, OPB, SPB):
            if btype == SPB:
                iface, t = 0, 0
                origlen = struct.unpack_from(e + "I", f, off + 8)[0]
            else:
                iface = struct.unpack_from(e + ("I" if btype == EPB else "H"), f, off + 8)[0]
                hi, lo, caplen, origlen = struct.unpack_from(e + "IIII", f, off + 12)
                t = hi << 32 | lo
            if iface >= len(ifaces) - sec_base:
                status = NO_IFACE
                break
            if btype == SPB:
                snap0 = ifaces[sec_base][2]
                caplen = min(origlen, snap0 if snap0 else origlen, ln - 16)
            elif caplen > ln - 32:
                status = CAPLEN
                break
            if caplen < origlen:
                snap_bytes += (origlen + 15) & ~15
            offs.append(off)
            pkt_if.append(sec_base + iface)
            packets.append((off + (12 if btype == SPB else 28), caplen, origlen, t))
        off += ln
    return Walk(status, len(offs), off, offs, pkt_if, ifaces, snap_bytes, e == ">",
                link or 0, snaplen or 0, n_sections, packets)


def expected_records(f: bytes, w: Walk):
    """Per packet of a walk: (sec, usec, data, origlen) -- what a classic record of it holds."""
    out = []
    for (doff, caplen, origlen, t), row in zip(w.packets, w.pkt_if):
        R, offset, _, binary = w.ifaces[row]
        sec, usec = ts_rule(t, R, binary, offset)
        out.append((sec, usec, f[doff:doff + caplen], origlen))
    return out


def equivalent_pcap(f: bytes, w: Walk) -> bytes:
    return P.pcap([(s, u, d, len(d), o) for s, u, d, o in expected_records(f, w)],
                  link=w.link_type)


# ---------------------------------------------------------------- classic -> pcapng
def read_pcap(file: bytes):
    """A classic capture -> (link, snaplen, [(sec, nanoseconds, data, origlen)])."""
    magic = struct.unpack("<I", file[:4])[0]
    e, nsec = {0xA1B2C3D4: ("<", False), 0xD4C3B2A1: (">", False), 0xA1B23C4D: ("<", True),
               0x4D3CB2A1: (">", True)}[magic]
    snaplen, link = struct.unpack(e + "II", file[16:24])
    recs, off = [], 24
    while off + 16 <= len(file):
        sec, frac, cap, wire = struct.unpack(e + "IIII", file[off:off + 16])
        recs.append((sec, frac if nsec else frac * 1000, file[off + 16:off + 16 + cap], wire))
        off += 16 + cap
    return link, snaplen, recs


Ng = namedtuple("Ng", "file equiv walk")


def from_pcap(file: bytes, swapped=False, ifaces=({},), assign=None, kind=None,
              epb_options=False, unknown_blocks=False, second_section_at=None, seed=0) -> Ng:
    """Re-emit a classic capture as pcapng.
    ifaces: one dict per interface with tsresol (the if_tsresol byte), tsoffset (seconds),
    snaplen (default: the classic file's when it cut packets, else 0);
    assign(i) -> the interface of packet i (default: round robin);
    kind(i) -> "epb" / "opb" / "spb" (default: all EPBs; an SPB goes to interface 0 and
    carries no time stamp);
    epb_options: options (a comment, flags) after every other EPB's data;
    unknown_blocks: Name Resolution / Interface Statistics / unknown-type blocks in between;
    second_section_at: packet index at which a second section starts (same interfaces).
    Returns (pcapng file, equivalent classic file, the Python walk of the pcapng file)."""
    e = ">" if swapped else "<"
    rng = np.random.default_rng(seed)
    link, file_snap, recs = read_pcap(file)
    cut = any(len(d) < o for _, _, d, o in recs)
    head = [shb(e, options=option(e, 4, b"pcapng_util") + end_of_options(e))]
    for d in ifaces:
        head.append(idb(e, link, d.get("snaplen", file_snap if cut else 0), d.get("tsresol"),
                        d.get("tsoffset")))
    out = list(head)
    for i, (sec, ns, data, origlen) in enumerate(recs):
        if second_section_at is not None and i == second_section_at:
            out += head
        if unknown_blocks and i % 37 == 5:
            junk = bytes(rng.integers(0, 256, 4 * int(rng.integers(0, 9)), dtype=np.uint8))
            out.append(block(e, (4, 5, 0x00000BAD)[(i // 37) % 3], junk))
        k = kind(i) if kind else "epb"
        if k == "spb":
            out.append(spb(e, data, origlen))
            continue
        j = assign(i) if assign else i % len(ifaces)
        R, _ = units(ifaces[j].get("tsresol"))
        sub = int(rng.integers(0, 1000)) if R > 10 ** 6 else 0       # below a microsecond
        t = ((sec - ifaces[j].get("tsoffset", 0)) * R + (ns + sub) * R // 10 ** 9) % M64
        opts = b""
        if epb_options and i % 2:
            opts = (option(e, 1, b"packet %d" % i) + option(e, 2, struct.pack(e + "I", 1))
                    + end_of_options(e))
        out.append((epb if k == "epb" else opb)(e, j, t, data, origlen, options=opts))
    f = b"".join(out)
    w = walk(f)
    assert w is not None and w.status == OK and w.n_records == len(recs)
    return Ng(f, equivalent_pcap(f, w), w)
