"""Crafted header layouts for the unpack kernels (test_gpu_unpack_layouts.py), built here so
that the CPU suite (test_wire_model_cpu.py) can assert from the model alone that every corpus
holds what it is meant to hold.  MgenMsg::Unpack takes dstAddrLen and hostAddrLen from the
wire unbounded and accepts any hostAddrType (mgenMsg.cpp:394-433); records that a sender
packed never carry such values, so these are written byte by byte.  Everything is
deterministic, cached and read-only."""
import functools
import zlib

import numpy as np

CHECKSUM, CONTINUES = 0x04, 0x01
DST_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 20, 36, 100, 231, 255)
HOST_LENS = (0, 1, 3, 4, 5, 8, 13, 16, 17, 20, 40, 255)
LATTICE_N = len(DST_LENS) * len(HOST_LENS)          # 204
LATTICE_SIZES = (65, 128, 301, 512, 1024, 4099)
GENERAL_SIZES = (65, 128, 301, 512)                 # the lattices of the GENERAL batch
FILL = 0xA5                                         # gap and tail bytes of a slab


def _cycle(values, period):
    """`values` repeated to `period` entries: the fields of a lattice record cycle with the
    record index at the periods 2, 3, 5, 7, 11, 13, 17, 19 (pairwise coprime), so that no two
    fields stay locked together."""
    return [values[k % len(values)] for k in range(period)]


DST_TYPES = _cycle((1, 2), 2)
PAYLOAD_TYPES = _cycle((0, 1, 255), 3)
HOST_TYPES = _cycle((0, 1, 2, 3, 255), 5)
GPS_STATUS = _cycle((0, 1, 2, 3, 255), 7)
PAYLOAD_LENS = _cycle(("zero", "one", "room", "room+1", "room-4", "max"), 11)
MSG_SIZES = _cycle(("L", "L-1", "L+1", "zero", "max"), 13)
FLAGS = _cycle((0, CHECKSUM, CHECKSUM, CHECKSUM | CONTINUES), 17)
TRAILERS = _cycle(("valid", "valid", "bit", "random"), 19)


def _put(rec, at, value, size):
    """big-endian `value` at rec[at:at + size]; the part of it past the record is not written"""
    raw = int(value & ((1 << (8 * size)) - 1)).to_bytes(size, "big")
    room = max(0, min(size, len(rec) - at))
    rec[at:at + room] = raw[:room]


def _trailer(rec, kind, bit=0):
    """the last four bytes: the CRC of the rest (valid), that with one bit wrong, or as is"""
    if kind == "random" or len(rec) < 4:
        return
    crc = zlib.crc32(bytes(rec[:-4]))
    if kind == "bit":
        crc ^= 1 << (bit % 32)
    rec[-4:] = crc.to_bytes(4, "big")


@functools.lru_cache(maxsize=None)
def lattice(L):
    """204 records of exactly L bytes: every (dstAddrLen, hostAddrLen) pair of DST_LENS x
    HOST_LENS once, the other crafted fields cycling with the record index, every other byte
    random and never zero, the trailer recomputed after the header was written."""
    rng = np.random.default_rng(0x1A77 + L)
    out = []
    for i in range(LATTICE_N):
        D, H = DST_LENS[i // len(HOST_LENS)], HOST_LENS[i % len(HOST_LENS)]
        k = i + L                   # the lattices of different L start their cycles apart
        rec = bytearray(rng.integers(1, 256, L, dtype=np.uint8).tobytes())
        end = 44 + D + H            # where payload_len ends
        room = L - end
        size = {"L": L, "L-1": L - 1, "L+1": L + 1, "zero": 0, "max": 65535}[MSG_SIZES[k % 13]]
        plen = {"zero": 0, "one": 1, "room": room, "room+1": room + 1, "room-4": room - 4,
                "max": 65535}[PAYLOAD_LENS[k % 11]]
        _put(rec, 0, size, 2)
        _put(rec, 2, 2, 1)
        _put(rec, 3, FLAGS[k % 17], 1)
        _put(rec, 22, DST_TYPES[k % 2], 1)
        _put(rec, 23, D, 1)
        _put(rec, 24 + D + 2, HOST_TYPES[k % 5], 1)
        _put(rec, 24 + D + 3, H, 1)
        _put(rec, 28 + D + H + 12, GPS_STATUS[k % 7], 1)
        _put(rec, 28 + D + H + 13, PAYLOAD_TYPES[k % 3], 1)
        _put(rec, 28 + D + H + 14, max(plen, 0), 2)
        _trailer(rec, TRAILERS[k % 19], bit=i)
        assert len(rec) == L
        out.append(bytes(rec))
    return tuple(out)


LADDER_LAYOUTS = tuple((d, h) for d in (4, 16) for h in (0, 4, 16))
LADDER_PAYLOAD = 20


def _well_formed(D, H, seq):
    """a complete record with a 20-byte payload: dst IPv4 / IPv6, host none / IPv4 / IPv6"""
    rng = np.random.default_rng(0x1ADD + 16 * D + H)
    L = 44 + D + H + LADDER_PAYLOAD
    rec = bytearray(rng.integers(1, 256, L, dtype=np.uint8).tobytes())
    _put(rec, 0, L, 2)
    _put(rec, 2, 2, 1)
    _put(rec, 3, CHECKSUM, 1)
    _put(rec, 8, seq, 4)
    _put(rec, 22, 1 if D == 4 else 2, 1)
    _put(rec, 23, D, 1)
    _put(rec, 24 + D + 2, {0: 0, 4: 1, 16: 2}[H], 1)
    _put(rec, 24 + D + 3, H, 1)
    _put(rec, 28 + D + H + 12, 2, 1)
    _put(rec, 28 + D + H + 13, 0, 1)
    _put(rec, 28 + D + H + 14, LADDER_PAYLOAD, 2)
    return rec


@functools.lru_cache(maxsize=None)
def ladder():
    """The six well-formed records cut at every received length from 0 to the full one (490
    records); every second length of 32 or more carries a valid trailer for that length.
    Returns (records, layout index of each)."""
    out, layout = [], []
    for j, (D, H) in enumerate(LADDER_LAYOUTS):
        full = _well_formed(D, H, j)
        for cut in range(len(full) + 1):
            rec = bytearray(full[:cut])
            if cut >= 32 and cut % 2 == 0:
                _trailer(rec, "valid")
            out.append(bytes(rec))
            layout.append(j)
    return tuple(out), tuple(layout)


@functools.lru_cache(maxsize=None)
def plain_errors():
    """three plain records Unpack refuses: a wrong version, dst types 0 and 7"""
    out = []
    for version, dst_type in ((3, 1), (2, 0), (2, 7)):
        rec = _well_formed(4, 0, 100 + dst_type)
        _put(rec, 2, version, 1)
        _put(rec, 22, dst_type, 1)
        _trailer(rec, "valid")
        out.append(bytes(rec))
    return tuple(out)


# Regression cases: a record on which a kernel once disagreed with the reference goes here
# by name, {name: record bytes}, and rides in general_batch() from then on.
REGRESSIONS = {}


@functools.lru_cache(maxsize=None)
def general_batch(sizes=GENERAL_SIZES):
    """the GENERAL batch: the lattices of `sizes`, the ladder, the plain errors and the
    regression records, in that order"""
    recs = [r for L in sizes for r in lattice(L)]
    recs += ladder()[0]
    recs += plain_errors()
    recs += [REGRESSIONS[k] for k in sorted(REGRESSIONS)]
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def long_extra():
    """8,200 bytes, IPv4 dst, no host, payloadLen exactly the room left (8,152), valid
    trailer: the payload fits the received bytes, but not the 8,192 a TCP receiver unpacks"""
    L = 8200
    rng = np.random.default_rng(0x10E6)
    rec = bytearray(rng.integers(1, 256, L, dtype=np.uint8).tobytes())
    _put(rec, 0, L, 2)
    _put(rec, 2, 2, 1)
    _put(rec, 3, CHECKSUM, 1)
    _put(rec, 22, 1, 1)
    _put(rec, 23, 4, 1)
    _put(rec, 30, 0, 2)
    _put(rec, 44, 0, 2)                     # gps status INVALID, payload type 0
    _put(rec, 46, L - 48, 2)
    _trailer(rec, "valid")
    return bytes(rec)


def place(records, kind):
    """A slab of the records in one of two layouts, gaps and a 64-byte tail of 0xA5 (never
    zero: a read past a record's length shows up as a wrong field):
      "offsets"  unaligned: first offset 3, a gap of i mod 7 bytes before record i + 1;
                 returns (slab, rec_off u64, rec_len u32);
      "stride"   back to back, one length; returns (slab, stride)."""
    if kind == "stride":
        L = len(records[0])
        assert all(len(r) == L for r in records)
        body = np.frombuffer(b"".join(records), np.uint8)
        return np.concatenate([body, np.full(64, FILL, np.uint8)]), L
    assert kind == "offsets"
    lens = np.array([len(r) for r in records], np.uint32)
    gaps = np.arange(len(records)) % 7
    offs = np.zeros(len(records), np.uint64)
    offs[0] = 3
    offs[1:] = 3 + np.cumsum(lens[:-1].astype(np.uint64) + gaps[:-1].astype(np.uint64))
    slab = np.full(int(offs[-1]) + int(lens[-1]) + 64, FILL, np.uint8)
    for r, o in zip(records, offs):
        slab[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    return slab, offs, lens


def fast_layout(rec):
    """The register-only decode's predicate as the dispatch applies it to a record of
    len(rec) received bytes (a Python copy, kept beside the tests on purpose): at least 64
    bytes, version 2, dst type 1 or 2, dst length 4 or 16, host length 0, 4 or 16 and dst +
    host at most 20 bytes."""
    if len(rec) < 64:
        return False
    D = rec[23]
    if rec[2] != 2 or rec[22] not in (1, 2) or D not in (4, 16):
        return False
    H = rec[24 + D + 3]
    return H in (0, 4, 16) and D + H <= 20


def interleaved_index():
    """Where interleaved() puts what: (n, {index: lattice record}) -- lattice record j at
    17 j (every position of a 16-record group and every quad lane, beside fillers), the rest
    of that part filled to a whole group; then 16 consecutive lattice records that are not
    fast layouts, 16 fillers, and three trailing records (lattice, filler, lattice), so the
    last group is partial.  interleaved() spoils the first two of those three: see there."""
    at = {17 * j: j for j in range(LATTICE_N)}
    n = (17 * (LATTICE_N - 1) + 1 + 15) // 16 * 16
    slow = [j for j in range(LATTICE_N)
            if (DST_LENS[j // len(HOST_LENS)], HOST_LENS[j % len(HOST_LENS)])
            not in ((4, 0), (4, 4), (4, 16), (16, 0), (16, 4))]
    for k in range(16):
        at[n + k] = slow[(k * 11) % len(slow)]
    n += 32
    at[n], at[n + 2] = slow[100], slow[150]
    return n + 3, at


def interleaved(L, filler):
    """The batch for the quad-broadcast kernels (see interleaved_index): `filler` is an
    [n, L] array of ordinary packed records of L bytes; returns the [n, L] records.  Of the
    three trailing records the lattice one gets version 3 and the filler dst type 0: Unpack
    refuses both before it assigns dst_len (a non-zero wire byte in both), so they are the
    records on which the fast decode's dst_len and the parsed one differ."""
    n, at = interleaved_index()
    recs = np.array(filler[:n], np.uint8)
    assert recs.shape == (n, L)
    lat = lattice(L)
    for i, j in at.items():
        recs[i] = np.frombuffer(lat[j], np.uint8)
    recs[n - 3, 2] = 3
    recs[n - 2, 22] = 0
    return recs


def fillers(oracle, gold, n, L, seed=0):
    """n ordinary records of L bytes packed by the checker's send path over the golden
    templates (IPv4 / IPv6 dst, host addresses, payloads), checksum on: [n, L]"""
    rng = np.random.default_rng(0xF111 + L + seed)
    desc = np.zeros(n, gold["desc"].dtype)
    desc["tmpl"] = rng.integers(0, len(gold["tmpl"]), n)
    desc["seq_num"] = np.arange(n) * 5 + 2
    desc["tx_sec"] = 1_700_000_000 + np.arange(n) // 64
    desc["tx_usec"] = rng.integers(0, 1_000_000, n)
    desc["msg_len"] = L
    desc["flags"] = rng.choice([0, 4], n)
    a, _ = oracle.udp_pack_batch(gold["tmpl"], desc, gold["pool"], n * L, stride=L, checksum=True)
    return a.reshape(n, L)


# ---- source addresses of the log lines (inet_ntop's IPv6 zero-run rules) ----
def ipv6_sources():
    """16-byte IPv6 addresses: all 256 patterns of zero and non-zero 16-bit groups, then
    ::, ::1, ::2, ::ffff:a.b.c.d, ::a.b.c.d, ::fffe:x:y, a run ending at group 7 and two
    equal runs."""
    out = []
    for mask in range(256):
        g = [0 if mask >> k & 1 else 0x1000 + 0x111 * k + mask for k in range(8)]
        out.append(b"".join(x.to_bytes(2, "big") for x in g))
    def groups(*g):
        return b"".join(x.to_bytes(2, "big") for x in g)
    out += [groups(0, 0, 0, 0, 0, 0, 0, 0), groups(0, 0, 0, 0, 0, 0, 0, 1),
            groups(0, 0, 0, 0, 0, 0, 0, 2), groups(0, 0, 0, 0, 0, 0xFFFF, 0x0A01, 0x0203),
            groups(0, 0, 0, 0, 0, 0, 0xC0A8, 0x0009), groups(0, 0, 0, 0, 0, 0xFFFE, 0x1234, 0x5678),
            groups(0x2001, 0xDB8, 1, 0, 0, 0, 0, 0), groups(1, 0, 0, 2, 3, 0, 0, 4),
            groups(0, 0, 1, 2, 3, 4, 0, 0), groups(0, 0, 0, 0, 0, 0, 1, 2)]
    return out
