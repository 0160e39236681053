"""Plain-Python model of binary log ingest (include/mgenx.h, mgenx_binlog_parse): one binary
log record -> the fields of its line, written from the record layouts (doc/mgen.xml, "Binary
Log File Format"; mgenMsg.cpp:1521-1891 for the record bodies, :315-500 for the stored message)
with ``struct``.  parse_record(bytes) returns a dict with logparse_ref.blank()'s keys.  Tests
only: the product decoder is mgen_amd/csrc/mgenx_binlogparse.hpp."""
import struct

import logparse_ref as R

RECV, SEND = 1, 3
ADDR_LEN = {1: 4, 2: 16}                 # IPv4, IPv6
ADDR_EVENTS = (1, 6, 7, 10, 11, 12, 13, 14, 15, 16)
WALK_NEXT, WALK_END = -1, -2
BINLOG_TOO_LONG, BINLOG_EVENT, BINLOG_SHORT = 2, 3, 4


def walk_step(rec: bytes, avail=None):
    """The record walk's rule at a record: (verdict, step)."""
    avail = len(rec) if avail is None else avail
    if avail < 4:
        return WALK_END, 0
    ev, _, rl = struct.unpack_from(">BBH", rec)
    if rl > 1024:
        return BINLOG_TOO_LONG, 0
    if 4 + rl > avail:
        return BINLOG_SHORT, 0
    if ev in (0, 2) or ev > 16:
        return BINLOG_EVENT, 0
    body = rec[4:4 + rl]
    # the fields each type reads: the event time; RECV 12 + source length; LISTEN / IGNORE
    # 12; JOIN / LEAVE 13 + group length + name length; ON ... RECONNECT 18 + address length
    need = 8
    if rl >= 8:
        if ev == 1:
            need = 12 + body[11] if rl >= 12 else 12
        elif ev in (4, 5):
            need = 12
        elif ev in (6, 7):
            need = 13
            if rl >= 13:
                need += body[11]
                if rl >= need:
                    need += body[12 + body[11]]
        elif ev >= 10:
            need = 18 + body[11] if rl >= 12 else 12
    if len(body) < need:
        return BINLOG_SHORT, 0
    if ev in ADDR_EVENTS and body[10] not in ADDR_LEN:
        return BINLOG_EVENT, 0
    return WALK_NEXT, 4 + rl


def _addr(atype, alen, port, raw):
    """An address of declared length alen whose bytes `raw` may have been cut short by the end
    of the message: the length stays as declared, the missing bytes read as zero."""
    return atype, alen, port, bytes(raw) + bytes(16 - len(raw))


def _message(m: bytes, r: dict, recv: bool) -> bool:
    """The stored message as MgenMsg::Unpack reads it; False when it is rejected."""
    if len(m) < 28:
        return False
    msg_len, version, flags, flow, seq, sec, usec, dport, dtype, dlen = struct.unpack_from(
        ">HBBIIIIHBB", m)
    if version != 2 or dtype not in ADDR_LEN or ADDR_LEN[dtype] != dlen:
        return False
    r["flow"], r["seq"], r["size"] = flow, seq, msg_len
    # Only the destination can be cut by the message's end (a 28-byte message holds 4 of an
    # IPv6 destination's 16 bytes): Unpack keeps the declared length and zero fill.  The host
    # address cannot (at + hlen > len(m) leaves the loop before it is read) and neither can
    # the source (the walk rule wants 12 + its length inside the record).
    r["dst"] = _addr(dtype, dlen, dport, m[24:24 + dlen])
    at = 24 + dlen
    gps, lat, lon, alt = 0, 10800000, 10800000, 0       # a fresh message: 0.0 degrees
    ptype, data = 0, b""
    while True:
        if at + 4 > len(m):
            break
        hport, htype, hlen = struct.unpack_from(">HBB", m, at)
        at += 4
        if at + hlen > len(m):
            break
        if htype in ADDR_LEN:
            if ADDR_LEN[htype] != hlen:
                return False
            r["host"] = _addr(htype, hlen, hport, m[at:at + hlen])
            r["present"] |= R.HAS_HOST
        at += hlen
        if at + 13 > len(m):
            break
        lat, lon, alt, gps = struct.unpack_from(">IIiB", m, at)
        at += 13
        if at + 1 > len(m):
            break
        ptype = m[at]
        at += 1
        if at + 2 > len(m):
            break
        plen, = struct.unpack_from(">H", m, at)
        at += 2
        if plen and at + plen <= len(m):
            start = at // 4 * 4                         # payload_data: the word-floored end
            data = m[start:start + plen]
        break
    if not recv:
        r["rx_sec"], r["rx_usec"] = sec, usec
        return True
    r["tx_sec"], r["tx_usec"] = sec, usec
    if gps > 2:
        return True
    r["present"] |= R.HAS_GPS
    r["gps"], r["lat_raw"], r["lon_raw"], r["alt"] = gps, lat, lon, alt
    if data and ptype == 0:
        r["present"] |= R.HAS_DATA
        r["data"] = data
    r["flags"] = flags & 0x13
    if r["flags"]:
        r["present"] |= R.HAS_FLAGS
    return True


def parse_record(rec: bytes) -> dict:
    r = R.blank()
    if len(rec) < 4:
        return r
    ev, proto, rl = struct.unpack_from(">BBH", rec)
    r["event"] = ev if ev <= 16 else 0
    if walk_step(rec)[0] != WALK_NEXT:
        return r
    body = rec[4:4 + rl]
    if ev == RECV:
        r["rx_sec"], r["rx_usec"], port, atype, alen = struct.unpack_from(">IIHBB", body)
        r["protocol"] = proto if proto in (1, 2, 3) else 0
        if ADDR_LEN[atype] != alen:
            return r
        r["src"] = _addr(atype, alen, port, body[12:12 + alen])
        if not _message(body[12 + alen:], r, True):
            return r
        r["status"], r["err"] = R.OK, 0
    elif ev == SEND:
        r["protocol"] = proto if proto in (1, 2, 3) else 0
        skip = 4 if proto == 2 else 0
        if not _message(body[skip:], r, False):
            return r
        if skip:
            r["size"], = struct.unpack_from(">I", body)
        r["status"] = R.OK
    else:
        r["rx_sec"], r["rx_usec"] = struct.unpack_from(">II", body)
        r["status"] = R.OK
    return r


def split_records(log: bytes, start: int) -> list:
    """The records of a well-formed log image from `start`, by their length fields."""
    out = []
    while start + 4 <= len(log):
        rl, = struct.unpack_from(">H", log, start + 2)
        out.append(log[start:start + 4 + rl])
        start += 4 + rl
    return out
