"""MgenMsg::Unpack and the three receive rules in plain Python: a second statement of the
decode, written from the reference source (src/common/mgenMsg.cpp:315-500,
src/common/mgenTransport.cpp:960-975, 1516-1564, 1996-2031) and the wire diagram
(doc/mgen.xml:4619-4839), independent of the C restatement the other tests check against.
It imports nothing of the oracle; the CRC is zlib's.

The walk runs on a fresh message (constructor defaults: version 2, latitude and longitude
0.0 degrees = raw word 10800000, everything else zero) and stops where Unpack returns.  Two
conventions are the project's own:
  * bytes of dstAddr past the received length read as zero (Unpack itself does not bound
    dstAddrLen, :394-398: there they are whatever the receive buffer held before);
  * packet_header_len stays 0 when the walk ends between payload_type and payload_len
    (:482 has no else branch).
Addresses are kept as their first 16 bytes; dst_len / host_len are the wire bytes.
"""
import zlib

import numpy as np

MIN_SIZE = 28
VERSION = 2
TX_BUFFER_SIZE = 8192
ERROR_NONE, ERROR_VERSION, ERROR_CHECKSUM, ERROR_LENGTH, ERROR_DSTADDR = 0, 1, 2, 3, 4
CONTINUES, END_OF_MSG, CHECKSUM, LAST_BUFFER, CHECKSUM_ERROR = 0x01, 0x02, 0x04, 0x08, 0x10
GPS_RAW_ZERO = 10800000          # (0.0 + 180) * 60000

# the members every decode reports (same names and types as the checker's record)
FIELDS_DTYPE = np.dtype([
    ("ok", "u1"), ("err", "u1"), ("version", "u1"), ("flags", "u1"),
    ("msg_len", "<u2"), ("hdr_len", "<u2"),
    ("flow_id", "<u4"), ("seq_num", "<u4"), ("tx_sec", "<u4"), ("tx_usec", "<u4"),
    ("dst_port", "<u2"), ("dst_type", "u1"), ("dst_len", "u1"), ("dst_addr", "u1", 16),
    ("host_port", "<u2"), ("host_type", "u1"), ("host_len", "u1"), ("host_addr", "u1", 16),
    ("lat_raw", "<u4"), ("lon_raw", "<u4"), ("alt", "<i4"),
    ("gps_status", "u1"), ("payload_type", "u1"), ("payload_len", "<u2"),
    ("payload_off", "<u4"),
])

# where the walk returned (the `stage` entry of unpack()'s result, not a message member)
(R_LENGTH, R_VERSION, R_DSTADDR, R_NO_HOST, R_NO_HOST_ADDR, R_NO_GPS, R_NO_PTYPE, R_NO_PLEN,
 R_PAYLOAD_DROPPED, R_PAYLOAD_KEPT) = range(10)
RULES = ("udp", "udp_force", "tcp_force")


def _be(b, at, size):
    return int.from_bytes(b[at:at + size], "big")


def fresh():
    return {"ok": 0, "err": 0, "version": VERSION, "flags": 0, "msg_len": 0, "hdr_len": 0,
            "flow_id": 0, "seq_num": 0, "tx_sec": 0, "tx_usec": 0,
            "dst_port": 0, "dst_type": 0, "dst_len": 0, "dst_addr": bytes(16),
            "host_port": 0, "host_type": 0, "host_len": 0, "host_addr": bytes(16),
            "lat_raw": GPS_RAW_ZERO, "lon_raw": GPS_RAW_ZERO, "alt": 0,
            "gps_status": 0, "payload_type": 0, "payload_len": 0, "payload_off": 0}


def _addr16(b, at, n):
    """the first 16 of the n address bytes at b[at:], zero where the buffer has ended"""
    a = b[at:at + min(n, 16)]
    return a + bytes(16 - len(a))


def unpack(buf):
    """MgenMsg::Unpack(buf, len(buf)) on a fresh message: the members plus `stage`."""
    b = bytes(buf)
    n = len(b)
    m = fresh()

    def done(stage, ok=1):
        m["ok"], m["stage"] = ok, stage
        return m

    if n < MIN_SIZE:                                             # :323-328
        m["err"] = ERROR_LENGTH
        return done(R_LENGTH, 0)
    m["msg_len"] = _be(b, 0, 2)
    m["version"] = b[2]
    if m["version"] != VERSION:                                  # :336-343
        m["err"] = ERROR_VERSION
        return done(R_VERSION, 0)
    m["flags"] = b[3]
    m["flow_id"], m["seq_num"] = _be(b, 4, 4), _be(b, 8, 4)
    m["tx_sec"], m["tx_usec"] = _be(b, 12, 4), _be(b, 16, 4)
    dst_port = _be(b, 20, 2)
    if b[22] not in (1, 2):                                      # :374-392
        m["err"] = ERROR_DSTADDR
        return done(R_DSTADDR, 0)
    m["dst_type"], m["dst_len"], m["dst_port"] = b[22], b[23], dst_port
    m["dst_addr"] = _addr16(b, 24, b[23])                        # :394-398, no bound
    at = 24 + b[23]
    if at + 4 > n:                                               # :400, :441-446
        m["hdr_len"] = at
        return done(R_NO_HOST)
    host_port, host_type, host_len = _be(b, at, 2), b[at + 2], b[at + 3]
    at += 4
    if at + host_len > n:                                        # :425, :434-439
        m["hdr_len"] = at
        return done(R_NO_HOST_ADDR)
    if host_type in (1, 2):                                      # :427-431: else stays invalid
        m["host_type"], m["host_len"], m["host_port"] = host_type, host_len, host_port
        m["host_addr"] = _addr16(b, at, host_len)
    at += host_len
    if at + 13 > n:                                              # :449, :466-470
        m["hdr_len"] = at
        return done(R_NO_GPS)
    m["lat_raw"], m["lon_raw"] = _be(b, at, 4), _be(b, at + 4, 4)
    alt = _be(b, at + 8, 4)
    m["alt"] = alt - (1 << 32) if alt >> 31 else alt
    m["gps_status"] = b[at + 12]
    at += 13
    if at + 1 > n:                                               # :472, :476-480
        m["hdr_len"] = at
        return done(R_NO_PTYPE)
    m["payload_type"] = b[at]
    at += 1
    if at + 2 > n:                                               # :482: packet_header_len untouched
        return done(R_NO_PLEN)
    plen = _be(b, at, 2)
    at += 2
    m["hdr_len"] = at                                            # :487
    if plen != 0 and at + plen <= n:                             # :488-492
        m["payload_len"] = plen
        m["payload_off"] = (at // 4) * 4                         # alignedBuffer + len/4
        return done(R_PAYLOAD_KEPT)
    return done(R_PAYLOAD_DROPPED)                               # :493-497


def _crc_ok(b):
    return int.from_bytes(b[-4:], "big") == zlib.crc32(b[:-4])


def recv(rec, rule):
    """One received record under a receive rule (RULES):
    udp / udp_force  MgenUdpTransport::OnEvent, mgenTransport.cpp:958-975: the CRC over all
                     but the last four received bytes is compared with them only when Unpack
                     returned true and the CHECKSUM flag or the force option asks;
    tcp_force        MgenTcpTransport: Unpack sees the first min(L, 8192) bytes
                     (CopyMsgBuffer :2024-2027); CalcRxChecksum (:1516-1564) runs over the
                     whole L-byte message whatever Unpack returned, on the flags rx_msg then
                     holds or the force option, and a mismatch also sets CHECKSUM_ERROR
                     (:1546-1547).  A message shorter than its four-byte trailer has nothing
                     to compare and is left as Unpack reported it."""
    b = bytes(rec)
    force = rule != "udp"
    if rule == "tcp_force":
        m = unpack(b[:TX_BUFFER_SIZE])
        if len(b) >= 4 and (force or m["flags"] & CHECKSUM) and not _crc_ok(b):
            m["err"] = ERROR_CHECKSUM
            m["flags"] |= CHECKSUM_ERROR
        return m
    m = unpack(b)
    if m["ok"] and (force or m["flags"] & CHECKSUM) and not _crc_ok(b):
        m["err"] = ERROR_CHECKSUM
    return m


def recv_batch(records, rule):
    """(FIELDS_DTYPE array, stage array) of recv() over a list of records."""
    out = np.zeros(len(records), FIELDS_DTYPE)
    stage = np.zeros(len(records), np.uint8)
    for i, r in enumerate(records):
        m = recv(r, rule)
        stage[i] = m["stage"]
        for name in FIELDS_DTYPE.names:
            v = m[name]
            out[name][i] = np.frombuffer(v, np.uint8) if isinstance(v, bytes) else v
    return out, stage
