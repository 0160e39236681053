"""Binary log records written byte by byte (test infrastructure): the records the golden matrix
and the oracle's log writers never produce -- fields pushed across a record's 128th byte by an
unknown host type's length, record lengths around the 16-byte staging chunks, every cut of the
stored message, type / length mismatches and the edge values of every field.  ``struct`` only:
no oracle, no golden matrix.

Layout (doc/mgen.xml, "Binary Log File Format"):
  record   {type u8, protocol u8, recordLength BE u16} body
  RECV     sec u32, usec u32, srcPort u16, addrType u8, addrLen u8, address, stored message
  SEND     [mgen_msg_len u32 when protocol is TCP] stored message
  message  msg_len u16, version u8, flags u8, flow u32, seq u32, tx sec u32, tx usec u32,
           dst port u16, dst type u8, dst len u8, dst (D bytes), host port u16, host type u8,
           host len u8, host (H bytes), then the 16 trailer bytes lat u32, lon u32, alt i32,
           gps u8, payload type u8, payload len u16, then the payload
so a RECV's stored message starts at mo = 16 + alen, its host header at mo + 24 + D and its
trailer at T = mo + 28 + D + H."""
import struct

import binlog_util as B

V4, V6 = 1, 2
T0 = 1_700_000_000
LAT, LON, ALT = 0x11121314, 0x21222324, 0x31323334     # distinct non-zero trailer bytes
UNKNOWN_HOST = 7                                        # a host type that is neither 1 nor 2
TRAILER = 16


def ramp(n, start=1):
    """n non-zero bytes, no two neighbours alike."""
    return bytes((start + k) % 251 + 1 for k in range(n))


def v4(start=10):
    return (V4, 4, ramp(4, start))


def v6(start=40):
    return (V6, 16, ramp(16, start))


def message(*, version=2, flags=0, flow=7, seq=9, tx_sec=T0, tx_usec=123456, dst=None,
            dst_port=5000, host=None, host_port=6000, gps=(LAT, LON, ALT, 1), ptype=0,
            payload=b"", plen=None, pad=b"", msg_len=None, cut=None):
    """A stored message.  dst, host: (type, length field, bytes) -- the bytes go in as given,
    whatever the length field says.  plen: the payload length field (default: len(payload)).
    msg_len: the msg_len field (default: the whole message's length).  cut: keep only the
    first `cut` bytes (the fields keep their values)."""
    dst = v4() if dst is None else dst
    host = v4(20) if host is None else host
    lat, lon, alt, status = gps
    body = struct.pack(">BBIIIIHBB", version, flags, flow, seq, tx_sec, tx_usec, dst_port, dst[0],
                       dst[1]) + dst[2]
    body += struct.pack(">HBB", host_port, host[0], host[1]) + host[2]
    body += struct.pack(">IIiBBH", lat, lon, alt if alt < 1 << 31 else alt - (1 << 32), status,
                        ptype, len(payload) if plen is None else plen)
    body += payload + pad
    m = struct.pack(">H", 2 + len(body) if msg_len is None else msg_len) + body
    return m if cut is None else m[:cut]


def record(ev, proto, body, record_length=None):
    return struct.pack(">BBH", ev, proto,
                       len(body) if record_length is None else record_length) + body


def recv(msg, src=None, port=4321, proto=1, time=(T0 + 5, 654321)):
    src = v4(30) if src is None else src
    return record(1, proto, struct.pack(">IIHBB", time[0], time[1], port, src[0], src[1]) +
                  src[2] + msg)


def send(msg, proto=1, tcp_len=None):
    """A SEND record; protocol TCP stores mgen_msg_len (tcp_len, default the msg_len field)."""
    head = b""
    if proto == 2:
        head = struct.pack(">I", struct.unpack_from(">H", msg)[0] if tcp_len is None else tcp_len)
    return record(3, proto, head + msg)


def layout(rec: bytes):
    """(mo, D, H, T) of a RECV / SEND record whose stored message reaches its trailer, by the
    record's own length fields; None for another event or a message that ends before T + 16."""
    if rec[0] == 1:
        mo = 16 + rec[15]
    elif rec[0] == 3:
        mo = 8 if rec[1] == 2 else 4
    else:
        return None
    if mo + 24 > len(rec):
        return None
    D = rec[mo + 23]
    if mo + 28 + D > len(rec):
        return None
    H = rec[mo + 27 + D]
    T = mo + 28 + D + H
    return (mo, D, H, T) if T + TRAILER <= len(rec) else None


KINDS = ("recv4", "recv6", "send_udp", "send_tcp")


def _wrap(kind, msg):
    if kind == "recv4":
        return recv(msg, src=v4(30))
    if kind == "recv6":
        return recv(msg, src=v6(60))
    return send(msg, proto=1 if kind == "send_udp" else 2)


def _mo(kind):
    return {"recv4": 20, "recv6": 32, "send_udp": 4, "send_tcp": 8}[kind]


def straddle_cases():
    """Record offset 128 on every trailer byte: an unknown host type with
    H = 128 - j - (mo + 28 + D), for RECV (v4 / v4 and v6 / v6 source and destination) and UDP /
    TCP SEND (either destination).  GPS status 2 and plen = 0x0103 keep the trailer's bytes
    distinct and, but for the payload type, non-zero; the payload fits, so data_pos and data_len
    hang on a straddled field."""
    out = []
    pay = ramp(0x0103, 90)
    for kind in KINDS:
        for dst in ((v4(),) if kind == "recv4" else (v6(),) if kind == "recv6" else (v4(), v6())):
            for j in range(16):
                H = 128 - j - (_mo(kind) + 28 + dst[1])
                m = message(dst=dst, host=(UNKNOWN_HOST, H, ramp(H, 3 * j)), payload=pay,
                            gps=(LAT, LON, ALT, 2), seq=1000 + j)
                out.append((f"byte128:{kind}:D{dst[1]}:j{j}", _wrap(kind, m)))
    return out


def phase_cases():
    """H = 0, 1, 2, 3 and 255 with an unknown host type: everything up to the host length is
    shared, the payload's word-floored start lies 0 .. 3 bytes before the end of plen."""
    out = []
    for H in (0, 1, 2, 3, 255):
        m = message(host=(UNKNOWN_HOST, H, ramp(H, 70)), payload=ramp(0x0102, 5), msg_len=400)
        out.append((f"phase:recv4:H{H}", recv(m)))
        out.append((f"phase:send_tcp:H{H}", send(m, proto=2)))
    return out


CHUNK_LENGTHS = [16 * k + d for k in range(1, 10) for d in (-1, 0, 1)]     # 15 .. 145
RECV_MIN, RECV_FULL = 48, 72    # v4 source: a bare 28-byte header; header + v4 host + trailer


def length_cases():
    """Whole records of 16 k and 16 k +- 1 bytes up to 145: RECV from 48 bytes on (the stored
    message cut below 72 bytes, padded with payload above), other events below."""
    out = []
    for L in CHUNK_LENGTHS:
        if L >= RECV_FULL:
            rec = recv(message(payload=ramp(L - RECV_FULL, L), seq=L))
        elif L >= RECV_MIN:
            rec = recv(message(payload=ramp(8), seq=L, cut=L - 20))
        elif L == 16:
            rec = B.listen(T0, 16, 1, 5000)
        elif L < 21:
            rec = B.ev_time(8, T0, L, ramp(L - 12))            # START with bytes nobody reads
        else:
            rec = B.join(T0, L, bytes([224, 1, 2, 3]), 5000, ramp(L - 21, 96))
        assert len(rec) == L
        out.append((f"length:{L}", rec))
    out += [("short:start", B.start(T0, 1)), ("short:stop", B.stop(T0, 2)),
            ("short:listen", B.listen(T0, 3, 2, 5001, ignore=True)),
            ("short:join6", B.join(T0, 4, ramp(16, 9), 7, b"a-long-interface-name\0xx")),
            ("short:leave", B.join(T0, 5, bytes([239, 0, 0, 1]), leave=True)),
            ("short:on6", B.conn(10, T0, 6, ramp(16, 5), 4000, 5000, 3, host=(ramp(16, 77), 6000))),
            ("short:off4", B.conn(14, T0, 7, ramp(4, 5), 4000, 5000, 3))]
    return out


def largest_cases():
    """recordLength 1024 (the reference's read buffer) with the data> bytes filling it; the same
    with 1025 is TOO_LONG."""
    return [("largest:1028", recv(message(payload=ramp(1028 - RECV_FULL, 17), seq=1028))),
            ("too_long:1029", recv(message(payload=ramp(1029 - RECV_FULL, 18), seq=1029)))]


def cut_cases():
    """Every cut of a v6 / v6 / v6 stored message with a 40-byte payload, from 20 bytes to
    whole: below 28 Unpack rejects it, from 28 to 39 the destination is cut."""
    whole = message(dst=v6(), host=v6(100), payload=ramp(40, 200), flags=0x02)
    out = []
    for kind in ("recv6", "send_tcp", "send_udp"):
        for c in range(20, len(whole) + 1):
            out.append((f"cut:{kind}:{c}", _wrap(kind, whole[:c])))
    return out


def mismatch_cases():
    out = []
    for t, n in ((1, 16), (2, 4), (0, 4), (3, 16), (1, 0)):
        tag = "reject" if t not in (1, 2) else "mismatch"
        out.append((f"{tag}:dst:{t},{n}", recv(message(dst=(t, n, ramp(n, 50))))))
        out.append((f"{tag}:send_dst:{t},{n}", send(message(dst=(t, n, ramp(n, 50))), proto=2)))
    for t, n in ((1, 16), (2, 4), (1, 0)):
        out.append((f"mismatch:host:{t},{n}", recv(message(host=(t, n, ramp(n, 60))))))
        out.append((f"mismatch:send_host:{t},{n}", send(message(host=(t, n, ramp(n, 60))))))
    out.append(("mismatch:src:2,4", recv(message(), src=(2, 4, ramp(4, 30)))))
    out.append(("mismatch:src:1,16", recv(message(), src=(1, 16, ramp(16, 30)))))
    for ver in (1, 3):
        out.append((f"reject:version:{ver}", recv(message(version=ver))))
        out.append((f"reject:send_version:{ver}", send(message(version=ver))))
    return out


def value_cases():
    out = []
    pay = ramp(12, 33)
    for g in (0, 1, 2, 3, 255):
        out.append((f"value:gps:{g}", recv(message(gps=(LAT, LON, ALT, g), payload=pay))))
    out.append(("value:gps:negative_alt", recv(message(gps=(1, 0xFFFFFFFF, -5, 2), payload=pay))))
    for p in (0, 1, 255):
        out.append((f"value:ptype:{p}", recv(message(ptype=p, payload=pay))))
    out.append(("value:plen:0", recv(message(payload=b"", pad=pay))))
    out.append(("value:plen:exact", recv(message(payload=pay))))
    out.append(("value:plen:one_past", recv(message(payload=pay, plen=len(pay) + 1))))
    out.append(("value:plen:padded", recv(message(payload=pay, pad=ramp(5)))))
    for f in (0x00, 0x01, 0x02, 0x10, 0x0C, 0xFF):
        out.append((f"value:flags:{f:#04x}", recv(message(flags=f, payload=pay))))
    for p in (0, 1, 2, 3, 4, 255):
        out.append((f"value:proto:recv:{p}", recv(message(payload=pay), proto=p)))
        out.append((f"value:proto:send:{p}", send(message(payload=pay), proto=p)))
    for n in (0, 65535):
        out.append((f"value:msg_len:recv:{n}", recv(message(msg_len=n, payload=pay))))
        out.append((f"value:msg_len:send:{n}", send(message(msg_len=n, payload=pay))))
    for n in (65536, 0xFFFFFFFF):
        out.append((f"value:tcp_len:{n}", send(message(payload=pay), proto=2, tcp_len=n)))
    out.append(("tx_usec>=1e6:recv", recv(message(tx_usec=2_000_000, payload=pay))))
    out.append(("tx_usec>=1e6:send", send(message(tx_usec=2_000_000, payload=pay))))
    out.append(("value:host6", recv(message(host=v6(100), dst=v6(), payload=pay), src=v6(60))))
    return out


def crafted():
    """The whole corpus as (name, record bytes), the same list every time.  The TOO_LONG record
    comes last: a record walk stops there, so everything before it is walked."""
    out = (straddle_cases() + phase_cases() + length_cases() + cut_cases() + mismatch_cases() +
           value_cases() + largest_cases())
    assert len({name for name, _ in out}) == len(out) and out[-1][0] == "too_long:1029"
    return out


def edge_log():
    """A log image without a header line for the every-offset and buffer-end tests:
    (bytes, record offsets, names).  A spread of the crafted records (no TOO_LONG one), then
    the 1028-byte record, a 129-byte RECV and a START at the very end."""
    keep = []
    for name, rec in crafted():
        part = name.split(":")
        if part[0] == "byte128" and part[3] not in ("j0", "j7", "j14", "j15"):
            continue
        if part[0] == "cut" and not (26 <= int(part[2]) <= 41 or int(part[2]) % 8 == 0):
            continue
        if part[0] in ("largest", "too_long") or name == "length:129":
            continue
        keep.append((name, rec))
    by_name = dict(crafted())
    keep += [(k, by_name[k]) for k in ("largest:1028", "length:129", "short:start")]
    buf, offs = pack([rec for _, rec in keep])
    return buf, offs, [name for name, _ in keep]


def owned(buf: bytes, at: int, nbytes=None) -> bytes:
    """The bytes the contract says a record at offset `at` owns:
    buf[at : min(at + 4 + recordLength, nbytes)]; nothing when fewer than 4 bytes remain."""
    nbytes = len(buf) if nbytes is None else nbytes
    if at < 0 or at >= nbytes or nbytes - at < 4:
        return b""
    rl, = struct.unpack_from(">H", buf, at + 2)
    return buf[at:min(at + 4 + rl, nbytes)]


def pack(records, pads=None, fill=0xEE):
    """The records laid into one buffer, pads[k] bytes of `fill` before record k:
    (buffer bytes, the records' offsets)."""
    buf, offs = bytearray(), []
    for k, rec in enumerate(records):
        if pads is not None:
            buf += bytes([fill]) * pads[k]
        offs.append(len(buf))
        buf += rec
    return bytes(buf), offs
