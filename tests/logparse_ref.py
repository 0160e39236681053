"""Plain-Python checker for the MGEN text log grammar ("text log ingest"; the line
format itself is doc/mgen.xml, "MGEN Log File Format"):

    <ts> SP+ <EVENT> (SP+ <key>'>'<value>)* SP* [CR] LF

Tokens are separated by runs of 0x20 only.  <ts> / sent> are "HH:MM:SS.uuuuuu" (HH < 24,
MM < 60, SS < 60) or "<u32>.uuuuuu"; an unsigned decimal is 1..10 digits and must fit its
field.  parse_line(bytes) returns a dict with the fields the device parser writes; a line
is OK iff its timestamp parses, its event is known, every required key is present and every
known key's value is valid.  Tests only: the product parser is mgen_amd/csrc/mgenx_logparse.hpp.
"""
EVENTS = ("RECV", "RERR", "SEND", "LISTEN", "IGNORE", "JOIN", "LEAVE", "START", "STOP", "ON",
          "ACCEPT", "DISCONNECT", "CONNECT", "OFF", "SHUTDOWN", "RECONNECT", "REPORT")
RECV, RERR, SEND = 1, 2, 3
OK, MALFORMED = 0, 1
HAS_HOST, HAS_TTL, HAS_GPS, HAS_DATA, HAS_FLAGS = 1, 2, 4, 8, 16
RX_LEGACY, TX_LEGACY = 1, 2
ERROR_NOT_RECV = 0x20
RERR_TYPES = {b"none": 0x40, b"version": 1, b"checksum": 2, b"length": 3, b"dstAddr": 4}
REQUIRED = {RECV: {"proto", "flow", "seq", "src", "dst", "sent", "size"},
            RERR: {"type", "src"},
            SEND: {"proto", "flow", "seq", "srcPort", "dst", "size"}}
DIGITS = b"0123456789"
HEX = b"0123456789abcdefABCDEF"
NO_ADDR = (0, 0, 0, bytes(16))


class Bad(Exception):
    pass


def _dec(s, maxv):
    if not 1 <= len(s) <= 10 or any(c not in DIGITS for c in s):
        raise Bad
    v = int(s)
    if v > maxv:
        raise Bad
    return v


def _fixed(s, k):
    if len(s) != k or any(c not in DIGITS for c in s):
        raise Bad
    return int(s)


def _ts(s):
    """(sec or time of day, usec, legacy)"""
    if len(s) == 15 and s[2:3] == b":":
        if s[5:6] != b":" or s[8:9] != b".":
            raise Bad
        h, m, sec, us = _fixed(s[0:2], 2), _fixed(s[3:5], 2), _fixed(s[6:8], 2), _fixed(s[9:], 6)
        if h > 23 or m > 59 or sec > 59:
            raise Bad
        return h * 3600 + m * 60 + sec, us, True
    if len(s) < 8 or s[-7:-6] != b".":
        raise Bad
    return _dec(s[:-7], 0xFFFFFFFF), _fixed(s[-6:], 6), False


def _ipv4(s):
    parts = s.split(b".")
    if len(s) > 15 or len(parts) != 4:
        raise Bad
    out = []
    for q in parts:
        if not 1 <= len(q) <= 3 or any(c not in DIGITS for c in q) or int(q) > 255:
            raise Bad
        out.append(int(q))
    return bytes(out)


def _ipv6(s):
    """What inet_ntop prints, read the way inet_pton reads it: groups of 1..4 hex digits, at
    most one '::', an optional dotted-decimal tail."""
    if len(s) > 45 or s.count(b"::") > 1 or b":::" in s:
        raise Bad
    tail = b""
    if b"." in s:
        cut = s.rfind(b":")
        if cut < 0:
            raise Bad
        tail = _ipv4(s[cut + 1:])
        s = s[:cut + 1]                     # ends with ':'
        if s.endswith(b"::"):
            pass
        else:
            s = s[:-1]
            if not s:
                raise Bad

    def groups(t):
        if not t:
            return b""
        out = b""
        for g in t.split(b":"):
            if not 1 <= len(g) <= 4 or any(c not in HEX for c in g):
                raise Bad
            out += int(g, 16).to_bytes(2, "big")
        return out

    if b"::" in s:
        a, b = s.split(b"::")
        head, rest = groups(a), groups(b) + tail
        if len(head) + len(rest) > 14:
            raise Bad
        return head + bytes(16 - len(head) - len(rest)) + rest
    full = groups(s) + tail
    if len(full) != 16:
        raise Bad
    return full


def _addr(s):
    """(type, len, port, 16 address bytes)"""
    cut = s.find(b"/")
    if cut < 0 or cut > 45:
        raise Bad
    port = _dec(s[cut + 1:], 65535)
    a = s[:cut]
    if b":" in a:
        return 2, 16, port, _ipv6(a)
    return 1, 4, port, _ipv4(a) + bytes(12)


def _deg(s):
    """%f text of raw / 60000 - 180 back to the raw word, in integers."""
    neg = s[:1] == b"-"
    if neg:
        s = s[1:]
    if len(s) < 8 or s[-7:-6] != b".":
        raise Bad
    micro = _dec(s[:-7], 9999999999) * 1000000 + _fixed(s[-6:], 6)
    if neg:
        micro = -micro
    t = (micro + 180000000) * 3
    if t < 0:
        raise Bad
    raw = (t + 25) // 50
    if raw > 0xFFFFFFFF:
        raise Bad
    return raw


def _gps(s):
    parts = s.split(b",")
    if len(parts) != 4:
        raise Bad
    status = {b"INVALID": 0, b"STALE": 1, b"CURRENT": 2}.get(parts[0])
    if status is None:
        raise Bad
    lat, lon = _deg(parts[1]), _deg(parts[2])
    a = parts[3]
    neg = a[:1] == b"-"
    alt = _dec(a[1:] if neg else a, 9999999999)
    alt = (-alt if neg else alt) & 0xFFFFFFFF
    return status, lat, lon, alt - (1 << 32) if alt >= 1 << 31 else alt


def _data(s):
    cut = s.find(b":")
    if cut < 0 or cut > 10:
        raise Bad
    n = _dec(s[:cut], 65535)
    h = s[cut + 1:]
    if len(h) != 2 * n or any(c not in HEX for c in h):
        raise Bad
    return bytes.fromhex(h.decode())


def blank():
    return dict(event=0, status=MALFORMED, protocol=0, present=0, kind=0, rx_sec=0, rx_usec=0,
                tx_sec=0, tx_usec=0, flow=0, seq=0, size=0, ttl=-1, flags=0, err=ERROR_NOT_RECV,
                gps=0, lat_raw=0, lon_raw=0, alt=0, data=b"", src=NO_ADDR, dst=NO_ADDR,
                host=NO_ADDR)


def parse_line(line: bytes) -> dict:
    r = blank()
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.endswith(b"\r"):
        line = line[:-1]
    if not line:
        r["status"] = OK
        return r
    cut = line.find(b" ")
    cut = len(line) if cut < 0 else cut
    ts_ok = True
    try:
        sec, usec, legacy = _ts(line[:cut])
        r["rx_sec"], r["rx_usec"] = sec, usec
        r["kind"] |= RX_LEGACY if legacy else 0
    except Bad:
        ts_ok = False
    toks = [t for t in line[cut:].split(b" ") if t]
    word = toks[0] if toks else b""
    names = [e.encode() for e in EVENTS]
    if word not in names:
        return r
    ev = r["event"] = names.index(word) + 1
    if not ts_ok:
        return r
    if ev not in (RECV, RERR, SEND):
        r["status"] = OK
        return r
    seen = set()
    rerr = 0
    try:
        for tok in toks[1:]:
            g = tok.find(b">")
            if g < 0:
                continue
            key, v = tok[:g].decode("latin-1"), tok[g + 1:]
            if ev == RERR:
                if key == "type":
                    if v not in RERR_TYPES:
                        raise Bad
                    rerr = RERR_TYPES[v]
                elif key == "src":
                    r["src"] = _addr(v)
                else:
                    continue
                seen.add(key)
                continue
            if key == "proto":
                r["protocol"] = {b"UDP": 1, b"TCP": 2, b"SINK": 3}.get(v, 0)
            elif key in ("flow", "seq", "size"):
                r[key] = _dec(v, 0xFFFFFFFF)
            elif key == "dst":
                r["dst"] = _addr(v)
            elif key == "host":
                r["host"] = _addr(v)
                r["present"] |= HAS_HOST
            elif ev == RECV and key == "src":
                r["src"] = _addr(v)
            elif ev == RECV and key == "sent":
                r["tx_sec"], r["tx_usec"], legacy = _ts(v)
                r["kind"] = (r["kind"] & ~TX_LEGACY) | (TX_LEGACY if legacy else 0)
            elif ev == RECV and key == "ttl":
                r["ttl"] = _dec(v, 255)
                r["present"] |= HAS_TTL
            elif ev == RECV and key == "gps":
                r["gps"], r["lat_raw"], r["lon_raw"], r["alt"] = _gps(v)
                r["present"] |= HAS_GPS
            elif ev == RECV and key == "data":
                r["data"] = _data(v)
                r["present"] |= HAS_DATA
            elif ev == RECV and key == "flags":
                if len(v) != 4 or v[:2] != b"0x" or any(c not in HEX for c in v[2:]):
                    raise Bad
                r["flags"] |= int(v[2:], 16)
                r["present"] |= HAS_FLAGS
            elif ev == SEND and key == "srcPort":
                r["src"] = (0, 0, _dec(v, 65535), bytes(16))
            else:
                continue
            seen.add(key)
    except Bad:
        return r
    if REQUIRED[ev] <= seen:
        r["status"] = OK
        r["err"] = 0 if ev == RECV else rerr if ev == RERR else ERROR_NOT_RECV
    return r


def split_lines(buf: bytes) -> list:
    """The lines of a buffer, each with its LF; a final piece without LF is a line."""
    out, at = [], 0
    while at < len(buf):
        end = buf.find(b"\n", at)
        end = len(buf) if end < 0 else end + 1
        out.append(buf[at:end])
        at = end
    return out


def parse_log(buf: bytes) -> list:
    return [parse_line(x) for x in split_lines(buf)]


def msg_len(r) -> int:
    return min(r["size"], 65535)
