"""IP fragmentation for the pcap2mgen tests (test infrastructure).

`fragment_v4` / `fragment_v6` cut an IP datagram into fragments at an MTU, `capture` builds
pcap_util-style flows of large messages and returns the capture twice -- unfragmented and
fragmented, each unfragmented frame at its last fragment's time, TTL and position -- and
`frag_ref` is the serial model of the reassembly contract (include/mgenx.h):
plain Python per packet, written from the contract's text, sharing no code with the product.
"""
import struct
from collections import namedtuple

import numpy as np

import pcap_util as P

UDP, BAD_IP, NOT_UDP, TRUNCATED, FRAGMENT = 0, 3, 4, 5, 8
MAX_FRAGS = 64


def be16(b, i):
    return b[i] << 8 | b[i + 1]


# ---------------------------------------------------------------- the fragmenters
def frag_v4(hdr: bytes, payload: bytes, off: int, mf: bool, ident: int, ttl=None) -> bytes:
    """One IPv4 fragment: hdr (an IPv4 header, options included) re-issued around payload."""
    h = bytearray(hdr)
    struct.pack_into(">H", h, 2, len(hdr) + len(payload))
    struct.pack_into(">HH", h, 4, ident, (0x2000 if mf else 0) | off >> 3)
    if ttl is not None:
        h[8] = ttl
    return bytes(h) + payload


def frag_v6(hdr: bytes, payload: bytes, off: int, mf: bool, ident: int, hops=None,
            inner=17) -> bytes:
    """One IPv6 fragment: the fixed header hdr, a Fragment extension header, payload."""
    h = bytearray(hdr[:40])
    struct.pack_into(">H", h, 4, 8 + len(payload))
    h[6] = 44
    if hops is not None:
        h[7] = hops
    return bytes(h) + struct.pack(">BBHI", inner, 0, off | (1 if mf else 0), ident) + payload


def fragment_v4(ip_datagram: bytes, mtu: int, ident: int, early_ttl=None):
    """The fragments (IPv4 packets) of an IPv4 datagram at an MTU, in order; early_ttl: the TTL
    of every fragment but the last."""
    ihl = (ip_datagram[0] & 15) * 4
    hdr, pay = ip_datagram[:ihl], ip_datagram[ihl:]
    step = (mtu - ihl) & ~7
    cuts = list(range(0, len(pay), step))
    return [frag_v4(hdr, pay[o:o + step], o, o != cuts[-1], ident,
                    early_ttl if o != cuts[-1] else None) for o in cuts]


def fragment_v6(ip_datagram: bytes, mtu: int, ident: int, early_ttl=None):
    hdr, pay = ip_datagram[:40], ip_datagram[40:]
    step = (mtu - 48) & ~7
    cuts = list(range(0, len(pay), step))
    return [frag_v6(hdr, pay[o:o + step], o, o != cuts[-1], ident,
                    early_ttl if o != cuts[-1] else None, inner=ip_datagram[6]) for o in cuts]


def fragment(ip_datagram: bytes, mtu: int, ident: int, early_ttl=None):
    f = fragment_v4 if ip_datagram[0] >> 4 == 4 else fragment_v6
    return f(ip_datagram, mtu, ident, early_ttl)


def payloads(frags):
    """(off, MF, payload) of each fragment of fragment_v4 / fragment_v6."""
    out = []
    for f in frags:
        if f[0] >> 4 == 4:
            ihl, F = (f[0] & 15) * 4, be16(f, 6)
            out.append(((F & 0x1FFF) * 8, bool(F & 0x2000), f[ihl:be16(f, 2)]))
        else:
            F = be16(f, 42)
            out.append((F & 0xFFF8, bool(F & 1), f[48:40 + be16(f, 4)]))
    return out


def link_frame(ip: bytes, link=1, vlan=None) -> bytes:
    return P.sll(ip) if link == 113 else P.eth(ip, vlan=vlan)


# ---------------------------------------------------------------- captures of large messages
SRC4 = [bytes([10, 0, 0, k]) for k in (5, 6, 7)]
DST4 = bytes([10, 0, 0, 2])
SRC6 = [bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [k]) for k in (1, 2)]
DST6 = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [0x99])


def datagram(O, flow, seq, t_us, size, v6=False, ttl=64, gps=False, lag=1500):
    """The IP datagram of one MGEN message of `size` bytes sent lag microseconds before t_us."""
    tx = divmod(t_us - lag, 1_000_000)
    if v6:
        pay = P.mgen_payload(O, flow, seq, tx, size, ("6", DST6, 6000 + flow), gps=gps)
        return P.ipv6(P.udp(pay, 40000 + flow, 6000 + flow), SRC6[flow % 2], DST6, hops=ttl)
    pay = P.mgen_payload(O, flow, seq, tx, size, ("4", DST4, 5000 + flow), gps=gps)
    return P.ipv4(P.udp(pay, 30000 + flow, 5000 + flow), SRC4[flow % 3], DST4, ttl=ttl)


def capture(O, seed, n=40, link=1, v6=False, mtu=1500, vlan=None, lo=1500, hi=3900,
            small=True):
    """n messages of lo..hi bytes in four flows (loss, late copies, with `small` a few
    unfragmented ones, an ARP between) -> (unfragmented pcap, fragmented pcap): every frame above the MTU
    is replaced by its fragments in order; the last fragment has the frame's time and TTL,
    the ones before it are a few microseconds earlier with another TTL."""
    rng = np.random.default_rng(seed)
    whole, cut, seqs = [], [], {}
    t_us = 1_700_000_000 * 1_000_000 + 250_000
    for i in range(n):
        t_us += int(rng.integers(200, 9000))
        flow = int(rng.integers(1, 5))
        seq = seqs.get(flow, 0)
        r = rng.random()
        seqs[flow] = seq + (2 if r < 0.05 else 1)
        if r > 0.95:
            seq = max(0, seq - 2)
        size = int(rng.integers(64, 900)) if small and i % 7 == 3 else int(rng.integers(lo, hi + 1))
        ttl = int(rng.integers(2, 250))
        if i % 11 == 5:
            frame = P.eth(bytes(28), etype=0x0806) if link != 113 else P.sll(bytes(28), 0x0806)
            frames = [frame]
        else:
            ip = datagram(O, flow, seq, t_us, size, v6, ttl, gps=rng.random() < 0.5,
                          lag=int(rng.integers(100, 5000)))
            frame = link_frame(ip, link, vlan)
            frames = [frame]
            if len(ip) > mtu:
                frames = [link_frame(f, link, vlan)
                          for f in fragment(ip, mtu, 0x4000 + i, early_ttl=ttl + 1)]
        sec, usec = divmod(t_us, 1_000_000)
        whole.append((sec, usec, frame))
        for k, f in enumerate(frames):
            s, u = divmod(t_us - (len(frames) - 1 - k) * 3, 1_000_000)
            cut.append((s, u, f))
    return P.pcap(whole, link=link), P.pcap(cut, link=link)


def records(file: bytes):
    """A native microsecond pcap -> [(sec, usec, data, origlen)]."""
    out, off = [], 24
    while off + 16 <= len(file):
        sec, usec, cap, wire = struct.unpack("<IIII", file[off:off + 16])
        out.append((sec, usec, file[off + 16:off + 16 + cap], wire))
        off += 16 + cap
    return out


# ---------------------------------------------------------------- the serial model
def classify(data: bytes, origlen: int, link: int):
    """The contract's 'which packets are fragments' for one packet: None (not examined or not a
    fragment: untouched), a status (BAD_IP / TRUNCATED: takes no part), or a dict."""
    num = min(len(data), 4094)
    if link == 113:
        if num < 16:
            return None
        et, ip0, ip_len = be16(data, 14), 16, num - 16
    else:
        if origlen > 4094 or origlen < 14 or num < 14:
            return None
        et, hl = be16(data, 12), 14
        if et == 0x8100:
            if origlen < 18 or num < 18:
                return None
            et, hl = be16(data, 16), 18
        ip0, ip_len = hl, origlen - hl
    if et not in (0x0800, 0x86DD) or ip_len < 1 or ip0 >= num:
        return None
    ver = data[ip0] >> 4
    if ver == 4:
        if ip_len < 20 or ip0 + 20 > num:
            return None
        ihl, tot = (data[ip0] & 15) * 4, be16(data, ip0 + 2)
        if ihl < 20 or tot < ihl or tot > ip_len:
            return None
        F = be16(data, ip0 + 6)
        mf, off = bool(F & 0x2000), (F & 0x1FFF) * 8
        if not mf and off == 0:
            return None
        if data[ip0 + 9] != 17:
            return None
        key = (4, bytes(data[ip0 + 12:ip0 + 20]), be16(data, ip0 + 4))
        lo, hi = ip0 + ihl, ip0 + tot
    elif ver == 6:
        if ip_len < 40 or ip0 + 40 > num:
            return None
        pl = be16(data, ip0 + 4)
        if 40 + pl > ip_len or data[ip0 + 6] != 44:
            return None
        if pl < 8:
            return BAD_IP
        if ip0 + 48 > num:
            return TRUNCATED
        if data[ip0 + 40] != 17:
            return None
        F = be16(data, ip0 + 42)
        mf, off = bool(F & 1), F & 0xFFF8
        key = (6, bytes(data[ip0 + 8:ip0 + 40]), struct.unpack_from(">I", data, ip0 + 44)[0])
        lo, hi = ip0 + 48, ip0 + 40 + pl
    else:
        return None
    n = hi - lo
    if n == 0 or (mf and n % 8) or off + n > 65535:
        return BAD_IP
    if hi > num:
        return TRUNCATED
    return dict(key=key, off=off, len=n, mf=mf, lo=lo)


Ref = namedtuple("Ref", "status udp_len port udp_rel datagrams scratch stats")
# udp_rel[p]: the UDP payload's offset from the scratch start (completing UDP packets, else -1)
# datagrams: (completing packet, L, assembled bytes, slot offset) in layout order


def frag_ref(recs, link, base_status, base_udp_len, base_port, timeout_us=30_000_000):
    """The contract over recs = [(sec, usec, data, origlen)] and the parse's per-packet status,
    udp_len and source port (what an untouched packet keeps)."""
    n = len(recs)
    status = np.array(base_status, np.uint8).copy()
    udp_len = np.array(base_udp_len, np.uint32).copy()
    port = np.array(base_port, np.uint16).copy()
    udp_rel = np.full(n, -1, np.int64)
    ctx, done = {}, []
    st = dict(n_fragments=0, n_datagrams=0, n_not_udp=0, n_incomplete=0, scratch_bytes=0)
    for p, (sec, usec, data, origlen) in enumerate(recs):
        if status[p] in (1, 2, 3, 6):
            continue
        c = classify(data, origlen, link)
        if c is None:
            continue
        udp_len[p], port[p] = 0, 0
        if not isinstance(c, dict):
            status[p] = c
            continue
        st["n_fragments"] += 1
        status[p] = FRAGMENT
        t = sec * 1_000_000 + usec
        off, ln, mf = c["off"], c["len"], c["mf"]
        end = off + ln
        x = ctx.get(c["key"])
        if x is not None and timeout_us > 0 and t - x["t0"] > timeout_us:
            x = None
            st["n_incomplete"] += 1
        if x is not None:
            clash = (any(off < e and o < end for o, e, _ in x["held"])
                     or (x["L"] is not None and (end > x["L"] or not mf))
                     or (not mf and any(end < e for _, e, _ in x["held"]))
                     or len(x["held"]) >= MAX_FRAGS)
            if clash:
                x = None
                st["n_incomplete"] += 1
        if x is None:
            x = dict(t0=t, held=[], L=None, sum=0)
        x["held"].append((off, end, data[c["lo"]:c["lo"] + ln]))
        x["sum"] += ln
        if not mf:
            x["L"] = end
        ctx[c["key"]] = x
        if x["L"] is not None and x["sum"] == x["L"]:
            del ctx[c["key"]]
            L = x["L"]
            D = bytearray(L)
            for o, e, b in x["held"]:
                D[o:e] = b
            slot = st["scratch_bytes"]
            st["scratch_bytes"] += (L + 15) & ~15
            st["n_datagrams"] += 1
            done.append((p, L, bytes(D), slot))
            ul = be16(D, 4) if L >= 8 else 0
            if L < 8 or ul < 8 or ul > L:
                status[p] = NOT_UDP
                st["n_not_udp"] += 1
            else:
                status[p], udp_len[p], port[p] = UDP, ul - 8, be16(D, 0)
                udp_rel[p] = slot + 8
    st["n_incomplete"] += len(ctx)
    scratch = bytearray(st["scratch_bytes"])
    for _, L, D, slot in done:
        scratch[slot:slot + L] = D
    return Ref(status, udp_len, port, udp_rel, done, bytes(scratch), st)


def base_from_oracle(O, recs, link):
    """The parse's status, udp_len and source port per packet, from the oracle's frame walk."""
    st, ul, port = [], [], []
    for sec, usec, data, origlen in recs:
        r = O.pcap_frame(struct.pack("<IIII", sec, usec, len(data), origlen) + data, link, 0)
        st.append(r[0])
        ul.append(r[2] if r[0] == 0 else 0)
        port.append(int(r[3]["port"]))
    return st, ul, port
