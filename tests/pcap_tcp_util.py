"""TCP segmentation for the pcap2mgen tests (test infrastructure).

`segment` cuts a byte stream into TCP segments (MSS, SYN, retransmissions, reordering, loss,
overlap, any initial sequence number), `Conn` wraps them into IP packets, `capture` builds a
mixed capture of pcap_util-style UDP flows plus TCP connections whose streams come from the
oracle's TCP transmit path, `tcp_ref` is the serial model of the stream contract (include/mgenx.h,
DESIGN.md 4.10.1) -- plain Python per packet, written from the contract's text, sharing no code
with the product -- and `frame_ref` gives the records and their completing packets from the
oracle's TCP framing plus the model's pieces.
"""
import struct
from collections import namedtuple

import numpy as np

import pcap_frag_util as F
import pcap_util as P

TRUNCATED, TCP = 5, 9
SYN_FLAG, GAP_FLAG = 1, 2                      # stream flags
FIN, SYN, RST, PSH, ACK = 1, 2, 4, 8, 16       # TCP header flags

A4, B4 = bytes([10, 0, 0, 5]), bytes([10, 0, 0, 2])
A6 = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1])
B6 = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [0x99])
F_ADDR = np.dtype([("type", "u1"), ("len", "u1"), ("port", "<u2"), ("addr", "u1", 16)])


def be16(b, i):
    return b[i] << 8 | b[i + 1]


# ---------------------------------------------------------------- the segmenter
def tcp_header(sport, dport, seq, flags=ACK, doff=20, ack=0) -> bytes:
    """A TCP header whose data-offset field says doff; at least 20 bytes are written, option
    bytes (NOPs) when doff is larger."""
    return struct.pack(">HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, ack, (doff // 4) << 4, flags,
                       65535, 0, 0) + b"\x01" * max(0, doff - 20)


class Conn:
    """One direction of a connection: addresses and ports."""

    def __init__(self, src=A4, dst=B4, sport=40000, dport=5000):
        self.src, self.dst, self.sport, self.dport = src, dst, sport, dport

    def ip(self, seq, payload=b"", flags=ACK, doff=20, **kw) -> bytes:
        l4 = tcp_header(self.sport, self.dport, seq, flags, doff) + payload
        if len(self.src) == 4:
            return P.ipv4(l4, self.src, self.dst, proto=6, **kw)
        return P.ipv6(l4, self.src, self.dst, nh=6, **kw)

    def reverse(self):
        return Conn(self.dst, self.src, self.dport, self.sport)

    def addr(self, which):
        a = np.zeros((), F_ADDR)
        raw, port = (self.src, self.sport) if which == "src" else (self.dst, self.dport)
        a["type"], a["len"], a["port"] = (1 if len(raw) == 4 else 2), len(raw), port
        a["addr"][:len(raw)] = np.frombuffer(raw, np.uint8)
        return a


def segment(stream: bytes, mss=1448, isn=1000, syn=True, rng=None, retx=0.0, reorder=0,
            lose=(), overlap=0):
    """(seq, flags, payload) of a stream's segments.  syn: a SYN at isn comes first and the data
    starts at isn + 1 (else at isn).  lose: indices of data segments left out.  overlap: every
    data segment but the first starts that many bytes early.  retx: the share of data segments
    sent again one to three places later.  reorder: data segments move at most that many places
    (the SYN stays first)."""
    base = isn + 1 if syn else isn
    data = []
    for k, off in enumerate(range(0, len(stream), mss)):
        if k in lose:
            continue
        lo = max(0, off - overlap)
        data.append((base + lo, ACK | PSH, bytes(stream[lo:off + mss])))
    if retx and rng is not None:
        out = []
        later = {}
        for k, s in enumerate(data):
            out.append(s)
            for c in later.pop(k, []):
                out.append(c)
            if rng.random() < retx:
                later.setdefault(k + int(rng.integers(1, 4)), []).append(s)
        for v in later.values():
            out += v
        data = out
    if reorder and rng is not None:
        order = sorted(range(len(data)), key=lambda k: k + rng.uniform(0, reorder))
        data = [data[k] for k in order]
    return ([(isn, SYN, b"")] if syn else []) + data


def pcap_of(items, link=1, vlan=None, dt=50, t0=1_700_000_000_000_000):
    """items: IP packets, (IP packet, caplen) or ("raw", link frame) -> a capture, dt
    microseconds apart."""
    recs = []
    for k, f in enumerate(items):
        ip, cap = f if isinstance(f, tuple) else (f, None)
        fr, cap = (cap, None) if isinstance(ip, str) else (F.link_frame(ip, link, vlan), cap)
        sec, usec = divmod(t0 + k * dt, 1_000_000)
        recs.append((sec, usec, fr) if cap is None else (sec, usec, fr, cap, len(fr)))
    return P.pcap(recs, link=link)


# ---------------------------------------------------------------- mixed captures
def mgen_stream(O, rng, sizes, flow, t_us, v6=False):
    """The TCP transmit stream of messages of the given sizes (oracle.tcp_tx), one flow."""
    out = []
    for seq, size in enumerate(sizes):
        t_us += int(rng.integers(200, 3000))
        tx = divmod(t_us, 1_000_000)
        dst = ("6", B6, 5000 + flow) if v6 else ("4", B4, 5000 + flow)
        kw = dict(lat=38.5, lon=-77.25, alt=120, gps_status=2) if rng.random() < 0.5 else {}
        m = O.make_msg(msg_len=int(size), flow_id=flow, seq=seq, tx_sec=tx[0], tx_usec=tx[1],
                       dst=dst, **kw)
        out.append(O.tcp_tx(m, checksum=True))
    return b"".join(out)


def capture(O, seed, link=1, v6=False, vlan=None, n_conn=4, n_msg=48, n_udp=40, retx=0.05,
            reorder=3, frag_mtu=None):
    """UDP flows and n_conn TCP connections, interleaved at random: n_msg messages of 28..8192
    bytes over the connections plus one of 20000 bytes; segments cut at MSS 1448 and 536 in
    turn, each connection with its SYN, its peer's SYN and pure ACKs in the other direction.
    frag_mtu: the UDP messages are 1500..3000 bytes and every datagram above that MTU is
    captured as its IP fragments.
    Returns (pcap, [(Conn, stream bytes)], whole): whole[p] is the pcap record whose log lines
    stand at packet p -- the packet itself, for a datagram's last fragment the unfragmented
    frame at that fragment's time, None for the fragments before it."""
    rng = np.random.default_rng(seed)
    t_us = 1_700_000_000 * 1_000_000 + 250_000
    src, dst = (A6, B6) if v6 else (A4, B4)
    queues, conns = [], []
    for c in range(n_conn):
        sizes = [int(x) for x in rng.integers(28, 8193, n_msg // n_conn)]
        if c == 1:
            sizes.insert(len(sizes) // 2, 20000)
        stream = mgen_stream(O, rng, sizes, 10 + c, t_us, v6)
        conn = Conn(src, dst, 41000 + c, 5010 + c)
        conns.append((conn, stream))
        isn = int(rng.integers(0, 2**32))
        segs = segment(stream, (1448, 536)[c % 2], isn, True, rng, retx, reorder)
        back = conn.reverse()
        q = []
        for k, (seq, flags, pay) in enumerate(segs):
            q.append(conn.ip(seq, pay, flags))
            if k == 0:
                q.append(back.ip(7000, b"", SYN | ACK))
            elif k % 3 == 0:
                q.append(back.ip(7001, b"", ACK))
        queues.append(q)
    seqs = {}
    udp = []
    for i in range(n_udp):
        flow = int(rng.integers(1, 4))
        seqs[flow] = seqs.get(flow, -1) + 1
        udp.append((flow, seqs[flow]))
    queues.append(udp)
    recs, whole = [], []
    left = [len(q) for q in queues]
    pos = [0] * len(queues)
    while sum(left):
        k = int(rng.choice(len(queues), p=np.array(left) / sum(left)))
        item = queues[k][pos[k]]
        pos[k] += 1
        left[k] -= 1
        t_us += int(rng.integers(20, 900))
        sec, usec = divmod(t_us, 1_000_000)
        cut = [item]
        if k == len(queues) - 1:
            flow, seq = item
            size = int(rng.integers(1500, 3001) if frag_mtu else rng.integers(64, 1200))
            ttl = int(rng.integers(2, 250))
            item = F.datagram(O, flow, seq, t_us, size, v6, ttl=ttl, gps=rng.random() < 0.5)
            cut = [item]
            if frag_mtu and len(item) > frag_mtu:
                cut = F.fragment(item, frag_mtu, 0x4000 + len(recs), early_ttl=ttl + 1)
        for j, f in enumerate(cut):
            s, u = divmod(t_us - (len(cut) - 1 - j) * 3, 1_000_000)
            recs.append((s, u, F.link_frame(f, link, vlan)))
            whole.append(None)
        whole[-1] = (sec, usec, F.link_frame(item, link, vlan))
    return P.pcap(recs, link=link), conns, whole


# ---------------------------------------------------------------- the serial model
def classify(data: bytes, origlen: int, link: int):
    """The contract's 'which packets are segments' for one packet: None (untouched), TRUNCATED
    (takes no part), or a dict."""
    num = len(data)
    if link == 113:
        if num < 16:
            return None
        et, ip0, ip_len = be16(data, 14), 16, num - 16
    else:
        if origlen < 14 or num < 14:
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
        if be16(data, ip0 + 6) & 0x3FFF or data[ip0 + 9] != 6:
            return None
        l4, ip_end = ip0 + ihl, ip0 + tot
        addrs = (bytes(data[ip0 + 12:ip0 + 16]), bytes(data[ip0 + 16:ip0 + 20]))
    elif ver == 6:
        if ip_len < 40 or ip0 + 40 > num:
            return None
        pl = be16(data, ip0 + 4)
        if 40 + pl > ip_len or data[ip0 + 6] != 6:
            return None
        l4, ip_end = ip0 + 40, ip0 + 40 + pl
        addrs = (bytes(data[ip0 + 8:ip0 + 24]), bytes(data[ip0 + 24:ip0 + 40]))
    else:
        return None
    if l4 + 20 > num or l4 + 20 > ip_end:
        return None
    doff = (data[l4 + 12] >> 4) * 4
    if doff < 20 or l4 + doff > ip_end:
        return None
    if ip_end > num:
        return TRUNCATED
    sport, dport = be16(data, l4), be16(data, l4 + 2)
    return dict(key=(ver, addrs[0], addrs[1], sport, dport),
                seq=struct.unpack_from(">I", data, l4 + 4)[0], syn=bool(data[l4 + 13] & 2),
                payload=bytes(data[l4 + doff:ip_end]))


Ref = namedtuple("Ref", "status streams scratch pieces stats")
# status[p]: the packet's status after the call (None: untouched)
# streams: dicts key, first_pkt, n_segments, flags, len, dropped, off (from the scratch start)
# pieces: (end offset from the scratch start, completing packet)


def tcp_ref(recs, link, examined=None):
    """The contract over recs = [(sec, usec, data, origlen)]; examined[p] False: the packet's
    status is OOB."""
    status = [None] * len(recs)
    keys, streams = {}, []
    st = dict(n_segments=0, n_streams=0, n_gap_streams=0, n_stale=0, dropped_bytes=0, n_pieces=0,
              scratch_bytes=0)
    for p, (_, _, data, origlen) in enumerate(recs):
        if examined is not None and not examined[p]:
            continue
        c = classify(data, origlen, link)
        if c is None:
            continue
        if c == TRUNCATED:
            status[p] = TRUNCATED
            continue
        status[p] = TCP
        st["n_segments"] += 1
        k = keys.setdefault(c["key"], dict(syn_seq=None, cur=None))
        if c["syn"] and c["seq"] != k["syn_seq"]:
            k["cur"] = dict(key=c["key"], first_pkt=p, n_segments=0, flags=SYN_FLAG,
                            base=(c["seq"] + 1) & 0xFFFFFFFF, segs=[])
            streams.append(k["cur"])
        elif k["cur"] is None:
            k["cur"] = dict(key=c["key"], first_pkt=p, n_segments=0, flags=0, base=None, segs=[])
            streams.append(k["cur"])
        if c["syn"]:
            k["syn_seq"] = c["seq"]
        s = k["cur"]
        s["n_segments"] += 1
        pay = b"" if c["syn"] else c["payload"]
        if not pay:
            continue
        if s["base"] is None:
            s["base"] = c["seq"]
        rel = (c["seq"] - s["base"]) & 0xFFFFFFFF
        if rel >= 2**31 or rel + len(pay) > 2**31:
            st["n_stale"] += 1
            continue
        s["segs"].append((rel, p, pay))
    scratch, pieces = bytearray(), []
    for s in streams:
        data, E, hole, last = bytearray(), 0, False, -1
        s["dropped"] = 0
        for rel, p, pay in sorted(s["segs"], key=lambda x: (x[0], x[1])):
            if not hole and rel > E:
                hole = True
                s["len"] = E
                s["flags"] |= GAP_FLAG
            lo, hi = max(rel, E), rel + len(pay)
            if hi > lo:
                if hole:
                    s["dropped"] += hi - lo
                else:
                    assert lo == len(data)
                    data += pay[lo - rel:]
                    last = max(last, p)
                    pieces.append((len(scratch) + hi, last))
            E = max(E, hi)
        if not hole:
            s["len"] = E
        assert s["len"] == len(data)
        s["off"] = len(scratch)
        s["data"] = bytes(data)
        scratch += data + bytes(-len(data) % 16)
        st["n_gap_streams"] += hole
        st["dropped_bytes"] += s["dropped"]
        del s["segs"], s["base"]
    st["n_streams"], st["n_pieces"], st["scratch_bytes"] = len(streams), len(pieces), len(scratch)
    return Ref(status, streams, bytes(scratch), pieces, st)


def frame_ref(O, ref: Ref):
    """Records of the model's streams by the oracle's TCP framing, with their completing
    packets, in output order (packet, stream, offset): (list of (offset from the scratch start,
    length, stream, packet), status per stream)."""
    out, status = [], []
    ends = [e for e, _ in ref.pieces]
    for s, t in enumerate(ref.streams):
        offs, lens, _, _, stt = O.tcp_scan(t["data"])
        status.append(stt)
        for o, n in zip(offs, lens):
            end = t["off"] + int(o) + int(n)
            k = next(i for i, e in enumerate(ends) if e >= end)
            out.append((t["off"] + int(o), int(n), s, ref.pieces[k][1]))
    out.sort(key=lambda r: (r[3], r[2], r[0]))
    return out, status


def expected_log(O, file: bytes, link, conns, whole):
    """The log of capture()'s pcap with tcp: per packet, the oracle's pcap2mgen lines of
    whole[p], then the oracle's proto>TCP lines (LogRecvEvent over its TCP receive of each
    ORIGINAL stream) of the records the model completes at p, at p's time.
    Returns (log, TCP lines, the model)."""
    recs = F.records(file)
    ref = tcp_ref(recs, link)
    frames, _ = frame_ref(O, ref)
    by_port = {c.sport: (c, s) for c, s in conns}
    at, scans = {}, {}
    for off, n, s, pkt in frames:
        t = ref.streams[s]
        conn, stream = by_port[t["key"][3]]
        assert t["data"] == stream, "the capture lost stream bytes"
        if s not in scans:
            scans[s] = O.tcp_scan(stream)
        offs, lens, f, _, _ = scans[s]
        j = int(np.searchsorted(offs, off - t["off"]))
        assert offs[j] == off - t["off"] and lens[j] == n
        at.setdefault(pkt, []).append(O.log_recv_text(
            f[j:j + 1], np.frombuffer(stream, np.uint8), offs[j:j + 1],
            conn.addr("src").reshape(1), [recs[pkt][0]], [recs[pkt][1]], protocol=2, ttl=None,
            opts=O.LOG_NO_DATA))
    out = []
    for p, w in enumerate(whole):
        if w is not None:
            out.append(O.pcap2mgen(P.pcap([w], link=link))[0])
        out += at.get(p, [])
    return b"".join(out), sum(len(v) for v in at.values()), ref
