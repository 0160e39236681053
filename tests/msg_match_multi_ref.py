"""A serial model of mgenx_msg_match_multi, written from the definitions in include/mgenx.h
alone: Python dicts and ints, record by record.  It shares no code with the product or with
msg_match_ref.py."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_RCV = 64
U64_MAX = 2**64 - 1
I64_MAX, I64_MIN = 2**63 - 1, -2**63

CELL = np.dtype([
    ("delivered", "<u8"), ("delivered_bytes", "<u8"), ("rx_dup", "<u8"), ("rx_orphan", "<u8"),
    ("lost_head", "<u8"), ("lost_tail", "<u8"), ("first_send", "<u4"), ("last_send", "<u4"),
    ("lat_sum", "<i8"), ("lat_min", "<i8"), ("lat_max", "<i8")])
FANOUT = np.dtype([
    ("sent", "<u8"), ("sent_bytes", "<u8"), ("send_dup", "<u8"), ("deliveries", "<u8"),
    ("reached_all", "<u8"), ("reach_hist", "<u8", (MAX_RCV + 1,))])
BIN = np.dtype([
    ("sent", "<u8"), ("sent_bytes", "<u8"), ("deliveries", "<u8"), ("delivered_bytes", "<u8"),
    ("reached_any", "<u8"), ("reached_all", "<u8"), ("reach_min", "<u8"), ("reach_max", "<u8")])
STATS = np.dtype([("send_skipped", "<u8"), ("recv_skipped", "<u8"), ("recv_unmatched", "<u8"),
                  ("send_dup", "<u8")])
SEND_COLS = ("flow_idx", "seq", "t_sec", "t_usec", "len")
RECV_COLS = ("flow_idx", "seq", "tx_sec", "tx_usec", "rx_sec", "rx_usec", "rcv")


def _to_i64(v):
    v %= 2**64
    return v - 2**64 if v >= 2**63 else v


def model(n_flows, n_rcv, send, recv, no_time=False, timeline=None):
    """send / recv: dicts of uint32 arrays (SEND_COLS / RECV_COLS).  timeline: None or
    (t0_us, width_us, n_bins).  Returns a dict: send_mask [ns] u64, recv_send [nr] u32,
    recv_first [nr] u8, cells [n_flows, n_rcv], fanout [n_flows], stats [1] and, with a
    timeline, bins [n_flows, n_bins] and outside [n_flows] u64."""
    assert 1 <= n_rcv <= MAX_RCV
    # (tolist: Python ints, one tuple per record)
    S = list(zip(*[np.asarray(send[k], np.uint32).tolist() for k in SEND_COLS]))
    R = list(zip(*[np.asarray(recv[k], np.uint32).tolist() for k in RECV_COLS]))
    st = dict.fromkeys(STATS.names, 0)

    # owners: the lowest send index of every identity among the counted send records
    owner_of = {}
    owners = [[] for _ in range(n_flows)]          # per flow, in send-log order
    dups = [0] * n_flows
    for i, (f, seq, sec, usec, _ln) in enumerate(S):
        if f >= n_flows:
            st["send_skipped"] += 1
            continue
        ident = (f, seq) if no_time else (f, seq, sec, usec)
        if ident in owner_of:
            st["send_dup"] += 1
            dups[f] += 1
        else:
            owner_of[ident] = i
            owners[f].append(i)

    # the recv records, in index order: the first seen of (owner, rcv) is the first arrival
    arrival = {}                                    # (owner, rcv) -> recv index
    with_owner = {}                                 # (flow, rcv) -> counted records with an owner
    orphans = {}
    recv_send = [NONE] * len(R)
    recv_first = [0] * len(R)
    for j, (f, seq, txs, txu, _rxs, _rxu, r) in enumerate(R):
        if f >= n_flows or r >= n_rcv:
            st["recv_skipped"] += 1
            continue
        o = owner_of.get((f, seq) if no_time else (f, seq, txs, txu))
        if o is None:
            st["recv_unmatched"] += 1
            orphans[f, r] = orphans.get((f, r), 0) + 1
            continue
        recv_send[j] = o
        with_owner[f, r] = with_owner.get((f, r), 0) + 1
        if (o, r) not in arrival:
            arrival[o, r] = j
            recv_first[j] = 1

    send_mask = [0] * len(S)
    for (o, r) in arrival:
        send_mask[o] |= 1 << r

    cells = np.zeros((n_flows, n_rcv), CELL)
    fanout = np.zeros(n_flows, FANOUT)
    for f in range(n_flows):
        sent = len(owners[f])
        hist = [0] * (MAX_RCV + 1)
        for i in owners[f]:
            hist[bin(send_mask[i]).count("1")] += 1
        fanout[f]["sent"] = sent
        fanout[f]["sent_bytes"] = sum(S[i][4] for i in owners[f])
        fanout[f]["send_dup"] = dups[f]
        fanout[f]["deliveries"] = sum(k * n for k, n in enumerate(hist))
        fanout[f]["reached_all"] = hist[n_rcv]
        fanout[f]["reach_hist"] = hist
        for r in range(n_rcv):
            got = [(rank, i) for rank, i in enumerate(owners[f]) if (send_mask[i] >> r) & 1]
            lats = []
            for _rank, i in got:
                j = arrival[i, r]
                lats.append((R[j][4] * 10**6 + R[j][5]) - (S[i][2] * 10**6 + S[i][3]))
            c = dict(delivered=len(got), delivered_bytes=sum(S[i][4] for _, i in got),
                     rx_dup=with_owner.get((f, r), 0) - len(got), rx_orphan=orphans.get((f, r), 0),
                     lost_head=got[0][0] if got else sent,
                     lost_tail=sent - 1 - got[-1][0] if got else 0,
                     first_send=got[0][1] if got else NONE, last_send=got[-1][1] if got else NONE,
                     lat_sum=_to_i64(sum(lats)), lat_min=min(lats) if lats else I64_MAX,
                     lat_max=max(lats) if lats else I64_MIN)
            for k, v in c.items():
                cells[f, r][k] = v

    stats = np.zeros(1, STATS)
    for k, v in st.items():
        stats[0][k] = v
    out = dict(send_mask=np.array(send_mask, np.uint64), recv_send=np.array(recv_send, np.uint32),
               recv_first=np.array(recv_first, np.uint8), cells=cells, fanout=fanout, stats=stats)
    if timeline is not None:
        t0, width, n_bins = (int(v) for v in timeline)
        bins = np.zeros((n_flows, n_bins), BIN)
        bins["reach_min"] = U64_MAX
        outside = [0] * n_flows
        for f in range(n_flows):
            for i in owners[f]:
                b = (S[i][2] * 10**6 + S[i][3] - t0) // width      # Python's // is a floor
                if not 0 <= b < n_bins:
                    outside[f] += 1
                    continue
                k = bin(send_mask[i]).count("1")
                e = bins[f, b]
                e["sent"] += 1
                e["sent_bytes"] += S[i][4]
                e["deliveries"] += k
                e["delivered_bytes"] += S[i][4] * k
                e["reached_any"] += 1 if k else 0
                e["reached_all"] += 1 if k == n_rcv else 0
                e["reach_min"] = min(int(e["reach_min"]), k)
                e["reach_max"] = max(int(e["reach_max"]), k)
        out["bins"] = bins
        out["outside"] = np.array(outside, np.uint64)
    return out


def cols(names, rows):
    """Column dict of uint32 arrays from a list of tuples."""
    a = np.array(rows, np.uint64).reshape(-1, len(names))
    return {k: a[:, c].astype(np.uint32) for c, k in enumerate(names)}


def hand_case():
    """2 flows, 3 receivers, 14 sends, 20 recvs.  Receiver 1 joins late (head loss there only),
    receiver 2 leaves early (tail loss).  Worked by hand in tests/test_msg_match_multi_cpu.py."""
    T = 2000
    send = cols(SEND_COLS, [
        # flow seq t_sec t_usec len
        (0, 1, T, 100, 64),      # 0  reaches 0 and 2
        (0, 2, T, 200, 64),      # 1  reaches 0 and 2
        (1, 1, T, 250, 100),     # 2  reaches 0
        (0, 3, T, 300, 64),      # 3  reaches all; receiver 1 logs it twice (recv 6, 7)
        (0, 4, T, 400, 64),      # 4  reaches none  \
        (0, 2, T, 200, 64),      # 5  a send duplicate of 1, inside the gap
        (0, 5, T, 500, 128),     # 6  reaches none  /
        (NONE, 9, T, 550, 64),   # 7  skipped: no flow
        (0, 6, T, 600, 64),      # 8  reaches 0 and 1
        (1, 2, T, 650, 100),     # 9  reaches 0 and 1
        (0, 7, T, 700, 64),      # 10 reaches 1
        (0, 8, T, 800, 64),      # 11 reaches 0 and 1
        (1, 3, T, 850, 100),     # 12 reaches none
        (0, 9, T, 900, 64),      # 13 reaches 0
    ])
    recv = cols(RECV_COLS, [
        # flow seq tx_sec tx_usec rx_sec rx_usec rcv
        (0, 1, T, 100, T, 150, 0),        # 0  -> send 0, lat 50
        (0, 2, T, 200, T, 260, 0),        # 1  -> send 1, lat 60
        (1, 1, T, 250, T, 300, 0),        # 2  -> send 2, lat 50
        (0, 3, T, 300, T, 370, 0),        # 3  -> send 3, lat 70
        (0, 6, T, 600, T, 640, 0),        # 4  -> send 8, lat 40
        (1, 2, T, 650, T, 700, 0),        # 5  -> send 9, lat 50
        (0, 3, T, 300, T + 1, 300, 1),    # 6  -> send 3 at receiver 1, lat 1000000
        (0, 3, T, 300, T, 310, 1),        # 7  -> send 3 again at receiver 1: not the first
        (0, 8, T, 800, T, 880, 0),        # 8  -> send 11, lat 80
        (0, 9, T, 900, T, 890, 0),        # 9  -> send 13, lat -10
        (0, 6, T, 600, T, 660, 1),        # 10 -> send 8, lat 60
        (1, 2, T, 650, T, 720, 1),        # 11 -> send 9, lat 70
        (0, 7, T, 700, T, 790, 1),        # 12 -> send 10, lat 90
        (0, 8, T, 800, T, 900, 1),        # 13 -> send 11, lat 100
        (0, 77, T, 990, T, 995, 1),       # 14 an orphan of (0, 1)
        (NONE, 1, T, 100, T, 150, 1),     # 15 skipped: no flow
        (0, 1, T, 100, T, 130, 2),        # 16 -> send 0 at receiver 2, lat 30
        (0, 2, T, 200, T, 220, 2),        # 17 -> send 1, lat 20
        (0, 3, T, 300, T, 330, 2),        # 18 -> send 3, lat 30
        (0, 1, T, 100, T, 150, 3),        # 19 skipped: rcv >= n_rcv
    ])
    return 2, 3, send, recv
