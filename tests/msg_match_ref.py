"""A serial model of mgenx_msg_match, written from the definitions in include/mgenx.h alone:
Python dicts and ints, record by record.  It shares no code with the product."""
import numpy as np

NONE = 0xFFFFFFFF
RUN_BINS = 18
I64_MAX, I64_MIN = 2**63 - 1, -2**63

FLOW = np.dtype([
    ("sent", "<u8"), ("sent_bytes", "<u8"), ("send_dup", "<u8"), ("delivered", "<u8"),
    ("delivered_bytes", "<u8"), ("rx_dup", "<u8"), ("rx_orphan", "<u8"), ("lost_head", "<u8"),
    ("lost_tail", "<u8"), ("loss_runs", "<u8"), ("loss_run_max", "<u8"),
    ("loss_run_hist", "<u8", (RUN_BINS,)), ("lat_sum", "<i8"), ("lat_min", "<i8"),
    ("lat_max", "<i8")])
STATS = np.dtype([("send_skipped", "<u8"), ("recv_skipped", "<u8"), ("recv_unmatched", "<u8"),
                  ("send_dup", "<u8")])
SEND_COLS = ("flow_idx", "seq", "t_sec", "t_usec", "len")
RECV_COLS = ("flow_idx", "seq", "tx_sec", "tx_usec", "rx_sec", "rx_usec")


def _wrap_i64(v):
    v &= 2**64 - 1
    return v - 2**64 if v >= 2**63 else v


def model(n_flows, send, recv, no_time=False):
    """send / recv: dicts of uint32 arrays (SEND_COLS / RECV_COLS).  Returns (send_rx_count,
    send_first_rx, recv_send, flows, stats)."""
    S = {k: [int(x) for x in send[k]] for k in SEND_COLS}
    R = {k: [int(x) for x in recv[k]] for k in RECV_COLS}
    ns, nr = len(S["flow_idx"]), len(R["flow_idx"])
    cnt = [0] * ns
    first = [NONE] * ns
    rs = [NONE] * nr
    stats = dict(send_skipped=0, recv_skipped=0, recv_unmatched=0, send_dup=0)
    orphan = [0] * n_flows

    owner = {}                      # identity -> the lowest send index
    is_owner = [False] * ns
    for i in range(ns):
        f = S["flow_idx"][i]
        if f >= n_flows:
            stats["send_skipped"] += 1
            continue
        ident = (f, S["seq"][i]) if no_time else (f, S["seq"][i], S["t_sec"][i], S["t_usec"][i])
        if ident in owner:
            stats["send_dup"] += 1
        else:
            owner[ident] = i
            is_owner[i] = True
    for j in range(nr):
        f = R["flow_idx"][j]
        if f >= n_flows:
            stats["recv_skipped"] += 1
            continue
        ident = (f, R["seq"][j]) if no_time else (f, R["seq"][j], R["tx_sec"][j], R["tx_usec"][j])
        o = owner.get(ident)
        if o is None:
            stats["recv_unmatched"] += 1
            orphan[f] += 1
            continue
        rs[j] = o
        cnt[o] += 1
        if first[o] == NONE:
            first[o] = j            # j ascends: the first seen is the lowest

    flows = np.zeros(n_flows, FLOW)
    per_flow = [[] for _ in range(n_flows)]
    dups = [0] * n_flows
    for i in range(ns):
        f = S["flow_idx"][i]
        if f >= n_flows:
            continue
        if is_owner[i]:
            per_flow[f].append(i)
        else:
            dups[f] += 1
    for f in range(n_flows):
        d = dict(sent=0, sent_bytes=0, send_dup=dups[f], delivered=0, delivered_bytes=0, rx_dup=0,
                 rx_orphan=orphan[f], lost_head=0, lost_tail=0, loss_runs=0, loss_run_max=0,
                 lat_sum=0, lat_min=I64_MAX, lat_max=I64_MIN)
        hist = [0] * RUN_BINS
        run = 0                     # the undelivered owners since the last delivered one
        seen_delivered = False

        def close(length):
            d["loss_runs"] += 1
            d["loss_run_max"] = max(d["loss_run_max"], length)
            hist[min(length.bit_length() - 1, RUN_BINS - 1)] += 1

        for i in per_flow[f]:
            d["sent"] += 1
            d["sent_bytes"] += S["len"][i]
            if cnt[i] == 0:
                run += 1
                continue
            if run:
                close(run)
                if not seen_delivered:
                    d["lost_head"] = run
            run = 0
            seen_delivered = True
            d["delivered"] += 1
            d["delivered_bytes"] += S["len"][i]
            d["rx_dup"] += cnt[i] - 1
            j = first[i]
            lat = (R["rx_sec"][j] - S["t_sec"][i]) * 10**6 + R["rx_usec"][j] - S["t_usec"][i]
            d["lat_sum"] += lat
            d["lat_min"] = min(d["lat_min"], lat)
            d["lat_max"] = max(d["lat_max"], lat)
        if run:
            close(run)
            if seen_delivered:
                d["lost_tail"] = run
            else:
                d["lost_head"] = run        # = sent
        d["lat_sum"] = _wrap_i64(d["lat_sum"])
        for k, v in d.items():
            flows[f][k] = v
        flows[f]["loss_run_hist"] = hist
    st = np.zeros(1, STATS)
    for k, v in stats.items():
        st[0][k] = v
    return (np.array(cnt, np.uint32), np.array(first, np.uint32), np.array(rs, np.uint32), flows,
            st)


def cols(names, rows):
    """Column dict of uint32 arrays from a list of tuples."""
    a = np.array(rows, np.uint64).reshape(-1, len(names))
    return {k: a[:, c].astype(np.uint32) for c, k in enumerate(names)}


def hand_case():
    """2 flows, 12 sends (one with MGENX_FLOW_NONE, one a send duplicate) and 8 recvs: head
    loss, a middle run of 3, tail loss, an rx duplicate, an orphan.  Worked by hand in
    tests/test_msg_match_cpu.py."""
    T = 1000
    send = cols(SEND_COLS, [
        # flow seq t_sec t_usec len
        (0, 1, T, 100, 64),      # 0  lost (head)
        (0, 2, T, 200, 64),      # 1  delivered, twice (recv 0 and 3)
        (1, 1, T, 250, 100),     # 2  delivered (recv 1)
        (0, 3, T, 300, 64),      # 3  lost   \
        (0, 4, T, 400, 64),      # 4  lost    > a middle run of 3
        (NONE, 9, T, 450, 64),   # 5  skipped
        (0, 5, T, 500, 64),      # 6  lost   /
        (0, 2, T, 200, 64),      # 7  a send duplicate of 1 (inside the run: does not break it)
        (0, 6, T, 600, 128),     # 8  delivered (recv 4, negative latency)
        (1, 2, T, 650, 100),     # 9  lost (tail of flow 1)
        (0, 7, T, 700, 64),      # 10 lost (tail)
        (0, 8, T, 800, 64),      # 11 lost (tail)
    ])
    recv = cols(RECV_COLS, [
        # flow seq tx_sec tx_usec rx_sec rx_usec
        (0, 2, T, 200, T, 900),        # 0 -> send 1
        (1, 1, T, 250, T + 1, 50),     # 1 -> send 2, latency 999800
        (0, 99, T, 990, T, 995),       # 2 orphan of flow 0
        (0, 2, T, 200, T, 300),        # 3 -> send 1 again: a later copy with an earlier rx time
        (0, 6, T, 600, T, 550),        # 4 -> send 8, latency -50
        (NONE, 1, T, 250, T, 600),     # 5 skipped
        (1, 1, T, 251, T, 700),        # 6 orphan of flow 1: the stamp differs by 1 us
        (1, 1, T, 250, T + 2, 0),      # 7 -> send 2 again
    ])
    return 2, send, recv
