"""A serial model of the three parts mgenx_msg_match_multi_ex adds to mgenx_msg_match_multi,
written from the definitions in include/mgenx.h alone: Python ints, owner by owner.  It takes
the masks and the cells from msg_match_multi_ref.model and shares no code with the product."""
import numpy as np

import msg_match_multi_ref as MM

NONE = MM.NONE
HEAD, TAIL = 1, 2
RUN_BINS = 18

RUNS = np.dtype([("loss_runs", "<u8"), ("loss_run_max", "<u8"),
                 ("loss_run_hist", "<u8", (RUN_BINS,))])
RUN = np.dtype([
    ("flow_idx", "<u4"), ("length", "<u4"), ("first_send", "<u4"), ("last_send", "<u4"),
    ("flags", "<u4"), ("rcv", "<u4"), ("t_first_us", "<i8"), ("t_last_us", "<i8")])
PAIR = np.dtype([("span", "<u8"), ("lost_a", "<u8"), ("lost_b", "<u8"), ("lost_both", "<u8")])


def owners_of(n_flows, send, no_time=False):
    """Per flow its owners (send indices) in send-log order."""
    owners = [[] for _ in range(n_flows)]
    seen = set()
    cols = [np.asarray(send[k], np.uint32).tolist() for k in ("flow_idx", "seq", "t_sec", "t_usec")]
    for i, (f, seq, sec, usec) in enumerate(zip(*cols)):
        if f >= n_flows:
            continue
        ident = (f, seq) if no_time else (f, seq, sec, usec)
        if ident not in seen:
            seen.add(ident)
            owners[f].append(i)
    return owners


def model(n_flows, n_rcv, send, recv, no_time=False, min_run=1, base=None):
    """Returns a dict: base (msg_match_multi_ref.model's dict), rcv_runs [n_flows, n_rcv] RUNS,
    runs RUN (by flow_idx, last_send, rcv; those of at least max(min_run, 1)), pairs
    [n_flows, n_rcv, n_rcv] PAIR."""
    if base is None:
        base = MM.model(n_flows, n_rcv, send, recv, no_time=no_time)
    mask = [int(m) for m in base["send_mask"]]
    sec = np.asarray(send["t_sec"], np.uint32).tolist()
    usec = np.asarray(send["t_usec"], np.uint32).tolist()
    stamp = [s * 10**6 + u for s, u in zip(sec, usec)]
    owners = owners_of(n_flows, send, no_time)
    want = max(int(min_run), 1)

    rcv_runs = np.zeros((n_flows, n_rcv), RUNS)
    pairs = np.zeros((n_flows, n_rcv, n_rcv), PAIR)
    runs = []
    for f in range(n_flows):
        own = owners[f]
        sent = len(own)
        span = []                                  # per receiver: (first rank, last rank) or None
        lost = []                                  # per receiver: bit k = rank k was not delivered
        for r in range(n_rcv):
            got = [(mask[i] >> r) & 1 for i in own]
            # the maximal runs of consecutive ranks not delivered to r
            cell_runs = []                         # (first rank, last rank)
            k = 0
            while k < sent:
                if got[k]:
                    k += 1
                    continue
                e = k
                while e + 1 < sent and not got[e + 1]:
                    e += 1
                cell_runs.append((k, e))
                k = e + 1
            hist = [0] * RUN_BINS
            for a, b in cell_runs:
                n = b - a + 1
                hist[min(n.bit_length() - 1, RUN_BINS - 1)] += 1
                if n >= want:
                    flags = (0 if any(got[:a]) else HEAD) | (0 if any(got[b + 1:]) else TAIL)
                    runs.append((f, n, own[a], own[b], flags, r, stamp[own[a]], stamp[own[b]]))
            rcv_runs[f, r]["loss_runs"] = len(cell_runs)
            rcv_runs[f, r]["loss_run_max"] = max([b - a + 1 for a, b in cell_runs], default=0)
            rcv_runs[f, r]["loss_run_hist"] = hist
            ranks = [k for k in range(sent) if got[k]]
            lost.append(sum(1 << k for k in range(sent) if not got[k]))
            span.append((ranks[0], ranks[-1]) if ranks else None)
        for a in range(n_rcv):
            for b in range(n_rcv):
                if span[a] is None or span[b] is None:
                    continue
                lo, hi = max(span[a][0], span[b][0]), min(span[a][1], span[b][1])
                if lo > hi:                        # the spans do not overlap
                    continue
                # the ranks of the common span as one long integer, bit k = rank k
                common = ((1 << (hi + 1)) - 1) ^ ((1 << lo) - 1)
                la, lb = lost[a] & common, lost[b] & common
                pairs[f, a, b] = (hi - lo + 1, bin(la).count("1"), bin(lb).count("1"),
                                  bin(la & lb).count("1"))
    runs.sort(key=lambda t: (t[0], t[3], t[5]))
    out = np.zeros(len(runs), RUN)
    for k, t in enumerate(runs):
        out[k] = t
    return dict(base=base, rcv_runs=rcv_runs, runs=out, pairs=pairs)


def one_receiver(recv, r):
    """Receiver r's records alone, as mgenx_msg_match's recv columns."""
    keep = np.asarray(recv["rcv"], np.uint32) == r
    return {k: np.asarray(recv[k], np.uint32)[keep] for k in MM.RECV_COLS if k != "rcv"}


def random_case(seed, ns, n_flows, n_rcv, t0_sec=1_700_000_000):
    """A seeded case with bursty loss, a late joiner (receiver 1) and an early leaver (the last
    receiver), send duplicates, skipped records of both sides, records logged twice and the
    receivers' logs shuffled within windows of 50 records.  Returns (send, recv)."""
    rng = np.random.default_rng(seed)
    flow = rng.integers(0, n_flows, ns).astype(np.uint32)
    seq = np.zeros(ns, np.uint32)
    nxt = [0] * n_flows
    for i in range(ns):
        seq[i] = nxt[flow[i]]
        nxt[flow[i]] += 1
    t = t0_sec * 10**6 + 999_000 + np.arange(ns, dtype=np.int64) * 137
    send = dict(flow_idx=flow.copy(), seq=seq, t_sec=(t // 10**6).astype(np.uint32),
                t_usec=(t % 10**6).astype(np.uint32),
                len=rng.integers(40, 1400, ns).astype(np.uint32))
    for i in rng.choice(np.arange(20, ns), max(ns // 60, 1), replace=False):
        j = i - 1 - int(rng.integers(0, 15))       # the line of an earlier message again
        for k in MM.SEND_COLS:
            send[k][i] = send[k][j]
    send["flow_idx"][rng.choice(ns, max(ns // 80, 1), replace=False)] = NONE
    rows = []
    for r in range(n_rcv):
        lo = ns // 4 if r == 1 else 0
        hi = ns - ns // 5 if r == n_rcv - 1 and n_rcv > 2 else ns
        down = 0
        mine = []
        for i in range(lo, hi):
            if down:
                down -= 1
                continue
            if rng.integers(0, 40) == 0:           # an outage of 1 .. 120 messages starts
                down = int(rng.integers(0, 120)) if rng.integers(0, 3) == 0 else 0
                continue
            rx = int(t[i]) + 200 + int(rng.integers(0, 3000))
            row = (send["flow_idx"][i], send["seq"][i], send["t_sec"][i], send["t_usec"][i],
                   rx // 10**6, rx % 10**6, r)
            mine.append(row)
            if rng.integers(0, 50) == 0:
                mine.append(row)                   # logged twice
            if rng.integers(0, 200) == 0:
                mine.append(row[:6] + (n_rcv,))    # a receiver out of range
        for w in range(0, len(mine), 50):          # reordering inside the log
            part = mine[w:w + 50]
            rows += [part[k] for k in rng.permutation(len(part))]
    return send, MM.cols(MM.RECV_COLS, rows)
