"""The inputs of the flow_reduce value-domain tests (test_gpu_flow_values.py), built here so
that the CPU suite (test_flow_value_cases_cpu.py) can assert from the oracle alone that every
input reaches the edge it is meant for.  A case holds the seven columns in receive order (the
flow index 0-based), n_flows, the window, per_flow and the call splits (each a tuple of call
starts, 0 first).  Everything is cached and read-only: the tests share one build per case and
one oracle run (oracle_run).  compare() is test_gpu_analytics.py's, plus the one NaN rule and
the check that nothing past the kept report slots was written."""
import functools
import math

import numpy as np

COLS = ("idx", "seq", "tx_sec", "tx_usec", "msg_len", "rx_sec", "rx_usec")
DT = {"idx": np.uint32, "seq": np.uint32, "tx_sec": np.uint32, "tx_usec": np.uint32,
      "msg_len": np.uint16, "rx_sec": np.uint32, "rx_usec": np.uint32}
M = 10**6
T0 = 1_700_000_000
FAMILIES = ("V1", "V2", "V3", "V4", "V5", "V6", "V7")
FILL = 0xA5


def window_add(window):
    """(seconds, microseconds) that ProtoTime += adds for flow_init(window): the quantized
    window's floor, then int(frac * 1e6 + 0.5)."""
    from oracle import oracle as O
    q = O.quantized_window(window)
    whole = math.floor(q)
    return int(whole), int((q - whole) * 1e6 + 0.5)


# ------------------------------------------------------------------ building blocks
def _seqs(rng, m, jumpy=True):
    """m sequence numbers: mostly +1, losses, and (jumpy) jumps past the mask span, near 2^24
    and past 2^31, from a random start."""
    inc = np.ones(m, np.uint64)
    u = rng.random(m)
    inc[u < 0.05] = rng.integers(2, 12, int((u < 0.05).sum()))
    if jumpy:
        inc[u < 0.01] = rng.integers(1024, 3000, int((u < 0.01).sum()))
        inc[u < 0.002] = (1 << 24) + rng.integers(-3, 3, int((u < 0.002).sum()))
        inc[u < 0.0005] = (1 << 31) + 7
    return ((np.cumsum(inc) + np.uint64(rng.integers(0, 1 << 32))) & np.uint64(0xFFFFFFFF)
            ).astype(np.int64)


def _flow(rng, m, t0_us, gap_us, lat, lens, dup=0.004, reorder_us=900.0, jumpy=True):
    """One flow in its own receive order: tx times from t0_us with exponential gaps, rx = tx +
    lat (int64 microseconds per record, any sign), duplicates 3 us after their original, local
    reordering.  Times are int64 microseconds ("tx", "rx"); split() makes the columns."""
    seq = _seqs(rng, m, jumpy)
    tx = t0_us + np.cumsum(rng.exponential(gap_us, m)).astype(np.int64)
    rx = tx + lat
    ln = np.asarray(lens, np.int64)
    d = rng.random(m) < dup
    seq, tx, ln = (np.concatenate([a, a[d]]) for a in (seq, tx, ln))
    rx = np.concatenate([rx, rx[d] + 3])
    o = np.argsort(rx + rng.uniform(-reorder_us, reorder_us, rx.size), kind="stable")
    return {"seq": seq[o], "tx": tx[o], "rx": rx[o], "msg_len": ln[o]}


def _lens(rng, m, values=(200,), zero=0.003):
    ln = np.asarray(values, np.int64)[rng.integers(0, len(values), m)]
    ln[rng.random(m) < zero] = 0
    return ln


def split(fl):
    """int64 microsecond times -> normalised sec / usec columns (kept if already split)"""
    out = {"seq": fl["seq"], "msg_len": fl["msg_len"]}
    for k in ("tx", "rx"):
        if k in fl:
            out[k + "_sec"], out[k + "_usec"] = fl[k] // M, fl[k] % M
        else:
            out[k + "_sec"], out[k + "_usec"] = fl[k + "_sec"], fl[k + "_usec"]
    return out


def merge(flows, rng):
    """Interleave the flows (each kept in its own order) evenly over the call."""
    flows = [split(f) for f in flows]
    key = np.concatenate([(np.arange(len(f["seq"])) + rng.random(len(f["seq"]))) / len(f["seq"])
                          for f in flows])
    o = np.argsort(key, kind="stable")
    cols = {"idx": np.concatenate([np.full(len(f["seq"]), i) for i, f in enumerate(flows)])}
    for k in COLS[1:]:
        cols[k] = np.concatenate([np.asarray(f[k], np.int64) for f in flows])
    out = {}
    for k in COLS:
        v = cols[k][o]
        assert v.min() >= 0 and v.max() <= np.iinfo(DT[k]).max, k
        out[k] = np.ascontiguousarray(v.astype(DT[k]))
        out[k].setflags(write=False)
    return out


def case(name, cols, n_flows, window, per_flow, splits=None, **meta):
    n = len(cols["seq"])
    if splits is None:
        splits = ((0,), (0, 1), (0, 1, n // 3, n // 3 + 5, 2 * n // 3))
    splits = tuple(tuple(sorted(set(min(s, n - 1) for s in sp))) for sp in splits)
    assert all(sp[0] == 0 for sp in splits) and any(len(sp) > 1 and sp[1] == 1 for sp in splits)
    return {"name": name, "cols": cols, "n": n, "n_flows": n_flows, "window": window,
            "per_flow": per_flow, "splits": splits, "meta": meta}


def flow_records(c, f):
    """the positions of flow f's records in the call, in order"""
    return np.flatnonzero(c["cols"]["idx"] == f)


# ------------------------------------------------------------------ V1: latency sign and size
V1_OFFSETS = (-3600 * M, -M - 1, -1, 0, 1, 999_999, M, 3600 * M)


def _v1(small):
    """Per-flow clock offsets from -1 h to +1 h with +-500 us of jitter (flows 2..4 cross zero),
    loss, duplicates and reordering; records with tx == rx in the flow of offset 0; in flows
    1..6, a duplicate or an early record (below seq_start, outside the mask) right after a
    silence of two windows: it closes the window and opens the next with latency 0.0."""
    rng = np.random.default_rng(101)
    m, window = (70, 0.001) if small else (3000, 0.05)
    wus = int(window * M)
    flows = []
    for f, off in enumerate(V1_OFFSETS):
        jit = rng.integers(-500, 501, m)
        if off == 0:
            jit[rng.random(m) < 0.02] = 0
            jit[m // 2] = 0
        # (the outer flows without sequence jumps: past 2^31 a flow's records are all "early",
        # none is counted, and its windows report the latency 0.0 they opened with)
        fl = _flow(rng, m, T0 * M + 7 * f, 60.0 if small else 700.0, off + jit, _lens(rng, m),
                   jumpy=f not in (0, 7))
        if 1 <= f <= 6:
            for e, p in enumerate(range(len(fl["seq"]) // 5, len(fl["seq"]), len(fl["seq"]) // 5)):
                early = e % 2 == 1
                new = {"seq": (fl["seq"][p - 1] - (2000 if early else 0)) & 0xFFFFFFFF,
                       "tx": fl["tx"][p - 1] + 2 * wus, "msg_len": 200}
                new["rx"] = new["tx"] + off
                for k in ("tx", "rx"):
                    fl[k][p:] += 3 * wus
                fl = {k: np.insert(v, p, new[k]) for k, v in fl.items()}
        flows.append(fl)
    return [case("V1", merge(flows, rng), 8, window, 128)]


# ------------------------------------------------------------------ V2: unnormalised tx_usec
V2_USEC = (M, M + 1, 2 * M, 1 << 31, (1 << 32) - 1)


def _v2(small):
    """tx_usec of 10^6 and more off the wire on 30 % of the records: flows 0 and 1 with tx_sec
    lowered to compensate (only the part below 10^6 differs: latencies within +-1 s), flows 2
    and 3 not (latencies down to -4294 s).  ProtoTime::Delta subtracts the fields as they
    are, widened to int64 first."""
    rng = np.random.default_rng(102)
    m = 120 if small else 1500
    flows = []
    for f in range(4):
        fl = _flow(rng, m, T0 * M, 700.0, rng.integers(50, 500, m), _lens(rng, m))
        n = len(fl["seq"])
        s = split(fl)
        pick = rng.random(n) < 0.3
        v = np.asarray(V2_USEC, np.int64)[np.arange(n) % len(V2_USEC)]
        if f < 2:      # tx_sec lowered by the whole seconds tx_usec holds
            s["tx_sec"] = np.where(pick, s["tx_sec"] - v // M, s["tx_sec"])
        s["tx_usec"] = np.where(pick, v, s["tx_usec"])
        flows.append(s)
    return [case("V2", merge(flows, rng), 4, 0.05, 64)]


# ------------------------------------------------------------------ V3: window-end ties
V3_WINDOWS = (0.001, 0.05, 1.0, 600.0)
V3_START_USEC = (999_999, 999_037, 0, 500_000)


def _tie_chain(rng, m, start, add):
    """m receive times (total microseconds) built from the window chain itself: 0-5 records
    inside the window, maybe a run at end - 1, then 1-3 records under one stamp at end or
    end + 1 (sometimes later): the first closes, the others lie in the window it opens."""
    rx = [start]
    t, end = start, start + add
    while len(rx) < m:
        k = int(rng.integers(0, 6))
        if k and end - 2 >= t:
            rx += sorted(int(x) for x in rng.integers(t, end - 1, k))
        if rng.random() < 0.5:
            rx += [end - 1] * int(rng.integers(1, 4))
        u = rng.random()
        c = end if u < 0.45 else end + 1 if u < 0.9 else end + int(rng.integers(2, add + 2))
        rx += [c] * int(rng.integers(1, 4))
        t, end = c, c + add
    return np.asarray(rx[:m], np.int64)


def _v3(small):
    rng = np.random.default_rng(103)
    out = []
    for w in V3_WINDOWS:
        a_sec, a_us = window_add(w)
        add = a_sec * M + a_us
        m = 50 if small else 4000
        flows = []
        for f in range(3):
            rx = _tie_chain(rng, m, (T0 + 11 * f) * M + V3_START_USEC[f], add)
            inc = rng.integers(1, 3, m)
            inc[rng.random(m) < 0.05] = 0                      # duplicates
            seq = (np.cumsum(inc) + int(rng.integers(0, 1 << 32))) & 0xFFFFFFFF
            flows.append({"seq": seq, "tx": rx - rng.integers(50, 500, m), "rx": rx,
                          "msg_len": _lens(rng, m, (256,), 0.03)})
        out.append(case(f"V3-w{w}", merge(flows, rng), 3, w, 1024, add=add))
    return out


# ------------------------------------------------------------------ V4: degenerate windows
V4_WINDOWS = (0.0, 4.9e-7, 5e-7)


def _v4(small):
    """Windows that quantize to 0 (every record closes) and to 1 us, receive time strictly
    increasing per flow by 1..4 us; 25 % duplicates (of the sequence number before) and 10 %
    messages of size 0, so many windows hold their opening record alone.  meta["counted"]: by
    construction, whether Update counts the record (a new, higher sequence number, size > 0).
    per_flow is below the closes: the count crosses it inside a call and, in the splits, is
    already past it when the last call starts.  The last case: ten records under one stamp at
    window 0 (durations of 0: rates of inf and 0 / 0)."""
    rng = np.random.default_rng(104)
    out = []
    m = 150 if small else 1500
    for w in V4_WINDOWS:
        flows, counted = [], []
        for f in range(3):
            rx = (T0 + f) * M + 999_000 + np.cumsum(rng.integers(1, 5, m))
            u = rng.random(m)
            dup, zero = u < 0.25, (u >= 0.25) & (u < 0.35)
            dup[0] = zero[0] = False
            inc = np.where(dup | zero, 0, rng.integers(1, 3, m))
            seq = np.cumsum(inc) + int(rng.integers(0, 1 << 31))
            ln = np.where(zero, 0, 300)
            flows.append({"seq": seq, "tx": rx - rng.integers(-200, 500, m), "rx": rx,
                          "msg_len": ln})
            counted.append(~(dup | zero))
        cols = merge(flows, rng)
        n = len(cols["seq"])
        out.append(case(f"V4-w{w}", cols, 3, w, 40 if small else 700,
                        splits=((0,), (0, 1), (0, 1, n // 3, 2 * n // 3)), counted=counted))
    if not small:
        one = {"seq": np.array([5, 6, 6, 7, 7, 8, 9, 9, 10, 11]), "msg_len": np.array(
            [100, 100, 100, 0, 100, 100, 100, 100, 0, 100]),
            "tx": np.full(10, T0 * M), "rx": np.full(10, T0 * M + 250)}
        out.append(case("V4-zero-duration", merge([one], rng), 1, 0.0, 16,
                        splits=((0,), (0, 1), (0, 1, 4))))
    return out


# ------------------------------------------------------------------ V5: the receive clock
def _v5(small):
    """Flow 0: the receive clock steps back by 1 s, forward again, back by 1 h and forward
    again.  Flow 1: a few records, a silence of two windows, then thousands of records under
    one stamp (the first closes, the rest lie in the window it opens).  Flow 2: rx_usec of 10^6
    and more, compensated in rx_sec or not, each after a silence so that it closes a window
    (window_end is normalised from it)."""
    rng = np.random.default_rng(105)
    window, wus = 0.05, 50_000
    m = 150 if small else 3000
    f0 = _flow(rng, m, T0 * M, 700.0, rng.integers(50, 500, m), _lens(rng, m))
    n0 = len(f0["seq"])
    for p, d in ((n0 // 5, -M), (2 * n0 // 5, M + 3 * wus), (3 * n0 // 5, -3600 * M),
                 (4 * n0 // 5, 3600 * M + 3 * wus)):
        f0["rx"][p:] += d
    k = 200 if small else 5000
    pre = _flow(rng, 40, T0 * M, 700.0, rng.integers(50, 500, 40), _lens(rng, 40), dup=0.0)
    stamp = int(pre["rx"].max()) + 2 * wus
    inc = rng.integers(1, 3, k)
    inc[rng.random(k) < 0.05] = 0
    f1 = {"seq": np.concatenate([pre["seq"], (int(pre["seq"][-1]) + 5000 + np.cumsum(inc))
                                 & 0xFFFFFFFF]),
          "tx": np.concatenate([pre["tx"], stamp - rng.integers(50, 500, k)]),
          "rx": np.concatenate([pre["rx"], np.full(k, stamp)]),
          "msg_len": np.concatenate([pre["msg_len"], _lens(rng, k)])}
    m2 = 100 if small else 2000
    f2 = _flow(rng, m2, T0 * M + 400_000, 700.0, rng.integers(50, 500, m2), _lens(rng, m2),
               reorder_us=0.0)
    n2 = len(f2["seq"])
    at = np.arange(n2 // 12, n2, n2 // 12)
    carry = (1, 2, 3, 4293, 1, 1000)             # seconds moved into rx_usec
    for e, p in enumerate(at):                   # a silence of carry + 1 s: the record closes
        for key in ("tx", "rx"):
            f2[key][p:] += (carry[e % len(carry)] + 1) * M
    s2 = split(f2)
    for e, p in enumerate(at):                   # the same instant, unnormalised
        s2["rx_sec"][p] -= carry[e % len(carry)]
        s2["rx_usec"][p] += carry[e % len(carry)] * M
    return [case("V5", merge([f0, f1, s2], rng), 3, window, 256, same_stamp=k)]


# ------------------------------------------------------------------ V6: high rx_sec
def _v6(small):
    """Receive times across 2^31 s, and from 2^32 - 700 s to the last second a u32 holds: every
    flow ends with records in second 0xFFFFFFFF after a silence, so a window closes there and
    the next one ends past 2^32 s -- with window 600 after the first close already.  The
    splits put a call boundary after that point (the state is loaded with such an end)."""
    rng = np.random.default_rng(106)
    m = 150 if small else 3000
    flows = [_flow(rng, m, ((1 << 31) - 1) * M + 100_000 * f, 700.0, rng.integers(50, 500, m),
                   _lens(rng, m)) for f in range(3)]
    out = [case("V6-2^31", merge(flows, rng), 3, 0.05, 128)]
    top = (1 << 32) - 1
    m = 150 if small else 2000
    for w in (1.0, 600.0):
        flows = []
        for f in range(3):
            rx = np.sort(rng.integers((top - 699) * M, (top - 3) * M, m))
            rx = np.concatenate([rx, top * M + np.array([5, 5, 100_000, 400_000, 999_998, 999_999])])
            n = len(rx)
            inc = rng.integers(1, 3, n)
            inc[rng.random(n) < 0.03] = 0
            flows.append({"seq": (np.cumsum(inc) + int(rng.integers(0, 1 << 32))) & 0xFFFFFFFF,
                          "tx": rx - rng.integers(50, 500, n), "rx": rx,
                          "msg_len": _lens(rng, n)})
        cols = merge(flows, rng)
        n = len(cols["seq"])
        out.append(case(f"V6-2^32-w{w}", cols, 3, w, 1024,
                        splits=((0,), (0, 1), (0, 1, n // 2, n - 9, n - 3))))
    return out


# ------------------------------------------------------------------ V7: sizes
V7_LONG = 1_200_000


def _v7_short(rng, m, t0_us):
    return [_flow(rng, m, t0_us + f, 700.0, rng.integers(50, 500, m),
                  _lens(rng, m, (0, 1, 65535), 0.0)) for f in range(3)]


def _v7(small):
    """Sizes 0, 1 and 65535 on three jumpy flows (V7-short); then, beside such flows, one flow
    of 1,200,000 in-order records of 65,535 B in one call: at window 600 with no close (the
    per-lane 32-bit byte partials reach their fold), and at window 1.0 with a close every few
    thousand records (the byte restart at msg_count == 1 meets pending partials)."""
    rng = np.random.default_rng(107)
    out = [case("V7-short", merge(_v7_short(rng, 100 if small else 3000, T0 * M), rng), 3, 0.05,
                128)]
    if small:
        return out
    for w, gap in ((600.0, 100), (1.0, 337)):
        rx = T0 * M + gap * np.arange(1, V7_LONG + 1, dtype=np.int64)
        big = {"seq": (np.arange(V7_LONG, dtype=np.int64) + 0xFFF00000) & 0xFFFFFFFF,
               "tx": rx - 150, "rx": rx, "msg_len": np.full(V7_LONG, 65535)}
        flows = [big] + _v7_short(rng, 400, T0 * M)
        out.append(case(f"V7-long-w{w}", merge(flows, rng), 4, w, 512, splits=((0,), (0, 1))))
    return out


_BUILD = {"V1": _v1, "V2": _v2, "V3": _v3, "V4": _v4, "V5": _v5, "V6": _v6, "V7": _v7}


@functools.lru_cache(maxsize=None)
def cases(family, small=False):
    """The family's cases; small: reduced copies of at most 600 records (the worker's)."""
    out = _BUILD[family](small)
    assert not small or all(c["n"] <= 600 for c in out), [(c["name"], c["n"]) for c in out]
    return tuple(out)


def by_name(name, small=False):
    return next(c for c in cases(name[:2], small) if c["name"] == name)


NAMES = {"V1": ("V1",), "V2": ("V2",), "V3": tuple(f"V3-w{w}" for w in V3_WINDOWS),
         "V4": tuple(f"V4-w{w}" for w in V4_WINDOWS) + ("V4-zero-duration",), "V5": ("V5",),
         "V6": ("V6-2^31", "V6-2^32-w1.0", "V6-2^32-w600.0"),
         "V7": ("V7-short", "V7-long-w600.0", "V7-long-w1.0")}
FULL_ONLY = ("V4-zero-duration", "V7-long-w600.0", "V7-long-w1.0")


def names(small=False, families=FAMILIES):
    """the case names, without building a case (test ids are made at collection)"""
    return [n for fam in families for n in NAMES[fam] if not (small and n in FULL_ONLY)]


@functools.lru_cache(maxsize=None)
def oracle_run(name, small=False, per_flow=None):
    """(flows, reports[n_flows, per_flow], counts) of the oracle over the whole case, computed
    once and shared."""
    from oracle import oracle as O
    c = by_name(name, small)
    d = c["cols"]
    return O.flow_reduce_batch(c["n_flows"], d["idx"], d["seq"], d["tx_sec"], d["tx_usec"],
                               d["msg_len"], d["rx_sec"], d["rx_usec"], window=c["window"],
                               per_flow=c["per_flow"] if per_flow is None else per_flow)


def numpy_latency(d, i):
    """ProtoTime::Delta(rx, tx) of records i in NumPy (which does not fuse the multiply-add)"""
    rs, ru, ts, tu = (d[k][i].astype(np.int64) for k in ("rx_sec", "rx_usec", "tx_sec", "tx_usec"))
    return (rs - ts).astype(np.float64) + 1e-6 * (ru - tu).astype(np.float64)


def v4_pins(c, ocnt):
    """V4's independent pin: [(flow, report index, latency)] for every kept report whose window
    was opened by a counted record (not the flow's first) and closed by one that is not counted
    -- it must have msg_count 1 and latency_ave == min == max == the opener's latency.  Every
    record after a flow's first closes a window, so record j closes report j - 1."""
    out = []
    for f, counted in enumerate(c["meta"]["counted"]):
        pos = flow_records(c, f)
        assert int(ocnt[f]) == len(pos) - 1
        j = np.flatnonzero(counted[1:-1] & ~counted[2:]) + 1         # openers
        j = j[j < c["per_flow"]]
        lat = numpy_latency(c["cols"], pos[j])
        out += [(f, int(r), float(x)) for r, x in zip(j, lat)]
    return out


# ------------------------------------------------------------------ comparing
F8 = ("duration", "rate", "loss", "latency_ave", "latency_min", "latency_max")


def reports_equal(got, want):
    """Byte-equal, except: where the oracle's double is NaN, the other must be NaN (any sign
    or payload)."""
    from oracle.oracle import REPORT_DTYPE
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1).view(REPORT_DTYPE).copy()
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1).view(REPORT_DTYPE).copy()
    for k in F8:
        nan = np.isnan(w[k])
        if not np.isnan(g[k][nan]).all():
            return False
        g[k][nan] = w[k][nan] = 0.0
    return g.tobytes() == w.tobytes()


def compare(st, rep, cnt, oflows, orep, ocnt, per_flow, rrec=None):
    """State, counts and kept reports against the oracle (as test_gpu_analytics.compare, with
    the NaN rule); every report slot -- and report_rec slot -- at or past min(count, per_flow)
    still holds the FILL bytes it was given."""
    assert np.array_equal(cnt, ocnt)
    raw = np.ascontiguousarray(rep).view(np.uint8).reshape(len(oflows), per_flow, -1)
    for f, a in enumerate(oflows):
        s = st[f]
        assert s["msg_count"] == a.msg_count and s["byte_count"] == a.byte_count, f
        assert s["dup_count"] == a.dup_msg_count and s["n_reports"] == a.n_reports, f
        assert s["seq_start"] == a.seq_start and s["window_valid"] == a.window_valid, f
        assert s["latency_sum"] == a.latency_sum, (f, s["latency_sum"], a.latency_sum)
        assert s["latency_min"] == a.latency_min and s["latency_max"] == a.latency_max, f
        assert (s["win_start_sec"], s["win_start_usec"]) == (a.window_start.sec,
                                                             a.window_start.usec), f
        assert (s["win_end_sec"], s["win_end_usec"]) == (a.window_end.sec, a.window_end.usec), f
        assert s["mask_n"] == a.nset, f
        if a.nset:
            assert s["mask_first"] == a.first, f
            assert s["mask"].tobytes() == bytes(a.bits), f
        k = min(int(ocnt[f]), per_flow)
        assert reports_equal(rep[f, :k], orep[f, :k]), f
        assert (raw[f, k:] == FILL).all(), f
        if rrec is not None:
            assert (rrec[f, k:] == FILL * 0x01010101).all(), f
