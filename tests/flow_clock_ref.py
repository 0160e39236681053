"""Serial model of mgenx_flow_clock (include/mgenx.h), written from the definitions with Python
integers: the points, Andrew's monotone chain for the lower hull, the edge over the mean send
time, the floored line, the residuals and the corrected stamps.  A different algorithm from the
product's chord search, and no code shared with it.  Also the data sets of the clock tests."""
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
I64_MIN = -2**63
COLS = ("tx_sec", "tx_usec", "rx_sec", "rx_usec")
CLOCK_DTYPE = np.dtype([
    ("n", "<u8"), ("xa", "<u8"), ("da", "<i8"), ("xb", "<u8"), ("db", "<i8"),
    ("resid_sum", "<i8"), ("resid_max", "<i8"), ("ia", "<u4"), ("ib", "<u4")])


def wrap64(v):
    """v modulo 2^64 as a signed value."""
    v &= 2**64 - 1
    return v - 2**64 if v >= 2**63 else v


def points(c):
    """x and d of every record as lists of Python integers."""
    ts, tu, rs, ru = ([int(v) for v in c[k]] for k in COLS)
    x = [a * 10**6 + b for a, b in zip(ts, tu)]
    d = [(p - a) * 10**6 + q - b for a, b, p, q in zip(ts, tu, rs, ru)]
    return x, d


def lower_hull(pts):
    """The vertices of the lower convex hull of a set of (x, d), in increasing x: among equal x
    the lowest d only, no collinear point."""
    h = []
    last_x = None
    for p in sorted(set(pts)):
        if p[0] == last_x:
            continue                    # a higher d at an x already seen
        last_x = p[0]
        while len(h) >= 2:
            (ox, od), (ax, ad) = h[-2], h[-1]
            if (ax - ox) * (p[1] - od) - (ad - od) * (p[0] - ox) <= 0:
                h.pop()                 # h[-1] lies on or above the segment h[-2] .. p
            else:
                break
        h.append(p)
    return h


def fit(pts, offset_only=False):
    """(A, B) of a non-empty list of points."""
    if offset_only:
        low = min(d for _, d in pts)
        a = (min(x for x, d in pts if d == low), low)
        return a, a
    h = lower_hull(pts)
    if len(h) == 1:
        return h[0], h[0]
    n, s = len(pts), sum(x for x, _ in pts)
    edges = [(h[k], h[k + 1]) for k in range(len(h) - 1) if n * h[k][0] <= s < n * h[k + 1][0]]
    assert len(edges) == 1
    return edges[0]


def line(a, b, x):
    if a[0] == b[0]:
        return a[1]
    return a[1] + (b[1] - a[1]) * (x - a[0]) // (b[0] - a[0])      # Python's // floors


def model(n_flows, fi, c, offset_only=False):
    """(clock [n_flows] of CLOCK_DTYPE, resid int64 [n], rx_sec_out, rx_usec_out uint32 [n])."""
    n = len(fi)
    x, d = points(c)
    per = [[] for _ in range(n_flows)]
    for i in range(n):
        if int(fi[i]) < n_flows:
            per[int(fi[i])].append(i)
    clock = np.zeros(n_flows, CLOCK_DTYPE)
    resid = np.full(n, I64_MIN, np.int64)
    sec = np.array(c["rx_sec"], np.uint32).copy()
    usec = np.array(c["rx_usec"], np.uint32).copy()
    for f, idx in enumerate(per):
        if not idx:
            clock[f] = (0, 0, 0, 0, 0, 0, I64_MIN, NONE, NONE)
            continue
        a, b = fit([(x[i], d[i]) for i in idx], offset_only)
        ia = min(i for i in idx if (x[i], d[i]) == a)
        ib = min(i for i in idx if (x[i], d[i]) == b)
        total, most = 0, I64_MIN
        for i in idx:
            ci = wrap64(d[i] - line(a, b, x[i]))
            resid[i] = ci
            r = (x[i] + ci) % 2**64
            sec[i] = (r // 10**6) % 2**32
            usec[i] = r % 10**6
            total += ci
            most = max(most, ci)
        clock[f] = (len(idx), a[0], a[1], b[0], b[1], wrap64(total), most, ia, ib)
    return clock, resid, sec, usec


def brute_force(pts):
    """The least sum of d - line(x) (exact, the line not floored) over every line through two
    points of different x that passes under all points; None when all x are equal."""
    best = None
    for i, (xa, da) in enumerate(pts):
        for (xb, db) in pts[i + 1:]:
            if xa == xb:
                continue
            slope = Fraction(db - da, xb - xa)
            gaps = [Fraction(d - da) - slope * (x - xa) for x, d in pts]
            if min(gaps) >= 0:
                total = sum(gaps)
                best = total if best is None or total < best else best
    return best


def cols_from(x, d):
    """Columns whose points are (x, d): x split at 10^6, the receive stamp x + d likewise."""
    x = np.asarray(x, np.int64)
    r = x + np.asarray(d, np.int64)
    assert (x >= 0).all() and (r >= 0).all() and (r < 2**32 * 10**6).all()
    return {"tx_sec": (x // 10**6).astype(np.uint32), "tx_usec": (x % 10**6).astype(np.uint32),
            "rx_sec": (r // 10**6).astype(np.uint32), "rx_usec": (r % 10**6).astype(np.uint32)}


def weave(rng, flows, nones=0, beyond=0, n_flows=None):
    """The flows' records interleaved in a random order (each flow's own order kept), with
    `nones` records of MGENX_FLOW_NONE and `beyond` records of an index >= n_flows between them.
    flows: a list of column dicts."""
    n_flows = len(flows) if n_flows is None else n_flows
    sizes = [len(c["tx_sec"]) for c in flows]
    fi = np.concatenate([np.full(s, f, np.uint32) for f, s in enumerate(sizes)] +
                        [np.full(nones, NONE, np.uint32),
                         np.full(beyond, n_flows + 5, np.uint32)])
    extra = nones + beyond
    c = {k: np.concatenate([fl[k] for fl in flows] +
                           [rng.integers(0, 2**32, extra, dtype=np.uint64).astype(np.uint32)])
         for k in COLS}
    lab = np.concatenate([np.full(s, g, np.int64) for g, s in enumerate(sizes + [nones, beyond])])
    rng.shuffle(lab)
    at = np.argsort(lab, kind="stable")     # group g's positions, ascending, group after group
    out_fi = np.empty_like(fi)
    out_fi[at] = fi
    out = {}
    for k, v in c.items():
        out[k] = np.empty_like(v)
        out[k][at] = v
    return out_fi, out


# ---- the data sets -------------------------------------------------------------------------
def hand_case():
    """2 flows (and an empty third), 11 records; the hulls are written out in
    tests/test_flow_clock_cpu.py."""
    base = 1_000_000_000
    rows = [  # flow, x - base, d
        (0, 0, 10), (0, 4, 2), (1, 5, -3), (0, 10, 8), (NONE, 3, -100), (0, 2, 6), (0, 4, 2),
        (0, 6, 3), (1, 5, 7), (0, 8, 4), (0, 4, 9)]
    fi = np.array([r[0] for r in rows], np.uint32)
    c = cols_from([base + r[1] for r in rows], [r[2] for r in rows])
    return 3, fi, c


def grid_corpus():
    """2,000 flows of 1..60 records on a small grid, x in 0..8 and d in -5..5: ties, duplicates and
    collinear points everywhere.  MGENX_FLOW_NONE records and indices past n_flows interleaved."""
    rng = np.random.default_rng(3)         # (a draw that meets the corpus condition)
    base = 1_700_000_000 * 10**6 + 999_995      # the grid straddles a second's edge
    flows = []
    for _ in range(2000):
        m = int(rng.integers(1, 61))
        flows.append(cols_from(base + rng.integers(0, 9, m), rng.integers(-5, 6, m)))
    fi, c = weave(rng, flows, nones=700, beyond=300)
    return len(flows), fi, c


def classify(pts):
    """The classes of the corpus condition a flow's point list belongs to."""
    out = set()
    n = len(pts)
    xs = {x for x, _ in pts}
    if len(xs) == 1:
        out.add("all_x_equal")
    if n == 1:
        out.add("n1")
    if n == 2:
        out.add("n2")
    a, b = fit(pts)
    if pts.count(a) > 1:
        out.add("a_repeated")
    if a != b:
        s = sum(x for x, _ in pts)
        if n * a[0] == s:
            out.add("mean_on_vertex")
        if any(a[0] < x < b[0] and (b[0] - a[0]) * (d - a[1]) == (b[1] - a[1]) * (x - a[0])
               for x, d in set(pts)):
            out.add("collinear_on_edge")
        out.add("negative" if b[1] < a[1] else "positive" if b[1] > a[1] else "zero")
        if all((b[0] - a[0]) * (d - a[1]) == (b[1] - a[1]) * (x - a[0]) for x, d in pts):
            out.add("one_line")
    else:
        out.add("zero")
    return out


def tiny_flows():
    """3,000 flows of 0..5 records."""
    rng = np.random.default_rng(2025)
    flows = []
    for _ in range(3000):
        m = int(rng.integers(0, 6))
        flows.append(cols_from(5_000_000 + rng.integers(0, 40, m), rng.integers(-20, 21, m)))
    fi, c = weave(rng, flows, nones=50)
    return len(flows), fi, c


def noisy(rng, m, ppm, offset_us, t_start, spacing_us):
    """m records of one flow: sent about spacing_us apart from t_start, received on a clock that
    runs ppm fast and offset_us ahead, after 150 us plus an exponential delay."""
    x = t_start + np.cumsum(rng.integers(1, 2 * spacing_us, m))
    delay = 150 + rng.exponential(400.0, m).astype(np.int64)
    d = offset_us + (x - t_start) * ppm // 10**6 + delay
    return cols_from(x, d)


def ladder_sizes(edges):
    sizes = []
    for e in edges:
        for s in (e - 1, e, e + 1):
            sizes += [s, 1]
    return sizes


def ladder(edges):
    """One flow at each of (edge - 1, edge, edge + 1) for every edge, flows of 1 record between."""
    rng = np.random.default_rng(2026)
    sizes = ladder_sizes(edges)
    flows = [noisy(rng, s, int(rng.integers(-60, 61)), int(rng.integers(-10**6, 10**6)),
                   1_600_000_000 * 10**6, 300) for s in sizes]
    fi, c = weave(rng, flows, nones=100)
    return len(flows), fi, c, sizes


def dominant(shuffled):
    """One flow of 200,000 records beside 500 small ones; drifts of +-50 ppm and offsets of +-3 s.
    In send order per flow, or with the log order shuffled."""
    rng = np.random.default_rng(2027)
    t0 = 1_650_000_000 * 10**6
    flows = [noisy(rng, 200_000, 50, -3_000_000, t0, 500)]
    for k in range(500):
        flows.append(noisy(rng, int(rng.integers(1, 40)), (-50, 50, 7)[k % 3],
                           (3_000_000, -3_000_000, 1234)[k % 3], t0, 200_000))
    fi, c = weave(rng, flows, nones=300)
    if shuffled:
        p = rng.permutation(len(fi))
        fi, c = fi[p], {k: v[p] for k, v in c.items()}
    return len(flows), fi, c


def parabola(k_tenths):
    """50,000 points d = (i - k)^2 at x = i: every point is a hull vertex.  k at k_tenths tenths
    of the range; a second, short flow beside it."""
    m = 50_000
    k = m * k_tenths // 10
    i = np.arange(m, dtype=np.int64)
    rng = np.random.default_rng(2028)
    big = cols_from(2_000_000_000 + i, (i - k) ** 2)
    p = rng.permutation(m)
    big = {n: v[p] for n, v in big.items()}
    fi, c = weave(rng, [big, cols_from([7, 9, 11], [5, 1, 5])], nones=10)
    return 2, fi, c


def value_domain():
    """The corners of the stamps: each flow a few records.  Returns (n_flows, fi, c, names)."""
    u32 = 2**32 - 1
    rows = {  # name -> list of (tx_sec, tx_usec, rx_sec, rx_usec)
        "tx_high_rx_low": [(u32, 5, 0, 7), (u32 - 1, 999_999, 0, 1), (u32, 900_000, 1, 3),
                           (u32 - 2, 0, 0, 0)],
        "tx_low_rx_high": [(0, 0, u32, 999_999), (1, 5, u32, 3), (2, 7, u32 - 1, 100),
                           (0, 999_999, u32, 0)],
        "usec_past_a_second": [(100, u32, 4400, 17), (100, u32 - 1, 4400, 900), (101, 2 * 10**6, 4400, 5),
                               (4000, 10**6, 4500, u32), (99, 3 * 10**6, 4300, 0)],
        # a latency step of 2^51.9 (the most the stamps hold) across one microsecond as the chosen
        # edge: the mean send time falls exactly on its first point
        "step": [(3000, 9, 3000, 14), (3000, 10, 3000, 11), (3000, 10, 3000, 60),
                 (3000, 11, u32, 11)],
        # the same edge with one record 5000 us to its left, balanced by 5000 records at its upper
        # end: that record's c is 5000 * 2^51.9, leaves 63 bits and is kept modulo 2^64
        "step_far": [(3000, 5000, 3000, 5009), (3000, 10000, 3000, 10001)] +
                    [(3000, 10001, u32, 10001)] * 5000,
        "x_zero": [(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 5)],
    }
    names = list(rows)
    fi = np.concatenate([np.full(len(rows[k]), f, np.uint32) for f, k in enumerate(names)])
    flat = [r for k in names for r in rows[k]]
    c = {k: np.array([r[j] for r in flat], np.uint32) for j, k in enumerate(COLS)}
    p = np.random.default_rng(2029).permutation(len(fi))
    return len(names), fi[p], {k: v[p] for k, v in c.items()}, {k: f for f, k in enumerate(names)}


def drift_log(m=4000):
    """A synthetic text log of two flows whose receive stamps are (1 + 40e-6) t + 2.5 s + delay,
    with its parsed columns: (log bytes, n_flows, fi, c) where c also holds seq and msg_len."""
    rng = np.random.default_rng(2030)
    t0 = 1_700_000_000 * 10**6
    tx = t0 + np.cumsum(rng.integers(200, 1800, m))
    delay = 120 + rng.exponential(300.0, m).astype(np.int64)
    rx = tx + (tx - t0) * 40 // 10**6 + 2_500_000 + delay
    fi = (np.arange(m) % 3 == 0).astype(np.uint32)
    seq = np.where(fi == 0, np.cumsum(fi == 0), np.cumsum(fi == 1)).astype(np.uint32) - 1
    lines = []
    for i in range(m):
        if i % 900 == 13:
            lines.append("1700000000.000001 START Mgen Version 5.1.1\n")
        lines.append("%d.%06d RECV proto>UDP flow>%d seq>%d src>10.0.0.%d/5001 dst>10.0.0.9/5000 "
                     "sent>%d.%06d size>%d \n" % (
                         rx[i] // 10**6, rx[i] % 10**6, fi[i] + 1, seq[i], fi[i] + 1,
                         tx[i] // 10**6, tx[i] % 10**6, 100 + i % 7))
    c = cols_from(tx, rx - tx)
    c["seq"] = seq
    c["msg_len"] = (100 + np.arange(m) % 7).astype(np.uint16)
    return "".join(lines).encode(), 2, fi, c
