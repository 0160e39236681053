"""Serial model of the windowed latency percentiles (mgenx_flow_series_quantiles in
include/mgenx.h), written from the contract alone: plain Python integers, every cell's latencies
collected, sorted and indexed by the rank rule; no code shared with the product.  The data sets
come from flow_dist_ref / flow_series_ref; the generators of the value-domain and size-ladder
tests are here because the CPU and GPU tests share them."""
import numpy as np

from flow_dist_ref import COLS, NONE  # noqa: F401  (data only)

I64_MIN = -2**63
PERMILLE = [1, 250, 500, 950, 990, 999, 1000]
WIDE = 2**40          # a window of 2**40 us: 3907 of them cover every u32 second


def rank(q: int, c: int) -> int:
    """1 <= rank <= c for permille q in 1..1000 over c >= 1 values."""
    return max(1, (q * c + 999) // 1000)


def cells(n_flows, n_bins, flow_idx, c, t0_us, width_us, n=None):
    """{(flow, bin): [lat, ...]} over the records that count, Python integers."""
    n = len(flow_idx) if n is None else n
    t0_us, width_us = int(t0_us), int(width_us)
    assert width_us >= 1 and n_bins >= 1
    fi = np.asarray(flow_idx[:n], np.uint32).tolist()
    ts, tu = c["tx_sec"][:n].tolist(), c["tx_usec"][:n].tolist()
    rs, ru = c["rx_sec"][:n].tolist(), c["rx_usec"][:n].tolist()
    out = {}
    for i in range(n):
        f = fi[i]
        if f >= n_flows:
            continue
        rx = rs[i] * 10**6 + ru[i]
        b = (rx - t0_us) // width_us                    # Python's // is the signed floor
        if 0 <= b < n_bins:
            out.setdefault((f, b), []).append((rs[i] - ts[i]) * 10**6 + ru[i] - tu[i])
    return out


def model(n_flows, n_bins, flow_idx, c, t0_us, width_us, permille, n=None, sizes=None):
    """int64 [n_flows, n_bins, len(permille)]; `sizes`, a dict, receives {(flow, bin): size}."""
    out = np.full((n_flows, n_bins, len(permille)), I64_MIN, np.int64)
    for (f, b), lat in cells(n_flows, n_bins, flow_idx, c, t0_us, width_us, n).items():
        lat.sort()
        if sizes is not None:
            sizes[(f, b)] = len(lat)
        for j, q in enumerate(permille):
            out[f, b, j] = lat[rank(int(q), len(lat)) - 1]
    return out


# ---------------------------------------------------------------------------- generators
def cols_for_lat(rx, lat):
    """Columns whose receive time is rx and whose latency is lat (Python / int64 microseconds):
    tx = rx - lat split into seconds and microseconds; every tx must fall in the u32 seconds."""
    rx = np.asarray(rx, np.int64)
    tx = rx - np.asarray(lat, np.int64)
    assert tx.min() >= 0 and tx.max() < 2**32 * 10**6
    return {"tx_sec": (tx // 10**6).astype(np.uint32), "tx_usec": (tx % 10**6).astype(np.uint32),
            "rx_sec": (rx // 10**6).astype(np.uint32), "rx_usec": (rx % 10**6).astype(np.uint32)}


def wild_cols(rng, m, rx_sec):
    """m records received within 2 s of rx_sec whose tx_sec and tx_usec are drawn over the whole
    u32 range (so tx_usec >= 10**6 occurs): latencies over about +-2**52 us."""
    return {"tx_sec": rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32),
            "tx_usec": rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32),
            "rx_sec": (rx_sec + rng.integers(0, 2, m)).astype(np.uint32),
            "rx_usec": rng.integers(0, 10**6, m).astype(np.uint32)}


def weave(rng, parts):
    """parts: one dict of columns per flow.  The flows' records interleaved in a shuffled input
    order that keeps every flow's own order; returns (flow_idx, columns)."""
    sizes = [len(p["rx_sec"]) for p in parts]
    flow = np.repeat(np.arange(len(parts)), sizes)
    flow = flow[rng.permutation(len(flow))]
    c = {k: np.zeros(len(flow), np.uint32) for k in ("tx_sec", "tx_usec", "rx_sec", "rx_usec")}
    for f, p in enumerate(parts):
        sel = np.nonzero(flow == f)[0]
        for k in c:
            c[k][sel] = p[k]
    return flow.astype(np.uint32), c


SEC_LOW, SEC_MID, SEC_HIGH = 5, 2**31, 2**32 - 2


def value_domain():
    """(n_flows, flow_idx, columns, t0, width, n_bins, what): every flow in one window of 2**40
    us.  `what` names the flows: wild_low / wild_mid / wild_high (tx over the whole u32 range,
    received near second 5, 2**31 and 2**32 - 2), high_bits (values that differ only above bit
    32), low_byte (only in the low byte), equal (5000 equal values), two (two distinct values),
    ascending / descending (the input order)."""
    rng = np.random.default_rng(71)
    mid = SEC_MID * 10**6
    parts, what = [], {}

    def add(name, p):
        what[name] = len(parts)
        parts.append(p)

    add("wild_low", wild_cols(rng, 3000, SEC_LOW))
    add("wild_mid", wild_cols(rng, 3000, SEC_MID))
    add("wild_high", wild_cols(rng, 3000, SEC_HIGH))
    k = rng.integers(-200, 200, 900)
    add("high_bits", cols_for_lat(mid + rng.integers(0, 10**6, 900), 123 + k * 2**32))
    add("low_byte", cols_for_lat(mid + rng.integers(0, 10**6, 700),
                                 0x1234500 + rng.integers(0, 256, 700)))
    add("equal", cols_for_lat(mid + rng.integers(0, 10**6, 5000), np.full(5000, 777)))
    add("two", cols_for_lat(mid + rng.integers(0, 10**6, 600),
                            np.where(rng.random(600) < 0.4, -5, 2**33 + 1)))
    up = np.sort(rng.integers(-10**6, 10**9, 1500))
    add("ascending", cols_for_lat(mid + rng.integers(0, 10**6, 1500), up))
    add("descending", cols_for_lat(mid + rng.integers(0, 10**6, 1500), up[::-1]))
    fi, c = weave(rng, parts)
    return len(parts), fi, c, 0, WIDE, 3907, what


def ladder_sizes(tier_edges):
    sizes = list(range(1, 131))
    for k in (256, 512, 1024, 2048, 4096, 8192, 16384, 20480, 32768):
        sizes += [k - 1, k, k + 1]
    for e in tier_edges:
        for s in (e - 1, e, e + 1):
            if s >= 1 and s not in sizes:
                sizes.append(s)
    return sizes


def ladder(tier_edges):
    """(n_flows, flow_idx, columns, t0, width, n_bins, sizes): flow f holds sizes[f] records, all
    in window f % 7 of 7 windows of 2**40 us; latencies as wild_cols draws them."""
    rng = np.random.default_rng(72)
    sizes = ladder_sizes(tier_edges)
    parts = [wild_cols(rng, s, (f % 7) * (WIDE // 10**6 + 1) + 10) for f, s in enumerate(sizes)]
    fi, c = weave(rng, parts)
    return len(sizes), fi, c, 0, WIDE, 7, sizes
