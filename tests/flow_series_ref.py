"""Serial model of the per-flow time series (mgenx_flow_series in include/mgenx.h), written from
the definitions alone: plain Python integers, one flow at a time, record by record, no code shared
with the product.  Also the data set `shuffled_rx`; the others come from flow_dist_ref."""
import numpy as np

from flow_dist_ref import COLS, NONE, _synth  # noqa: F401  (data only)

I64_MAX, I64_MIN = 2**63 - 1, -2**63
U64, U32 = 2**64, 2**32

# struct mgenx_flow_series_bin / mgenx_flow_series_state, restated
BIN = np.dtype([
    ("n", "<u8"), ("bytes", "<u8"), ("lat_sum", "<i8"), ("lat_min", "<i8"), ("lat_max", "<i8"),
    ("jitter_sum", "<u8"), ("advance", "<u8"), ("fresh", "<u4"), ("late", "<u4")])
STATE = np.dtype([
    ("n", "<u8"), ("last_lat", "<i8"), ("outside", "<u8"), ("seq_max", "<u4"), ("rsv", "<u4")])


def fresh(n_flows: int, n_bins: int):
    state = np.zeros(n_flows, STATE)
    bins = np.zeros((n_flows, n_bins), BIN)
    bins["lat_min"] = I64_MAX
    bins["lat_max"] = I64_MIN
    return state, bins


def _wrap64(v: int) -> int:
    """v modulo 2**64 as a signed value."""
    v %= U64
    return v - U64 if v >= 2**63 else v


def update(state, bins, flow_idx, c, t0_us, width_us, n=None):
    """The records of c (dict of COLS) in receive order, added to state / bins in place."""
    n = len(flow_idx) if n is None else n
    n_flows, n_bins = bins.shape
    t0_us, width_us = int(t0_us), int(width_us)
    assert width_us >= 1 and n_bins >= 1
    fi = np.asarray(flow_idx[:n], np.uint32)
    col = {k: c[k][:n].tolist() for k in COLS}
    for f in np.unique(fi[fi < n_flows]).tolist():
        st = state[f]
        cnt, last_lat, outside = int(st["n"]), int(st["last_lat"]), int(st["outside"])
        m = int(st["seq_max"])
        touched = {}                                    # bin -> dict of python integers
        for i in np.nonzero(fi == f)[0].tolist():       # receive order
            seq, size = col["seq"][i], col["msg_len"][i]
            rx = col["rx_sec"][i] * 10**6 + col["rx_usec"][i]
            lat = (col["rx_sec"][i] - col["tx_sec"][i]) * 10**6 + col["rx_usec"][i] - col["tx_usec"][i]
            first = cnt == 0
            b = (rx - t0_us) // width_us                # Python's // is the signed floor
            if 0 <= b < n_bins:
                e = touched.get(b)
                if e is None:
                    e = touched[b] = {k: int(bins[f, b][k]) for k in BIN.names}
                e["n"] += 1
                e["bytes"] += size
                e["lat_sum"] += lat
                e["lat_min"] = min(e["lat_min"], lat)
                e["lat_max"] = max(e["lat_max"], lat)
                if not first:
                    e["jitter_sum"] += abs(lat - last_lat)
                if first:
                    e["fresh"] += 1
                    e["advance"] += 1
                elif seq > m:
                    e["fresh"] += 1
                    e["advance"] += seq - m
                elif seq < m:
                    e["late"] += 1
            else:
                outside += 1
            m = seq if first else max(m, seq)
            last_lat = lat
            cnt += 1
        for b, e in touched.items():
            bins[f, b] = (e["n"] % U64, e["bytes"] % U64, _wrap64(e["lat_sum"]), e["lat_min"],
                          e["lat_max"], e["jitter_sum"] % U64, e["advance"] % U64,
                          e["fresh"] % U32, e["late"] % U32)
        state[f] = (cnt, last_lat, outside, m, 0)


def model(n_flows, n_bins, flow_idx, c, t0_us, width_us, n=None):
    state, bins = fresh(n_flows, n_bins)
    update(state, bins, flow_idx, c, t0_us, width_us, n)
    return state, bins


def rx_us(c):
    return c["rx_sec"].astype(np.int64) * 10**6 + c["rx_usec"].astype(np.int64)


def span(n_flows, flow_idx, c):
    """(lowest, highest) receive time over the counted records."""
    rx = rx_us(c)[np.asarray(flow_idx) < n_flows]
    return int(rx.min()), int(rx.max())


# ---------------------------------------------------------------------------- data set
def shuffled_rx(n=8000):
    """4 flows, n records: within each flow the receive times are permuted in blocks of 50, so a
    flow's bins are not contiguous in sorted order (the latency moves with them: tx stays)."""
    rng = np.random.default_rng(41)
    flow = rng.integers(0, 4, n)
    seq = np.zeros(n, np.int64)
    for f in range(4):
        sel = np.nonzero(flow == f)[0]
        seq[sel] = np.arange(len(sel))
    fi, c = _synth(flow, seq, 42)
    rx = rx_us(c)
    for f in range(4):
        sel = np.nonzero(flow == f)[0]
        for a in range(0, len(sel), 50):
            blk = sel[a:a + 50]
            rx[blk] = rx[blk][rng.permutation(len(blk))]
    c = dict(c)
    c["rx_sec"] = (rx // 10**6).astype(np.uint32)
    c["rx_usec"] = (rx % 10**6).astype(np.uint32)
    return 4, fi, c
