"""mgenx_flow_series_quantiles beside mgenx_flow_series and beside a library-sort form of the
same result, in one run: config 4's columns (poisson_flows(8_388_608, 1024)), device-resident,
windows of 1 s and of 1 ms, permille (500, 950, 990).

The library-sort form is the yardstick and is written here from torch operations: latency and
cell id by tensor arithmetic, torch.sort by latency, a stable torch.sort by cell, ranks by index
arithmetic.  Its columns are widened to int64 outside the timed window (which favours it).  It
must give the array the new call gives before anything is timed.

Device events around each call, outputs preallocated, the three calls taking turns; median of
--iters after --warmup with min-max.  Prints one JSON line per width.  The bar: the new call's
median is no slower than the library-sort form's median by more than that form's own min-max
spread in the same run.  --only quant|series|sort with --width-us runs a single call kind (for a
kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/flow_quant_time.py --only quant
--width-us 1000).  --rehearse runs the library-sort form on the CPU at a tiny size against a
serial loop and needs no device."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd.workloads import poisson_flows  # noqa: E402

I64_MIN = -2**63

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width-us", type=int, action="append")
ap.add_argument("--permille", default="500,950,990")
ap.add_argument("--only", choices=("quant", "series", "sort"))
ap.add_argument("--rehearse", action="store_true")
a = ap.parse_args()
permille = [int(v) for v in a.permille.split(",")]
assert 1 <= len(permille) <= 32 and all(1 <= q <= 1000 for q in permille)
widths = a.width_us or [1_000_000, 1_000]


def sort_form(fi, ts, tu, rs, ru, n_flows, n_bins, t0, width, out):
    """int64 columns (fi: the flow index widened, 2**32 - 1 for MGENX_FLOW_NONE) -> out
    [n_flows * n_bins, n_q]."""
    n_cells = n_flows * n_bins
    rx = rs * 1_000_000 + ru
    lat = (rs - ts) * 1_000_000 + ru - tu
    b = torch.div(rx - t0, width, rounding_mode="floor")
    ok = (fi < n_flows) & (b >= 0) & (b < n_bins)
    cell = torch.where(ok, fi * n_bins + b, n_cells)
    lat, by_lat = torch.sort(lat)
    cell, by_cell = torch.sort(cell[by_lat], stable=True)
    lat = lat[by_cell]
    count = torch.bincount(cell, minlength=n_cells + 1)[:n_cells]
    start = torch.cumsum(count, 0) - count
    last = lat.numel() - 1
    for j, q in enumerate(permille):
        r = torch.clamp((q * count + 999) // 1000, min=1)
        v = lat[torch.clamp(start + r - 1, max=last)]
        out[:, j] = torch.where(count > 0, v, I64_MIN)
    return out


def columns(n, flows):
    d = poisson_flows(n, flows)
    fi = (d["flow_id"] - 1).astype(np.uint32)
    return fi, {k: np.ascontiguousarray(d[k]) for k in
                ("seq", "tx_sec", "tx_usec", "msg_len", "rx_sec", "rx_usec")}


def span(c):
    rx = c["rx_sec"].astype(np.int64) * 10**6 + c["rx_usec"].astype(np.int64)
    return int(rx.min()), int(rx.max())


if a.rehearse:
    n, flows = min(a.n, 20_000), min(a.flows, 16)
    fi, c = columns(n, flows)
    fi[::97] = 0xFFFFFFFF
    lo, hi = span(c)
    for width in widths:
        t0 = lo + 3 * width // 2                     # some records before the first window
        n_bins = max((hi - t0) // width, 1)          # and some past the last
        wide = [torch.from_numpy(v.astype(np.int64)) for v in
                (fi, c["tx_sec"], c["tx_usec"], c["rx_sec"], c["rx_usec"])]
        got = sort_form(*wide, flows, n_bins, t0, width,
                        torch.empty((flows * n_bins, len(permille)), dtype=torch.int64)).numpy()
        cells = {}
        for i in range(len(fi)):
            rx = int(c["rx_sec"][i]) * 10**6 + int(c["rx_usec"][i])
            b = (rx - t0) // width
            if fi[i] < flows and 0 <= b < n_bins:
                cells.setdefault(int(fi[i]) * n_bins + b, []).append(
                    (int(c["rx_sec"][i]) - int(c["tx_sec"][i])) * 10**6 +
                    int(c["rx_usec"][i]) - int(c["tx_usec"][i]))
        want = np.full((flows * n_bins, len(permille)), I64_MIN, np.int64)
        for k, v in cells.items():
            v.sort()
            want[k] = [v[max(1, (q * len(v) + 999) // 1000) - 1] for q in permille]
        assert np.array_equal(got, want), width
        print(json.dumps({"rehearsal": "ok", "width_us": width, "records": len(fi),
                          "cells": flows * n_bins, "non_empty": len(cells)}), flush=True)
    sys.exit(0)

assert torch.cuda.is_available(), "this measurement needs the GPU"
from mgen_amd import Engine, _ptr, _stream  # noqa: E402

eng = Engine(0)
fi, c = columns(a.n, a.flows)
n = len(fi)
lo, hi = span(c)
idx = torch.from_numpy(fi).cuda()
col = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
wide = [torch.from_numpy(v.astype(np.int64)).cuda() for v in
        (fi, c["tx_sec"], c["tx_usec"], c["rx_sec"], c["rx_usec"])]


def timed(setup, call):
    setup()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for width in widths:
    t0, n_bins = lo, (hi - lo) // width + 1
    n_cells = a.flows * n_bins
    out = torch.empty((a.flows, n_bins, len(permille)), dtype=torch.int64, device="cuda")
    out2 = torch.empty((n_cells, len(permille)), dtype=torch.int64, device="cuda")
    state, bins = eng.flow_series_init(a.flows, n_bins)
    lib, ctx, s = eng.lib, eng.ctx, _stream(0)

    def quant():
        eng.flow_series_quantiles(a.flows, n_bins, t0, width, permille, idx, col["tx_sec"],
                                  col["tx_usec"], col["rx_sec"], col["rx_usec"], out=out)

    def series():
        eng.flow_series(state, bins, a.flows, n_bins, t0, width, idx, col["seq"], col["tx_sec"],
                        col["tx_usec"], col["msg_len"], col["rx_sec"], col["rx_usec"])

    def sort():
        sort_form(*wide, a.flows, n_bins, t0, width, out2)

    def init_series():
        lib.mgenx_flow_series_init(ctx, _ptr(state), _ptr(bins), a.flows, n_bins, s)

    # the gate: the yardstick and the new call agree on every element
    quant()
    sort()
    torch.cuda.synchronize()
    assert torch.equal(out.view(n_cells, len(permille)), out2), "library-sort form differs"
    non_empty = int((out2[:, 0] != I64_MIN).sum().item())

    kinds = {"quant": (lambda: None, quant), "series": (init_series, series),
             "sort": (lambda: None, sort)}
    if a.only:
        kinds = {a.only: kinds[a.only]}
    ms = {k: [] for k in kinds}
    for it in range(a.warmup + a.iters):
        for k, (setup, call) in kinds.items():     # taking turns: the same drift for each
            t = timed(setup, call)
            if it >= a.warmup:
                ms[k].append(t)
    res = {"width_us": width, "records": n, "flows": a.flows, "n_bins": n_bins, "cells": n_cells,
           "non_empty_cells": non_empty, "permille": permille, "iters": a.iters,
           "algorithmic_bytes": 20 * n + n_cells * len(permille) * 8}
    name = {"quant": "flow_series_quantiles", "series": "flow_series", "sort": "library_sort"}
    for k, v in ms.items():
        res[name[k] + "_ms"] = round(statistics.median(v), 4)
        res[name[k] + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    if "quant" in ms and "sort" in ms:
        spread = max(ms["sort"]) - min(ms["sort"])
        res["bar_ms"] = round(statistics.median(ms["sort"]) + spread, 4)
        res["bar_met"] = statistics.median(ms["quant"]) <= statistics.median(ms["sort"]) + spread
    if "quant" in ms and "series" in ms:
        res["ratio_to_flow_series"] = round(statistics.median(ms["quant"]) /
                                            statistics.median(ms["series"]), 3)
    print(json.dumps(res), flush=True)
    del out, out2, state, bins
eng.close()
