"""mgenx_flow_clock beside mgenx_flow_dist (no histogram) in one run.  Two shapes:
  config4   poisson_flows(8_388_608, 1024) with a synthetic drift added to the receive stamps
            (flow f's receiver clock runs (f % 101 - 50) ppm fast and (f % 7 - 3) s ahead);
  oneflow   the same records as one flow (the known weak case: one workgroup walks them all).
Columns device-resident, device events around each call, the two calls taking turns; median of
--iters after --warmup, with min and max.  Also the rounds of the chord search that the longest
flow took, counted by a numpy model of the search in this script (not a library output).  Prints
one JSON line.  --only clock|dist runs a single call kind (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/flow_clock_time.py --only clock --iters 5)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import Engine, FLOW_CLOCK_DTYPE, _ptr, _stream  # noqa: E402
from mgen_amd.workloads import poisson_flows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--shape", choices=("config4", "oneflow"), default="config4")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=("clock", "dist"))
ap.add_argument("--outputs", choices=("all", "none"), default="all",
                help="with or without the three per-record outputs")
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
d = poisson_flows(a.n, a.flows)
n = len(d["seq"])
flow = (d["flow_id"] - 1).astype(np.uint32)
tx = d["tx_sec"].astype(np.int64) * 10**6 + d["tx_usec"]
rx = d["rx_sec"].astype(np.int64) * 10**6 + d["rx_usec"]
f64 = flow.astype(np.int64)
rx = rx + (f64 % 7 - 3) * 10**6 + (tx - tx.min()) * (f64 % 101 - 50) // 10**6
assert rx.min() >= 0
n_flows = a.flows
if a.shape == "oneflow":
    flow = np.zeros(n, np.uint32)
    n_flows = 1
cols = dict(flow_idx=flow, seq=d["seq"], tx_sec=d["tx_sec"], tx_usec=d["tx_usec"],
            rx_sec=(rx // 10**6).astype(np.uint32), rx_usec=(rx % 10**6).astype(np.uint32))


def search_rounds(x, lat):
    """The rounds of the product's chord search on one flow (floats would not do: int64 holds
    these keys, the spans here being far below 2^31 us and 2^31 us)."""
    n_pts, s = len(x), int(x.sum())
    il = np.lexsort((lat, x))[0]
    ir = np.lexsort((lat, -x))[0]
    L, R = (int(x[il]), int(lat[il])), (int(x[ir]), int(lat[ir]))
    rounds = 0
    while L[0] != R[0]:
        rounds += 1
        inside = (x > L[0]) & (x < R[0])
        if not inside.any():
            break
        xi, di = x[inside], lat[inside]
        key = (R[0] - L[0]) * (di - L[1]) - (R[1] - L[1]) * (xi - L[0])
        k = int(key.min())
        if k >= 0:
            break
        m = np.flatnonzero(key == k)
        j = m[np.argmin(xi[m])]
        M = (int(xi[j]), int(di[j]))
        if n_pts * M[0] <= s:
            L = M
        else:
            R = M
    return rounds


big = int(np.bincount(flow, minlength=n_flows).argmax())
sel = flow == big
x0 = tx[sel] - tx.min()
rounds = search_rounds(x0, (rx - tx)[sel])


def cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).cuda()


C = {k: cuda(v) for k, v in cols.items()}
msg_len = torch.from_numpy(np.ascontiguousarray(d["msg_len"])).cuda()
dist, _ = eng.flow_dist_init(n_flows, hist=False)
lib, ctx, s = eng.lib, eng.ctx, _stream(0)
clock = torch.empty(n_flows * FLOW_CLOCK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
resid = sec = usec = None
if a.outputs == "all":
    resid = torch.empty(n, dtype=torch.int64, device="cuda")
    sec = torch.empty(n, dtype=torch.int32, device="cuda")
    usec = torch.empty(n, dtype=torch.int32, device="cuda")


def fit():
    rc = lib.mgenx_flow_clock(ctx, _ptr(C["flow_idx"]), _ptr(C["tx_sec"]), _ptr(C["tx_usec"]),
                              _ptr(C["rx_sec"]), _ptr(C["rx_usec"]), n, n_flows, 0, _ptr(clock),
                              _ptr(resid), _ptr(sec), _ptr(usec), s)
    assert rc == 0


def timed(setup, call):
    setup()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = {
    "clock": (lambda: None, fit),
    "dist": (lambda: lib.mgenx_flow_dist_init(ctx, _ptr(dist), None, n_flows, s),
             lambda: eng.flow_dist(dist, None, n_flows, C["flow_idx"], C["seq"], C["tx_sec"],
                                   C["tx_usec"], msg_len, C["rx_sec"], C["rx_usec"])),
}
if a.only:
    kinds = {a.only: kinds[a.only]}
ms = {k: [] for k in kinds}
for it in range(a.warmup + a.iters):
    for k, (setup, call) in kinds.items():     # taking turns: the same drift for each
        t = timed(setup, call)
        if it >= a.warmup:
            ms[k].append(t)
out = {"shape": a.shape, "records": n, "flows": n_flows, "iters": a.iters, "outputs": a.outputs,
       "longest_flow": int(sel.sum()), "search_rounds_longest_flow": rounds}
if "clock" in ms:
    f = clock.cpu().numpy().view(FLOW_CLOCK_DTYPE)
    e = f[big]
    out.update(fitted=int((f["ia"] != 0xFFFFFFFF).sum()),
               longest_flow_skew_ppb=10**9 * int(e["db"] - e["da"]) // max(int(e["xb"] - e["xa"]), 1))
for k, v in ms.items():
    name = {"clock": "flow_clock", "dist": "flow_dist_nohist"}[k]
    out[name + "_ms"] = round(statistics.median(v), 4)
    out[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
if len(ms) == 2:
    out["ratio_to_flow_dist"] = round(out["flow_clock_ms"] / out["flow_dist_nohist_ms"], 3)
print(json.dumps(out), flush=True)
eng.close()
