"""mgenx_flow_dist beside mgenx_flow_reduce on the same records, in one run: config 4's shape
(poisson_flows(8_388_608, 1024)) and its one-dominant-flow form (half of the records rewritten
to flow 0).  Device events around each call, outputs preallocated and set up again outside the
timed window, the three calls taking turns; median of --iters after --warmup.  Prints one JSON
line per shape.  --only hist|nohist|reduce with --shape runs a single call kind (for a kernel
trace: rocprofv3 --kernel-trace --stats -- python scripts/flow_dist_time.py --only hist ...)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import Engine, _ptr, _stream  # noqa: E402
from mgen_amd.workloads import poisson_flows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", choices=("hist", "nohist", "reduce"))
ap.add_argument("--shape", choices=("balanced", "skewed"))
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
d = poisson_flows(a.n, a.flows)
n = len(d["seq"])
base = (d["flow_id"] - 1).astype(np.uint32)
skewed = base.copy()
skewed[np.random.default_rng(1).random(n) < 0.5] = 0
col = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda()
       for k in ("seq", "tx_sec", "tx_usec", "msg_len", "rx_sec", "rx_usec")}
args = (col["seq"], col["tx_sec"], col["tx_usec"], col["msg_len"], col["rx_sec"], col["rx_usec"])


def timed(setup, call):
    setup()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for shape, fi in (("balanced", base), ("skewed", skewed)):
    if a.shape and a.shape != shape:
        continue
    idx = torch.from_numpy(fi).cuda()
    dist, hist = eng.flow_dist_init(a.flows)
    dist2, _ = eng.flow_dist_init(a.flows, hist=False)
    flows = eng.flow_init(a.flows, 1.0)
    lib, ctx, s = eng.lib, eng.ctx, _stream(0)

    def init_hist():
        lib.mgenx_flow_dist_init(ctx, _ptr(dist), _ptr(hist), a.flows, s)

    def init_nohist():
        lib.mgenx_flow_dist_init(ctx, _ptr(dist2), None, a.flows, s)

    def init_reduce():
        lib.mgenx_flow_init(ctx, _ptr(flows), a.flows, 1.0, s)

    kinds = {
        "hist": (init_hist, lambda: eng.flow_dist(dist, hist, a.flows, idx, *args)),
        "nohist": (init_nohist, lambda: eng.flow_dist(dist2, None, a.flows, idx, *args)),
        "reduce": (init_reduce, lambda: eng.flow_reduce(flows, a.flows, idx, *args)),
    }
    if a.only:
        kinds = {a.only: kinds[a.only]}
    ms = {k: [] for k in kinds}
    for it in range(a.warmup + a.iters):
        for k, (setup, call) in kinds.items():     # taking turns: the same drift for each
            t = timed(setup, call)
            if it >= a.warmup:
                ms[k].append(t)
    out = {"shape": shape, "records": n, "flows": a.flows, "iters": a.iters,
           "largest_flow": int(np.bincount(fi).max())}
    for k, v in ms.items():
        name = {"hist": "flow_dist_hist", "nohist": "flow_dist_nohist", "reduce": "flow_reduce"}[k]
        out[name + "_ms"] = round(statistics.median(v), 4)
        out[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    print(json.dumps(out), flush=True)
eng.close()
