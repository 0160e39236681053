"""mgenx_msg_match beside mgenx_flow_dist (no histogram) in one run, on config 4's shape: the recv
side is poisson_flows(8_388_608, 1024) with its 1 % loss, the send side the same flows without
the loss (every sequence number of every flow once, in round-robin order; a lost message keeps
the stamp of its flow's last delivered one plus a microsecond).  Columns device-resident, device
events around each call, the two calls taking turns; median of --iters after --warmup.  Prints
one JSON line.  --only match|dist runs a single call kind (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/msg_match_time.py --only match --iters 5)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import Engine, FLOW_MATCH_DTYPE, _ptr, _stream  # noqa: E402
from mgen_amd.workloads import poisson_flows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=("match", "dist"))
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
d = poisson_flows(a.n, a.flows)
nr = len(d["seq"])
flow = (d["flow_id"] - 1).astype(np.uint32)

# the send side: seq 0 .. the flow's highest, round-robin over the flows
per = int(d["seq"].max()) + 1
tx = d["tx_sec"].astype(np.int64) * 10**6 + d["tx_usec"]
stamp = np.full((per, a.flows), -1, np.int64)
stamp[d["seq"], flow] = tx
known = stamp >= 0
filled = np.where(known, stamp, 0)
np.maximum.accumulate(filled, axis=0, out=filled)          # the last delivered stamp so far
stamp = np.where(known, stamp, np.maximum(filled, tx.min()) + 1)
ns = per * a.flows
send = dict(flow_idx=np.tile(np.arange(a.flows, dtype=np.uint32), per),
            seq=np.repeat(np.arange(per, dtype=np.uint32), a.flows),
            t_sec=(stamp.reshape(-1) // 10**6).astype(np.uint32),
            t_usec=(stamp.reshape(-1) % 10**6).astype(np.uint32),
            len=np.full(ns, int(d["msg_len"][0]), np.uint32))
recv = dict(flow_idx=flow, seq=d["seq"], tx_sec=d["tx_sec"], tx_usec=d["tx_usec"],
            rx_sec=d["rx_sec"], rx_usec=d["rx_usec"])


def cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).cuda()


S = {k: cuda(v) for k, v in send.items()}
R = {k: cuda(v) for k, v in recv.items()}
msg_len = torch.from_numpy(np.ascontiguousarray(d["msg_len"])).cuda()
dist, _ = eng.flow_dist_init(a.flows, hist=False)
lib, ctx, s = eng.lib, eng.ctx, _stream(0)
cnt = torch.empty(ns, dtype=torch.int32, device="cuda")
first = torch.empty(ns, dtype=torch.int32, device="cuda")
rs = torch.empty(nr, dtype=torch.int32, device="cuda")
flows = torch.empty(a.flows * FLOW_MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
stats = torch.empty(32, dtype=torch.uint8, device="cuda")


def match():
    rc = lib.mgenx_msg_match(ctx, _ptr(S["flow_idx"]), _ptr(S["seq"]), _ptr(S["t_sec"]),
                             _ptr(S["t_usec"]), _ptr(S["len"]), ns, _ptr(R["flow_idx"]),
                             _ptr(R["seq"]), _ptr(R["tx_sec"]), _ptr(R["tx_usec"]),
                             _ptr(R["rx_sec"]), _ptr(R["rx_usec"]), nr, a.flows, 0, _ptr(cnt),
                             _ptr(first), _ptr(rs), _ptr(flows), _ptr(stats), s)
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
    "match": (lambda: None, match),
    "dist": (lambda: lib.mgenx_flow_dist_init(ctx, _ptr(dist), None, a.flows, s),
             lambda: eng.flow_dist(dist, None, a.flows, R["flow_idx"], R["seq"], R["tx_sec"],
                                   R["tx_usec"], msg_len, R["rx_sec"], R["rx_usec"])),
}
if a.only:
    kinds = {a.only: kinds[a.only]}
ms = {k: [] for k in kinds}
for it in range(a.warmup + a.iters):
    for k, (setup, call) in kinds.items():     # taking turns: the same drift for each
        t = timed(setup, call)
        if it >= a.warmup:
            ms[k].append(t)
out = {"send_records": ns, "recv_records": nr, "flows": a.flows, "iters": a.iters}
if "match" in ms:
    f = flows.cpu().numpy().view(FLOW_MATCH_DTYPE)
    out.update(sent=int(f["sent"].sum()), delivered=int(f["delivered"].sum()),
               loss_runs=int(f["loss_runs"].sum()), rx_dup=int(f["rx_dup"].sum()),
               rx_orphan=int(f["rx_orphan"].sum()))
for k, v in ms.items():
    name = {"match": "msg_match", "dist": "flow_dist_nohist"}[k]
    out[name + "_ms"] = round(statistics.median(v), 4)
    out[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
if len(ms) == 2:
    out["ratio_to_flow_dist"] = round(out["msg_match_ms"] / out["flow_dist_nohist_ms"], 3)
print(json.dumps(out), flush=True)
eng.close()
