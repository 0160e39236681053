"""mgenx_msg_match beside mgenx_msg_match_ex with a full timeline, on the shape of
scripts/msg_match_time.py (config 4: poisson_flows(8_388_608, 1024) with its 1 % loss on the recv
side, every sequence number of every flow once on the send side).  In one process, taking turns:

    parent   mgenx_msg_match of another build of the library (--parent-lib, a libmgenx.so of the
             commit before the timeline; left out when the option is not given)
    plain    mgenx_msg_match of this tree
    timeline mgenx_msg_match_ex with a 1-second series, the run list at min_run = 1 (its
             capacity sized by one call before the timed ones) and the owner column

Columns device-resident, device events around each call, median of --iters after --warmup.
Prints one JSON line.  --only plain|timeline runs a single call kind (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/match_timeline_time.py --only timeline
--iters 5)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import (Engine, FLOW_MATCH_DTYPE, LOSS_RUN_DTYPE, MATCH_BIN_DTYPE,  # noqa: E402
                      MatchTimeline, _ptr, _stream)
from mgen_amd.workloads import poisson_flows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width-us", type=int, default=1_000_000)
ap.add_argument("--parent-lib")
ap.add_argument("--only", choices=("plain", "timeline"))
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
d = poisson_flows(a.n, a.flows)
nr = len(d["seq"])
flow = (d["flow_id"] - 1).astype(np.uint32)

# the send side: seq 0 .. the flow's highest, round-robin over the flows (msg_match_time.py)
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
t0_us = int(stamp.min())
n_bins = int((int(stamp.max()) - t0_us) // a.width_us + 1)


def cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).cuda()


S = {k: cuda(v) for k, v in send.items()}
R = {k: cuda(v) for k, v in recv.items()}
s = _stream(0)
cnt = torch.empty(ns, dtype=torch.int32, device="cuda")
first = torch.empty(ns, dtype=torch.int32, device="cuda")
owner = torch.empty(ns, dtype=torch.int32, device="cuda")
rs = torch.empty(nr, dtype=torch.int32, device="cuda")
flows = torch.empty(a.flows * FLOW_MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
stats = torch.empty(32, dtype=torch.uint8, device="cuda")
bins = torch.empty(a.flows * n_bins * MATCH_BIN_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
outside = torch.empty(a.flows, dtype=torch.int64, device="cuda")
n_runs = torch.zeros(1, dtype=torch.int64, device="cuda")
tl = MatchTimeline(t0_us=t0_us, width_us=a.width_us, n_bins=n_bins, min_run=1,
                   dev_bins=bins.data_ptr(), dev_outside=outside.data_ptr(), dev_runs=None,
                   run_cap=0, dev_n_runs=n_runs.data_ptr(), dev_send_owner=owner.data_ptr())


def args():
    return (_ptr(S["flow_idx"]), _ptr(S["seq"]), _ptr(S["t_sec"]), _ptr(S["t_usec"]),
            _ptr(S["len"]), ns, _ptr(R["flow_idx"]), _ptr(R["seq"]), _ptr(R["tx_sec"]),
            _ptr(R["tx_usec"]), _ptr(R["rx_sec"]), _ptr(R["rx_usec"]), nr, a.flows, 0, _ptr(cnt),
            _ptr(first), _ptr(rs), _ptr(flows), _ptr(stats))


def plain():
    assert eng.lib.mgenx_msg_match(eng.ctx, *args(), s) == 0


def timeline():
    assert eng.lib.mgenx_msg_match_ex(eng.ctx, *args(), ctypes.byref(tl), s) == 0


kinds = {"plain": plain, "timeline": timeline}
if a.parent_lib and not a.only:
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    old = ctypes.CDLL(os.path.abspath(a.parent_lib))
    old.mgenx_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(P)]
    old.mgenx_ctx_destroy.argtypes = [P]
    old.mgenx_msg_match.argtypes = [P, P, P, P, P, P, u32, P, P, P, P, P, P, u32, u32, u32, P, P,
                                    P, P, P, P]
    old_ctx = P()
    assert old.mgenx_ctx_create(0, ctypes.byref(old_ctx)) == 0

    def parent():
        assert old.mgenx_msg_match(old_ctx, *args(), s) == 0

    kinds = {"parent": parent, **kinds}
if a.only:
    kinds = {a.only: kinds[a.only]}

# the run list's capacity: one call with none, as every caller sizes it
timeline()
torch.cuda.synchronize()
count = int(n_runs.item())
runs = torch.empty(max(count, 1) * LOSS_RUN_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
tl.dev_runs, tl.run_cap = runs.data_ptr(), count


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms = {k: [] for k in kinds}
for it in range(a.warmup + a.iters):
    for k, call in kinds.items():     # taking turns: the same drift for each
        t = timed(call)
        if it >= a.warmup:
            ms[k].append(t)
f = flows.cpu().numpy().view(FLOW_MATCH_DTYPE)
out = {"send_records": ns, "recv_records": nr, "flows": a.flows, "iters": a.iters,
       "width_us": a.width_us, "n_bins": n_bins, "listed_runs": count,
       "sent": int(f["sent"].sum()), "delivered": int(f["delivered"].sum()),
       "loss_runs": int(f["loss_runs"].sum())}
if "timeline" in ms:
    b = bins.cpu().numpy().view(MATCH_BIN_DTYPE)
    out.update(bins_sent=int(b["sent"].sum()), outside=int(outside.sum().item()))
for k, v in ms.items():
    out[k + "_ms"] = round(statistics.median(v), 4)
    out[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
if "parent" in ms:
    spread = (out["parent_min_max_ms"][1] - out["parent_min_max_ms"][0]) / out["parent_ms"]
    out["plain_to_parent"] = round(out["plain_ms"] / out["parent_ms"], 4)
    out["parent_spread"] = round(spread, 4)
    out["timeline_to_parent"] = round(out["timeline_ms"] / out["parent_ms"], 3)
print(json.dumps(out), flush=True)
if "parent" in kinds:
    old.mgenx_ctx_destroy(old_ctx)
eng.close()
