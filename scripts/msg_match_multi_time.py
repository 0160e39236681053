"""mgenx_msg_match_multi beside what a user did before it, one mgenx_msg_match call per receiver,
in one run on config 4's shape: the send side is scripts/msg_match_time.py's (every sequence
number of every flow of poisson_flows(8_388_608, 1024) once, in round-robin order), and each of
--rcv receivers logs it with an independent 1 % loss.  Columns device-resident, device events
around each side, the two sides taking turns; median of --iters after --warmup.  Prints one JSON
line.  --only multi|single runs one side (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/msg_match_multi_time.py --only multi --iters 5)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import (Engine, FLOW_FANOUT_DTYPE, FLOW_MATCH_DTYPE, RCV_CELL_DTYPE,  # noqa: E402
                      _ptr, _stream)
from mgen_amd.workloads import poisson_flows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--rcv", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=("multi", "single"))
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
d = poisson_flows(a.n, a.flows)
flow = (d["flow_id"] - 1).astype(np.uint32)

# the send side: seq 0 .. the flow's highest, round-robin over the flows
per = int(d["seq"].max()) + 1
tx = d["tx_sec"].astype(np.int64) * 10**6 + d["tx_usec"]
stamp = np.full((per, a.flows), -1, np.int64)
stamp[d["seq"], flow] = tx
known = stamp >= 0
filled = np.where(known, stamp, 0)
np.maximum.accumulate(filled, axis=0, out=filled)          # the last delivered stamp so far
stamp = np.where(known, stamp, np.maximum(filled, tx.min()) + 1).reshape(-1)
ns = per * a.flows
send = dict(flow_idx=np.tile(np.arange(a.flows, dtype=np.uint32), per),
            seq=np.repeat(np.arange(per, dtype=np.uint32), a.flows),
            t_sec=(stamp // 10**6).astype(np.uint32), t_usec=(stamp % 10**6).astype(np.uint32),
            len=np.full(ns, int(d["msg_len"][0]), np.uint32))


def cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).cuda()


# the receivers: each keeps 99 % of the send records, in the sender's order, 200..1200 us later
rng = np.random.default_rng(4)
S = {k: cuda(v) for k, v in send.items()}
parts = []
for r in range(a.rcv):
    keep = np.nonzero(rng.random(ns) >= 0.01)[0]
    rx = stamp[keep] + rng.integers(200, 1200, len(keep))
    parts.append({k: cuda(v) for k, v in dict(
        flow_idx=send["flow_idx"][keep], seq=send["seq"][keep], tx_sec=send["t_sec"][keep],
        tx_usec=send["t_usec"][keep], rx_sec=(rx // 10**6).astype(np.uint32),
        rx_usec=(rx % 10**6).astype(np.uint32), rcv=np.full(len(keep), r, np.uint32)).items()})
R = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
nrs = [p["seq"].numel() for p in parts]
nr = sum(nrs)

lib, ctx, s = eng.lib, eng.ctx, _stream(0)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")  # noqa: E731
mask = torch.empty(ns, dtype=torch.int64, device="cuda")
rs = torch.empty(nr, dtype=torch.int32, device="cuda")
first = u8(nr)
cells = u8(a.flows * a.rcv * RCV_CELL_DTYPE.itemsize)
fanout = u8(a.flows * FLOW_FANOUT_DTYPE.itemsize)
stats = u8(32)
cnt = torch.empty(ns, dtype=torch.int32, device="cuda")
first_rx = torch.empty(ns, dtype=torch.int32, device="cuda")
flows = [u8(a.flows * FLOW_MATCH_DTYPE.itemsize) for _ in range(a.rcv)]


def multi():
    rc = lib.mgenx_msg_match_multi(
        ctx, _ptr(S["flow_idx"]), _ptr(S["seq"]), _ptr(S["t_sec"]), _ptr(S["t_usec"]),
        _ptr(S["len"]), ns, _ptr(R["flow_idx"]), _ptr(R["seq"]), _ptr(R["tx_sec"]),
        _ptr(R["tx_usec"]), _ptr(R["rx_sec"]), _ptr(R["rx_usec"]), _ptr(R["rcv"]), nr, a.rcv,
        a.flows, 0, _ptr(mask), _ptr(rs), _ptr(first), _ptr(cells), _ptr(fanout), _ptr(stats),
        None, s)
    assert rc == 0


def single():
    at = 0
    for r, p in enumerate(parts):          # what a user did before: one join per receiver
        rc = lib.mgenx_msg_match(
            ctx, _ptr(S["flow_idx"]), _ptr(S["seq"]), _ptr(S["t_sec"]), _ptr(S["t_usec"]),
            _ptr(S["len"]), ns, _ptr(p["flow_idx"]), _ptr(p["seq"]), _ptr(p["tx_sec"]),
            _ptr(p["tx_usec"]), _ptr(p["rx_sec"]), _ptr(p["rx_usec"]), nrs[r], a.flows, 0,
            _ptr(cnt), _ptr(first_rx), ctypes_at(rs, at), _ptr(flows[r]), _ptr(stats), s)
        assert rc == 0
        at += nrs[r]


def ctypes_at(t, elem):
    return ctypes.c_void_p(t.data_ptr() + 4 * elem)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = {"multi": multi, "single": single}
if a.only:
    kinds = {a.only: kinds[a.only]}
ms = {k: [] for k in kinds}
for it in range(a.warmup + a.iters):
    for k, call in kinds.items():     # taking turns: the same drift for each (the workspace is
        t = timed(call)               # sized for the larger call after the first round)
        if it >= a.warmup:
            ms[k].append(t)
out = {"send_records": ns, "recv_records": nr, "receivers": a.rcv, "flows": a.flows,
       "iters": a.iters}
if "multi" in ms:
    c = cells.cpu().numpy().view(RCV_CELL_DTYPE).reshape(a.flows, a.rcv)
    f = fanout.cpu().numpy().view(FLOW_FANOUT_DTYPE)
    out.update(sent=int(f["sent"].sum()), deliveries=int(f["deliveries"].sum()),
               reached_all=int(f["reached_all"].sum()), rx_dup=int(c["rx_dup"].sum()),
               rx_orphan=int(c["rx_orphan"].sum()))
    if "single" in ms:               # the two sides agree on every receiver's column
        for r in range(a.rcv):
            one = flows[r].cpu().numpy().view(FLOW_MATCH_DTYPE)
            for k in ("delivered", "lost_head", "lost_tail", "lat_sum", "lat_min", "lat_max"):
                assert (c[:, r][k] == one[k]).all(), (r, k)
for k, v in ms.items():
    name = {"multi": "msg_match_multi", "single": "msg_match_per_receiver"}[k]
    out[name + "_ms"] = round(statistics.median(v), 4)
    out[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
if len(ms) == 2:
    out["ratio_multi_to_per_receiver"] = round(
        out["msg_match_multi_ms"] / out["msg_match_per_receiver_ms"], 3)
print(json.dumps(out), flush=True)
eng.close()
