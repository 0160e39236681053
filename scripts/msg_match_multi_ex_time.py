"""mgenx_msg_match_multi_ex on scripts/msg_match_multi_time.py's shape (every sequence number of
every flow of poisson_flows(8_388_608, 1024) once, in round-robin order; each of --rcv receivers
logs it with an independent 1 % loss), in one run:
  base           mgenx_msg_match_multi itself (run the script again with --tree on a checkout of
                 the parent commit, built, for the other half of a pair: a tree without the ex
                 call runs base and per_receiver alone);
  stats / list / pairs / all
                 the ex call with each part alone and with all three, the list at its full size
                 (the sizing call of the two-pass convention is not in the time);
  per_receiver   what a user did before for the run statistics and the list: one
                 mgenx_msg_match_ex call with a run list per receiver.
Columns device-resident, device events around each call, the kinds taking turns; median of
--iters after --warmup.  Prints one JSON line.  --only KIND[,KIND] runs some of them (for a
kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/msg_match_multi_ex_time.py
--only all --iters 5)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

KINDS = ("base", "stats", "list", "pairs", "all", "per_receiver")
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the built checkout whose mgen_amd is measured (default: this one)")
ap.add_argument("--n", type=int, default=8_388_608)
ap.add_argument("--flows", type=int, default=1024)
ap.add_argument("--rcv", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", default=",".join(KINDS))
a = ap.parse_args()
only = a.only.split(",")
assert all(k in KINDS for k in only), KINDS

sys.path.insert(0, os.path.abspath(a.tree))
import mgen_amd  # noqa: E402
from mgen_amd import (Engine, FLOW_FANOUT_DTYPE, FLOW_MATCH_DTYPE, LOSS_RUN_DTYPE,  # noqa: E402
                      RCV_CELL_DTYPE, MatchTimeline, _ptr, _stream)
from mgen_amd.workloads import poisson_flows  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
eng = Engine(0)
has_ex = hasattr(eng.lib, "mgenx_msg_match_multi_ex") and hasattr(mgen_amd, "MultiLoss")
if not has_ex:                      # the parent commit's library: the base call alone
    only = [k for k in only if k in ("base", "per_receiver")]
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
u8 = lambda n: torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")  # noqa: E731
mask = torch.empty(ns, dtype=torch.int64, device="cuda")
rs = torch.empty(nr, dtype=torch.int32, device="cuda")
first = u8(nr)
cells = u8(a.flows * a.rcv * RCV_CELL_DTYPE.itemsize)
fanout = u8(a.flows * FLOW_FANOUT_DTYPE.itemsize)
stats = u8(32)
n_runs = torch.zeros(1, dtype=torch.int64, device="cuda")
join = [_ptr(S[k]) for k in ("flow_idx", "seq", "t_sec", "t_usec", "len")] + [ns] + \
    [_ptr(R[k]) for k in ("flow_idx", "seq", "tx_sec", "tx_usec", "rx_sec", "rx_usec", "rcv")] + \
    [nr, a.rcv, a.flows, 0, _ptr(mask), _ptr(rs), _ptr(first), _ptr(cells), _ptr(fanout),
     _ptr(stats), None]


def base():
    assert lib.mgenx_msg_match_multi(ctx, *join, s) == 0


calls = {"base": base}
if has_ex:
    from mgen_amd import MultiLoss, RCV_LOSS_RUN_DTYPE, RCV_PAIR_DTYPE, RCV_RUNS_DTYPE
    rcv_runs = u8(a.flows * a.rcv * RCV_RUNS_DTYPE.itemsize)
    pair = u8(a.flows * a.rcv * a.rcv * RCV_PAIR_DTYPE.itemsize)
    # the list's size: the first pass of two
    lx0 = MultiLoss(dev_n_runs=n_runs.data_ptr(), run_cap=0, min_run=1)
    assert lib.mgenx_msg_match_multi_ex(ctx, *join, ctypes.byref(lx0), s) == 0
    count = int(n_runs.item())
    runs = u8(count * RCV_LOSS_RUN_DTYPE.itemsize)

    def ex_call(want):
        lx = MultiLoss(min_run=1)
        if "s" in want:
            lx.dev_rcv_runs = rcv_runs.data_ptr()
        if "l" in want:
            lx.dev_n_runs, lx.dev_runs, lx.run_cap = n_runs.data_ptr(), runs.data_ptr(), count
        if "p" in want:
            lx.dev_pairs = pair.data_ptr()

        def go():
            assert lib.mgenx_msg_match_multi_ex(ctx, *join, ctypes.byref(lx), s) == 0
        return go
    calls.update(stats=ex_call("s"), list=ex_call("l"), pairs=ex_call("p"), all=ex_call("slp"))

# one mgenx_msg_match_ex with a run list per receiver
cnt = torch.empty(ns, dtype=torch.int32, device="cuda")
first_rx = torch.empty(ns, dtype=torch.int32, device="cuda")
flows = [u8(a.flows * FLOW_MATCH_DTYPE.itemsize) for _ in range(a.rcv)]
one_n = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(a.rcv)]
one_runs = [u8(0)] * a.rcv
one_cap = [0] * a.rcv


def per_receiver():
    at = 0
    for r, p in enumerate(parts):
        tl = MatchTimeline(n_bins=0, min_run=1, dev_runs=one_runs[r].data_ptr(),
                           run_cap=one_cap[r], dev_n_runs=one_n[r].data_ptr())
        rc = lib.mgenx_msg_match_ex(
            ctx, _ptr(S["flow_idx"]), _ptr(S["seq"]), _ptr(S["t_sec"]), _ptr(S["t_usec"]),
            _ptr(S["len"]), ns, _ptr(p["flow_idx"]), _ptr(p["seq"]), _ptr(p["tx_sec"]),
            _ptr(p["tx_usec"]), _ptr(p["rx_sec"]), _ptr(p["rx_usec"]), nrs[r], a.flows, 0,
            _ptr(cnt), _ptr(first_rx), ctypes.c_void_p(rs.data_ptr() + 4 * at), _ptr(flows[r]),
            _ptr(stats), ctypes.byref(tl), s)
        assert rc == 0
        at += nrs[r]


if "per_receiver" in only:
    per_receiver()                  # the lists' sizes: the first pass of two
    one_cap = [int(t.item()) for t in one_n]
    one_runs = [u8(c * LOSS_RUN_DTYPE.itemsize) for c in one_cap]
calls["per_receiver"] = per_receiver


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = {k: calls[k] for k in only}
ms = {k: [] for k in kinds}
for it in range(a.warmup + a.iters):
    for k, call in kinds.items():     # taking turns: the same drift for each (the workspace is
        t = timed(call)               # sized for the largest call after the first round)
        if it >= a.warmup:
            ms[k].append(t)
out = {"library": os.path.realpath(mgen_amd.LIB_PATH), "send_records": ns, "recv_records": nr,
       "receivers": a.rcv, "flows": a.flows, "iters": a.iters}
if "all" in ms:
    kinds["all"]()
    torch.cuda.synchronize()
    rr = rcv_runs.cpu().numpy().view(RCV_RUNS_DTYPE).reshape(a.flows, a.rcv)
    pp = pair.cpu().numpy().view(RCV_PAIR_DTYPE).reshape(a.flows, a.rcv, a.rcv)
    out.update(runs_listed=int(n_runs.item()), loss_runs=int(rr["loss_runs"].sum()),
               longest_run=int(rr["loss_run_max"].max()),
               lost_both_off_diagonal=int(pp["lost_both"].sum() -
                                          pp["lost_both"][:, range(a.rcv), range(a.rcv)].sum()))
    if "per_receiver" in ms:          # the two sides agree on every receiver's column
        for r in range(a.rcv):
            one = flows[r].cpu().numpy().view(FLOW_MATCH_DTYPE)
            for k in ("loss_runs", "loss_run_max", "loss_run_hist"):
                assert (rr[:, r][k] == one[k]).all(), (r, k)
        assert sum(one_cap) == out["runs_listed"]
for k, v in ms.items():
    out[k + "_ms"] = round(statistics.median(v), 4)
    out[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
print(json.dumps(out), flush=True)
eng.close()
