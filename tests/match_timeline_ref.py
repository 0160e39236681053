"""A serial model of the timeline of mgenx_msg_match_ex, written from the definitions in
include/mgenx.h alone: Python ints, record by record.  It takes the per-record counts from
msg_match_ref.model and shares no code with the product."""
import numpy as np

import msg_match_ref as M

NONE = M.NONE
I64_MAX, I64_MIN = M.I64_MAX, M.I64_MIN
HEAD, TAIL = 1, 2

BIN = np.dtype([
    ("sent", "<u8"), ("sent_bytes", "<u8"), ("delivered", "<u8"), ("delivered_bytes", "<u8"),
    ("rx_dup", "<u8"), ("lat_sum", "<i8"), ("lat_min", "<i8"), ("lat_max", "<i8")])
RUN = np.dtype([
    ("flow_idx", "<u4"), ("length", "<u4"), ("first_send", "<u4"), ("last_send", "<u4"),
    ("flags", "<u4"), ("rsv", "<u4"), ("t_first_us", "<i8"), ("t_last_us", "<i8")])


def model(n_flows, send, recv, t0_us, width_us, n_bins, min_run=1, no_time=False):
    """Returns (base, owner, bins[n_flows, n_bins], outside[n_flows], runs): base is
    msg_match_ref.model's tuple."""
    base = M.model(n_flows, send, recv, no_time=no_time)
    cnt, first = [int(x) for x in base[0]], [int(x) for x in base[1]]
    S = {k: [int(x) for x in send[k]] for k in M.SEND_COLS}
    R = {k: [int(x) for x in recv[k]] for k in M.RECV_COLS}
    ns = len(S["flow_idx"])
    stamp = [S["t_sec"][i] * 10**6 + S["t_usec"][i] for i in range(ns)]

    # the owner column: the lowest counted index of the record's identity
    owner = [NONE] * ns
    seen = {}
    for i in range(ns):
        f = S["flow_idx"][i]
        if f >= n_flows:
            continue
        ident = (f, S["seq"][i]) if no_time else (f, S["seq"][i], S["t_sec"][i], S["t_usec"][i])
        owner[i] = seen.setdefault(ident, i)

    cells = [[dict(sent=0, sent_bytes=0, delivered=0, delivered_bytes=0, rx_dup=0, lat_sum=0,
                   lat_min=I64_MAX, lat_max=I64_MIN) for _ in range(n_bins)]
             for _ in range(n_flows)]
    outside = [0] * n_flows
    runs = []
    want = max(int(min_run), 1)
    per_flow = [[] for _ in range(n_flows)]
    for i in range(ns):
        if owner[i] == i:
            per_flow[S["flow_idx"][i]].append(i)
    for f in range(n_flows):
        owners = per_flow[f]
        if n_bins:
            for i in owners:
                b = (stamp[i] - t0_us) // width_us          # Python's // is the signed floor
                if not 0 <= b < n_bins:
                    outside[f] += 1
                    continue
                c = cells[f][b]
                c["sent"] += 1
                c["sent_bytes"] += S["len"][i]
                if cnt[i]:
                    j = first[i]
                    lat = R["rx_sec"][j] * 10**6 + R["rx_usec"][j] - stamp[i]
                    c["delivered"] += 1
                    c["delivered_bytes"] += S["len"][i]
                    c["rx_dup"] += cnt[i] - 1
                    c["lat_sum"] += lat
                    c["lat_min"] = min(c["lat_min"], lat)
                    c["lat_max"] = max(c["lat_max"], lat)
        # the runs of the flow: consecutive undelivered owners
        cur = []
        delivered_before = False
        for i in owners + [None]:
            if i is not None and cnt[i] == 0:
                cur.append(i)
                continue
            if cur and len(cur) >= want:
                flags = (0 if delivered_before else HEAD) | (TAIL if i is None else 0)
                runs.append((f, len(cur), cur[0], cur[-1], flags, 0, stamp[cur[0]],
                             stamp[cur[-1]]))
            cur = []
            delivered_before = True
    bins = np.zeros((n_flows, n_bins), BIN)
    for f in range(n_flows):
        for b in range(n_bins):
            for k, v in cells[f][b].items():
                bins[f][b][k] = M._wrap_i64(v) if k == "lat_sum" else v
    out_runs = np.zeros(len(runs), RUN)
    for k, r in enumerate(runs):
        out_runs[k] = r
    return (base, np.array(owner, np.uint32), bins, np.array(outside, np.uint64), out_runs)
