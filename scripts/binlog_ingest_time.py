"""Time binary log ingest on one GPU over one binary RECV log of N records (default 1,048,576
messages of 64..256 bytes, written on the GPU by mgenx_log_recv_binary):

  host_index_ms   mgenx_binlog_index over the host image (one core)
  ingest_ms       mgenx_binlog_parse: records -> columns, one call
  text_route_ms   the route without it: mgenx_convert_binary_log -> mgenx_text_index ->
                  mgenx_log_parse_text over the same records (the converter's host size round
                  trips included, as every caller pays them)

Wall time between device synchronisations, best and median of --reps runs after one warm-up.
Prints one JSON line.

    python scripts/binlog_ingest_time.py [--records N] [--reps R]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_log(torch, eng, n):
    from mgen_amd import PACK_CHECKSUM, to_device
    from mgen_amd.workloads import udp_mixed
    tmpl, pool, desc, offs, sizes = udp_mixed(n, 64, 256, n_flows=64)
    slab_bytes = int(offs[-1] + sizes[-1] + 16)
    d_tmpl, d_pool, d_desc = to_device(tmpl), to_device(pool), to_device(desc)
    d_offs = to_device(offs).view(torch.int64)
    crc = torch.empty(len(tmpl), dtype=torch.int32, device="cuda")
    eng.pack_prepare(d_tmpl, len(tmpl), d_pool, crc)
    slab = torch.zeros(slab_bytes, dtype=torch.uint8, device="cuda")
    eng.pack(d_tmpl, crc, d_desc, n, d_pool, slab, rec_off=d_offs, opts=PACK_CHECKSUM)
    cols = eng.unpack(slab, n, rec_off=d_offs, rec_len=to_device(sizes).view(torch.int32),
                      ext=True)
    src = torch.zeros(n, 20, dtype=torch.uint8, device="cuda")
    src[:, 0], src[:, 1], src[:, 2], src[:, 3] = 1, 4, 0x89, 0xE7
    src[:, 4], src[:, 7] = 10, 1
    rx_s = torch.full((n,), 1_700_000_001, dtype=torch.int32, device="cuda")
    rx_u = torch.arange(n, dtype=torch.int32, device="cuda") % 1_000_000
    binrec, _ = eng.log_recv_binary(slab, n, cols, src.view(-1), rx_s, rx_u, rec_off=d_offs)
    hdr = b"mgen version=5.1.1 type=binary_log\n\0"
    return torch.cat([torch.tensor(list(hdr), dtype=torch.uint8, device="cuda"), binrec])


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(min(out), 3), round(statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import mgen_amd
    from mgen_amd import LOG_EPOCH, Engine
    eng = Engine(0)
    n = a.records
    log = build_log(torch, eng, n)
    host = log.cpu().numpy()
    idx = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        offs, info = mgen_amd.binlog_index(host)
        idx.append((time.perf_counter() - t0) * 1e3)
    assert info.status == 0 and info.n_records == n
    ro = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    text, _ = eng.convert_binary_log(log, ro, n, 0, LOG_EPOCH)
    cap = text.numel()

    def ingest():
        return eng.binlog_parse(log, ro, n)

    def text_route():
        t, _ = eng.convert_binary_log(log, ro, n, 0, LOG_EPOCH, cap=cap)
        line_off, n_lines = eng.text_index(t)
        return eng.log_parse_text(t, line_off, n_lines)
    p, q = ingest(), text_route()
    for name in ("event", "status", "flow_id", "seq_num", "tx_usec", "rx_usec", "msg_len"):
        assert torch.equal(p[name], q[name]), name
    ing, txt = timed(torch, ingest, a.reps), timed(torch, text_route, a.reps)
    print(json.dumps({
        "records": n, "binary_bytes": int(log.numel()), "text_bytes": int(cap),
        "host_index_ms": {"best": round(min(idx[1:]), 3),
                          "median": round(statistics.median(idx[1:]), 3)},
        "ingest_ms": {"best": ing[0], "median": ing[1]},
        "text_route_ms": {"best": txt[0], "median": txt[1]},
        "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
