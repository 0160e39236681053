"""Config 2 unpack (fixed 512- and 1024-byte records, checksummed, 32-B rows) through the
ring-kernel shapes of the diagnostics build (MGENX_TUNE_UNPACK_VARIANT, the table in
launch_unpack): waves per workgroup, rows per load block, blocks in the ring, groups of row
output held, and plain or non-temporal row loads.  The shapes that lost were retired with
their numbers on record (profiles/r08/ring_shapes.txt).  Batches of 65,536, 131,072 (the pcie_inclusive_config2 chunk) and 1,048,576
records.  Every shape's rows are compared with the product kernel's (bit-exact) before timing;
the slab carries bit flips, so the CRC verdicts are part of the comparison."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import PACK_CHECKSUM, Engine, to_device  # noqa: E402
from mgen_amd.workloads import udp_fixed  # noqa: E402

N = 1 << 20
SHAPES = {0: "product", 17: "(16, 4, 1, 16)", 18: "(8, 8, 2, 32)", 28: "(16, 4, 1, 16) nt"}
VARIANTS = [int(v) for v in os.environ.get("VARIANTS", "17,18,28,0").split(",")]
BATCHES = [int(v) for v in os.environ.get("BATCHES", "65536,131072,1048576").split(",")]
eng = Engine(0, diag=True)
rows = {"rows": eng.alloc_rows(N)}


def timed(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for L in (1024, 512):
    t, p, d = udp_fixed(N, L)
    dt, dp = to_device(t), to_device(p)
    c = torch.empty(len(t), dtype=torch.int32, device="cuda")
    eng.pack_prepare(dt, len(t), dp, c)
    slab = torch.empty(N * L + 64, dtype=torch.uint8, device="cuda")
    eng.pack(dt, c, to_device(d), N, dp, slab, stride=L, opts=PACK_CHECKSUM)
    # a bit flip in every 1000th record, at a position that walks through the record
    recs = torch.arange(0, N, 1000, device="cuda", dtype=torch.int64)
    slab[recs * L + (recs * 7) % L] ^= 0x10
    variants = VARIANTS
    for n in BATCHES:
        def run():
            eng.unpack(slab, n, stride=L, fixed_len=L, cols=rows)
        eng.set_unpack_variant(0)
        rows["rows"].zero_()
        run()
        torch.cuda.synchronize()
        ref = rows["rows"].clone()
        for v in variants:
            eng.set_unpack_variant(v)
            rows["rows"].zero_()
            run()
            torch.cuda.synchronize()
            same = bool(torch.equal(rows["rows"], ref))
            print(f"{L} B n {n} variant {v:2d} {SHAPES[v]}: rows "
                  f"{'== product' if same else 'DIFFER'} kernel {eng.last_unpack_kernel()}", flush=True)
        res = {v: [] for v in variants}
        for _ in range(int(os.environ.get("ROUNDS", "5"))):
            for v in variants:
                eng.set_unpack_variant(v)
                res[v].append(timed(run, 50 if n == N else 200))
        for v in variants:
            s = sorted(res[v])
            print(f"{L} B n {n} variant {v:2d} {SHAPES[v]}: median {s[len(s) // 2] * 1e3:.1f} us "
                  f"min {s[0] * 1e3:.1f}  all {' '.join(f'{x * 1e3:.1f}' for x in res[v])}", flush=True)
    eng.set_unpack_variant(0)
    del slab
