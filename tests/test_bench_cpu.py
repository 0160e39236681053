"""bench.py's command line and its --dump-outputs writer, without a GPU: the options a plain
and a --full run take, and the dumped arrays (float32 / float64, exact values, the same
sample from call to call, under the 64 MB budget at the benchmark's size)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in p.stdout, opt


def test_dump_outputs_exact_and_repeatable(tmp_path):
    import torch

    import bench
    from mgen_amd import REC_DTYPE
    n = 4099
    base = 0xFFFFF000 - n          # 32-bit keys a float32 could not hold
    rng = np.random.default_rng(5)
    rec = np.zeros(n, REC_DTYPE)
    for name in REC_DTYPE.names:
        hi = 1 << (8 * REC_DTYPE[name].itemsize)
        rec[name] = rng.integers(0, hi, n, dtype=np.uint64)
    rec["seq_num"] = base + np.arange(n)
    rows = torch.from_numpy(rec.view(np.uint8).copy())
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), rows)
    bench.dump_outputs(str(b), rows)
    assert sorted(os.listdir(a)) == sorted(f"{name}.npy" for name in REC_DTYPE.names)
    # the sample: sorted row indices, the first and the last row among them, about half
    idx = (np.load(a / "seq_num.npy") - base).astype(np.int64)
    assert idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) > 0)
    assert n // 2 - 2 <= idx.size <= n // 2
    for name in REC_DTYPE.names:
        x, y = np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and x.shape == idx.shape
        assert np.array_equal(x, y), name
        assert np.array_equal(x.astype(np.uint64), rec[name][idx].astype(np.uint64)), name
    # at the benchmark's size the files stay under 64 MB
    per_row = sum(8 if REC_DTYPE[k].itemsize > 2 else 4 for k in REC_DTYPE.names)
    assert (bench.N_REC // 2) * per_row + 128 * len(REC_DTYPE.names) <= 64_000_000
