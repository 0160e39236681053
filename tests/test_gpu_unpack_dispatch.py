"""Which kernel launch_unpack picks (product library), case by case, with the output of each
case checked against the oracle as test_fixed_len_pipelined_vs_oracle checks it: every golden
template layout, checksummed and plain records mixed, bit flips, bad version / dst type, a
partial last group and records past the end of the slab, under the UDP, forced-UDP and TCP
receive rules."""
import numpy as np
import pytest

from test_gpu_parity import COLMAP, compare_cols, dev, host_cols, rows_to_cols

pytestmark = pytest.mark.gpu

N = 16 * 20 + 7      # a partial last group
N_OOB = 3


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def eng(torch):
    from mgen_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return dict(np.load(os.path.join(root, "tests", "golden", "udp_matrix.npz"),
                        allow_pickle=False))


_records = {}


def records(gold, size, n, damaged=True):
    """n records of `size` bytes back to back (host bytes), built once per key and left
    unchanged, the caller CHECKSUM flag mixed.  Undamaged: every record checksummed and
    intact (what a receiver that skips the CRC check reports is then what one that checks
    reports).  Damaged: 70% checksummed, bit flips, bad version, bad dst type."""
    key = (size, n, damaged)
    if key not in _records:
        from oracle import oracle as O
        tmpl, pool = gold["tmpl"], gold["pool"]
        rng = np.random.default_rng(size + 7 * n)
        desc = np.zeros(n, gold["desc"].dtype)
        desc["tmpl"] = rng.integers(0, len(tmpl), n)
        desc["seq_num"] = np.arange(n) * 3 + 1
        desc["tx_sec"] = 1_700_000_000 + np.arange(n) // 100
        desc["tx_usec"] = rng.integers(0, 1_000_000, n)
        desc["msg_len"] = size
        desc["flags"] = rng.choice([0, 4], n)
        a, _ = O.udp_pack_batch(tmpl, desc, pool, n * size, stride=size, checksum=True)
        b, _ = O.udp_pack_batch(tmpl, desc, pool, n * size, stride=size, checksum=False)
        recs = a.reshape(n, size).copy()
        if damaged:
            # 30% packed without a checksum (those whose caller flag asks for one then fail it)
            plain = rng.random(n) >= 0.7
            recs[plain] = b.reshape(n, size)[plain]
            flip = np.nonzero(rng.random(n) < 0.1)[0]
            pos = rng.integers(0, size, flip.size)
            recs[flip, pos] ^= (1 << rng.integers(0, 8, flip.size)).astype(np.uint8)
            recs[rng.random(n) < 0.02, 2] = 3          # version
            recs[rng.random(n) < 0.02, 22] = 7         # dst type
        _records[key] = np.ascontiguousarray(recs).reshape(-1)
    return _records[key]


def check_core(c, f, live, n, what):
    from mgen_amd import ERROR_OOB
    for gname, oname, dt in COLMAP[:13]:
        got = c[gname].view(dt)[:live]
        want = f[oname].astype(dt)[:live]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, gname, bad[:8], got[bad[:4]], want[bad[:4]])
    assert np.array_equal(c["dst_addr4"].view(np.uint8).reshape(-1, 4)[:live],
                          f["dst_addr"][:live, :4]), what
    assert np.all(c["err"][live:n] == ERROR_OOB), what
    assert np.all(c["msg_len"].view(np.uint16)[live:n] == 0), what


# id -> (record size, output, how the batch is given, expected kernel)
CASES = {
    "skip_crc": (700, "cols", "skip_crc", "HEADER"),
    "700_cols": (700, "cols", "stride", "FIXED"),
    "700_rows": (700, "rows", "stride", "FIXED"),
    "256_cols": (256, "cols", "stride", "FIXED"),
    "512_cols": (512, "cols", "stride", "FIXED"),
    "512_rows": (512, "rows", "stride", "FIXED_RING"),
    "1024_rows": (1024, "rows", "stride", "FIXED_RING"),
    "64": (64, "cols", "stride", "GENERAL"),
    "1025": (1025, "cols", "stride", "GENERAL"),
    "700_ext": (700, "ext", "stride", "GENERAL"),
    "700_rec_off": (700, "cols", "rec_off", "GENERAL"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_dispatch_and_output(torch, eng, gold, case):
    import mgen_amd
    from mgen_amd import OPT_CHECKSUM_FORCE, OPT_SKIP_CRC, OPT_TCP
    from oracle import oracle as O
    size, out, given, kernel = CASES[case]
    n = N
    skip = given == "skip_crc"
    # without the CRC check nothing may depend on it: the records are left intact
    host = records(gold, size, n, damaged=not skip)
    slab = dev(torch, host).view(torch.uint8)
    live = n - N_OOB
    slab_bytes = live * size + size // 2   # the first dead record straddles the end
    place = {"stride": size, "fixed_len": size}
    if given == "rec_off":
        place = {"rec_off": dev(torch, np.arange(n, dtype=np.uint64) * size).view(torch.int64),
                 "fixed_len": size}
    for opts in ((OPT_SKIP_CRC,) if skip else (0, OPT_CHECKSUM_FORCE, OPT_TCP | OPT_CHECKSUM_FORCE)):
        f = O.udp_recv_batch(host, n, stride=size, fixed_len=size,
                             force=bool(opts & OPT_CHECKSUM_FORCE), tcp=bool(opts & OPT_TCP))
        if out == "rows":
            rows = eng.alloc_rows(n)
            eng.unpack(slab, n, opts=opts, slab_bytes=slab_bytes, cols={"rows": rows}, **place)
            which = eng.last_unpack_kernel()
            torch.cuda.synchronize()
            c = rows_to_cols(rows, n)
        else:
            cols = eng.unpack(slab, n, opts=opts, slab_bytes=slab_bytes, ext=out == "ext", **place)
            which = eng.last_unpack_kernel()
            c = host_cols(cols, n)
        assert which == getattr(mgen_amd, "UNPACK_K_" + kernel), (case, opts, which)
        check_core(c, f, live, n, (case, opts))
        if out == "ext":   # the extended columns of the live records too
            compare_cols(cols, f[:live], live, (case, opts))


def test_fixed_needs_a_slab_of_three_rows(torch, eng, gold):
    """launch_unpack takes a fixed batch to the pipelined kernel only when slab_bytes >=
    64 (nr + 1) + 16, nr = ceil(fixed_len / 64): its dead lanes read inside the slab.  65-byte
    records (nr = 2), the slab exactly n records long (the binding passes the tensor's size):
    the smallest n that meets the bound runs the fixed kernel, one record fewer the general
    one, and both decode as the oracle does."""
    from mgen_amd import UNPACK_K_FIXED, UNPACK_K_GENERAL
    from oracle import oracle as O
    size = 65
    need = 64 * ((size + 63) // 64 + 1) + 16
    n_hi = -(-need // size)
    n_lo = n_hi - 1
    assert n_lo * size < need <= n_hi * size and n_lo >= 1
    for n, kernel in ((n_lo, UNPACK_K_GENERAL), (n_hi, UNPACK_K_FIXED)):
        host = records(gold, size, n)
        slab = dev(torch, host).view(torch.uint8)
        assert slab.numel() == n * size
        cols = eng.unpack(slab, n, stride=size, fixed_len=size)
        assert eng.last_unpack_kernel() == kernel, (n, eng.last_unpack_kernel())
        f = O.udp_recv_batch(host, n, stride=size, fixed_len=size)
        check_core(host_cols(cols, n), f, n, n, ("slab edge", n))
