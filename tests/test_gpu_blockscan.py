"""GPU: the segmented scan of the per-flow passes (mgen_amd/csrc/mgenx_blockscan.hpp) driven
alone through the diagnostics build (mgenx_diag_blockscan, mgenx_diag_chunk_carry;
include/mgenx_diag.h) at its lane, wave and round edges, against a serial loop.  Integer
arithmetic: every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES, WAVE = 1024, 64
I64_MIN, I64_MAX, NONE = -2**63, 2**63 - 1, -1          # NONE: kNone
SUM, MIN, MAX = 0, 1, 2
# per kind of mgenx_diag_blockscan: the fields' operators and the value's numpy type
KINDS = {0: ([SUM], np.uint32), 1: ([MAX], np.int64), 2: ([SUM, MIN, MAX] * 4, np.uint64)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from mgen_amd import Engine
    e = Engine(0, diag=True)
    yield e.lib
    e.close()


def dev(torch, a):
    """a's bytes on the device (torch has no unsigned 32- and 64-bit tensors)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _signed(x):
    return x - 2**64 if x >> 63 else x


COMBINE = {SUM: lambda a, b: (a + b) & (2**64 - 1),
           MIN: lambda a, b: a if _signed(a) < _signed(b) else b,
           MAX: lambda a, b: a if _signed(a) > _signed(b) else b}


def serial(fields, head, ops):
    """The segmented inclusive scan, entry by entry, in Python integers.  fields: (n, F) uint64,
    one column per field; ops: F of SUM (modulo 2^64), MIN, MAX (as int64).  Returns the scanned
    fields and open[t] = no head at or before t."""
    fn = [COMBINE[o] for o in ops]
    out, is_open = [], []
    acc, seen = None, False
    for t, (v, h) in enumerate(zip(fields.tolist(), head.tolist())):
        seen = seen or bool(h)
        acc = v if h or t == 0 else [f(a, b) for f, a, b in zip(fn, acc, v)]
        out.append(acc)
        is_open.append(not seen)
    return np.array(out, np.uint64).reshape(len(out), len(ops)), np.array(is_open, bool)


def values(kind, n, seed):
    """n input values of the kind, with the extremes the operator can meet."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        v = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        v[rng.integers(0, n, max(n // 16, 1))] = 0xFFFFFFFF           # wrap-around
        return v
    if kind == 1:
        v = rng.integers(-2**40, 2**40, n, dtype=np.int64)
        for x in (NONE, I64_MIN, I64_MAX):
            v[rng.integers(0, n, max(n // 32, 1))] = x
        return v
    return rng.integers(0, 2**64, n, dtype=np.uint64)


def fields_of(kind, val):
    """The (n, F) uint64 fields that a kind's input values stand for (kind 2: the header's rule)."""
    if kind == 0:
        return val.astype(np.uint64)[:, None]
    if kind == 1:
        return val.view(np.uint64)[:, None]
    k = np.arange(12, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return val[:, None] * (2 * k + 1) + k


def result_of(kind, fields):
    """The device's output layout of a kind from the scanned fields."""
    if kind == 0:
        return (fields[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if kind == 1:
        return fields[:, 0].view(np.int64)
    return fields


def head_patterns():
    def at(*lanes):
        h = np.zeros(LANES, np.uint32)
        h[list(lanes)] = 1
        return h
    pats = {"none": at(), "every lane": np.ones(LANES, np.uint32),
            "last lane of every wave": at(*range(WAVE - 1, LANES, WAVE)),
            "first lane of every wave": at(*range(0, LANES, WAVE)),
            "waves 3 to 9": at(3 * WAVE + 31, 9 * WAVE + 33)}
    for lane in (0, 1, 63, 64, 65, 127, 128, 1023):
        pats[f"lane {lane}"] = at(lane)
    rng = np.random.default_rng(20261021)
    for name, p in (("1/2", 1 / 2), ("1/64", 1 / 64), ("1/700", 1 / 700)):
        for i in range(2):
            pats[f"density {name} #{i}"] = (rng.random(LANES) < p).astype(np.uint32)
    pats["lane 128"][128] = 0x80000000            # any non-zero word is a head
    return pats


def run_scan(torch, lib, kind, val, head, want_open=True):
    n_fields = len(KINDS[kind][0])
    d_val, d_head = dev(torch, val), dev(torch, head)
    d_out = torch.full((LANES * n_fields * val.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    d_open = torch.full((LANES * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.mgenx_diag_blockscan(kind, d_val.data_ptr(), d_head.data_ptr(), d_out.data_ptr(),
                                  d_open.data_ptr() if want_open else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(KINDS[kind][1])
    out = out.reshape(LANES, n_fields) if kind == 2 else out
    return out, d_open.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scan_against_a_serial_loop(torch, lib, kind):
    val = values(kind, LANES, 100 + kind)
    fields = fields_of(kind, val)
    for name, head in head_patterns().items():
        want, want_open = serial(fields, head, KINDS[kind][0])
        got, got_open = run_scan(torch, lib, kind, val, head)
        bad = np.argwhere(got != result_of(kind, want))
        assert len(bad) == 0, (name, bad[:4].tolist())
        assert np.array_equal(got_open, want_open.astype(np.uint32)), name


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scan_without_open(torch, lib, kind):
    """The form the callers without a use for `open` compile: the same values, dev_open left."""
    val = values(kind, LANES, 200 + kind)
    for name in ("waves 3 to 9", "density 1/64 #0", "none"):
        head = head_patterns()[name]
        want, _ = serial(fields_of(kind, val), head, KINDS[kind][0])
        got, got_open = run_scan(torch, lib, kind, val, head, want_open=False)
        assert np.array_equal(got, result_of(kind, want)), name
        assert (got_open == 0xA5A5A5A5).all(), name


def carry_heads(n):
    """Head layouts over n entries: a segment open across both round edges (1023 -> 1024 and
    2047 -> 2048), a head exactly at entry 1024, none anywhere, and a random one."""
    def at(*entries):
        h = np.zeros(n, np.uint32)
        h[[e for e in entries if e < n]] = 1
        return h
    return {"open across the round edges": at(5, 700, 2500), "head at 1024": at(3, 1024, 2100),
            "none": at(),
            "density 1/64": (np.random.default_rng(n).random(n) < 1 / 64).astype(np.uint32)}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_chunk_carry_against_a_serial_loop(torch, lib, kind):
    """kind 2 is the sum without segments (match_run_base_kernel's): its heads are not read."""
    scan_kind = 0 if kind == 2 else kind
    for n in (1, 1023, 1024, 1025, 2048, 2049, 3000):
        val = values(scan_kind, n, 300 + n)
        for name, head in carry_heads(n).items():
            used = np.zeros(n, np.uint32) if kind == 2 else head
            want, _ = serial(fields_of(scan_kind, val), used, KINDS[scan_kind][0])
            d_val, d_head = dev(torch, val), dev(torch, head)
            d_out = torch.full((n * val.itemsize + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            rc = lib.mgenx_diag_chunk_carry(kind, d_val.data_ptr(), d_head.data_ptr(), n,
                                            d_out.data_ptr(), None)
            assert rc == 0
            torch.cuda.synchronize()
            h = d_out.cpu().numpy()
            assert (h[n * val.itemsize:] == 0xA5).all(), (n, name, "write past the end")
            got = h[:n * val.itemsize].view(val.dtype)
            bad = np.nonzero(got != result_of(scan_kind, want))[0]
            assert len(bad) == 0, (n, name, bad[:4].tolist())
