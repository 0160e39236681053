"""Loop edges of the headline row kernel (unpack_fixed_ring_kernel: 512- and 1024-byte records
into 32-byte rows).  A wave owns groups w, w + W, w + 2W, ... (16 records each) and runs them
in two loops: pipelined groups, whose body rows stream through the load ring, and header-only
groups, entered after a group in which no record asks for the checksum and left at the first
group in which one does.  The cases here reach every edge of those loops at the smallest
sizes that do: every trip count 1..6 with a partial last group, waves without a group, each
order of mode switches per wave, CRC verdicts on both sides of a switch, the forced and TCP
receive rules, and records past the end of the slab.  Rows are compared field by field with
the oracle (on every record a case touched), with the column kernel on the same slab (every
record) and with the descriptors the slab was packed from (every untouched record)."""
import numpy as np
import pytest

from test_gpu_parity import COLMAP, _config2, host_cols, rows_to_cols

pytestmark = pytest.mark.gpu

CORE = COLMAP[:13]
M_MAX = 5   # groups per wave of the largest slab (some waves run M_MAX + 1)


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
def full_waves(torch):
    """W of a launch with at least one group per wave: 16 waves per workgroup, one workgroup
    per CU (mgenx_unpack_batch: grid = min(ceil(groups / 16), CUs))."""
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count


def n_waves(n, full):
    groups = (n + 15) // 16
    return min(16 * ((groups + 15) // 16), full)


def trip_n(W, m):
    """n = 16 (W m + r) + t: waves 0 .. r run m + 1 groups (wave r's last one is the partial
    group of t = 3 records), the others m."""
    r = W // 3 + 7
    return 16 * (W * m + r) + 3


_packed = {}


def packed(torch, eng, size, full):
    """(descriptors, pristine slab) of the largest case of `size`, packed once on the GPU;
    every case works on a clone of a prefix."""
    if size not in _packed:
        n = trip_n(full, M_MAX)
        desc, slab, out_len = _config2(torch, eng, n, size)
        assert int((out_len != size).sum()) == 0
        _packed[size] = (desc, slab)
    return _packed[size]


def flip(torch, slab, size, recs, pos, bits):
    at = torch.from_numpy((np.asarray(recs) * size + np.asarray(pos)).astype(np.int64)).cuda()
    slab[at] ^= torch.from_numpy((1 << np.asarray(bits)).astype(np.uint8)).cuda()


def clear_flag(torch, slab, size, recs):
    """CHECKSUM flag (byte 3, bit 2) off: the receiver does not check these records."""
    at = torch.from_numpy((np.asarray(recs) * size + 3).astype(np.int64)).cuda()
    slab[at] &= 0xFB


def check(torch, eng, slab, desc, n, size, touched, opts=0, slab_bytes=None, n_dead=0):
    """Rows of the ring kernel against the column kernel (all records), the oracle (touched
    records) and the descriptors (the rest); the last n_dead records lie past slab_bytes."""
    from mgen_amd import ERROR_OOB, OPT_CHECKSUM_FORCE, OPT_TCP, UNPACK_K_FIXED_RING
    from oracle import oracle as O
    kw = {} if slab_bytes is None else {"slab_bytes": slab_bytes}
    c = host_cols(eng.unpack(slab, n, stride=size, fixed_len=size, opts=opts, **kw), n)
    rows = eng.alloc_rows(n)
    eng.unpack(slab, n, stride=size, fixed_len=size, opts=opts, cols={"rows": rows}, **kw)
    assert eng.last_unpack_kernel() == UNPACK_K_FIXED_RING   # the kernel under test ran
    torch.cuda.synchronize()
    r = rows_to_cols(rows, n)
    for gname, _, dt in CORE:
        bad = np.nonzero(r[gname].view(dt)[:n] != c[gname].view(dt)[:n])[0]
        assert bad.size == 0, (size, opts, "rows vs cols", gname, bad[:8])
    assert np.array_equal(r["dst_addr4"][:n], c["dst_addr4"][:n])
    live = n - n_dead
    touched = np.unique(np.asarray(touched, np.int64))
    touched = touched[touched < live]
    host = slab.cpu().numpy()
    sub = np.ascontiguousarray(host[: n * size].reshape(n, size)[touched]).reshape(-1)
    f = O.udp_recv_batch(sub, touched.size, stride=size, fixed_len=size,
                         force=bool(opts & OPT_CHECKSUM_FORCE), tcp=bool(opts & OPT_TCP))
    for gname, oname, dt in CORE:
        got = r[gname].view(dt)[touched]
        want = f[oname].astype(dt)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (size, opts, "rows vs oracle", gname, touched[bad[:8]],
                               got[bad[:4]], want[bad[:4]])
    rest = np.setdiff1d(np.arange(live), touched)
    assert np.all(r["err"][rest] == 0)
    assert np.array_equal(r["seq_num"].view(np.uint32)[rest], desc["seq_num"][rest])
    assert np.array_equal(r["flow_id"].view(np.uint32)[rest], desc["tmpl"][rest] + 1)
    assert np.array_equal(r["tx_usec"].view(np.uint32)[rest], desc["tx_usec"][rest])
    if n_dead:   # exactly as the column kernel (compared above): OOB, every field zero
        assert np.all(r["err"][live:n] == ERROR_OOB)
        assert np.all(r["msg_len"].view(np.uint16)[live:n] == 0)
        assert np.all(r["seq_num"].view(np.uint32)[live:n] == 0)
    return r, f, touched


@pytest.mark.parametrize("size", [512, 1024])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_trip_counts(torch, eng, full_waves, size, m):
    """Waves of m and of m + 1 groups in one launch, the last group partial (3 records):
    bit flips in every owned position (first .. last group of a wave) are caught there."""
    W = full_waves
    n = trip_n(W, m)
    assert n_waves(n, W) == W
    desc, pristine = packed(torch, eng, size, W)
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(100 * m + size)
    # waves 0, r (m + 1 groups, the last one partial), r + 1 and W - 1 (m groups): a flip in
    # every group they own; and random records
    r_ = W // 3 + 7
    groups = [w + k * W for w in (0, r_, r_ + 1, W - 1) for k in range(m + 1)]
    groups = np.array([g for g in groups if g * 16 < n])
    recs = np.minimum(groups * 16 + rng.integers(0, 16, groups.size), n - 1)
    recs = np.unique(np.concatenate([recs, rng.integers(0, n, 300), [n - 1, n - 3]]))
    pos = rng.integers(0, size, recs.size)
    flip(torch, slab, size, recs, pos, rng.integers(0, 8, recs.size))
    # the partial group and its neighbours are compared with the oracle too
    touched = np.concatenate([recs, np.arange(n - 40, n)])
    r, f, t = check(torch, eng, slab, desc[:n], n, size, touched)
    assert (f["err"] == 2).sum() > 200    # the flips are seen as checksum errors


@pytest.mark.parametrize("size", [512, 1024])
def test_waves_without_a_group(torch, eng, full_waves, size):
    """n < 16 W: the last workgroup has waves with no group (they leave after the barrier)."""
    groups = 16 * 9 + 5
    n = 16 * (groups - 1) + 3
    assert n_waves(n, full_waves) == 16 * 10 > groups
    desc, pristine = packed(torch, eng, size, full_waves)
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(size)
    recs = np.unique(rng.integers(0, n, 64))
    flip(torch, slab, size, recs, rng.integers(0, size, recs.size), rng.integers(0, 8, recs.size))
    check(torch, eng, slab, desc[:n], n, size, np.concatenate([recs, np.arange(n - 20, n)]))


# k-th owned group of a wave -> does it ask for the checksum?  (True = crc, False = none)
PATTERNS = [
    (True, False, False, True, True),      # crc, none, none, crc
    (False, True, True, True, True),       # none first
    (True, True, True, True, False),       # none last
    (False, False, False, False, False),   # all none
    (False, True, False, True, False),     # alternating
    (True, False, True, False, True),      # alternating, other phase
]


def mode_slab(torch, eng, full_waves, size=512):
    """5 groups per wave; waves 3, 3 + 16, ... follow PATTERNS (one wave each, in different
    workgroups), wave 200's second group keeps the flag on a single record.  Flips: in the
    group before and after every switch, in flag-cleared groups, in trailer words."""
    W = full_waves
    m = 5
    n = 16 * (W * m) + 3          # wave 0 runs a sixth, partial group
    desc, pristine = packed(torch, eng, size, W)
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(77)
    cleared, seams = [], []
    for i, pat in enumerate(PATTERNS):
        w = 3 + 16 * i
        for k, crc in enumerate(pat):
            g = w + k * W
            if not crc:
                cleared.append(np.arange(16) + 16 * g)
            seams.append(g)      # every group of a patterned wave takes flips
    g1 = 200 + W                  # one record of this flag-cleared group keeps the flag
    cleared.append(np.delete(np.arange(16), 5) + 16 * g1)
    seams += [200, g1, 200 + 2 * W]
    cleared = np.concatenate(cleared)
    clear_flag(torch, slab, size, cleared)
    seams = np.array(seams)
    # two flips per seam group: one in the body, one in the trailer word (different records)
    body = seams * 16 + rng.integers(0, 8, seams.size)
    trail = seams * 16 + 8 + rng.integers(0, 8, seams.size)
    body[seams == g1], trail[seams == g1] = g1 * 16 + 5, g1 * 16 + 6   # the record that checks
    flip(torch, slab, size, body, rng.integers(64, size - 4, seams.size),
         rng.integers(0, 8, seams.size))
    flip(torch, slab, size, trail, rng.integers(size - 4, size, seams.size),
         rng.integers(0, 8, seams.size))
    groups = np.unique(np.concatenate([seams, cleared // 16]))
    touched = (groups[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    touched = np.concatenate([touched, np.arange(n - 20, n)])
    return desc[:n], slab, n, size, touched, cleared, body, trail, g1


@pytest.mark.parametrize("mode", ["udp", "udp_force", "tcp_force"])
def test_mode_switches(torch, eng, full_waves, mode):
    """Every order of pipelined and header-only groups per wave, with flips at the seams,
    under the three receive rules of test_unpack_matrix_all_receive_rules."""
    from mgen_amd import OPT_CHECKSUM_FORCE, OPT_TCP
    opts = {"udp": 0, "udp_force": OPT_CHECKSUM_FORCE,
            "tcp_force": OPT_TCP | OPT_CHECKSUM_FORCE}[mode]
    desc, slab, n, size, touched, cleared, body, trail, g1 = mode_slab(torch, eng, full_waves)
    r, f, t = check(torch, eng, slab, desc, n, size, touched, opts=opts)
    err = r["err"]
    flipped = np.concatenate([body, trail])
    is_cleared = np.isin(flipped, cleared)
    if mode == "udp":
        # a flag-cleared record is not checked: its flip goes unseen; the others are errors
        assert np.all(err[flipped[is_cleared]] == 0)
        assert np.all(err[flipped[~is_cleared]] == 2)
        assert err[g1 * 16 + 5] == 2 and err[g1 * 16 + 6] == 0
        assert np.all(r["flags"][cleared] & 0x04 == 0)
    else:
        assert np.all(err[flipped] == 2)   # forced: every record is checked


def test_dead_lanes_past_the_slab(torch, eng, full_waves):
    """slab_bytes short of n * stride: the last records (two whole groups, a partial one and
    a record that straddles the end) are dead lanes -- ERROR_OOB with every field zero, exactly
    as the column kernel reports them -- in waves that run pipelined and header-only groups."""
    size = 512
    W = full_waves
    n = 16 * (W * 2 + 40) + 3
    n_dead = 16 * 2 + 3 + 2
    desc, pristine = packed(torch, eng, size, W)
    slab = pristine[: n * size].clone()
    live = n - n_dead
    slab_bytes = live * size + size // 2
    rng = np.random.default_rng(5)
    # the groups that own the dead records' predecessors (one wave trip earlier) header-only
    g_last = (n - 1) // 16
    cl = ((np.array([g_last - W, g_last - 1 - W])[:, None]) * 16 + np.arange(16)[None, :]).reshape(-1)
    clear_flag(torch, slab, size, cl)
    recs = np.unique(np.concatenate([rng.integers(0, live, 64), np.arange(live - 8, live)]))
    flip(torch, slab, size, recs, rng.integers(64, size, recs.size), rng.integers(0, 8, recs.size))
    touched = np.concatenate([recs, cl, np.arange(live - 48, live)])
    from mgen_amd import OPT_CHECKSUM_FORCE
    for opts in (0, OPT_CHECKSUM_FORCE):
        check(torch, eng, slab, desc[:n], n, size, touched, opts=opts, slab_bytes=slab_bytes,
              n_dead=n_dead)
