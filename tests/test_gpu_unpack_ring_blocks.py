"""Loop edges of unpack_fixed_ring_kernel for every ring shape that has loop structure of its
own: the product shape (16 waves per workgroup, one 4-row block, 16 groups of row output held,
non-temporal row loads) and the diagnostics build's two-block shape 18 (8 waves, two 8-row
blocks, 32 groups held), whose 512-byte form keeps two groups in the ring and runs two groups
per loop trip.  Variants 17 and 28 are the product shape with plain and with non-temporal loads
whatever the batch size (the dispatch picks plain loads for 512-byte batches under 393,216
records and never for 1024-byte ones, so every case here also runs the instantiations the
product reaches only at other sizes).  SHAPES is the one place that states each shape's wave count and K; every size
below is derived from it, so that the cases land on the edges of W = waves x CUs: trip counts
1, 2, 3 (odd and even) with a partial last group, waves without a group, bit flips on both
sides of the block seam and in the first rows of each reloaded block, every order of
pipelined and header-only groups over three groups of a wave, records past the slab's end, and
the burst edge of the held row output (K and K + 1 groups per wave).

Rows are compared with the oracle (every record a case touched), with the column kernel of
the product library on the same slab (every record) and with the descriptors the slab was
packed from (every untouched record)."""
import itertools

import numpy as np
import pytest

from test_gpu_parity import COLMAP, _config2, host_cols, rows_to_cols

pytestmark = pytest.mark.gpu

CORE = COLMAP[:13]
# unpack variant of the diagnostics build (0 = the product library's dispatch) ->
# (waves per workgroup, K = groups of row output held per wave); see launch_unpack
SHAPES = {0: (16, 16), 18: (8, 32), 17: (16, 16), 28: (16, 16)}
SHAPE_IDS = {0: "product", 18: "two_blocks", 17: "plain_loads", 28: "nt_loads"}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def engs(torch):
    """variant -> engine: the product library, and the diagnostics library set to each shape."""
    from mgen_amd import Engine
    out = {0: Engine(0)}
    for v in SHAPES:
        if v:
            out[v] = Engine(0, diag=True)
            out[v].set_unpack_variant(v)
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def waves(shape, cus, n=None):
    """W of a launch: grid = min(ceil(groups / waves per workgroup), CUs)."""
    wpb = SHAPES[shape][0]
    if n is None:
        return wpb * cus
    groups = (n + 15) // 16
    return wpb * min((groups + wpb - 1) // wpb, cus)


def trip_n(W, m):
    """n = 16 (W m + r) + 3: waves 0 .. r run m + 1 groups (wave r's last one is the partial
    group of 3 records), the others m."""
    return 16 * (W * m + W // 3 + 7) + 3


_packed = {}


def packed(torch, eng, size, n):
    """(descriptors, pristine slab) of at least n records of `size` bytes, packed once on the
    GPU (a slab of n records is a prefix of a larger one); cases work on clones of prefixes."""
    have = _packed.get(size)
    if have is None or len(have[0]) < n:
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


def group_recs(groups):
    return (np.asarray(groups)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)


def seam_flips(size, groups, n):
    """(record, byte position) pairs in `groups`: the last byte of row 7 and the first byte of
    row 8 (1024-byte records: the seam of the two 8-row blocks), the last byte of row 0, the
    first body byte of the record's second half, and the trailer word -- each in a record of
    its own."""
    half = size // 2
    pos = [half - 1, half, 63, half + 64, size - 1, size - 4]
    recs, at = [], []
    for g in groups:
        for k, p in enumerate(pos):
            r = 16 * g + (2 * k + g) % 16
            if r < n:
                recs.append(r)
                at.append(p)
    return np.array(recs), np.array(at)


def check(torch, engs, shape, slab, desc, n, size, touched, opts=0, slab_bytes=None, n_dead=0):
    """Rows of the ring kernel in `shape` against the product library's column kernel (all
    records), the oracle (touched records) and the descriptors (the rest); the last n_dead
    records lie past slab_bytes."""
    from mgen_amd import ERROR_OOB, OPT_CHECKSUM_FORCE, OPT_TCP, UNPACK_K_FIXED_RING
    from oracle import oracle as O
    kw = {} if slab_bytes is None else {"slab_bytes": slab_bytes}
    c = host_cols(engs[0].unpack(slab, n, stride=size, fixed_len=size, opts=opts, **kw), n)
    eng = engs[shape]
    rows = eng.alloc_rows(n)
    eng.unpack(slab, n, stride=size, fixed_len=size, opts=opts, cols={"rows": rows}, **kw)
    assert eng.last_unpack_kernel() == UNPACK_K_FIXED_RING   # the kernel under test ran
    torch.cuda.synchronize()
    r = rows_to_cols(rows, n)
    for gname, _, dt in CORE:
        bad = np.nonzero(r[gname].view(dt)[:n] != c[gname].view(dt)[:n])[0]
        assert bad.size == 0, (size, shape, opts, "rows vs cols", gname, bad[:8])
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
        assert bad.size == 0, (size, shape, opts, "rows vs oracle", gname, touched[bad[:8]],
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


def largest_n(cus):
    """records of the largest slab short of the burst-edge one: four groups per wave"""
    return max(16 * 4 * waves(s, cus) + 3 for s in SHAPES)


shape_param = pytest.mark.parametrize("shape", list(SHAPES), ids=[SHAPE_IDS[s] for s in SHAPES])


@shape_param
@pytest.mark.parametrize("size", [512, 1024])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_trip_counts_and_seams(torch, engs, cus, shape, size, m):
    """Waves of m and of m + 1 groups in one launch (odd and even counts: at 512 bytes the
    two-block shape runs two groups per trip), the last group partial (3 records).  Every
    group of waves 0, r (whose last group is the partial one), r + 1 and W - 1 takes a flip on
    both sides of the block seam, in the first rows of the blocks and in the trailer word."""
    W = waves(shape, cus)
    n = trip_n(W, m)
    assert waves(shape, cus, n) == W
    desc, pristine = packed(torch, engs[0], size, largest_n(cus))
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(100 * m + size + shape)
    r_ = W // 3 + 7
    groups = [w + k * W for w in (0, r_, r_ + 1, W - 1) for k in range(m + 1)]
    groups = np.array([g for g in groups if g * 16 < n])
    recs, pos = seam_flips(size, groups, n)
    extra = np.setdiff1d(np.unique(np.concatenate([rng.integers(0, n, 200), [n - 1, n - 3]])), recs)
    recs = np.concatenate([recs, extra])
    pos = np.concatenate([pos, rng.integers(64, size, extra.size)])
    flip(torch, slab, size, recs, pos, rng.integers(0, 8, recs.size))
    touched = np.concatenate([recs, group_recs(groups), np.arange(n - 40, n)])
    r, f, t = check(torch, engs, shape, slab, desc[:n], n, size, touched)
    body = recs[pos >= 64]   # a flip past the header is a checksum error, nothing else
    assert np.all(r["err"][body] == 2)


@shape_param
@pytest.mark.parametrize("size", [512, 1024])
def test_waves_without_a_group(torch, engs, cus, shape, size):
    """Fewer groups than waves: the last workgroup has waves with no group (they leave after
    the barrier), and every other wave has exactly one (at 512 bytes the two-block shape then
    has no second group for its ring)."""
    wpb = SHAPES[shape][0]
    groups = wpb * 9 + 5
    n = 16 * (groups - 1) + 3
    assert waves(shape, cus, n) == wpb * 10 > groups
    desc, pristine = packed(torch, engs[0], size, largest_n(cus))
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(size + shape)
    recs, pos = seam_flips(size, np.array([0, 1, groups - 2, groups - 1]), n)
    flip(torch, slab, size, recs, pos, rng.integers(0, 8, recs.size))
    check(torch, engs, shape, slab, desc[:n], n, size,
          np.concatenate([recs, np.arange(n - 20, n)]))


# does the k-th of three consecutive groups of a wave ask for the checksum?
ORDERS = list(itertools.product([True, False], repeat=3))


def mode_slab(torch, engs, cus, shape, size):
    """Waves 3, 3 + wpb, ... (one per workgroup) run four groups: the first three follow one of
    ORDERS each, the fourth asks for the checksum; a second set of waves has the three groups
    behind a checksummed first one.  One group keeps the flag on a single record.  Every group
    of those waves takes the seam flips."""
    W = waves(shape, cus)
    wpb = SHAPES[shape][0]
    n = 16 * (W * 4) + 3          # wave 0 runs a fifth, partial group
    desc, pristine = packed(torch, engs[0], size, largest_n(cus))
    slab = pristine[: n * size].clone()
    rng = np.random.default_rng(77 + shape)
    cleared, seams = [], []
    for i, order in enumerate(ORDERS):
        for first, w in ((0, 3 + wpb * i), (1, 5 + wpb * (i + len(ORDERS)))):
            for k, crc in enumerate(order):
                if not crc:
                    cleared.append(group_recs([w + (k + first) * W]))
            seams += [w + k * W for k in range(4)]
    g1 = 200 + W                  # one record of this flag-cleared group keeps the flag
    cleared.append(np.delete(np.arange(16), 5) + 16 * g1)
    seams += [200, g1, 200 + 2 * W]
    cleared = np.concatenate(cleared)
    clear_flag(torch, slab, size, cleared)
    recs, pos = seam_flips(size, np.array(seams), n)
    keep = pos != 63              # header bytes stay: the flags decide the mode here
    recs, pos = recs[keep], pos[keep]
    recs = np.concatenate([recs, [g1 * 16 + 5]])
    pos = np.concatenate([pos, [size - 7]])
    recs, first = np.unique(recs, return_index=True)
    pos = pos[first]
    flip(torch, slab, size, recs, pos, rng.integers(0, 8, recs.size))
    touched = np.concatenate([group_recs(np.unique(seams)), np.arange(n - 20, n)])
    return desc[:n], slab, n, touched, cleared, recs, g1


@shape_param
@pytest.mark.parametrize("size", [512, 1024])
@pytest.mark.parametrize("mode", ["udp", "udp_force", "tcp_force"])
def test_mode_switch_orders(torch, engs, cus, shape, size, mode):
    """Every order of pipelined and header-only groups over three consecutive groups of a
    wave, from the wave's first group and from its second, with flips in the group before and
    after each switch, under the plain, forced and TCP receive rules."""
    from mgen_amd import OPT_CHECKSUM_FORCE, OPT_TCP
    opts = {"udp": 0, "udp_force": OPT_CHECKSUM_FORCE,
            "tcp_force": OPT_TCP | OPT_CHECKSUM_FORCE}[mode]
    desc, slab, n, touched, cleared, flipped, g1 = mode_slab(torch, engs, cus, shape, size)
    r, f, t = check(torch, engs, shape, slab, desc, n, size, touched, opts=opts)
    err = r["err"]
    is_cleared = np.isin(flipped, cleared)
    if mode == "udp":
        # a flag-cleared record is not checked: its flip goes unseen; the others are errors
        assert np.all(err[flipped[is_cleared]] == 0)
        assert np.all(err[flipped[~is_cleared]] == 2)
        assert err[g1 * 16 + 5] == 2
        assert np.all(r["flags"][cleared] & 0x04 == 0)
    else:
        assert np.all(err[flipped] == 2)   # forced: every record is checked


@shape_param
@pytest.mark.parametrize("size", [512, 1024])
@pytest.mark.parametrize("n_dead", [2, 3, 16 + 3 + 2])
def test_records_past_the_slab(torch, engs, cus, shape, size, n_dead):
    """slab_bytes short of n * stride: dead lanes in the last (partial) group, a whole dead
    last group, and a dead group before it -- ERROR_OOB with every field zero, as the column
    kernel reports them; the first dead record straddles the end."""
    from mgen_amd import OPT_CHECKSUM_FORCE
    W = waves(shape, cus)
    n = 16 * (W * 2 + 40) + 3
    desc, pristine = packed(torch, engs[0], size, largest_n(cus))
    slab = pristine[: n * size].clone()
    live = n - n_dead
    slab_bytes = live * size + size // 2
    rng = np.random.default_rng(5 + shape)
    # the groups one wave trip before the dead ones run header-only
    g_last = (n - 1) // 16
    cl = group_recs([g_last - W, g_last - 1 - W])
    clear_flag(torch, slab, size, cl)
    recs = np.unique(np.concatenate([rng.integers(0, live, 64), np.arange(live - 8, live)]))
    flip(torch, slab, size, recs, rng.integers(64, size, recs.size), rng.integers(0, 8, recs.size))
    touched = np.concatenate([recs, cl, np.arange(live - 48, live)])
    for opts in (0, OPT_CHECKSUM_FORCE):
        check(torch, engs, shape, slab, desc[:n], n, size, touched, opts=opts,
              slab_bytes=slab_bytes, n_dead=n_dead)


@shape_param
def test_row_burst_edge(torch, engs, cus, shape):
    """512-byte records, n = 16 (W K + r) + 3: waves 0 .. r hold K + 1 groups of row output (a
    burst of K, then one of 1), the others exactly K (one burst).  Full rows of the waves on
    both sides of r against the oracle, every row against the column kernel."""
    size = 512
    W, K = waves(shape, cus), SHAPES[shape][1]
    r_ = W // 3 + 7
    n = 16 * (W * K + r_) + 3
    n_max = max(16 * (waves(s, cus) * SHAPES[s][1] + waves(s, cus) // 3 + 7) + 3 for s in SHAPES)
    desc, pristine = packed(torch, engs[0], size, n_max)
    slab = pristine[: n * size]
    rng = np.random.default_rng(9 + shape)
    groups = np.array([w + k * W for w in (r_ - 1, r_, r_ + 1) for k in range(K + 1)])
    groups = groups[groups * 16 < n]
    recs = groups * 16 + rng.integers(0, 16, groups.size)
    recs = recs[recs < n]
    pos, bits = rng.integers(64, size, recs.size), rng.integers(0, 8, recs.size)
    flip(torch, slab, size, recs, pos, bits)
    try:
        r, f, t = check(torch, engs, shape, slab, desc[:n], n, size, group_recs(groups))
    finally:
        flip(torch, slab, size, recs, pos, bits)   # the shared slab stays pristine
    assert np.all(r["err"][recs] == 2)
