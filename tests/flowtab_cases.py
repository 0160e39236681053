"""The inputs of the FindFlow edge cases (test_gpu_flowtab_edges.py), built here so that the
CPU suite (test_flowtab_ref_cpu.py) can assert from the model alone that every input reaches
the edge it is meant for.  A case is a list of calls on one table; a call is a batch (see
flowtab_ref).  Everything is cached and read-only: the tests share one build per case."""
import functools

import numpy as np

import flowtab_ref as R

SMALL = 2048      # max_flows of the LDS-staged path: 4096 slots
LARGE = 4096      # the smallest table on the HBM path: 8192 slots
STAGED = 1536     # the small path stages keys with an index below this
MAX_PROBE = 1024
SWEEP_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096)
COLS = ("dst_addr", "dst_len", "dst_port", "src", "flow_id", "err")


def make_pool(k, seed, fid0):
    """k distinct keys, one record each, zero past every address length: flow ids fid0 ..
    fid0 + k - 1 (pools of one table take disjoint ranges) over a few IPv4 / IPv6
    destinations, sources and ports, so many keys differ in one field only."""
    rng = np.random.default_rng(seed)
    i = np.arange(k)
    dsts = rng.integers(0, 256, (6, 16), dtype=np.uint8)
    srcs = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    dv6 = i % 5 == 4
    sv6 = i % 3 == 2
    b = {"dst_addr": dsts[rng.integers(0, 6, k)], "dst_len": np.where(dv6, 16, 4).astype(np.uint8),
         "dst_port": (5000 + rng.integers(0, 8, k)).astype(np.uint16),
         "src": np.zeros((k, 20), np.uint8), "flow_id": (fid0 + i).astype(np.uint32),
         "err": np.zeros(k, np.uint8)}
    b["src"][:, 0] = np.where(sv6, 2, 1)
    b["src"][:, 1] = np.where(sv6, 16, 4)
    b["src"][:, 2:4] = (7000 + rng.integers(0, 16, k)).astype("<u2").reshape(k, 1).view(np.uint8)
    b["src"][:, 4:] = srcs[rng.integers(0, 40, k)]
    return zero_tail(b)


def _tail(b, fill):
    pos = np.arange(16, dtype=np.uint8)[None, :]
    b["dst_addr"] = np.where(pos < b["dst_len"][:, None], b["dst_addr"], fill(0)).astype(np.uint8)
    b["src"][:, 4:] = np.where(pos < b["src"][:, 1:2], b["src"][:, 4:], fill(1))
    return b


def zero_tail(b):
    return _tail(b, lambda _: 0)


def garbage(b, rng):
    """random bytes at and past each address's length (not part of the key)"""
    n = len(b["dst_len"])
    return _tail(b, lambda _: rng.integers(0, 256, (n, 16), dtype=np.uint8))


def draw(pool, idx, rng=None, err_rate=0.0):
    """the records pool[idx], each with its own garbage padding; err_rate of them in error"""
    b = {c: pool[c][idx].copy() for c in COLS}
    if rng is not None:
        garbage(b, rng)
        if err_rate:
            b["err"] = (rng.random(len(idx)) < err_rate).astype(np.uint8)
    return b


def concat(*bs):
    return {c: np.concatenate([b[c] for b in bs]) for c in COLS}


def model(calls, max_keys=None):
    """[(indices, count)] of the calls on one fresh table, by the first-seen model"""
    t = R.FirstSeen(max_keys)
    return [t.lookup(R.batch_keys(b), b["err"]) for b in calls]


def first_good(b):
    """{key bytes: index of its first record without an error} of one batch"""
    rec = np.flatnonzero(b["err"] == 0)
    u, f = np.unique(R._void(R.batch_keys(b)[rec]), return_index=True)
    return {k.tobytes(): int(rec[j]) for k, j in zip(u, f)}


@functools.lru_cache(None)
def sweep(n):
    """a: n records, every one its own key (K == n), then the same batch again"""
    b = draw(make_pool(n, 1000 + n, 1), np.arange(n), np.random.default_rng(n))
    return [b, b]


@functools.lru_cache(None)
def sequence():
    """b: (five calls on one table, two calls on a second): new keys / only known keys / every
    record in error (its keys unknown: none may be created) / more new keys mixed with known /
    call 2 again; then all-error first, followed by call 1."""
    rng = np.random.default_rng(21)
    pool = make_pool(1300, 22, 1)
    c1 = draw(pool, np.concatenate([rng.permutation(600), rng.integers(0, 600, 4400)]), rng, 0.03)
    c1["err"][:600] = 0                                     # all 600 keys are created
    c2 = draw(pool, rng.integers(0, 600, 5000), rng, 0.03)
    c3 = draw(pool, rng.integers(0, 1300, 5000), rng)
    c3["err"][:] = rng.integers(1, 256, 5000)
    i4 = np.concatenate([600 + rng.permutation(300), rng.integers(0, 900, 4700)])
    c4 = draw(pool, rng.permutation(i4), rng, 0.03)
    return [c1, c2, c3, c4, c2], [c3, c1]


@functools.lru_cache(None)
def contention(n=8192, n_wave=250, n_spread=450):
    """c: one hot key and n_wave + n_spread others with two or three records each.  The hot
    key is on every record that is not one of theirs (79% of 8192: 700 keys of two or three
    records leave no room for more); its records in the first 4000/8192 of the batch are in
    error, so it is first seen there, after some of the others and before the rest.  n_wave
    of the others have all their records at random lanes of one 64-record wave, n_spread
    anywhere in the batch: a key's first record often sits in a higher lane, a later wave or
    a later 1024-record chunk than the second record of a key first seen after it.  Returns
    (calls, key number per record, the hot key's first good record)."""
    rng = np.random.default_rng(31 + n)
    hot_at, nw = n * 4000 // 8192, n // 64
    g = -(-n_wave // (nw // 2))                             # keys per chosen wave
    pool = make_pool(1 + n_wave + n_spread, 32, 1)
    key = np.zeros(n, np.int64)                             # pool[0]: the hot key
    free = np.ones(n, bool)
    free[hot_at] = False
    w = rng.choice(np.delete(np.arange(nw), hot_at // 64), -(-n_wave // g), replace=False)
    lanes = np.argsort(rng.random((w.size, 64)), axis=1)[:, :3 * g].reshape(-1, 3)
    at = (np.repeat(w, g)[:, None] * 64 + lanes)[:n_wave]
    free[at.reshape(-1)] = False
    at = np.concatenate([at, rng.permutation(np.flatnonzero(free))[:3 * n_spread].reshape(-1, 3)])
    two = rng.random(at.shape[0]) < 0.5                     # two records, not three
    k = np.arange(1, 1 + at.shape[0])
    key[at[:, 0]], key[at[:, 1]] = k, k
    key[at[~two, 2]] = k[~two]
    b = draw(pool, key, rng)
    b["err"] = ((key == 0) & (np.arange(n) < hot_at)).astype(np.uint8)
    return [b], key, hot_at


# (n, keys in one wave, keys anywhere, max_flows): 8192 records on both paths, and on the large
# path a batch of more records than the device runs threads at once (256 CUs x 2048)
CONTENTION = ((8192, 250, 450, SMALL), (8192, 250, 450, LARGE),
              (1 << 20, 2000, 6000, 65_536))


FAMILIES = ("base", "dst3", "dst15", "dst_len", "dst_port", "src_port", "src_len", "src15",
            "flow_id")


@functools.lru_cache(None)
def families():
    """d: a base record and one family per key field, the members differing in that field
    only; every member 12 times -- four copies for each source type byte 0, 1, 2 -- each copy
    with its own random bytes past the address lengths.  Returns (calls, member id per
    record, number of members)."""
    def rec(**kw):
        r = {"dst": bytes([224, 1, 2, 3]), "dst_len": 4, "dst_port": 5000,
             "src": bytes([10, 1, 2, 3]), "src_len": 4, "src_port": 7000, "flow_id": 5}
        r.update(kw)
        return r
    v6 = bytes(range(0x20, 0x2F))                            # 15 bytes; byte 15 is the member
    mem = [("base", rec())]
    mem += [("dst3", rec(dst=bytes([224, 1, 2, x]))) for x in (4, 0, 255)]
    mem += [("dst15", rec(dst=v6 + bytes([x]), dst_len=16)) for x in (0, 1, 255)]
    mem += [("dst_len", rec(dst=bytes([224, 9, 9, 9]), dst_len=x)) for x in (4, 16)]
    mem += [("dst_port", rec(dst_port=x)) for x in (0, 1, 0x8000, 0xFFFF)]
    mem += [("src_port", rec(src_port=x)) for x in (0, 1, 0x8000, 0xFFFF)]
    mem += [("src_len", rec(src=bytes([10, 9, 9, 9]), src_len=x)) for x in (0, 4, 16)]
    mem += [("src15", rec(src=v6 + bytes([x]), src_len=16)) for x in (0, 1, 255)]
    mem += [("flow_id", rec(flow_id=x)) for x in (0, 1, 0x80000000, 0xFFFFFFFF)]
    assert {f for f, _ in mem} == set(FAMILIES)
    m = len(mem)
    pool = {"dst_addr": np.zeros((m, 16), np.uint8), "dst_len": np.zeros(m, np.uint8),
            "dst_port": np.zeros(m, np.uint16), "src": np.zeros((m, 20), np.uint8),
            "flow_id": np.zeros(m, np.uint32), "err": np.zeros(m, np.uint8)}
    for j, (_, r) in enumerate(mem):
        pool["dst_addr"][j, :len(r["dst"])] = np.frombuffer(r["dst"], np.uint8)
        pool["dst_len"][j], pool["dst_port"][j], pool["flow_id"][j] = (
            r["dst_len"], r["dst_port"], r["flow_id"])
        pool["src"][j, 1] = r["src_len"]
        pool["src"][j, 2:4] = np.frombuffer(np.uint16(r["src_port"]).tobytes(), np.uint8)
        pool["src"][j, 4:4 + len(r["src"])] = np.frombuffer(r["src"], np.uint8)
    rng = np.random.default_rng(41)
    member = rng.permutation(np.repeat(np.arange(m), 12))
    b = draw(pool, member, rng)
    for j in range(m):                                       # types 0, 1, 2: four copies each
        b["src"][np.flatnonzero(member == j), 0] = np.repeat([0, 1, 2], 4)
    return [b], member, m


@functools.lru_cache(None)
def past_staged():
    """e (small path): 2,000 keys, one record each (indices 1536 and above are not staged in
    LDS); 20,000 records over all of them and 30 new keys; the same again."""
    rng = np.random.default_rng(51)
    pool = make_pool(2030, 52, 1)
    c1 = draw(pool, np.arange(2000), rng)
    i2 = np.concatenate([np.arange(2030), rng.integers(0, 2030, 20_000 - 2030)])
    c2 = draw(pool, rng.permutation(i2), rng)
    return [c1, c2, c2]


F_N, F_KEYS, F_FLOWS = 1_100_000, 20_000, 65_536


@functools.lru_cache(None)
def above_1m():
    """f (large path): 1,100,000 records (1075 chunks of 1024: the first / number kernels loop
    over their 512 blocks, the chunk scan takes a second pass of 1024) over 20,000 keys first
    seen all along the batch, 3,000 of them past record 1,048,576; 2% errors.  Then as many
    records over the same keys and 500 new ones, first seen in the last 40,000 records."""
    n, k, rng = F_N, F_KEYS, np.random.default_rng(61)
    pool = make_pool(k + 500, 62, 1)
    first = np.concatenate([rng.choice(1 << 20, k - 3000, replace=False),
                            (1 << 20) + rng.choice(n - (1 << 20), 3000, replace=False)])
    first.sort()
    first[0] = 0
    seen = np.searchsorted(first, np.arange(n), side="right")   # keys met up to each record
    key = (rng.random(n) * seen).astype(np.int64)
    key[first] = np.arange(k)
    c1 = draw(pool, key, rng, 0.02)
    c1["err"][first] = 0                                    # every key is seen where placed
    key2 = rng.integers(0, k, n)
    at = n - 40_000 + rng.choice(40_000, 2000, replace=False)
    key2[at] = k + np.concatenate([np.arange(500), rng.integers(0, 500, 1500)])
    c2 = draw(pool, key2, rng, 0.02)
    c2["err"][at] = 0
    return [c1, c2]


@functools.lru_cache(None)
def bound(max_flows):
    """g: exactly max_flows distinct keys (all admitted: each creator reads fewer held), then
    1,000 further keys among 2,000 records of held ones: refused, every one."""
    rng = np.random.default_rng(71 + max_flows)
    pool = make_pool(max_flows + 1000, 72, 1)
    c1 = draw(pool, rng.permutation(max_flows), rng)
    i2 = np.concatenate([max_flows + np.arange(1000), rng.integers(0, max_flows, 2000)])
    c2 = draw(pool, rng.permutation(i2), rng)
    return [c1, c2]


@functools.lru_cache(None)
def overflow():
    """h (large path): 60,000 records over 6,000 keys on a table that takes 4096; returns
    (calls, key number per record)"""
    rng = np.random.default_rng(81)
    key = rng.integers(0, 6000, 60_000)
    b = draw(make_pool(6000, 82, 1), key, rng)
    return [b, b], key


CLUSTER_SEED = 7
CLUSTER_FID0 = 1 << 31      # make_pool's flow ids stay far below the clusters'


def _ordinary(k, seed):
    p = make_pool(k, seed, 1)
    assert p["flow_id"].max() < CLUSTER_FID0
    return p


@functools.lru_cache(None)
def wrap(cap):
    """i: 300 keys whose home is the table's last slot (at least 299 of them sit in slot 0 and
    beyond, whatever the order) among 500 ordinary keys, 3,000 shuffled records; then all of
    them again with 50 more keys of the cluster.  Returns (calls, the cluster's batch)."""
    rng = np.random.default_rng(91 + cap)
    cl = R.cluster(cap, cap - 1, 350, CLUSTER_SEED)
    pool = concat(cl, _ordinary(500, 92))
    i1 = np.concatenate([np.arange(300), 350 + np.arange(500)])
    i1 = np.concatenate([i1, rng.choice(i1, 3000 - i1.size)])
    i2 = np.concatenate([np.arange(850), rng.integers(0, 850, 2150)])
    return [draw(pool, rng.permutation(i1), rng), draw(pool, rng.permutation(i2), rng)], cl


@functools.lru_cache(None)
def probe_limit():
    """j (small path): 1,100 keys with home 4095.  The first 1,024, one record each, fit inside
    1,024 probes in any order; then those again mixed with the other 76, which find no room
    within the probe limit.  Returns (calls, the cluster's batch)."""
    rng = np.random.default_rng(101)
    cl = R.cluster(2 * SMALL, 2 * SMALL - 1, 1100, CLUSTER_SEED)
    i2 = np.concatenate([np.arange(1100), rng.integers(0, 1100, 1100)])
    return [draw(cl, rng.permutation(MAX_PROBE), rng), draw(cl, rng.permutation(i2), rng)], cl


@functools.lru_cache(None)
def hash_pin():
    """4,096 varied keys for the device's home slots"""
    return draw(make_pool(4096, 111, 1), np.arange(4096), np.random.default_rng(112))
