"""CPU: the first-seen model of FindFlow (flowtab_ref) against a per-record dict walk and
hand-written keys, and the preconditions of every case of test_gpu_flowtab_edges.py, asserted
from the model alone: a GPU case cannot go green on an input that missed its edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flowtab_cases as C  # noqa: E402
import flowtab_ref as R  # noqa: E402

NONE = R.FLOW_NONE


def test_first_seen_equals_dict_walk():
    """5,000 records over three calls (errors, IPv4 and IPv6, garbage padding): FirstSeen
    equals the per-record dict.setdefault walk of test_gpu_flowtab.py."""
    rng = np.random.default_rng(3)
    pool = C.make_pool(700, 4, 1)
    table, ref = R.FirstSeen(), {}
    for n, hi in ((2000, 300), (1000, 300), (2000, 700)):
        b = C.draw(pool, rng.integers(0, hi, n), rng, 0.05)
        got, cnt = table.lookup(R.batch_keys(b), b["err"])
        want = np.zeros(n, np.uint32)
        for i in range(n):
            if b["err"][i]:
                want[i] = NONE
                continue
            dl, sl = int(b["dst_len"][i]), int(b["src"][i, 1])
            key = (b["dst_addr"][i, :dl].tobytes(), int(b["dst_port"][i]),
                   b["src"][i, 4:4 + sl].tobytes(), b["src"][i, 2:4].tobytes(),
                   int(b["flow_id"][i]))
            want[i] = ref.setdefault(key, len(ref))
        assert np.array_equal(got, want)
        assert cnt == len(ref) == len(table)
    assert len(ref) > 600 and (b["dst_len"] == 16).any() and (b["src"][:, 1] == 16).any()


def test_first_seen_max_keys():
    b = C.draw(C.make_pool(10, 5, 1), np.array([0, 1, 0, 2, 3, 1, 4, 2]))
    got, cnt = R.FirstSeen(max_keys=3).lookup(R.batch_keys(b), b["err"])
    assert got.tolist() == [0, 1, 0, 2, NONE, 1, NONE, 2] and cnt == 3


def _one(dst=(224, 1, 2, 3), dst_len=4, dst_port=5000, src=(10, 1, 2, 3), src_type=1, src_len=4,
         src_port=7000, flow_id=5, dst_tail=0, src_tail=0):
    da = np.full(16, dst_tail, np.uint8)
    da[:len(dst)] = dst
    s = np.full(20, src_tail, np.uint8)
    s[0], s[1] = src_type, src_len
    s[2:4] = np.frombuffer(np.uint16(src_port).tobytes(), np.uint8)
    s[4:4 + len(src)] = src
    return R.key_bytes(da, [dst_len], [dst_port], s, [flow_id])[0].tobytes()


def test_key_bytes_hand_written():
    base = _one()
    assert base == bytes([0, 4, 0x88, 0x13, 224, 1, 2, 3] + [0] * 12 +
                         [0, 4, 0x58, 0x1B, 10, 1, 2, 3] + [0] * 12 + [5, 0, 0, 0])
    assert len(base) == R.KEY_BYTES
    # garbage past the lengths, another source type byte: the same key
    assert _one(dst_tail=0xEE, src_tail=0x77) == base
    assert _one(src_type=0) == _one(src_type=2) == base
    v6 = tuple(range(0x20, 0x30))
    assert _one(dst=v6, dst_len=16, dst_tail=9) == _one(dst=v6, dst_len=16)
    assert _one(src_len=0, src_tail=0xAB) == _one(src_len=0, src=())
    # each single-field change: another key
    other = [_one(dst=(224, 1, 2, 4)), _one(dst=v6, dst_len=16),
             _one(dst=v6[:15] + (0,), dst_len=16), _one(dst_len=16), _one(dst_port=5001),
             _one(dst_port=0x8813), _one(src_port=7001), _one(src_port=0x9B58),
             _one(src_len=0), _one(src_len=16), _one(src=v6, src_len=16),
             _one(src=v6[:15] + (0,), src_len=16), _one(src=(10, 1, 2, 4)), _one(flow_id=4),
             _one(flow_id=5 | 1 << 31), _one(flow_id=0)]
    assert len(set(other + [base])) == len(other) + 1


def test_slot_hash_by_hand():
    """slot_hash against the same steps in plain Python integers"""
    keys = R.batch_keys(C.hash_pin())[:64]
    M = 0xFFFFFFFF
    for k, got in zip(keys, R.slot_hash(keys)):
        w = [int.from_bytes(k[4 * j:4 * j + 4].tobytes(), "little") for j in range(11)]
        words = w[1:5] + w[6:10] + [int(k[1]) | (w[0] >> 16) << 16,
                                     int(k[21]) | (w[5] >> 16) << 16, w[10]]
        h = 0x9E3779B9
        for x in words:
            h ^= x
            h = (h << 13 | h >> 19) & M
            h = (h * 5 + 0xE6546B64) & M
        h ^= h >> 16
        h = h * 0x7FEB352D & M
        h ^= h >> 15
        h = h * 0x846CA68B & M
        h ^= h >> 16
        assert h == int(got)


@pytest.mark.parametrize("cap,home,count", [(8192, 8191, 350), (4096, 4095, 1100), (4096, 7, 20)])
def test_cluster_has_its_home(cap, home, count):
    cl = R.cluster(cap, home, count, C.CLUSTER_SEED)
    keys = R.batch_keys(cl)
    assert len({k.tobytes() for k in keys}) == count == len(cl["flow_id"])
    assert np.all(R.slot_hash(keys) & (cap - 1) == home)
    assert cl["flow_id"].min() >= C.CLUSTER_FID0


# ---- the preconditions of the GPU cases

@pytest.mark.parametrize("n", C.SWEEP_N)
def test_pre_sweep(n):
    (i1, k1), (i2, k2) = C.model(C.sweep(n))
    assert np.array_equal(i1, np.arange(n)) and np.array_equal(i2, i1) and k1 == k2 == n


def test_pre_sequence():
    main, fresh = C.sequence()
    k = [cnt for _, cnt in C.model(main)]
    assert 0 < k[0] == k[1] == k[2] < k[3] == k[4]          # calls 2, 3, 5 create no key
    assert 550 <= k[0] <= 650 and 250 <= k[3] - k[0] <= 350
    assert all(len(b["err"]) == 5000 for b in main)
    assert np.all(main[2]["err"] != 0)
    # the all-error call carries keys the table never saw: none may be created by it
    assert len(C.first_good({**main[2], "err": np.zeros(5000, np.uint8)})) > k[3]
    (i0, k0), (_, k1) = C.model(fresh)
    assert k0 == 0 and np.all(i0 == NONE) and k1 == k[0]


@pytest.mark.parametrize("args", C.CONTENTION)
def test_pre_contention(args):
    n, n_wave, n_spread, max_flows = args
    (b,), key, hot_at = C.contention(n, n_wave, n_spread)
    nk = 1 + n_wave + n_spread
    assert n == len(key) and hot_at == n * 4000 // 8192 and nk <= max_flows
    assert (key == 0).mean() > 0.75
    first = C.first_good(b)
    hot = R.batch_keys(b)[hot_at].tobytes()
    assert key[hot_at] == 0 and first[hot] == hot_at and len(first) == nk
    assert (key[:hot_at] == 0).sum() > 0.3 * n              # in error: not the key's first
    order = np.argsort(key, kind="stable")
    pos = np.split(order, np.cumsum(np.bincount(key))[:-1])[1:]
    assert len(pos) == nk - 1 and all(2 <= p.size <= 3 for p in pos)
    assert sum(len(set(p // 64)) == 1 for p in pos) >= 100
    assert sum(len(set(p // 1024)) == p.size for p in pos) >= 100
    idx, cnt = C.model([b])[0]
    assert cnt == nk and 0.1 * nk < idx[hot_at] < 0.9 * nk
    f = np.array(sorted(first.values()))
    assert np.array_equal(idx[f], np.arange(nk))            # numbered by first record


def test_pre_families():
    (b,), member, m = C.families()
    idx, cnt = C.model([b])[0]
    assert cnt == m == len(set(member.tolist())) == 27
    assert len(b["err"]) == 12 * m
    # copies share an index, members do not
    assert len({(int(a), int(c)) for a, c in zip(member, idx)}) == m
    for j in range(m):
        at = np.flatnonzero(member == j)
        assert sorted(b["src"][at, 0].tolist()) == [0] * 4 + [1] * 4 + [2] * 4
        # the copies differ in their padding wherever there is any
        if b["dst_len"][at[0]] < 16:
            assert len({r.tobytes() for r in b["dst_addr"][at]}) == 12
        if b["src"][at[0], 1] < 16:
            assert len({r.tobytes() for r in b["src"][at, 4:]}) == 12


def test_pre_past_staged():
    calls = C.past_staged()
    (i1, k1), (i2, k2), (i3, k3) = C.model(calls)
    assert np.array_equal(i1, np.arange(2000)) and k1 == 2000 and k2 == k3 == 2030 <= C.SMALL
    assert len(i2) == 20_000 and np.array_equal(i2, i3)
    looked = set(i2.tolist())
    assert len([x for x in looked if C.STAGED <= x < 2000]) >= 400
    assert {C.STAGED - 1, C.STAGED} <= looked and len(looked) == 2030


def test_pre_above_1m():
    c1, c2 = C.above_1m()
    n = C.F_N
    assert len(c1["err"]) == len(c2["err"]) == n and (n + 1023) // 1024 > 1024
    f1 = np.array(list(C.first_good(c1).values()))
    assert f1.size == C.F_KEYS <= C.F_FLOWS
    assert (f1 > 1_048_576).sum() >= 1000
    assert ((f1 > 524_288) & (f1 <= 1_048_576)).sum() >= 1000
    assert (f1 < 524_288).sum() >= 1000
    for c in (c1, c2):
        assert 0.015 < c["err"].mean() < 0.025
    g1, g2 = C.first_good(c1), C.first_good(c2)
    new = [v for k, v in g2.items() if k not in g1]
    assert len(new) == 500 and min(new) >= n - 40_000 and len(g2) == C.F_KEYS + 500


@pytest.mark.parametrize("max_flows", [C.SMALL, C.LARGE])
def test_pre_bound(max_flows):
    c1, c2 = C.bound(max_flows)
    (i1, k1), (i2, k2) = C.model([c1, c2], max_keys=max_flows)
    assert np.array_equal(i1, np.arange(max_flows)) and k1 == k2 == max_flows
    assert (i2 == NONE).sum() == 1000 and len(C.first_good(c2)) >= 1000 + 1000
    assert i2[i2 != NONE].max() < max_flows


def test_pre_overflow():
    (b, b2), key = C.overflow()
    assert b is b2 and len(key) == 60_000 and len(C.first_good(b)) == 6000 > C.LARGE


@pytest.mark.parametrize("cap", [2 * C.SMALL, 2 * C.LARGE])
def test_pre_wrap(cap):
    (c1, c2), cl = C.wrap(cap)
    keys = R.batch_keys(cl)
    assert len({k.tobytes() for k in keys}) == 350
    assert np.all(R.slot_hash(keys) & (cap - 1) == cap - 1)
    cl_keys = {k.tobytes() for k in keys[:300]}
    g1, g2 = C.first_good(c1), C.first_good(c2)
    assert len(c1["err"]) == len(c2["err"]) == 3000
    assert cl_keys <= set(g1) and len(g1) == 800 and len(g2) == 850 and set(g1) <= set(g2)
    assert {k.tobytes() for k in keys[300:]} == set(g2) - set(g1)
    assert C.model([c1, c2])[1][1] == 850 <= C.SMALL


def test_pre_probe_limit():
    (c1, c2), cl = C.probe_limit()
    keys = R.batch_keys(cl)
    assert len({k.tobytes() for k in keys}) == 1100
    assert np.all(R.slot_hash(keys) & 4095 == 4095)
    (i1, k1), (i2, k2) = C.model([c1, c2], max_keys=C.MAX_PROBE)
    assert sorted(i1.tolist()) == list(range(1024)) and k1 == k2 == 1024
    assert len(C.first_good(c2)) == 1100
    assert len(set(R.batch_keys(c2)[i2 == NONE].view("V44")[:, 0].tolist())) == 76
    assert set(i2[i2 != NONE].tolist()) == set(range(1024))


def test_pre_hash_pin():
    b = C.hash_pin()
    home = R.slot_hash(R.batch_keys(b)) & 4095
    assert len(b["err"]) == 4096 and len(set(home.tolist())) > 2000
