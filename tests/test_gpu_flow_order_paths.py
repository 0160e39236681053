"""GPU: every ordering path in front of mgenx_flow_reduce's update, forced through the
diagnostics build (MGENX_AN_SCAN1 / MGENX_AN_RADIX / MGENX_AN_TILE) at the flow, tile and
record counts where their index arithmetic has its edges: the counting sort with the
single-pass scan and with colpart / colbase / colscan, the radix sort, tiles of 4096 and 4608
records, and the product library's own dispatch.  State, counts, reports and report_rec are
byte-equal across the paths and equal to the oracle (report_rec: the record with the closing
receive time; receive times are unique here).  Then the single-pass scan's give-up branch,
forced (MGENX_AN_C1_GIVEUP), and its epoch wrap (MGENX_AN_C1_WRAP)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_value_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, TILE_BIG, BIG_MAX_FLOWS = 4096, 4608, 1222
PER_FLOW, WINDOW, FILL = 4, 0.05, C.FILL
M, T0 = 10**6, 1_700_000_000


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
def eng_diag(torch):
    from mgen_amd import Engine
    e = Engine(0, diag=True)
    yield e
    e.close()


@functools.lru_cache(maxsize=4)
def records(n_flows, n, kind):
    """n records with unique, increasing receive times 100-ish us apart; flow indices by kind:
    u uniform; first / last: one flow; absent: each tile (of either size) draws from a third
    of the flows; junk: 10 % with an index >= n_flows or 0xFFFFFFFF; skipped: all of them."""
    rng = np.random.default_rng(n_flows * 1000003 + n)
    if kind == "first":
        idx = np.zeros(n, np.int64)
    elif kind == "last":
        idx = np.full(n, n_flows - 1, np.int64)
    elif kind == "absent":
        third = (np.arange(n) // 13824) % 3               # 13824 = 3 x 4608: whole tiles
        idx = (rng.integers(0, n_flows, n) // 3 * 3 + third) % n_flows
    else:
        idx = rng.integers(0, n_flows, n)
    if kind in ("junk", "skipped"):
        bad = rng.random(n) < (0.1 if kind == "junk" else 2.0)
        idx[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0xFFFFFFFF,
                            n_flows + rng.integers(0, 9, int(bad.sum())))
    o = np.argsort(idx, kind="stable")                    # per-flow sequence numbers: 1, 2, ..
    start = np.flatnonzero(np.r_[True, np.diff(idx[o]) != 0])
    seq = np.empty(n, np.int64)
    seq[o] = np.arange(n) - np.repeat(start, np.diff(np.r_[start, n])) + 1
    seq += rng.integers(0, 2, n)                          # (a few duplicates and losses)
    rx = T0 * M + np.cumsum(rng.integers(60, 140, n))
    tx = rx - rng.integers(50, 500, n)
    d = {"idx": idx.astype(np.uint32), "seq": seq.astype(np.uint32),
         "tx_sec": (tx // M).astype(np.uint32), "tx_usec": (tx % M).astype(np.uint32),
         "msg_len": np.full(n, 200, np.uint16), "rx_sec": (rx // M).astype(np.uint32),
         "rx_usec": (rx % M).astype(np.uint32)}
    from oracle import oracle as O
    of, orep, ocnt = O.flow_reduce_batch(n_flows, d["idx"], d["seq"], d["tx_sec"], d["tx_usec"],
                                         d["msg_len"], d["rx_sec"], d["rx_usec"], window=WINDOW,
                                         per_flow=PER_FLOW)
    want_rec = np.full((n_flows, PER_FLOW), FILL * 0x01010101, np.uint32)
    for f in range(n_flows):
        k = min(int(ocnt[f]), PER_FLOW)
        t = orep[f, :k]["rx_sec"] * M + orep[f, :k]["rx_usec"]
        i = np.searchsorted(rx, t)
        assert (rx[i] == t).all() and (idx[i] == f).all()
        want_rec[f, :k] = i
    return d, (of, orep, ocnt), want_rec


def upload(torch, d):
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def run(torch, e, n_flows, t):
    """One mgenx_flow_reduce_ex call on fresh state (t: upload()'s columns): the raw bytes of
    state, reports, counts and report_rec (report buffers pre-filled with FILL)."""
    flows = e.flow_init(n_flows, WINDOW)
    reports = torch.full((n_flows * PER_FLOW * 96,), FILL, dtype=torch.uint8, device="cuda")
    rrec = torch.full((n_flows * PER_FLOW * 4,), FILL, dtype=torch.uint8, device="cuda")
    count = torch.zeros(n_flows, dtype=torch.int32, device="cuda")
    e.flow_reduce(flows, n_flows, t["idx"], t["seq"], t["tx_sec"], t["tx_usec"], t["msg_len"],
                  t["rx_sec"], t["rx_usec"], reports=reports, per_flow=PER_FLOW,
                  report_count=count, report_rec=rrec)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (flows, reports, count, rrec)]


def check(out, n_flows, ref, want_rec):
    from mgen_amd import FLOW_REPORT_DTYPE, FLOW_STATE_DTYPE
    st = out[0].view(FLOW_STATE_DTYPE)
    rep = out[1].view(FLOW_REPORT_DTYPE).reshape(n_flows, PER_FLOW)
    rrec = out[3].view(np.uint32).reshape(n_flows, PER_FLOW)
    C.compare(st, rep, out[2].view(np.uint32), *ref, PER_FLOW, rrec)
    assert np.array_equal(rrec, want_rec)


PATHS = {"scan1": {"MGENX_AN_SCAN1": "1"}, "three": {"MGENX_AN_SCAN1": "0"},
         "radix": {"MGENX_AN_RADIX": "1"}}
ENV = ("MGENX_AN_SCAN1", "MGENX_AN_RADIX", "MGENX_AN_TILE", "MGENX_AN_C1_GIVEUP",
       "MGENX_AN_C1_WRAP")

# (n_flows, tiles, records past the last full tile, kind, the tile size the counts refer to)
SHAPES = [
    (1, 1, 0, "u", TILE), (1, 2, -1, "first", TILE), (15, 1, 1, "u", TILE),
    (15, 33, 0, "last", TILE), (16, 2, 0, "u", TILE), (16, 129, 0, "u", TILE),
    (17, 15, -1, "u", TILE), (17, 16, 0, "absent", TILE), (17, 17, 1, "u", TILE),
    (17, 64, 0, "skipped", TILE), (255, 2, 0, "absent", TILE), (255, 17, 0, "junk", TILE),
    (255, 129, -1, "first", TILE), (256, 16, 1, "u", TILE), (256, 65, -1, "u", TILE),
    (257, 17, -1, "absent", TILE), (257, 33, 0, "u", TILE), (1222, 1, -1, "u", TILE),
    (1222, 17, 1, "junk", TILE), (1222, 64, 0, "u", TILE), (1222, 65, 1, "absent", TILE),
    (1535, 1, 0, "u", TILE), (1535, 2, 1, "last", TILE), (1535, 15, -1, "junk", TILE),
    (1535, 16, 1, "skipped", TILE), (1535, 17, 0, "first", TILE),
    (1535, 33, 1, "absent", TILE), (1535, 64, -1, "u", TILE), (1535, 65, 0, "last", TILE),
    (1535, 129, 1, "junk", TILE),
    (1, 1, 0, "u", TILE_BIG), (16, 33, -1, "last", TILE_BIG), (17, 17, 1, "u", TILE_BIG),
    (255, 129, 0, "u", TILE_BIG), (257, 16, -1, "absent", TILE_BIG),
    (1222, 2, 0, "first", TILE_BIG), (1222, 17, 0, "junk", TILE_BIG),
    (1222, 65, 1, "u", TILE_BIG),
]


@pytest.mark.parametrize("n_flows,tiles,past,kind,tile", SHAPES)
def test_flow_order_paths_agree(torch, eng, eng_diag, monkeypatch, n_flows, tiles, past, kind,
                                tile):
    n = tiles * tile + past
    d, ref, want_rec = records(n_flows, n, kind)
    d = upload(torch, d)
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    outs = {"product": run(torch, eng, n_flows, d)}
    sizes = (TILE, TILE_BIG) if n_flows <= BIG_MAX_FLOWS else (TILE,)
    for name, env in PATHS.items():
        for ts in sizes if name != "radix" else (None,):
            for v in ENV:
                monkeypatch.delenv(v, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            if ts:
                monkeypatch.setenv("MGENX_AN_TILE", str(ts))
            outs[f"{name}-{ts}"] = run(torch, eng_diag, n_flows, d)
    for name, out in outs.items():
        for a, b in zip(out, outs["product"]):
            assert np.array_equal(a, b), name
    check(outs["product"], n_flows, ref, want_rec)
    assert (ref[2] > 0).any() or kind == "skipped"          # windows closed


def giveups(e):
    v = ctypes.c_uint64(0)
    assert e.lib.mgenx_diag_c1_giveups(ctypes.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("n_flows", [17, 257, 1535])
@pytest.mark.parametrize("tiles", [1, 17, 129])
def test_single_pass_scan_give_up_branch(torch, eng_diag, monkeypatch, n_flows, tiles):
    """Blocks whose look-back gives up (forced: every block, every second, every seventh) sum
    the histogram themselves: the results equal the unforced run's and the oracle's, and the
    counter shows exactly the forced blocks took the branch."""
    d, ref, want_rec = records(n_flows, tiles * TILE + 1, "junk")
    d = upload(torch, d)
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("MGENX_AN_SCAN1", "1")
    monkeypatch.setenv("MGENX_AN_TILE", str(TILE))
    giveups(eng_diag)                                       # (clears the count)
    plain = run(torch, eng_diag, n_flows, d)
    assert giveups(eng_diag) == 0
    check(plain, n_flows, ref, want_rec)
    blocks = (n_flows + 1 + 15) // 16
    for m in (1, 2, 7):
        monkeypatch.setenv("MGENX_AN_C1_GIVEUP", str(m))
        out = run(torch, eng_diag, n_flows, d)
        assert giveups(eng_diag) == sum(1 for j in range(1, blocks) if j % m == m - 1), m
        for a, b in zip(out, plain):
            assert np.array_equal(a, b), m


def test_single_pass_scan_epoch_wrap(torch, monkeypatch):
    """A context whose scan epochs start two below the wrap: four consecutive calls (the third
    restarts the epochs from cleared words; the second and third with forced give-ups), each
    equal to the oracle."""
    from mgen_amd import Engine
    n_flows = 257
    d, ref, want_rec = records(n_flows, 17 * TILE + 1, "junk")
    d = upload(torch, d)
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("MGENX_AN_SCAN1", "1")
    monkeypatch.setenv("MGENX_AN_C1_WRAP", "1")
    e = Engine(0, diag=True)
    try:
        giveups(e)
        for call in range(4):
            if call in (1, 2):
                monkeypatch.setenv("MGENX_AN_C1_GIVEUP", "2")
            else:
                monkeypatch.delenv("MGENX_AN_C1_GIVEUP", raising=False)
            check(run(torch, e, n_flows, d), n_flows, ref, want_rec)
            assert giveups(e) == (8 if call in (1, 2) else 0), call
    finally:
        e.close()
