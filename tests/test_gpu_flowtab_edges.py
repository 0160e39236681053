"""GPU: mgenx_flow_lookup / mgenx_flow_keys at their edges, both code paths -- small: a table
of 2048 flows (4096 slots, keys staged in LDS); large: 4096 flows (8192 slots, the smallest
table probed in HBM) -- against the first-seen model of flowtab_ref.  Every comparison is
exact: array_equal on the uint32 indices, == on the flow count.  The inputs come from
flowtab_cases, whose preconditions test_flowtab_ref_cpu.py asserts from the model alone."""
import contextlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flowtab_cases as C  # noqa: E402
import flowtab_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = R.FLOW_NONE
PATHS = pytest.mark.parametrize("max_flows", [C.SMALL, C.LARGE], ids=["small", "large"])


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


def upload(torch, b, rows=False):
    """(cols, src) on the device: one upload per column; rows: the 32-B mgenx_rec rows carry
    the key fields and err, with the dst_addr column beside them"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    src = t(b["src"].reshape(-1))
    if not rows:
        return {"dst_addr": t(b["dst_addr"].reshape(-1)), "dst_len": t(b["dst_len"]),
                "dst_port": t(b["dst_port"].view(np.int16)),
                "flow_id": t(b["flow_id"].view(np.int32)), "err": t(b["err"])}, src
    from mgen_amd import REC_DTYPE
    n = len(b["err"])
    r = np.zeros(n, REC_DTYPE)
    r["flow_id"], r["dst_port"], r["err"], r["dst_len"] = (b["flow_id"], b["dst_port"], b["err"],
                                                           b["dst_len"])
    r["dst_addr4"] = np.ascontiguousarray(b["dst_addr"][:, :4]).view("<u4")[:, 0]
    r["dst_type"] = np.where(b["dst_len"] == 4, 1, 2)
    rng = np.random.default_rng(n)                   # not part of the key
    r["seq_num"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    r["msg_len"], r["flags"] = rng.integers(0, 2**16, n), rng.integers(0, 256, n)
    return {"rows": t(r.view(np.uint8)), "dst_addr": t(b["dst_addr"].reshape(-1))}, src


@contextlib.contextmanager
def table_of(eng, max_flows):
    t = eng.flow_table(max_flows)
    try:
        yield t
    finally:
        eng.flow_table_destroy(t)


def lookup(torch, eng, table, b, rows=False):
    cols, src = upload(torch, b, rows)
    idx, nf = eng.flow_lookup(table, cols, src, len(b["err"]))
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint32), int(nf.cpu()[0])


def check_calls(torch, eng, table, calls, want, rows=False):
    for c, (b, (widx, wcnt)) in enumerate(zip(calls, want)):
        idx, cnt = lookup(torch, eng, table, b, rows)
        bad = np.flatnonzero(idx != widx)
        assert bad.size == 0, (c, bad.size, bad[:8], idx[bad[:8]], widx[bad[:8]])
        assert np.array_equal(idx, widx)
        assert cnt == wcnt, (c, cnt, wcnt)


def check_bounded(idx, k, idx2, k2, key, bound):
    """More keys than the table takes, in one call.  Which keys are held depends on timing (a
    soft bound), so properties only: at least `bound` are; the held indices are exactly
    0 .. k-1, one per held key, on every held record of it, in the order of the keys' first
    held records; and a second, identical call (idx2, k2) returns the same."""
    held = idx != NONE
    assert bound <= k <= len(set(key.tolist()))
    assert np.array_equal(np.unique(idx[held]), np.arange(k))
    pairs = np.unique(np.stack([key[held], idx[held].astype(np.int64)]), axis=1)
    assert pairs.shape[1] == k                       # key <-> index, one to one
    assert len(set(pairs[0].tolist())) == k
    _, first = np.unique(idx[held], return_index=True)
    assert np.all(np.diff(first) > 0)                # numbered in first-record order
    assert k2 == k
    assert np.array_equal(idx2, idx)


@PATHS
@pytest.mark.parametrize("form", ["cols", "rows"])
@pytest.mark.parametrize("n", C.SWEEP_N)
def test_batch_size_sweep(torch, eng, max_flows, form, n):
    """a: n records, each its own key on a fresh table (K == n; n = 4096 fills the large
    table to its bound exactly): arange(n) and n; then the same batch again, no new key.
    The small table takes 2048 keys, so n = 2049 and 4096 pass its bound in one call: there
    the properties of a bounded table hold instead (check_bounded)."""
    calls = C.sweep(n)
    with table_of(eng, max_flows) as t:
        if n <= max_flows:
            want = [(np.arange(n, dtype=np.uint32), n)] * 2
            check_calls(torch, eng, t, calls, want, rows=form == "rows")
        else:
            (idx, k), (idx2, k2) = (lookup(torch, eng, t, b, form == "rows") for b in calls)
            check_bounded(idx, k, idx2, k2, np.arange(n), max_flows)


@PATHS
def test_call_sequences(torch, eng, max_flows):
    """b: new keys / known keys only / every record in error / more new keys / known keys
    only, on one table (the new-key count alternates between two words, each call clearing
    the other); a fresh table whose first call is all-error; and an empty batch (n == 0),
    which reports the table's count -- 0 on a fresh table."""
    main, fresh = C.sequence()
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    with table_of(eng, max_flows) as t:
        _, nf = eng.flow_lookup(t, {}, empty, 0,
                                n_flows=torch.full((1,), -1, dtype=torch.int32, device="cuda"))
        assert int(nf.cpu()[0]) == 0
        want = C.model(main)
        check_calls(torch, eng, t, main, want)
        _, nf = eng.flow_lookup(t, {}, empty, 0)
        assert int(nf.cpu()[0]) == want[-1][1] > 0
        check_calls(torch, eng, t, main[1:2], want[4:5])    # and the empty call changed nothing
    with table_of(eng, max_flows) as t:
        check_calls(torch, eng, t, fresh, C.model(fresh))


@pytest.mark.parametrize("args", C.CONTENTION, ids=lambda a: f"{a[0]}-{a[3]}")
def test_first_record_order_under_contention(torch, eng, args):
    """c: a hot key on most of the records, first seen at 4000/8192 of the batch, and keys of
    two or three records laid out against lane, wave and chunk order: numbered by first
    record.  8192 records on both paths.  The large path's insert kernel runs one record per
    thread, all 8192 at once: a lower record that reaches its key's slot only after a higher
    one has published it -- what the atomicMin of the plain-load path is for -- takes a batch
    of more records than the device runs threads at once, the third size (measured: without
    that atomicMin 8192, 65,536 and 262,144 records stay exact, 1,048,576 do not)."""
    n, n_wave, n_spread, max_flows = args
    calls = C.contention(n, n_wave, n_spread)[0]
    with table_of(eng, max_flows) as t:
        check_calls(torch, eng, t, calls, C.model(calls))


@PATHS
def test_padding_and_near_identical_keys(torch, eng, max_flows):
    """d and k: copies of a record that differ only past the address lengths or in the source
    type byte share an index; records that differ in one key field do not.  Then
    mgenx_flow_keys over that table: field by field the model's keys in index order (zero
    past the length, type 1 / 2 / 0 by length), and with cap below the flow count only the
    first cap keys, the rest of the buffer untouched."""
    from mgen_amd import REPORT_KEY_DTYPE
    calls, _, m = C.families()
    model = R.FirstSeen()
    want = [model.lookup(R.batch_keys(b), b["err"]) for b in calls]
    with table_of(eng, max_flows) as t:
        check_calls(torch, eng, t, calls, want)
        nf = want[-1][1]
        assert nf == m
        k = model.keys_in_order()
        ref = np.zeros(nf, REPORT_KEY_DTYPE)
        for side, o in (("dst", 0), ("src", 20)):
            ref[side]["len"] = k[:, o + 1]
            ref[side]["type"] = np.where(k[:, o + 1] == 4, 1, np.where(k[:, o + 1] == 16, 2, 0))
            ref[side]["port"] = np.ascontiguousarray(k[:, o + 2:o + 4]).view("<u2")[:, 0]
            ref[side]["addr"] = k[:, o + 4:o + 20]
        ref["flow_id"] = np.ascontiguousarray(k[:, 40:44]).view("<u4")[:, 0]
        for protocol in (1, 2):
            ref["protocol"] = protocol
            got = eng.flow_keys(t, nf, protocol).cpu().numpy().view(REPORT_KEY_DTYPE)
            for f in ("len", "type", "port", "addr"):
                assert np.array_equal(got["dst"][f], ref["dst"][f]), f
                assert np.array_equal(got["src"][f], ref["src"][f]), f
            assert np.array_equal(got["flow_id"], ref["flow_id"])
            assert np.all(got["protocol"] == protocol) and not got["rsv"].any()
            assert got.tobytes() == ref.tobytes()
        cap = nf - 5
        buf = torch.full((nf * REPORT_KEY_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        got = eng.flow_keys(t, cap, 2, keys=buf).cpu().numpy()
        assert got[:cap * 48].tobytes() == ref[:cap].tobytes()
        assert np.all(got[cap * 48:] == 0xA5)


def test_small_path_past_the_staged_range(torch, eng):
    """e: 2,000 keys on the small table, whose LDS copy holds indices below 1536; then 20,000
    records over all of them (indices 1535 and 1536 among them) and 30 new keys; and again."""
    calls = C.past_staged()
    with table_of(eng, C.SMALL) as t:
        check_calls(torch, eng, t, calls, C.model(calls))


def test_large_path_above_1m_records(torch, eng):
    """f: 1,100,000 records on a table of 65,536 flows: 1075 chunks of 1024, so the chunk
    scan carries into a second pass and the first / number kernels loop over their grid;
    20,000 keys first seen all along the batch, then 500 more first seen at its end."""
    t0 = time.perf_counter()
    calls = C.above_1m()
    want = C.model(calls)
    t1 = time.perf_counter()
    with table_of(eng, C.F_FLOWS) as t:
        check_calls(torch, eng, t, calls, want)
    print(f"above_1m: inputs and model {t1 - t0:.2f} s, device and compare "
          f"{time.perf_counter() - t1:.2f} s")
    assert want[0][1] == C.F_KEYS and want[1][1] == C.F_KEYS + 500


@PATHS
def test_key_bound_two_calls(torch, eng, max_flows):
    """g: exactly max_flows distinct keys are all admitted (each creator reads fewer held);
    1,000 further keys in the next call are all refused, the held ones keep their indices and
    the count stays: FirstSeen(max_keys = the bound)."""
    calls = C.bound(max_flows)
    with table_of(eng, max_flows) as t:
        check_calls(torch, eng, t, calls, C.model(calls, max_keys=max_flows))


def test_key_bound_one_call(torch, eng):
    """h: 60,000 records over 6,000 keys in one call on the table of 4096 flows: the
    properties of a bounded table (check_bounded)."""
    calls, key = C.overflow()
    with table_of(eng, C.LARGE) as t:
        idx, k = lookup(torch, eng, t, calls[0])
        idx2, k2 = lookup(torch, eng, t, calls[1])
    check_bounded(idx, k, idx2, k2, key, C.LARGE)


@PATHS
def test_cluster_across_the_last_slot(torch, eng, max_flows):
    """i: 300 keys whose home is the last slot wrap to slot 0 and beyond, among 500 ordinary
    keys; then everything again with 50 more keys of the cluster."""
    calls, _ = C.wrap(2 * max_flows)
    with table_of(eng, max_flows) as t:
        check_calls(torch, eng, t, calls, C.model(calls))


def test_probe_limit_small_path(torch, eng):
    """j: 1,024 keys with home 4095 fit inside the 1,024-slot probe limit in any order; 76
    more keys of that home then find no room within it and map to MGENX_FLOW_NONE (mgenx.h: a
    key past the probe limit), while the 1,024 keep their indices and the count stays.  For
    this input that is FirstSeen(max_keys=1024)."""
    calls, _ = C.probe_limit()
    with table_of(eng, C.SMALL) as t:
        check_calls(torch, eng, t, calls, C.model(calls, max_keys=C.MAX_PROBE))


def test_hash_pin(torch, eng_diag, monkeypatch):
    """flowtab_ref.slot_hash, which chooses the cluster cases' inputs, against the device:
    with MGENX_FT_MODE=1 the diagnostics build's probe kernel writes each record's home slot
    to flow_idx and touches no table.  A table of 4096 slots shows the hash's low 12 bits;
    the large path's cluster cases also rely on bit 12, which this cannot check."""
    b = C.hash_pin()
    monkeypatch.setenv("MGENX_FT_MODE", "1")
    with table_of(eng_diag, C.SMALL) as t:
        idx, cnt = lookup(torch, eng_diag, t, b)
    assert cnt == 0
    assert np.array_equal(idx, R.slot_hash(R.batch_keys(b)) & 4095)
