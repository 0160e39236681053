"""GPU numerics of the REPORT path against two references that never touch the engine: the
oracle (the reference's formulas through host libm and glibc printf) and plain Python
("%f", socket.inet_ntop, float arithmetic).  Covered: put_f6 over the whole double range,
the time / rate / loss quantizers at and around every threshold, the unquantizers and the
received-report lines for every 16-bit rate and loss code, put_ipv6 and put_ts."""
import re
import socket
import time

import numpy as np
import pytest

import report_probe as P

pytestmark = pytest.mark.gpu


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy().view(np.uint8)).cuda()


def _v4_key(oracle, flow_id, n=1):
    from mgen_amd import REPORT_KEY_DTYPE
    s = np.zeros(1, oracle.ADDR_DTYPE)
    s["type"], s["len"], s["port"] = 1, 4, 63684
    s["addr"][0, :4] = [10, 0, 200, 1]
    d = s.copy()
    d["port"] = 5002
    d["addr"][0, :4] = [192, 168, 7, 255]
    k = np.zeros(n, REPORT_KEY_DTYPE)
    k["src"], k["dst"] = s[0], d[0]
    k["flow_id"], k["protocol"] = flow_id, 1
    return s, d, k


def _first_diff(got, exp, goff, eoff):
    """The first line that differs, for the assertion message."""
    for i in range(len(eoff) - 1):
        g, e = got[goff[i]:goff[i + 1]], exp[eoff[i]:eoff[i + 1]]
        if g != e:
            return i, g, e
    return None


VALUES = re.compile(rb"window>(\S+) rate>(\S+) kbps loss>(\S+) latency ave>(\S+) min>(\S+) "
                    rb"max>(\S+?)(?:, count>\d+)?\n")


def test_report_lines_print_any_double(torch, eng, oracle):
    """put_f6 and put_ts: REPORT lines whose six doubles are report_probe.f6_values() with
    both signs (every exponent, sixth-decimal ties, carries, inf, nan; the rate field prints
    rate * 8e-3), timestamps at the seconds / microseconds edges, both timestamp formats."""
    from mgen_amd import FLOW_REPORT_DTYPE
    O = oracle
    t0 = time.perf_counter()
    vals, count, sec, usec = P.f6_rows()
    n = len(vals)
    reps = np.zeros(n, FLOW_REPORT_DTYPE)
    reps["flow"] = np.arange(n)
    for c, name in enumerate(P.F6_FIELDS):
        reps[name] = vals[:, c]
    reps["msg_count"], reps["rx_sec"], reps["rx_usec"] = count, sec, usec
    # the items give the lines their key fields only: built from all-zero reports
    s, d, keys = _v4_key(O, 7, n)
    ones = dev(torch, np.ones(n, np.uint32))
    items, ilen = eng.report_build(dev(torch, np.zeros(n, FLOW_REPORT_DTYPE)), n, 1, ones,
                                   dev(torch, keys), dev(torch, np.zeros(n, np.uint8)))
    item, _ = O.report_build(s, d, 7, 1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    want_items = np.zeros((n, 52), np.uint8)
    want_items[:, :len(item)] = np.frombuffer(item, np.uint8)
    assert np.array_equal(items.cpu().numpy().reshape(n, 52), want_items)
    assert (ilen.cpu().numpy() == len(item)).all()
    expect_f = [[P.pct_f(v) if np.isfinite(v) else None for v in row]
                for row in np.column_stack([vals[:, 0], vals[:, 1] * 8e-3, vals[:, 2:]])]
    for opts in (0, 1):
        text, lo = eng.log_report_text(items, dev(torch, reps), n, 1, ones, opts=opts)
        got, lo = text.cpu().numpy().tobytes(), lo.cpu().numpy()
        exp, eo = O.log_report_batch(want_items, vals, count, sec, usec, opts)
        assert len(exp) > n * 220                       # the first pass overflowed its text_cap
        assert got == exp, _first_diff(got, exp, lo, eo)
        assert np.array_equal(lo, eo) and int(lo[-1]) == len(got)
        nums = VALUES.findall(got)
        assert len(nums) == n
        for i, (line, want) in enumerate(zip(nums, expect_f)):
            for g, w in zip(line, want):
                assert w is None or g.decode() == w, (i, g, w)
    print(f"f6: {vals.size} doubles in {n} rows x 2 formats, {time.perf_counter() - t0:.2f} s")


def test_report_build_at_quantizer_thresholds(torch, eng, oracle):
    """mgenx_report_build, one flow per probe: QuantizeTimeValue at the first double of every
    code 2..255 and 4 ulp around it (as duration, as |ave - min| / |max - ave|, as |ave|),
    the rate exponent at the first double of every decade e = -323..308 and 4 ulp around it,
    the rate mantissa where 409.6 * x + 0.5 crosses an integer, and the loss at every
    (m + 0.5) / 65535 with both neighbours.  Left out because the reference's double -> int
    conversion is undefined there: nan into any quantizer, +-inf into the rate."""
    from mgen_amd import FLOW_REPORT_DTYPE
    O = oracle
    t0 = time.perf_counter()
    tp, rp = P.time_probes(O), P.rate_probes()
    rows = P.quantizer_rows(O, tp, rp)
    n = len(rows)
    assert not np.isnan(rows).any() and np.isfinite(rows[:, 4]).all()
    s, d, keys = _v4_key(O, 1, n)
    want, wlen = O.report_build_batch(s, d, 1, 1, rows)
    assert (wlen == 24).all()
    # the loss code again, from NumPy alone; the oracle's scalar entry on a sample
    wloss = P.loss_code(rows[:, 5])
    assert np.array_equal(want[:, 22].astype(np.uint16) << 8 | want[:, 23], wloss)
    for i in list(range(len(P.LOSS_NAMED))) + list(range(0, n, 64)):
        assert O.q_loss(rows[i, 5]) == wloss[i], (i, rows[i, 5])
    assert set(wloss.tolist()) == set(range(65536))
    for col in (16, 17, 18, 19):
        assert set(want[:, col].tolist()) == set(range(256)), col   # every time code is reached
    reps = np.zeros(n, FLOW_REPORT_DTYPE)
    reps["flow"] = np.arange(n)
    reps["duration"], reps["latency_ave"] = rows[:, 0], rows[:, 1]
    reps["latency_min"], reps["latency_max"] = rows[:, 2], rows[:, 3]
    reps["rate"], reps["loss"] = rows[:, 4], rows[:, 5]
    sign = dev(torch, np.zeros(n, np.uint8))
    items, ilen = eng.report_build(dev(torch, reps), n, 1, dev(torch, np.ones(n, np.uint32)),
                                   dev(torch, keys), sign)
    got = items.cpu().numpy().reshape(n, 52)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} items differ\n" + "\n".join(
        f"flow {i}: {[float.hex(x) for x in rows[i, :6]]} got {got[i, 16:24].tobytes().hex()} "
        f"want {want[i, 16:24].tobytes().hex()}" for i in bad[:12])
    assert (ilen.cpu().numpy() == 24).all()
    assert np.array_equal(sign.cpu().numpy() != 0, rows[:, 1] < 0.0)
    print(f"quantizers: {len(tp)} time, {len(rp)} rate, {len(P.loss_probes())} loss probes in "
          f"{n} flows, {time.perf_counter() - t0:.2f} s")


ADDRS = re.compile(rb" src>([0-9a-f:.]+)/\d+ dst>([0-9a-f:.]+)/\d+ reporter>([0-9a-f:.]+)/\d+ ")


def test_report_recv_lines_all_codes(torch, eng, oracle):
    """Report::Log of received items: every 16-bit rate code and loss code, every time code in
    each of its four fields, offset fields of 256 and more (the reference truncates them to 8
    bits), the sign flag, and IPv6 addresses of every zero-run shape in src, dst and reporter."""
    from mgen_amd import to_device
    O = oracle
    t0 = time.perf_counter()
    v4, rate_q, loss_q = P.v4_items()
    v6, v6_src, v6_dst, v6_rep = P.v6_items()
    n4, n6 = len(v4), len(v6)
    n = n4 + n6
    slab_np = np.frombuffer(v4.tobytes() + b"".join(v6) + bytes(64), np.uint8)
    offs = np.concatenate([np.arange(n4) * 24,
                           n4 * 24 + np.cumsum([0] + [len(b) for b in v6[:-1]])]).astype(np.int64)
    pairs = np.stack([np.arange(n, dtype=np.int64), offs], axis=1)
    rng = np.random.default_rng(0x4EC)
    reporter = np.zeros(n, O.ADDR_DTYPE)
    reporter["type"][:n4], reporter["len"][:n4] = 1, 4
    reporter["addr"][:n4, :4] = rng.integers(0, 256, (n4, 4))
    reporter["type"][n4:], reporter["len"][n4:] = 2, 16
    reporter["addr"][n4:] = np.frombuffer(b"".join(v6_rep), np.uint8).reshape(n6, 16)
    reporter["port"] = rng.integers(0, 65536, n)
    rx_sec = np.array(P.TS_SEC, np.uint32)[np.arange(n) % len(P.TS_SEC)]
    rx_usec = rng.integers(0, 1_000_000, n).astype(np.uint32)
    slab = to_device(slab_np).view(torch.uint8)
    d_pairs = torch.from_numpy(pairs.reshape(-1)).cuda()
    d_rep, d_sec, d_usec = to_device(reporter.view(np.uint8)), to_device(rx_sec), to_device(rx_usec)
    # the independent expectations: Python float arithmetic, CPython "%f", inet_ntop
    want_rate = [P.pct_f(((q >> 4) * (10 / 4096) * 10.0 ** (q & 15)) * 8e-3)
                 for q in rate_q.tolist()]
    want_loss = [P.pct_f(q / 65535) for q in loss_q.tolist()]
    assert set(rate_q.tolist()) == set(loss_q.tolist()) == set(range(65536))
    ntop = [tuple(socket.inet_ntop(socket.AF_INET6, a).encode() for a in t)
            for t in zip(v6_src, v6_dst, v6_rep)]
    for opts in (0, 1):
        text, lo = eng.log_report_recv_text(slab, d_pairs, n, d_rep, d_sec, d_usec, opts=opts)
        got, lo = text.cpu().numpy().tobytes(), lo.cpu().numpy()
        exp, eo = O.log_report_recv_batch(slab_np, pairs, reporter, rx_sec, rx_usec, opts)
        assert got == exp, _first_diff(got, exp, lo, eo)          # per item, byte for byte
        assert np.array_equal(lo, eo) and int(lo[-1]) == len(got)
        nums = VALUES.findall(got)
        assert len(nums) == n
        for i in range(n4):
            assert nums[i][1].decode() == want_rate[i], (i, nums[i][1], want_rate[i])
            assert nums[i][2].decode() == want_loss[i], (i, nums[i][2], want_loss[i])
        adr = ADDRS.findall(got[lo[n4]:])
        assert adr == ntop, next((i, a, b) for i, (a, b) in enumerate(zip(adr, ntop)) if a != b)
    print(f"recv: {n4} IPv4 + {n6} IPv6 items x 2 formats, {time.perf_counter() - t0:.2f} s")
