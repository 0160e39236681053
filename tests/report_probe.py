"""Probe values for the numeric half of the REPORT path (test infrastructure): doubles for
the "%lf" formatter, doubles at and around the quantizers' thresholds, and received report
items of every rate / loss code.  Thresholds are bisected over double bit patterns against
the oracle (host libm), never read from the engine."""
import ctypes
import ctypes.util
import math
import socket

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
DENORM_MIN = 5e-324
NAN_BITS = 0x7FF8000000000000


def bits(v):
    return int(np.float64(v).view(np.uint64))


def from_bits(b):
    return float(np.uint64(b).view(np.float64))


def step(v, k):
    """The double k places after (k < 0: before) the non-negative finite v."""
    b = bits(v) + k
    assert 0 <= b <= bits(DBL_MAX), (v, k)
    return from_bits(b)


def around(v, r=4):
    """v and the r doubles on each side of it that exist (non-negative, finite)."""
    b = bits(v)
    return [from_bits(x) for x in range(max(0, b - r), min(bits(DBL_MAX), b + r) + 1)]


def first_true(lo, hi, pred):
    """Smallest double in [lo, hi] (0 <= lo <= hi) with pred; pred goes false -> true once."""
    a, b = bits(lo), bits(hi)
    while a < b:
        m = (a + b) // 2
        if pred(from_bits(m)):
            b = m
        else:
            a = m + 1
    return from_bits(a)


# ---------------------------------------------------------------- "%lf"
def f6_values():
    """Non-negative doubles for the six-decimal formatter, +inf and +nan last (the tests use
    every one with both signs)."""
    rng = np.random.default_rng(0xF6)
    out = []
    for ex in range(2047):                                   # every biased exponent
        for frac in (0, 1, (1 << 52) - 1, 1 << 51, int(rng.integers(0, 1 << 52))):
            out.append(from_bits(ex << 52 | frac))
    out += [j / 128 for j in range(1, 4000, 2)]              # v * 1e6 ends in .5 exactly
    for v in (0.9999995, 9.9999995, 99999.9999995, 0.0000005, 1.5e-6, 2.5e-6,
              float(2 ** 53 - 1), 2.0 ** 63, 2.0 ** 64, 1e22, 1e23):
        out += [step(v, -1), v, step(v, 1)]
    out += [math.inf, from_bits(NAN_BITS)]
    return np.array(out, np.float64)


def f6_signed():
    v = f6_values()
    return np.concatenate([v, (v.view(np.uint64) | np.uint64(1 << 63)).view(np.float64)])


TS_SEC = (0, 86399, 86400, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
TS_USEC = (0, 999999)
F6_FIELDS = ("duration", "rate", "loss", "latency_ave", "latency_min", "latency_max")


def f6_rows():
    """(values [rows x 6] in F6_FIELDS order, msg_count, rx_sec, rx_usec): every signed probe
    in turn, then one row per non-finite value with all six fields set to it."""
    s = f6_signed()
    special = s[~np.isfinite(s)]
    pad = (-len(s)) % 6
    vals = np.concatenate([s, np.zeros(pad)]).reshape(-1, 6)
    vals = np.concatenate([vals, np.repeat(special[:, None], 6, axis=1)])
    n = len(vals)
    i = np.arange(n)
    sec = np.array(TS_SEC, np.int64)[i % len(TS_SEC)]
    usec = np.array(TS_USEC, np.int64)[(i // len(TS_SEC)) % len(TS_USEC)]
    count = (i.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 40)
    return vals, count, sec, usec


def pct_f(v):
    """CPython's correctly rounded "%f"."""
    return "%f" % float(v)


# ---------------------------------------------------------------- time quantizer
def time_thresholds(O):
    """T[k], k = 2..255: the first double with O.q_time >= k."""
    return {k: first_true(1e-6, 660.0, lambda v, k=k: O.q_time(v) >= k) for k in range(2, 256)}


def time_probes(O, thr=None):
    thr = thr or time_thresholds(O)
    out = [0.0, -0.0, -1e-9, -3.0, -math.inf, math.inf, DENORM_MIN, DBL_MAX, 700.0]
    for v in (5e-7, 1e-6, 660.0, 1.1 * 600.0):
        out += around(v, 2)
    for k, t in thr.items():
        out += around(t, 4)
        out.append(O.uq_time(k))
    out += [O.uq_time(0), O.uq_time(1)]
    return np.array(out, np.float64)


def latency_plan(t):
    """(ave, min, max) triples from the time probes t: |ave - min| = |max - ave| = |x| exactly
    with ave = 0, then ave = +x and ave = -x with min = max = 0."""
    z = np.zeros(len(t))
    a = np.stack([z, -t, t], axis=1)
    b = np.stack([t, z, z], axis=1)
    c = np.stack([-t, z, z], axis=1)
    return np.concatenate([a, b, c])


# ---------------------------------------------------------------- rate quantizer
_libm = None


def libm_log10(v):
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.log10.argtypes, _libm.log10.restype = [ctypes.c_double], ctypes.c_double
    return _libm.log10(v)


def rate_exponent(v):
    """(int)log10(v) as the reference computes it: host libm, truncated toward zero."""
    return int(libm_log10(v))


LOG10_E = range(-323, 309)


def log10_thresholds():
    """e -> the first positive double with (int)log10 >= e, e = -323..308."""
    return {e: first_true(DENORM_MIN, DBL_MAX, lambda v, e=e: rate_exponent(v) >= e)
            for e in LOG10_E}


def rate_probes(thr=None):
    thr = thr or log10_thresholds()
    out = [DENORM_MIN, DBL_MAX, 0.0, -0.0, -3.0]
    for t in thr.values():
        out += around(t, 4)
    for e in (-2, 0, 3, 9):
        p = 10.0 ** e
        for m in range(4096):                                # 409.6 * x + 0.5 crosses m + 1
            v = (m + 0.5) / 409.6 * p
            out += [step(v, -1), v, step(v, 1)]
        out += around(10.0 * p, 4)                           # mantissa 4096: the code wraps
        out += [9.995 * p, 9.9988 * p, 9.999 * p]
    return np.array(out, np.float64)


# ---------------------------------------------------------------- loss quantizer
LOSS_NAMED = (0.0, DENORM_MIN, 1.0, float(np.nextafter(1.0, 2.0)), 1.2, math.inf)


def loss_probes():
    """The named values first, then (m + 0.5) / 65535 and its two neighbours for every m."""
    v = (np.arange(65536, dtype=np.float64) + 0.5) / 65535.0
    tri = np.stack([np.nextafter(v, 0.0), v, np.nextafter(v, 2.0)], axis=1).reshape(-1)
    return np.concatenate([np.array(LOSS_NAMED, np.float64), tri])


def loss_code(loss):
    """QuantizeLoss in NumPy float64: one multiply, one add, one truncation."""
    loss = np.asarray(loss, np.float64)
    x = loss * 65535.0
    x = x + 0.5
    q = np.trunc(np.clip(x, 1.0, 65535.0)).astype(np.uint32)
    return np.where(loss == 0.0, 0, q).astype(np.uint16)


def quantizer_rows(O, t=None, r=None):
    """Rows [n x 7] (duration, lat_ave, lat_min, lat_max, rate, loss, offset = 0) that carry
    every time, rate and loss probe at least once."""
    t = time_probes(O) if t is None else t
    r = rate_probes() if r is None else r
    ls = loss_probes()
    lat = latency_plan(t)
    n = max(len(ls), len(r), len(lat))
    i = np.arange(n)
    rows = np.zeros((n, 7))
    rows[:, 0] = t[i % len(t)]
    rows[:, 1:4] = lat[i % len(lat)]
    rows[:, 4] = r[i % len(r)]
    rows[:, 5] = ls[i % len(ls)]
    return rows


# ---------------------------------------------------------------- received items
def v4_items(n=65536):
    """n 24-byte IPv4 report items, item i with rate code i and every other field a fixed
    function of i.  Returns (bytes [n x 24], rate codes, loss codes)."""
    i = np.arange(n, dtype=np.uint64)
    b = np.zeros((n, 24), np.uint8)
    b[:, 0] = (1 << 4) | (i % 4).astype(np.uint8)            # type 1, protocol 0..3
    b[:, 1] = 24
    field = (((i >> np.uint64(3)) & np.uint64(1)) << np.uint64(14)) | (i & np.uint64(0x1FFF))
    b[:, 2], b[:, 3] = field >> np.uint64(8), field & np.uint64(255)
    rng = np.random.default_rng(0x24)
    b[:, 4:16] = rng.integers(0, 256, (n, 12))               # dst, src, ports
    b[:, 16] = i & np.uint64(255)
    b[:, 17] = (i >> np.uint64(8)) & np.uint64(255)
    b[:, 18] = (i * np.uint64(7)) & np.uint64(255)
    b[:, 19] = (i * np.uint64(13)) & np.uint64(255)
    rate = (i & np.uint64(0xFFFF)).astype(np.uint16)
    loss = ((i * np.uint64(40503)) & np.uint64(0xFFFF)).astype(np.uint16)
    b[:, 20], b[:, 21] = rate >> 8, rate & 255
    b[:, 22], b[:, 23] = loss >> 8, loss & 255
    return b, rate, loss


V6_GROUP_VALUES = (1, 0xFFFF, 0x0ABC, 0x00F0, 0x100)


def v6_mask_addr(mask, salt):
    """16 address bytes: group g is non-zero iff bit g of mask, values from V6_GROUP_VALUES."""
    out = bytearray(16)
    for g in range(8):
        if mask >> g & 1:
            v = V6_GROUP_VALUES[(g + salt) % len(V6_GROUP_VALUES)]
            out[2 * g], out[2 * g + 1] = v >> 8, v & 255
    return bytes(out)


def _v6(text):
    return socket.inet_pton(socket.AF_INET6, text)


V6_NAMED = tuple(_v6(t) for t in (
    "::", "::1", "::ffff:192.168.0.1", "::ffff:0.0.0.0", "::ffff:255.255.255.255",
    "::10.1.2.3", "::0.1.0.0", "::255.255.255.255", "::ffff:0:0:1", "0:0:0:0:0:fffe:102:304",
    "1::", "1::1", "1:0:0:2:0:0:0:3", "1:0:0:0:2:0:0:3", "0:0:1:0:0:1:0:0"))


def v6_items():
    """(items, src, dst, reporter): for every zero / non-zero group mask a 48-byte and a
    52-byte (flow id) report item whose src, dst and the record's reporter each sweep all 256
    masks, then the named addresses in each of the three places."""
    trip = []
    for form in (0, 1):
        for m in range(256):
            trip.append((v6_mask_addr(m, m + form), v6_mask_addr((m * 37 + 11) & 255, m >> 3),
                         v6_mask_addr(m ^ 0x5A, form + (m >> 5)), form))
    k = len(V6_NAMED)
    for j, a in enumerate(V6_NAMED):
        trip.append((a, V6_NAMED[(j + 1) % k], V6_NAMED[(j + 2) % k], j & 1))
    items, rep = [], []
    for j, (s, d, r, form) in enumerate(trip):
        b = bytearray(52 if form else 48)
        b[0], b[1] = (2 << 4) | (1 + j % 3), len(b)
        field = (form << 13) | ((j >> 2 & 1) << 14) | (j * 29 & 0x1FFF)
        b[2], b[3] = field >> 8, field & 255
        b[4:20], b[20:36] = d, s
        b[36:38] = (5000 + j).to_bytes(2, "big")
        b[38:40] = (0xFFFF - j).to_bytes(2, "big")
        o = 40
        if form:
            b[40:44] = (0x01020304 * (j % 3) + j).to_bytes(4, "big")
            o = 44
        b[o:o + 4] = bytes([j & 255, (j * 3) & 255, (j * 5) & 255, (j * 11) & 255])
        b[o + 4:o + 6] = ((j * 127 + 16) & 0xFFFF).to_bytes(2, "big")
        b[o + 6:o + 8] = ((j * 509) & 0xFFFF).to_bytes(2, "big")
        items.append(bytes(b))
        rep.append(r)
    return items, [t[0] for t in trip], [t[1] for t in trip], rep
