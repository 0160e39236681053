"""A first-seen model of mgenx_flow_lookup (MgenAnalyticTable::FindFlow for batches,
mgenAnalytic.cpp:312-328), NumPy only: the canonical key of a record, the dense index every
record must get (new keys numbered in the order of their first record), and a restatement of
the device's slot hash that the tests use to *choose* inputs (clusters of keys with one home
slot).

A batch is a dict of column arrays, the ones the device takes:
    dst_addr (n, 16) uint8, dst_len (n,) uint8, dst_port (n,) uint16, src (n, 20) uint8
    (mgenx_addr: type, len, port, 16 address bytes), flow_id (n,) uint32, err (n,) uint8.
"""
import numpy as np

FLOW_NONE = 0xFFFFFFFF
KEY_BYTES = 44
_M32 = np.uint64(0xFFFFFFFF)


def key_bytes(dst_addr, dst_len, dst_port, src20, flow_id):
    """(n, 44) uint8 canonical keys: for the destination a zero byte, the length, the port
    (little endian) and the 16 address bytes with the bytes at and past the length zeroed; the
    same 20 bytes for the source, taken from the 20-byte mgenx_addr; then the flow id (little
    endian).  The source *type* byte is not part of the key (the zero byte stands in its
    place), as in MgenAnalyticTable::FindFlow (mgenAnalytic.cpp:312-328), which keys on
    addresses, ports and the flow id alone.

    The key carries the two address lengths.  The reference's key is the plain concatenation
    dst addr | dst port | src addr | src port | flowId, which cannot tell a (4, 16) length pair
    from a (16, 4) pair with the same bytes; the device's make_key can, these tests follow
    make_key, and that case is not probed."""
    dst_addr = np.asarray(dst_addr, np.uint8).reshape(-1, 16)
    n = dst_addr.shape[0]
    src20 = np.asarray(src20, np.uint8).reshape(n, 20)
    dst_len = np.asarray(dst_len, np.uint8).reshape(n)
    pos = np.arange(16, dtype=np.uint8)[None, :]
    k = np.zeros((n, KEY_BYTES), np.uint8)
    k[:, 1] = dst_len
    k[:, 2:4] = np.asarray(dst_port).astype("<u2").reshape(n, 1).view(np.uint8)
    k[:, 4:20] = np.where(pos < dst_len[:, None], dst_addr, 0)
    k[:, 21] = src20[:, 1]
    k[:, 22:24] = src20[:, 2:4]
    k[:, 24:40] = np.where(pos < src20[:, 1:2], src20[:, 4:20], 0)
    k[:, 40:44] = np.asarray(flow_id).astype("<u4").reshape(n, 1).view(np.uint8)
    return k


def batch_keys(b):
    return key_bytes(b["dst_addr"], b["dst_len"], b["dst_port"], b["src"], b["flow_id"])


def _void(keys):
    return np.ascontiguousarray(keys, np.uint8).reshape(-1, KEY_BYTES).view(f"V{KEY_BYTES}")[:, 0]


class FirstSeen:
    """The table across calls: a dict from key bytes to dense index."""

    def __init__(self, max_keys=None):
        self.index = {}
        self.max_keys = max_keys

    def __len__(self):
        return len(self.index)

    def lookup(self, keys, err=None):
        """(uint32 indices, flow count) of one call: FLOW_NONE where err != 0, existing keys
        keep their index, new keys are numbered in the order of their first record; with
        max_keys, new keys past that many held map to FLOW_NONE."""
        keys = np.asarray(keys, np.uint8).reshape(-1, KEY_BYTES)
        n = keys.shape[0]
        out = np.full(n, FLOW_NONE, np.uint32)
        good = np.ones(n, bool) if err is None else np.asarray(err).reshape(n) == 0
        rec = np.flatnonzero(good)
        if rec.size == 0:
            return out, len(self.index)
        uniq, first, inv = np.unique(_void(keys[rec]), return_index=True, return_inverse=True)
        idx = np.full(uniq.size, FLOW_NONE, np.uint32)
        for u in np.argsort(first, kind="stable"):     # new keys: in first-record order
            kb = uniq[u].tobytes()
            j = self.index.get(kb)
            if j is None and (self.max_keys is None or len(self.index) < self.max_keys):
                j = self.index[kb] = len(self.index)
            if j is not None:
                idx[u] = j
        out[rec] = idx[inv.reshape(-1)]
        return out, len(self.index)

    def keys_in_order(self):
        """(n_flows, 44) uint8: the held keys by dense index."""
        out = np.zeros((len(self.index), KEY_BYTES), np.uint8)
        for kb, j in self.index.items():
            out[j] = np.frombuffer(kb, np.uint8)
        return out


def _step(h, w):
    h = h ^ w
    h = ((h << np.uint64(13)) | (h >> np.uint64(19))) & _M32
    return (h * np.uint64(5) + np.uint64(0xE6546B64)) & _M32


def _mix32(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & _M32
    return h ^ (h >> np.uint64(16))


def key_words(keys):
    """(n, 11) uint64: the device key's words 0-10 (make_key): four destination address words,
    four source address words, dst len | port << 16, src len | port << 16, flow id."""
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, KEY_BYTES)
    w = keys.view("<u4").astype(np.uint64)            # (n, 11): d0, da0-3, s0, sa0-3, fid
    d0 = (w[:, 0] >> np.uint64(8)) & np.uint64(0xFF) | (w[:, 0] >> np.uint64(16)) << np.uint64(16)
    s0 = (w[:, 5] >> np.uint64(8)) & np.uint64(0xFF) | (w[:, 5] >> np.uint64(16)) << np.uint64(16)
    return np.column_stack([w[:, 1:5], w[:, 6:10], d0, s0, w[:, 10]])


def slot_hash(keys):
    """key_hash of mgenx_flowtab.hip restated: 0x9E3779B9, then per key word xor, rotate left
    13, times 5 plus 0xE6546B64, and one mix32; uint32.  Only chooses inputs: no assertion on
    device output depends on it (test_gpu_flowtab_edges pins its low bits on the device)."""
    w = key_words(keys)
    h = np.full(w.shape[0], 0x9E3779B9, np.uint64)
    for j in range(11):
        h = _step(h, w[:, j])
    return _mix32(h).astype(np.uint32)


_clusters = {}


def cluster(cap, home, count, seed):
    """`count` distinct keys whose slot_hash & (cap - 1) == home, as a batch (one record per
    key, err 0): one IPv4 destination and source chosen by `seed`, the flow ids found by
    hashing candidates in blocks.  Cached per (cap, home, seed): a longer cluster starts with
    the shorter one."""
    ck = (cap, home, seed)
    fids = _clusters.get(ck, np.zeros(0, np.uint32))
    rng = np.random.default_rng(seed)
    base = {"dst_addr": np.zeros((1, 16), np.uint8), "dst_len": np.array([4], np.uint8),
            "dst_port": np.array([5000 + seed % 1000], np.uint16),
            "src": np.zeros((1, 20), np.uint8), "flow_id": np.zeros(1, np.uint32)}
    base["dst_addr"][0, :4] = (224, 1, seed & 255, 1)
    base["src"][0, :8] = (1, 4, 0x39, 0x1B, 10, rng.integers(0, 256), rng.integers(0, 256), 9)
    if fids.size < count:
        w = key_words(batch_keys(base))[0]
        h10 = np.full(1, 0x9E3779B9, np.uint64)
        for j in range(10):
            h10 = _step(h10, w[j:j + 1])
        found, start, block = [], 1 << 31, 1 << 20     # flow ids from 2^31 up
        while sum(f.size for f in found) < count:
            assert start < 1 << 32, "no cluster found"
            cand = np.arange(start, start + block, dtype=np.uint64)
            hit = (_mix32(_step(h10, cand)) & np.uint64(cap - 1)) == np.uint64(home)
            found.append(cand[hit].astype(np.uint32))
            start += block
        fids = _clusters[ck] = np.concatenate(found)
    fids = fids[:count]
    return {"dst_addr": np.repeat(base["dst_addr"], count, 0),
            "dst_len": np.repeat(base["dst_len"], count),
            "dst_port": np.repeat(base["dst_port"], count),
            "src": np.repeat(base["src"], count, 0), "flow_id": fids.copy(),
            "err": np.zeros(count, np.uint8)}
