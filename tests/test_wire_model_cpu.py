"""The plain-Python statement of MgenMsg::Unpack and the receive rules (wire_model.py)
against the C restatement every GPU test is checked with, on the crafted corpora of
wire_cases.py -- and the preconditions of those corpora, asserted from the model alone, so
that test_gpu_unpack_layouts.py cannot quietly stop reaching the decode paths it is for."""
import numpy as np
import pytest

import wire_cases as C
import wire_model as M

RULE_ARGS = {"udp": dict(force=False, tcp=False), "udp_force": dict(force=True, tcp=False),
             "tcp_force": dict(force=True, tcp=True)}


def _oracle_fields(oracle, records, rule):
    slab, offs, lens = C.place(list(records), "offsets")
    return oracle.udp_recv_batch(slab, len(records), rec_off=offs, rec_len=lens, **RULE_ARGS[rule])


def _agree(oracle, records, what):
    assert M.FIELDS_DTYPE.names == oracle.FIELDS_DTYPE.names
    for rule in M.RULES:
        want = _oracle_fields(oracle, records, rule)
        got, _ = M.recv_batch(records, rule)
        for name in M.FIELDS_DTYPE.names:
            g, w = got[name], want[name]
            bad = np.nonzero((g != w).reshape(len(records), -1).any(axis=1))[0]
            assert bad.size == 0, (what, rule, name, bad[:8], g[bad[:4]], w[bad[:4]])


@pytest.mark.parametrize("L", C.LATTICE_SIZES)
def test_model_equals_oracle_on_lattice(oracle, L):
    _agree(oracle, C.lattice(L), f"lattice({L})")


def test_model_equals_oracle_on_ladder_and_plain_errors(oracle):
    _agree(oracle, C.ladder()[0] + C.plain_errors() + (C.long_extra(),), "ladder")


def test_rules_differ_where_the_reference_says():
    """the 8,200-byte record: payload kept by a UDP receiver, dropped by a TCP one"""
    rec = C.long_extra()
    u, t = M.recv(rec, "udp"), M.recv(rec, "tcp_force")
    assert u["err"] == 0 and u["payload_len"] == 8152 and u["payload_off"] == 48
    assert t["err"] == 0 and t["payload_len"] == 0 and t["payload_off"] == 0 and t["hdr_len"] == 48
    # a TCP receiver checks the CRC whatever Unpack said, and flags the message
    bad = bytearray(C.plain_errors()[0])
    bad[-1] ^= 1
    t = M.recv(bytes(bad), "tcp_force")
    assert t["err"] == M.ERROR_CHECKSUM and t["flags"] == M.CHECKSUM_ERROR and t["ok"] == 0
    assert M.recv(bytes(bad), "udp_force")["err"] == M.ERROR_VERSION


# ---------------------------------------------------------------- the corpora
def _pair(rec):
    D = rec[23]
    at = 24 + D + 3
    return D, (rec[at] if at < len(rec) else None)


def _host_type(rec):
    at = 24 + rec[23] + 2
    return rec[at] if at < len(rec) else None


@pytest.mark.parametrize("L", C.LATTICE_SIZES)
def test_lattice_shape(L):
    recs = C.lattice(L)
    assert len(recs) == C.LATTICE_N == 204 and all(len(r) == L for r in recs)
    assert [r[23] for r in recs] == [d for d in C.DST_LENS for _ in C.HOST_LENS]
    for r, i in zip(recs, range(204)):
        at = 24 + r[23] + 3
        if at < L - 4:                       # not overwritten by the trailer, not past L
            assert r[at] == C.HOST_LENS[i % 12]
    assert all(r[2] == 2 and r[22] in (1, 2) for r in recs)
    # every fast layout the dispatch accepts, and (16,16), which it does not
    fast = [r for r in recs if C.fast_layout(r)]
    assert {_pair(r) for r in fast} == {(4, 0), (4, 4), (4, 16), (16, 0), (16, 4)}
    assert any(_pair(r) == (16, 16) and not C.fast_layout(r) for r in recs)
    assert sum(not C.fast_layout(r) for r in recs) >= 190
    # a fast layout whose host type Unpack does not accept
    bad_host = [r for r in fast if _host_type(r) not in (1, 2)]
    assert bad_host
    f, _ = M.recv_batch(bad_host, "udp")
    assert np.all(f["ok"] == 1) and np.all(f["host_type"] == 0) and np.all(f["host_len"] == 0)


def test_lattice_field_cycles_are_coprime_and_complete():
    periods = [len(c) for c in (C.DST_TYPES, C.PAYLOAD_TYPES, C.HOST_TYPES, C.GPS_STATUS,
                                C.PAYLOAD_LENS, C.MSG_SIZES, C.FLAGS, C.TRAILERS)]
    assert all(np.gcd(a, b) == 1 for i, a in enumerate(periods) for b in periods[i + 1:])
    assert set(C.DST_TYPES) == {1, 2} and set(C.HOST_TYPES) == {0, 1, 2, 3, 255}
    assert set(C.GPS_STATUS) == {0, 1, 2, 3, 255} and set(C.PAYLOAD_TYPES) == {0, 1, 255}
    assert set(C.PAYLOAD_LENS) == {"zero", "one", "room", "room+1", "room-4", "max"}
    assert set(C.MSG_SIZES) == {"L", "L-1", "L+1", "zero", "max"}
    assert set(C.FLAGS) == {0, C.CHECKSUM, C.CHECKSUM | C.CONTINUES}
    assert set(C.TRAILERS) == {"valid", "bit", "random"}


def test_lattice_outcome_cells():
    """Over the four lattices of the GENERAL batch, under the UDP rule: err 0 and err
    CHECKSUM x host accepted or not x payload kept or dropped, at least 30 records each;
    and exact-fit and one-too-many payload lengths both occur on both decode paths."""
    recs = [r for L in C.GENERAL_SIZES for r in C.lattice(L)]
    f, stage = M.recv_batch(recs, "udp")
    for err in (0, M.ERROR_CHECKSUM):
        for host in (False, True):
            for kept in (False, True):
                cell = (f["err"] == err) & ((f["host_type"] != 0) == host) & \
                       ((f["payload_len"] != 0) == kept)
                assert int(cell.sum()) >= 30, (err, host, kept, int(cell.sum()))
    fast = np.array([C.fast_layout(r) for r in recs])
    end = f["hdr_len"].astype(np.int64)
    lens = np.array([len(r) for r in recs])
    wire_plen = np.array([int.from_bytes(r[e - 2:e], "big") if e else -1 for r, e in zip(recs, end)])
    for path in (fast, ~fast):
        assert np.any(path & (stage == M.R_PAYLOAD_KEPT) & (end + wire_plen == lens))
        assert np.any(path & (stage == M.R_PAYLOAD_DROPPED) & (end + wire_plen == lens + 1))
    assert np.any(f["gps_status"] >= 3) and np.any(fast & (f["gps_status"] >= 3))
    # a payload offset that the word floor moves (header end not a multiple of four)
    assert np.any((f["payload_len"] != 0) & (f["payload_off"] != f["hdr_len"]))


def test_whole_corpus_reaches_every_error():
    f, _ = M.recv_batch(C.general_batch(), "udp")
    assert len(C.general_batch()) == 4 * 204 + 490 + 3 + len(C.REGRESSIONS)
    for err in (M.ERROR_NONE, M.ERROR_VERSION, M.ERROR_CHECKSUM, M.ERROR_LENGTH, M.ERROR_DSTADDR):
        assert np.any(f["err"] == err), err
    e, _ = M.recv_batch(C.plain_errors(), "udp")
    assert e["err"].tolist() == [M.ERROR_VERSION, M.ERROR_DSTADDR, M.ERROR_DSTADDR]


def test_ladder_reaches_every_return():
    """Each of the six layouts, cut at every length, ends the walk at every return that
    truncation can reach: too short, no host header, no host address (layouts with a host
    address; with hostAddrLen 0 that check cannot fail), no GPS, no payload type, no payload
    length (a successful decode with hdr_len 0), payload dropped and payload kept."""
    recs, layout = C.ladder()
    assert len(recs) == 490
    layout = np.array(layout)
    assert [len(r) for r in recs] == [c for D, H in C.LADDER_LAYOUTS
                                      for c in range(44 + D + H + 20 + 1)]
    f, stage = M.recv_batch(recs, "udp")
    for j, (D, H) in enumerate(C.LADDER_LAYOUTS):
        want = {M.R_LENGTH, M.R_NO_HOST, M.R_NO_GPS, M.R_NO_PTYPE, M.R_NO_PLEN,
                M.R_PAYLOAD_DROPPED, M.R_PAYLOAD_KEPT} | ({M.R_NO_HOST_ADDR} if H else set())
        # (a trailer written over the host length byte can add R_NO_HOST_ADDR where H is 0)
        assert set(stage[layout == j].tolist()) >= want, (D, H)
        full = f[layout == j][-1]
        assert full["err"] == 0 and full["payload_len"] == 20 and full["hdr_len"] == 44 + D + H
        assert full["host_len"] == H and full["dst_len"] == D
    assert np.any((f["ok"] == 1) & (f["err"] == 0) & (f["hdr_len"] == 0))
    # every second length from 32 up passes its CRC, the ones between do not
    lens = np.array([len(r) for r in recs])
    ok = f["ok"] == 1
    assert np.all(f["err"][ok & (lens >= 32) & (lens % 2 == 0)] == 0)
    assert np.all(f["err"][ok & (lens % 2 == 1)] == M.ERROR_CHECKSUM)


def test_place_layouts():
    recs = list(C.general_batch())
    slab, offs, lens = C.place(recs, "offsets")
    assert offs[0] == 3 and lens.tolist() == [len(r) for r in recs]
    gaps = offs[1:].astype(np.int64) - (offs[:-1].astype(np.int64) + lens[:-1])
    assert gaps.tolist() == [i % 7 for i in range(len(recs) - 1)]
    covered = np.zeros(len(slab), bool)
    for r, o in zip(recs, offs):
        assert bytes(slab[int(o):int(o) + len(r)]) == r
        covered[int(o):int(o) + len(r)] = True
    assert np.all(slab[~covered] == C.FILL) and not covered[-64:].any()
    assert np.any(offs % 4 != 0) and np.any(offs % 16 == 0)
    slab, stride = C.place(list(C.lattice(301)), "stride")
    assert stride == 301 and len(slab) == 204 * 301 + 64 and np.all(slab[-64:] == C.FILL)
    assert bytes(slab[301:602]) == C.lattice(301)[1]


def test_interleaved_positions():
    n, at = C.interleaved_index()
    assert n % 16 == 3                                    # a partial last group
    first = {i: j for i, j in at.items() if i <= 17 * 203}
    assert sorted(first.values()) == list(range(204))
    assert {i % 16 for i in first} == set(range(16))
    assert all(i + 1 not in at and i - 1 not in at for i in first)    # filler neighbours
    groups = {}
    for i in at:
        groups.setdefault(i // 16, []).append(i)
    whole = [g for g, m in groups.items() if len(m) == 16]
    assert len(whole) == 1 and whole[0] + 1 not in groups             # then 16 fillers
    for L in (65, 301, 512, 1024):
        lat = C.lattice(L)
        assert not any(C.fast_layout(lat[at[i]]) for i in groups[whole[0]])
        filler = np.zeros((n, L), np.uint8)
        recs = C.interleaved(L, filler)
        assert recs.shape == (n, L)
        assert all(bytes(recs[i]) == lat[j] for i, j in at.items() if i != n - 3)
        assert not recs[[i for i in range(n) if i not in at]].any()
        # the two spoilt trailing records: refused, with a non-zero dstAddrLen on the wire
        filler = np.full((n, L), 9, np.uint8)
        filler[:, 2], filler[:, 22] = 2, 1
        recs = C.interleaved(L, filler)
        f, _ = M.recv_batch([recs[n - 3].tobytes(), recs[n - 2].tobytes()], "udp")
        assert f["err"].tolist() == [M.ERROR_VERSION, M.ERROR_DSTADDR]
        assert recs[n - 3, 23] != 0 and recs[n - 2, 23] != 0 and not f["dst_len"].any()
        assert not C.fast_layout(recs[n - 1].tobytes())


def test_ipv6_sources_cover_every_zero_group_pattern():
    src = C.ipv6_sources()
    pats = {tuple(a[2 * k:2 * k + 2] == b"\0\0" for k in range(8)) for a in src[:256]}
    assert len(pats) == 256 and all(len(a) == 16 for a in src) and len(src) > 256 + 8
