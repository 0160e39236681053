"""The reassembly contract's serial model and the test fragmenters (tests/pcap_frag_util.py),
checked on their own: the GPU tests compare mgenx_pcap_defrag with this model, so a hand-worked
case pins the model to the contract's text (include/mgenx.h)."""
import struct

import numpy as np
import pytest

import pcap_frag_util as F
import pcap_util as P


def _v4(payload, off, mf, ident, src=5, proto=17):
    hdr = P.ipv4(b"", bytes([10, 0, 0, src]), F.DST4, proto=proto)
    return F.frag_v4(hdr, payload, off, mf, ident)


def test_model_on_a_hand_worked_case():
    """Eleven packets, every value below worked by hand from the contract.
    Datagram A (id 7): UDP header (sport 0x1234, length 40) + 32 bytes, cut 16 + 16 + 8.
    Datagram B (id 9): 24 bytes cut 16 + 8 whose UDP length field says 200 (> L)."""
    a = struct.pack(">HHHH", 0x1234, 5001, 40, 0) + bytes(range(32))
    b = struct.pack(">HHHH", 1, 2, 200, 0) + bytes(16)
    plain = P.ipv4(P.udp(bytes(30), 77, 88), bytes([10, 0, 0, 5]), F.DST4)
    ips = [
        _v4(a[0:16], 0, True, 7),        # 0  A first
        plain,                           # 1  not a fragment: untouched
        _v4(a[32:40], 32, False, 7),     # 2  A last: L = 40, sum 24
        _v4(b[0:16], 0, True, 9),        # 3  B first
        _v4(a[16:32], 16, True, 7),      # 4  A middle: sum 40 = L -> complete, UDP, slot 0
        _v4(b[16:24], 16, False, 9),     # 5  B complete: L 24, ul 200 > L -> NOT_UDP, slot 48
        _v4(a[0:16], 0, True, 7),        # 6  id 7 again: a new context
        _v4(a[8:24], 8, True, 7),        # 7  overlaps [0,16): context dropped, a new one opens
        _v4(a[0:12], 0, True, 7, src=6), # 8  MF with len % 8: BAD_IP, no part
        _v4(bytes(16), 8, False, 7, proto=6),   # 9  TCP fragment: untouched (NOT_UDP)
        _v4(bytes(8), 65528, False, 11), # 10 off + len = 65536 > 65535: BAD_IP
    ]
    recs = [(100, 10 * k, P.eth(ip), len(P.eth(ip))) for k, ip in enumerate(ips)]
    base_status = [4, 0, 4, 4, 4, 4, 4, 4, 4, 4, 4]     # what the parse gives (first fragments:
    base_len = [0, 30, 0, 0, 0, 0, 0, 0, 0, 0, 0]       # UDP length past the packet; later ones:
    base_port = [0, 77, 0, 0, 0, 0, 0, 0, 0, 0, 0]      # zero fill read as a UDP header)
    r = F.frag_ref(recs, 1, base_status, base_len, base_port)
    assert r.status.tolist() == [8, 0, 8, 8, 0, 4, 8, 8, 3, 4, 3]
    assert r.udp_len.tolist() == [0, 30, 0, 0, 32, 0, 0, 0, 0, 0, 0]
    assert r.port.tolist() == [0, 77, 0, 0, 0x1234, 0, 0, 0, 0, 0, 0]
    assert r.udp_rel.tolist() == [-1, -1, -1, -1, 8, -1, -1, -1, -1, -1, -1]
    assert r.stats == dict(n_fragments=7, n_datagrams=2, n_not_udp=1, n_incomplete=2,
                           scratch_bytes=48 + 32)
    assert r.scratch == a + bytes(8) + b + bytes(8)
    assert [(p, L, slot) for p, L, _, slot in r.datagrams] == [(4, 40, 0), (5, 24, 48)]


def test_model_timeout_and_limits():
    frag = lambda k, t: (0, t, P.eth(_v4(bytes(8), 8 * k, True, 3)), 0)
    recs = [(s, u, d, len(d)) for s, u, d, _ in (frag(0, 0), frag(1, 100), frag(2, 101))]
    z = [4] * 3, [0] * 3, [0] * 3
    assert F.frag_ref(recs, 1, *z, timeout_us=100).stats["n_incomplete"] == 2   # 101 > 100
    assert F.frag_ref(recs, 1, *z, timeout_us=101).stats["n_incomplete"] == 1   # exactly: kept
    assert F.frag_ref(recs, 1, *z, timeout_us=0).stats["n_incomplete"] == 1
    many = [P.eth(_v4(bytes(8), 8 * k, True, 3)) for k in range(66)]
    recs = [(0, k, d, len(d)) for k, d in enumerate(many)]
    r = F.frag_ref(recs, 1, [4] * 66, [0] * 66, [0] * 66)
    assert r.stats["n_incomplete"] == 2 and r.stats["n_fragments"] == 66    # the 65th drops it


@pytest.mark.parametrize("v6,mtu", [(False, 1500), (False, 576), (True, 1280), (False, 68)])
def test_fragmenter_round_trip(oracle, v6, mtu):
    """Concatenating the payloads by offset restores the datagram; every fragment fits the
    MTU, all but the last carry MF and a multiple of 8 bytes."""
    for size in (1473, 1500, 3900, 8192):
        ip = F.datagram(oracle, 3, 5, 1_700_000_000_000_000, size, v6)
        frags = F.fragment(ip, mtu, 0xBEEF, early_ttl=9)
        assert all(len(f) <= mtu for f in frags) and len(frags) > 1
        body = ip[40:] if v6 else ip[20:]
        got = bytearray(len(body))
        for k, (off, mf, pay) in enumerate(F.payloads(frags)):
            assert mf == (k < len(frags) - 1) and (not mf or len(pay) % 8 == 0)
            got[off:off + len(pay)] = pay
            c = F.classify(P.eth(frags[k]), len(P.eth(frags[k])), 1)
            assert (c["off"], c["len"], c["mf"]) == (off, len(pay), mf)
        assert bytes(got) == body
        assert sum(len(p) for _, _, p in F.payloads(frags)) == len(body)
        ttl_at = 7 if v6 else 8
        assert frags[0][ttl_at] == 9 and frags[-1][ttl_at] == ip[ttl_at] != 9
    whole, cut = F.capture(oracle, seed=1, n=12, v6=v6, mtu=max(mtu, 576))
    assert len(F.records(cut)) > len(F.records(whole)) == 12


def test_python_layouts_match_the_header():
    import mgen_amd
    from mgen_amd import _abi
    assert _abi.PCAP_FRAGMENT == F.FRAGMENT == 8 and _abi.ENOSPC == -4
    assert _abi.DEFRAG_MAX_FRAGS == F.MAX_FRAGS
    assert [n for n, _ in _abi.DefragStats._fields_] == [
        "n_fragments", "n_datagrams", "n_not_udp", "n_incomplete", "scratch_bytes"]
    L = mgen_amd.load()
    for s in ("mgenx_pcap_defrag", "mgenx_pcapng_defrag"):
        assert s in mgen_amd.EXPORTED_SYMBOLS and hasattr(L, s)
