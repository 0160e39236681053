"""The serial model of the TCP stream contract (tests/pcap_tcp_util.py) pinned by hand-worked
cases, and the binding's view of the ABI.  No GPU."""
import numpy as np

import pcap_frag_util as F
import pcap_tcp_util as T


def _ref(items, link=1):
    f = T.pcap_of(items, link)
    return T.tcp_ref(F.records(f), link)


def _rows(ref):
    return [(s["first_pkt"], s["n_segments"], s["flags"], s["len"], s["dropped"], s["off"])
            for s in ref.streams]


def test_retransmission_overlap_and_hole():
    c = T.Conn()
    ref = _ref([c.ip(100, flags=T.SYN),
                c.ip(101, b"abcdefghij"),
                c.ip(101, b"abcdefghij"),            # an exact duplicate: nothing
                c.ip(106, b"fghijKLMNO"),            # overlaps [5, 10): contributes [10, 15)
                c.ip(121, b"vwxyz"),                 # rel 20 > E 15: the hole
                c.ip(123, b"xyz012")])               # past the hole: [25, 28) counted as dropped
    assert ref.status == [9] * 6
    assert _rows(ref) == [(0, 6, 3, 15, 8, 0)]
    assert ref.pieces == [(10, 1), (15, 3)]
    assert ref.scratch == b"abcdefghijKLMNO\0"
    assert ref.stats == dict(n_segments=6, n_streams=1, n_gap_streams=1, n_stale=0,
                             dropped_bytes=8, n_pieces=2, scratch_bytes=16)


def test_no_syn_wrapping_seq_reversed_order_stale_and_the_other_direction():
    c = T.Conn()
    ref = _ref([c.ip(0xFFFFFFFC, b"wxyz"),           # the first payload: base
                c.ip(4, b"EFGH"),                    # rel 8, ahead of
                c.ip(0, b"abcd"),                    # rel 4
                c.reverse().ip(900),                 # a pure ACK the other way: its own stream
                c.ip(0xFFFFFFF2, b"old")])           # rel = -10: stale
    assert ref.status == [9] * 5
    assert _rows(ref) == [(0, 4, 0, 12, 0, 0), (3, 1, 0, 0, 0, 16)]
    assert ref.pieces == [(4, 0), (8, 2), (12, 2)]
    assert ref.scratch == b"wxyzabcdEFGH" + bytes(4)
    assert ref.stats == dict(n_segments=5, n_streams=2, n_gap_streams=0, n_stale=1,
                             dropped_bytes=0, n_pieces=3, scratch_bytes=16)
    assert [s["key"] for s in ref.streams] == [(4, T.A4, T.B4, 40000, 5000),
                                               (4, T.B4, T.A4, 5000, 40000)]


def test_tuple_reuse_repeated_syn_data_before_syn_truncated_and_bad_offset():
    c = T.Conn()
    cut = c.ip(5007, b"0123456789")
    ref = _ref([c.ip(50, b"pre"),                    # before the first SYN: a stream of its own
                c.ip(1000, flags=T.SYN),
                c.ip(1000, flags=T.SYN),             # repeated: changes nothing
                c.ip(1001, b"hello"),
                c.ip(5000, b"ignored", flags=T.SYN),  # another seq: a new stream; payload ignored
                c.ip(5001, b"world!"),
                c.ip(5007, b"nothing", doff=16),     # data offset below 20: untouched
                (cut, 14 + len(cut) - 4),            # cut by the snapshot length
                c.ip(5017, b"zz")])                  # behind what the cut packet held: a hole
    assert ref.status == [9, 9, 9, 9, 9, 9, None, 5, 9]
    assert _rows(ref) == [(0, 1, 0, 3, 0, 0), (1, 3, 1, 5, 0, 16), (4, 3, 3, 6, 2, 32)]
    assert ref.pieces == [(3, 0), (21, 3), (38, 5)]
    assert ref.scratch == b"pre" + bytes(13) + b"hello" + bytes(11) + b"world!" + bytes(10)
    assert ref.stats == dict(n_segments=7, n_streams=3, n_gap_streams=1, n_stale=0,
                             dropped_bytes=2, n_pieces=3, scratch_bytes=48)


def test_padding_options_v6_sll_and_fragments():
    c6 = T.Conn(T.A6, T.B6, 1, 2)
    c = T.Conn()
    frag = bytearray(c.ip(1, b"frag"))
    frag[6] = 0x20                                   # MF: IP-fragmented TCP is not followed
    items = [c6.ip(7, b"six"), c.ip(7, b"opt", doff=24), bytes(frag)]
    for link in (1, 113):
        ref = _ref(items, link)
        assert ref.status == [9, 9, None]
        assert _rows(ref) == [(0, 1, 0, 3, 0, 0), (1, 1, 0, 3, 0, 16)]
        assert ref.scratch == b"six" + bytes(13) + b"opt" + bytes(13)   # no Ethernet padding
    # a hole at offset 0: the SYN fixes the base, the first byte never came
    ref = _ref([c.ip(10, flags=T.SYN), c.ip(12, b"late")])
    assert _rows(ref) == [(0, 2, 3, 0, 4, 0)] and ref.pieces == [] and ref.scratch == b""


def test_segmenter_round_trip():
    rng = np.random.default_rng(5)
    stream = bytes(rng.integers(0, 256, 20000, dtype=np.uint8))
    c = T.Conn()
    segs = T.segment(stream, 536, 0xFFFFFF00, True, rng, retx=0.2, reorder=3, overlap=7)
    ref = _ref([c.ip(s[0], s[2], s[1]) for s in segs])
    assert len(ref.streams) == 1 and ref.streams[0]["data"] == stream
    assert ref.streams[0]["flags"] == T.SYN_FLAG and ref.stats["n_segments"] == len(segs)
    assert [e for e, _ in ref.pieces] == sorted({e for e, _ in ref.pieces})
    assert [p for _, p in ref.pieces] == sorted(p for _, p in ref.pieces)
    lost = T.segment(stream, 536, 5, True, rng, lose=(3,))
    ref = _ref([c.ip(s[0], s[2], s[1]) for s in lost])
    assert ref.streams[0]["len"] == 3 * 536 and ref.streams[0]["flags"] == 3
    assert ref.streams[0]["dropped"] == 20000 - 4 * 536


def test_abi_constants_and_symbols():
    import mgen_amd
    from mgen_amd import _abi
    assert _abi.PCAP_TCP == T.TCP == 9 and (_abi.TCP_SYN, _abi.TCP_GAP) == (1, 2)
    assert _abi.TCP_STREAM_DTYPE.itemsize == 80
    assert [n for n, _ in _abi.TcpStats._fields_] == [
        "n_segments", "n_streams", "n_gap_streams", "n_stale", "dropped_bytes", "n_pieces",
        "scratch_bytes"]
    L = mgen_amd.load()
    for s in ("mgenx_pcap_tcp", "mgenx_pcapng_tcp", "mgenx_tcp_frame"):
        assert s in mgen_amd.EXPORTED_SYMBOLS and hasattr(L, s)
