"""No GPU: the serial model of mgenx_msg_match_multi_ex (tests/msg_match_multi_ex_ref.py) against
the model of mgenx_msg_match_ex run once per receiver, the identities include/mgenx.h states, the
struct sizes of mgen_amd._abi, and the two new formatters of python -m mgen_amd.match_multi."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_timeline_ref as TL  # noqa: E402
import msg_match_multi_ex_ref as MX  # noqa: E402
import msg_match_multi_ref as MM  # noqa: E402


def hand_model(min_run=1):
    nf, n_rcv, send, recv = MM.hand_case()
    return nf, n_rcv, send, recv, MX.model(nf, n_rcv, send, recv, min_run=min_run)


CASES = {
    "hand": lambda: MM.hand_case(),
    "random": lambda: (3, 4) + MX.random_case(7, 700, 3, 4),
    "one flow": lambda: (1, 2) + MX.random_case(11, 300, 1, 2),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    nf, n_rcv, send, recv = CASES[request.param]()
    return nf, n_rcv, send, recv, MX.model(nf, n_rcv, send, recv)


def test_each_receiver_alone_is_msg_match_ex(case):
    nf, n_rcv, send, recv, m = case
    for r in range(n_rcv):
        base, _own, _bins, _out, runs = TL.model(nf, send, MX.one_receiver(recv, r), 0, 1, 0)
        flows = base[3]
        for fld in ("loss_runs", "loss_run_max", "loss_run_hist"):
            assert m["rcv_runs"][:, r][fld].tolist() == flows[fld].tolist(), (r, fld)
        mine = m["runs"][m["runs"]["rcv"] == r].copy()
        mine["rcv"] = 0                                  # (where mgenx_loss_run has rsv)
        assert mine.tobytes() == runs.tobytes(), r


def test_min_run_filters_the_list_only(case):
    nf, n_rcv, send, recv, m = case
    longest = int(m["rcv_runs"]["loss_run_max"].max())
    for want in (0, 2, longest, longest + 1):
        f = MX.model(nf, n_rcv, send, recv, min_run=want, base=m["base"])
        assert f["rcv_runs"].tobytes() == m["rcv_runs"].tobytes()
        keep = m["runs"][m["runs"]["length"] >= max(want, 1)]
        assert f["runs"].tobytes() == keep.tobytes()
    assert len(MX.model(nf, n_rcv, send, recv, min_run=longest + 1, base=m["base"])["runs"]) == 0


def test_the_identities_of_the_header(case):
    nf, n_rcv, _send, _recv, m = case
    cells, fan = m["base"]["cells"], m["base"]["fanout"]
    for f in range(nf):
        sent = int(fan[f]["sent"])
        for r in range(n_rcv):
            mine = m["runs"][(m["runs"]["flow_idx"] == f) & (m["runs"]["rcv"] == r)]
            c = cells[f, r]
            # the run lengths of a cell sum to sent - delivered
            assert int(mine["length"].sum()) == sent - int(c["delivered"])
            assert len(mine) == int(m["rcv_runs"][f, r]["loss_runs"])
            assert int(m["rcv_runs"][f, r]["loss_run_hist"].sum()) == len(mine)
            head = mine[(mine["flags"] & MX.HEAD) != 0]
            tail = mine[(mine["flags"] & MX.TAIL) != 0]
            assert int(head["length"].sum()) == int(c["lost_head"])
            if int(c["delivered"]):
                assert int(tail["length"].sum()) == int(c["lost_tail"])
            # the diagonal: the receiver's own span and its loss in the middle
            d = m["pairs"][f, r, r]
            mid = sent - int(c["delivered"]) - int(c["lost_head"]) - int(c["lost_tail"])
            if int(c["delivered"]):
                assert int(d["span"]) == sent - int(c["lost_head"]) - int(c["lost_tail"])
                assert (int(d["lost_a"]), int(d["lost_b"]), int(d["lost_both"])) == (mid,) * 3
            else:
                assert d.tobytes() == bytes(32)
            for b in range(n_rcv):
                e, t = m["pairs"][f, r, b], m["pairs"][f, b, r]
                assert (int(e["span"]), int(e["lost_a"]), int(e["lost_b"]), int(e["lost_both"])) == \
                    (int(t["span"]), int(t["lost_b"]), int(t["lost_a"]), int(t["lost_both"]))
                assert int(e["lost_both"]) <= min(int(e["lost_a"]), int(e["lost_b"]))
                assert max(int(e["lost_a"]), int(e["lost_b"])) <= int(e["span"])


def test_the_hand_case_by_hand():
    # flow 0's owners are sends 0 1 3 4 6 8 10 11 13 (5 repeats 1, 7 has no flow) with masks
    # 5 5 7 0 0 3 2 3 1; flow 1's are 2 9 12 with masks 1 3 0
    nf, n_rcv, send, recv, m = hand_model()
    rr = m["rcv_runs"]
    assert rr["loss_runs"].tolist() == [[2, 3, 1], [1, 2, 1]]
    assert rr["loss_run_max"].tolist() == [[2, 2, 6], [1, 1, 3]]
    assert rr["loss_run_hist"][0, 1].tolist() == [1, 2] + [0] * 16
    assert rr["loss_run_hist"][0, 2].tolist() == [0, 0, 1] + [0] * 15
    T = 2000 * 10**6
    runs = [tuple(int(v) for v in r) for r in m["runs"]]
    assert runs == [
        # flow length first last flags rcv t_first t_last: by flow, last_send, rcv
        (0, 2, 0, 1, 1, 1, T + 100, T + 200),       # receiver 1 joins at send 3
        (0, 2, 4, 6, 0, 0, T + 400, T + 500),       # the gap, the duplicate 5 inside it
        (0, 2, 4, 6, 0, 1, T + 400, T + 500),
        (0, 1, 10, 10, 0, 0, T + 700, T + 700),
        (0, 1, 13, 13, 2, 1, T + 900, T + 900),     # receiver 1's tail
        (0, 6, 4, 13, 2, 2, T + 400, T + 900),      # receiver 2 left after send 3
        (1, 1, 2, 2, 1, 1, T + 250, T + 250),       # flow 1: receiver 1 joins at send 9
        (1, 1, 12, 12, 2, 0, T + 850, T + 850),
        (1, 1, 12, 12, 2, 1, T + 850, T + 850),
        (1, 3, 2, 12, 3, 2, T + 250, T + 850),      # never delivered: head and tail
    ]
    p = m["pairs"]
    # flow 0: spans in ranks are 0..8, 2..7 and 0..2; (0, 1) meet in 2..7 where 0 misses ranks
    # 3 4 6 and 1 misses 3 4: both 3 4
    assert tuple(int(v) for v in p[0, 0, 1]) == (6, 3, 2, 2)
    assert tuple(int(v) for v in p[0, 1, 0]) == (6, 2, 3, 2)
    assert tuple(int(v) for v in p[0, 0, 2]) == (3, 0, 0, 0)
    assert tuple(int(v) for v in p[0, 1, 2]) == (1, 0, 0, 0)     # the spans touch in rank 2
    assert tuple(int(v) for v in p[0, 0, 0]) == (9, 3, 3, 3)
    assert p[1, :, 2].tobytes() == bytes(32 * 3) and p[1, 2, :].tobytes() == bytes(32 * 3)
    assert tuple(int(v) for v in p[1, 0, 1]) == (1, 0, 0, 0)


def test_abi_sizes():
    import ctypes

    from mgen_amd import _abi
    assert _abi.RCV_RUNS_DTYPE.itemsize == 160
    assert _abi.RCV_LOSS_RUN_DTYPE.itemsize == 40
    assert _abi.RCV_PAIR_DTYPE.itemsize == 32
    assert ctypes.sizeof(_abi.MultiLoss) == 48
    for mine, theirs in ((_abi.RCV_RUNS_DTYPE, MX.RUNS), (_abi.RCV_LOSS_RUN_DTYPE, MX.RUN),
                         (_abi.RCV_PAIR_DTYPE, MX.PAIR)):
        assert mine.names == theirs.names
        assert [mine.fields[n][1] for n in mine.names] == [theirs.fields[n][1] for n in theirs.names]


def hand_keys():
    from mgen_amd._abi import REPORT_KEY_DTYPE
    keys = np.zeros(2, REPORT_KEY_DTYPE)
    keys["flow_id"] = [7, 9]
    return keys


def test_format_outages_sorts_by_flow_receiver_line():
    from mgen_amd.match_multi import _addr, format_cells, format_outages
    nf, n_rcv, send, recv, m = hand_model(min_run=2)
    keys = hand_keys()
    dst = _addr(keys[0]["dst"])
    T = 2000 * 10**6
    text = format_outages(keys, m["runs"])
    assert text.splitlines() == [
        "# flow dst rcv length first_line last_line t_first_us t_last_us head tail",
        "7 %s 0 2 5 7 %d %d 0 0" % (dst, T + 400, T + 500),
        "7 %s 1 2 1 2 %d %d 1 0" % (dst, T + 100, T + 200),
        "7 %s 1 2 5 7 %d %d 0 0" % (dst, T + 400, T + 500),
        "7 %s 2 6 5 14 %d %d 0 1" % (dst, T + 400, T + 900),
        "9 %s 2 3 3 13 %d %d 1 1" % (dst, T + 250, T + 850),
    ]
    assert text.endswith("\n")
    assert format_outages(keys, m["runs"][:0]).count("\n") == 1
    # the cell rows gain two columns and lose nothing
    cells, fan = m["base"]["cells"], m["base"]["fanout"]
    plain = format_cells(keys, cells, fan).splitlines()
    more = format_cells(keys, cells, fan, m["rcv_runs"]).splitlines()
    assert more[0] == plain[0] + " loss_runs longest_run"
    tails = [b[len(a):] for a, b in zip(plain[1:], more[1:])]
    assert tails == [" 2 2", " 3 2", " 1 6", " 1 1", " 2 1", " 1 3"]


def test_format_pairs_cuts_the_ratio():
    from mgen_amd.match_multi import _addr, format_pairs
    nf, n_rcv, send, recv, m = hand_model()
    keys = hand_keys()
    dst = _addr(keys[0]["dst"])
    lines = format_pairs(keys, m["pairs"]).splitlines()
    assert lines[0] == "# flow dst a b span lost_a lost_b lost_both cond"
    assert len(lines) == 1 + nf * n_rcv * (n_rcv - 1)
    assert lines[1] == "7 %s 0 1 6 3 2 2 0.666666" % dst          # 2 / 3, cut not rounded
    assert lines[2] == "7 %s 0 2 3 0 0 0 -" % dst                  # receiver 0 lost nothing there
    assert lines[3] == "7 %s 1 0 6 2 3 2 1.000000" % dst
    assert lines[7] == "9 %s 0 1 1 0 0 0 -" % dst
