"""mgenx_msg_match_multi without a GPU: the serial model (tests/msg_match_multi_ref.py) on a case
worked by hand and against the one-receiver model (tests/msg_match_ref.py) on random inputs, the
ABI layout against a C probe, argument checks, and the three formatters on hand-made arrays."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msg_match_multi_ref as MM  # noqa: E402
import msg_match_ref as M1  # noqa: E402

N = MM.NONE
I64_MAX, I64_MIN = 2**63 - 1, -2**63
# worked out by hand from the definitions (see msg_match_multi_ref.hand_case)
# flow 0: owners 0 1 3 4 6 8 10 11 13 (ranks 0..8), send 5 repeats send 1; flow 1: owners 2 9 12
HAND_MASK = [5, 5, 1, 7, 0, 0, 0, 0, 3, 3, 2, 3, 0, 1]
HAND_RECV_SEND = [0, 1, 2, 3, 8, 9, 3, 3, 11, 13, 8, 9, 10, 11, N, N, 0, 1, 3, N]
HAND_RECV_FIRST = [1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0]
HAND_CELLS = {
    (0, 0): dict(delivered=6, delivered_bytes=384, rx_dup=0, rx_orphan=0, lost_head=0, lost_tail=0,
                 first_send=0, last_send=13, lat_sum=290, lat_min=-10, lat_max=80),
    # the late joiner: ranks 2 5 6 7; send 3 logged twice, its first arrival is recv 6
    (0, 1): dict(delivered=4, delivered_bytes=256, rx_dup=1, rx_orphan=1, lost_head=2, lost_tail=1,
                 first_send=3, last_send=11, lat_sum=1000250, lat_min=60, lat_max=1000000),
    # the one that leaves early: ranks 0 1 2
    (0, 2): dict(delivered=3, delivered_bytes=192, rx_dup=0, rx_orphan=0, lost_head=0, lost_tail=6,
                 first_send=0, last_send=3, lat_sum=80, lat_min=20, lat_max=30),
    (1, 0): dict(delivered=2, delivered_bytes=200, rx_dup=0, rx_orphan=0, lost_head=0, lost_tail=1,
                 first_send=2, last_send=9, lat_sum=100, lat_min=50, lat_max=50),
    (1, 1): dict(delivered=1, delivered_bytes=100, rx_dup=0, rx_orphan=0, lost_head=1, lost_tail=1,
                 first_send=9, last_send=9, lat_sum=70, lat_min=70, lat_max=70),
    (1, 2): dict(delivered=0, delivered_bytes=0, rx_dup=0, rx_orphan=0, lost_head=3, lost_tail=0,
                 first_send=N, last_send=N, lat_sum=0, lat_min=I64_MAX, lat_max=I64_MIN),
}
HAND_FANOUT = {
    0: dict(sent=9, sent_bytes=640, send_dup=1, deliveries=13, reached_all=1),
    1: dict(sent=3, sent_bytes=300, send_dup=0, deliveries=3, reached_all=0),
}
HAND_HIST = {0: [2, 2, 4, 1], 1: [1, 1, 1, 0]}


def test_model_on_the_hand_case():
    nf, n_rcv, send, recv = MM.hand_case()
    assert (nf, n_rcv, len(send["seq"]), len(recv["seq"])) == (2, 3, 14, 20)
    out = MM.model(nf, n_rcv, send, recv)
    assert out["send_mask"].tolist() == HAND_MASK
    assert out["recv_send"].tolist() == HAND_RECV_SEND
    assert out["recv_first"].tolist() == HAND_RECV_FIRST
    for (f, r), want in HAND_CELLS.items():
        assert {k: int(out["cells"][f, r][k]) for k in want} == want, (f, r)
    for f, want in HAND_FANOUT.items():
        assert {k: int(out["fanout"][f][k]) for k in want} == want, f
        assert out["fanout"][f]["reach_hist"].tolist() == HAND_HIST[f] + [0] * 61, f
    assert {k: int(out["stats"][0][k]) for k in MM.STATS.names} == dict(
        send_skipped=1, recv_skipped=2, recv_unmatched=1, send_dup=1)
    # the loss at r and its middle part
    c = out["cells"]
    assert [9 - int(c[0, r]["delivered"]) for r in range(3)] == [3, 5, 6]
    assert [9 - int(c[0, r]["delivered"] + c[0, r]["lost_head"] + c[0, r]["lost_tail"])
            for r in range(3)] == [3, 2, 0]


def test_model_series_on_the_hand_case():
    nf, n_rcv, send, recv = MM.hand_case()
    t0 = 2000 * 10**6 + 300
    out = MM.model(nf, n_rcv, send, recv, timeline=(t0, 300, 2))
    assert out["outside"].tolist() == [3, 1]
    want = {
        (0, 0): dict(sent=3, sent_bytes=256, deliveries=3, delivered_bytes=192, reached_any=1,
                     reached_all=1, reach_min=0, reach_max=3),
        (0, 1): dict(sent=3, sent_bytes=192, deliveries=5, delivered_bytes=320, reached_any=3,
                     reached_all=0, reach_min=1, reach_max=2),
        (1, 0): dict(sent=0, sent_bytes=0, deliveries=0, delivered_bytes=0, reached_any=0,
                     reached_all=0, reach_min=2**64 - 1, reach_max=0),
        (1, 1): dict(sent=2, sent_bytes=200, deliveries=2, delivered_bytes=200, reached_any=1,
                     reached_all=0, reach_min=0, reach_max=2),
    }
    for (f, b), w in want.items():
        assert {k: int(out["bins"][f, b][k]) for k in w} == w, (f, b)


def test_model_without_the_time_stamps():
    nf, n_rcv, send, recv = MM.hand_case()
    recv["tx_usec"][12] += 1          # -> send 10 only when the stamp does not count
    out = MM.model(nf, n_rcv, send, recv)
    assert out["recv_send"][12] == N and int(out["cells"][0, 1]["rx_orphan"]) == 2
    assert out["send_mask"][10] == 0
    out = MM.model(nf, n_rcv, send, recv, no_time=True)
    assert out["recv_send"].tolist() == HAND_RECV_SEND and out["send_mask"].tolist() == HAND_MASK


def _random_case(rng, n_flows, n_rcv, ns, nr):
    send = MM.cols(MM.SEND_COLS, [
        (rng.integers(0, n_flows + 1) if rng.random() < 0.95 else N, rng.integers(0, 12), 50,
         rng.integers(0, 3), rng.integers(1, 200)) for _ in range(ns)])
    recv = MM.cols(MM.RECV_COLS, [
        (rng.integers(0, n_flows + 1), rng.integers(0, 14), 50, rng.integers(0, 3),
         rng.integers(49, 52), rng.integers(0, 10**6), rng.integers(0, n_rcv + 1))
        for _ in range(nr)])
    return send, recv


def test_model_against_the_one_receiver_model():
    rng = np.random.default_rng(20240607)
    for trial in range(30):
        n_flows, n_rcv = int(rng.integers(1, 4)), int(rng.integers(1, 6))
        send, recv = _random_case(rng, n_flows, n_rcv, int(rng.integers(0, 60)),
                                  int(rng.integers(0, 120)))
        no_time = bool(trial & 1)
        out = MM.model(n_flows, n_rcv, send, recv, no_time=no_time)
        cells, fan = out["cells"], out["fanout"]
        in_range = recv["rcv"] < n_rcv
        sub = lambda keep: {k: recv[k][keep] for k in M1.RECV_COLS}  # noqa: E731
        for r in range(n_rcv):
            _c, _f, _rs, flows, _st = M1.model(n_flows, send, sub(recv["rcv"] == r), no_time)
            for f in range(n_flows):
                for k in ("delivered", "delivered_bytes", "rx_dup", "rx_orphan", "lost_head",
                          "lost_tail", "lat_sum", "lat_min", "lat_max"):
                    assert int(cells[f, r][k]) == int(flows[f][k]), (trial, f, r, k)
        _c, _f, _rs, flows, st = M1.model(n_flows, send, sub(in_range), no_time)
        for f in range(n_flows):
            hist = [int(v) for v in fan[f]["reach_hist"]]
            sent = int(fan[f]["sent"])
            assert sent == int(flows[f]["sent"])
            assert hist[0] == sent - int(flows[f]["delivered"])
            assert sum(hist) == sent and not any(hist[n_rcv + 1:])
            assert (sum(int(cells[f, r]["delivered"]) for r in range(n_rcv))
                    == int(fan[f]["deliveries"]) == sum(k * n for k, n in enumerate(hist)))
            assert int(fan[f]["reached_all"]) == hist[n_rcv]
        assert int(out["stats"][0]["send_dup"]) == int(st[0]["send_dup"])
        assert int(out["stats"][0]["recv_unmatched"]) == int(st[0]["recv_unmatched"])
        assert int(out["stats"][0]["recv_skipped"]) == int(st[0]["recv_skipped"]) + int(
            (~in_range).sum())


def test_layout_matches_header_and_symbols(tmp_path):
    import mgen_amd
    from mgen_amd import FLOW_FANOUT_DTYPE, MULTI_BIN_DTYPE, RCV_CELL_DTYPE
    assert "mgenx_msg_match_multi" in mgen_amd.EXPORTED_SYMBOLS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %zu %zu %zu\\n", sizeof(struct mgenx_rcv_cell), '
             'sizeof(struct mgenx_flow_fanout), sizeof(struct mgenx_multi_bin), '
             'sizeof(mgenx_multi_timeline));']
    mine = {"cell": ("mgenx_rcv_cell", RCV_CELL_DTYPE, MM.CELL),
            "fanout": ("mgenx_flow_fanout", FLOW_FANOUT_DTYPE, MM.FANOUT),
            "bin": ("mgenx_multi_bin", MULTI_BIN_DTYPE, MM.BIN)}
    for st, (name, dt, _ref) in mine.items():
        for f in dt.names:
            lines.append(f'printf("{st} {f} %zu\\n", offsetof(struct {name}, {f}));')
    for f, _t in mgen_amd.MultiTimeline._fields_:
        lines.append(f'printf("tl {f} %zu\\n", offsetof(mgenx_multi_timeline, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["80", "560", "64", str(ctypes.sizeof(mgen_amd.MultiTimeline))]
    assert (RCV_CELL_DTYPE.itemsize, FLOW_FANOUT_DTYPE.itemsize, MULTI_BIN_DTYPE.itemsize) == \
        (80, 560, 64) == (MM.CELL.itemsize, MM.FANOUT.itemsize, MM.BIN.itemsize)
    assert FLOW_FANOUT_DTYPE["reach_hist"].shape == (65,) == MM.FANOUT["reach_hist"].shape
    seen = 0
    for line in out[1:]:
        if not line:
            continue
        st, name, off = line.split()
        if st == "tl":
            assert getattr(mgen_amd.MultiTimeline, name).offset == int(off), line
        else:
            _n, dt, ref = mine[st]
            assert dt.fields[name][1] == int(off) == ref.fields[name][1], line
        seen += 1
    assert seen == len(MM.CELL.names) + len(MM.FANOUT.names) + len(MM.BIN.names) + 5


def test_bad_arguments_are_rejected_without_hip():
    from mgen_amd import MultiTimeline, load
    L = load()
    one = ctypes.c_void_p(16)     # a non-null pointer that is never followed
    send, recv, outs = (one,) * 5, (one,) * 7, (one,) * 6
    # no context; the other checks need one and run in tests/test_gpu_msg_match_multi.py
    assert L.mgenx_msg_match_multi(None, *send, 4, *recv, 4, 2, 2, 0, *outs, None, None) == -1
    tl = MultiTimeline(t0_us=0, width_us=0, n_bins=4, dev_bins=16, dev_outside=16)
    assert L.mgenx_msg_match_multi(None, *send, 4, *recv, 4, 2, 2, 0, *outs, ctypes.byref(tl),
                                   None) == -1


def _keys():
    from mgen_amd import REPORT_KEY_DTYPE
    keys = np.zeros(2, REPORT_KEY_DTYPE)
    for f, fid in enumerate((7, 4000000000)):
        keys[f]["flow_id"] = fid
        keys[f]["src"]["port"] = 5001
        keys[f]["dst"]["len"] = 4
        keys[f]["dst"]["port"] = 5000
        keys[f]["dst"]["addr"][:4] = (224, 225, 1, 2)
    keys[1]["dst"]["len"] = 16
    keys[1]["dst"]["addr"][:] = [0xff, 0x0e] + [0] * 13 + [1]
    return keys


def test_format_cells_and_reach_on_hand_made_arrays():
    from mgen_amd import FLOW_FANOUT_DTYPE, RCV_CELL_DTYPE
    from mgen_amd.match_multi import format_cells, format_reach
    keys = _keys()
    cells = np.zeros((2, 2), RCV_CELL_DTYPE)
    cells["lat_min"], cells["lat_max"] = I64_MAX, I64_MIN
    cells["first_send"] = cells["last_send"] = N
    for k, v in dict(delivered=4, rx_dup=1, rx_orphan=1, lost_head=2, lost_tail=1,
                     lat_sum=1000251, lat_min=-60, lat_max=1000000).items():
        cells[0, 1][k] = v
    cells[0, 0]["lost_head"] = 9
    for k, v in dict(delivered=2**40, lat_sum=-3 * 2**40 + 1, lat_min=-7,
                     lat_max=2**53 + 1).items():
        cells[1, 0][k] = v
    cells[1, 1]["lost_head"] = 2**40
    fanout = np.zeros(2, FLOW_FANOUT_DTYPE)
    fanout["sent"] = (9, 2**40)
    fanout["reached_all"] = (1, 0)
    fanout[0]["reach_hist"][:3] = (5, 3, 1)
    fanout[1]["reach_hist"][:3] = (0, 2**40, 0)
    assert format_cells(keys, cells, fanout) == (
        "# flow dst rcv sent delivered lost lost_head lost_tail rx_dup orphans lat_min lat_mean "
        "lat_max\n"
        "7 224.225.1.2/5000 0 9 0 9 9 0 0 0 - - -\n"
        "7 224.225.1.2/5000 1 9 4 5 2 1 1 1 -60 250062 1000000\n"
        "4000000000 ff0e::1/5000 0 1099511627776 1099511627776 0 0 0 0 0 -7 -3 9007199254740993\n"
        "4000000000 ff0e::1/5000 1 1099511627776 0 1099511627776 1099511627776 0 0 0 - - -\n")
    assert format_reach(keys, fanout, 2) == (
        "# flow dst sent reached_all all_ratio reach_0 reach_1 reach_2\n"
        "7 224.225.1.2/5000 9 1 0.111111 5 3 1\n"
        "4000000000 ff0e::1/5000 1099511627776 0 0.000000 0 1099511627776 0\n")
    assert format_cells(keys[:0], cells[:0], fanout[:0]).count("\n") == 1
    fanout[0]["sent"] = 0
    assert format_reach(keys[:1], fanout[:1], 2).split("\n")[1] == "7 224.225.1.2/5000 0 1 - 5 3 1"


def test_format_multi_series_on_a_hand_made_array():
    from mgen_amd import MULTI_BIN_DTYPE
    from mgen_amd.match_multi import format_multi_series
    keys = _keys()
    bins = np.zeros((2, 3), MULTI_BIN_DTYPE)
    bins["reach_min"] = 2**64 - 1
    for k, v in dict(sent=3, reached_any=2, reached_all=1, deliveries=5).items():
        bins[0, 0][k] = v
    for k, v in dict(sent=4, reached_any=4, reached_all=4, deliveries=12).items():
        bins[0, 2][k] = v
    bins[1, 1]["sent"] = 7
    assert format_multi_series(keys, bins, 10**15, 250000, 3) == (
        "# flow>7 src>-/5001 dst>224.225.1.2/5000\n"
        "# bin_start_us sent reached_any reached_all delivery_ratio\n"
        "1000000000000000 3 2 1 0.555555\n"
        "1000000000500000 4 4 4 1.000000\n"
        "\n\n"
        "# flow>4000000000 src>-/5001 dst>ff0e::1/5000\n"
        "# bin_start_us sent reached_any reached_all delivery_ratio\n"
        "1000000000250000 7 0 0 0.000000\n")
