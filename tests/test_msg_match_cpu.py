"""mgenx_msg_match without a GPU: the serial model (tests/msg_match_ref.py) on a case worked by
hand, the ABI layout against a C probe, argument checks, and format_match on a hand-made array."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msg_match_ref as M  # noqa: E402

N = M.NONE
EMPTY_HIST = [0] * 18
HAND_FLOWS = {   # worked out by hand from the definitions (see msg_match_ref.hand_case)
    # owners 0 1 3 4 6 8 10 11 = U D U U U D U U; send 7 repeats send 1
    0: dict(sent=8, sent_bytes=7 * 64 + 128, send_dup=1, delivered=2, delivered_bytes=192,
            rx_dup=1, rx_orphan=1, lost_head=1, lost_tail=2, loss_runs=3, loss_run_max=3,
            lat_sum=650, lat_min=-50, lat_max=700),
    # owners 2 9 = D U
    1: dict(sent=2, sent_bytes=200, send_dup=0, delivered=1, delivered_bytes=100, rx_dup=1,
            rx_orphan=1, lost_head=0, lost_tail=1, loss_runs=1, loss_run_max=1,
            lat_sum=999800, lat_min=999800, lat_max=999800),
}
HAND_HIST = {0: [1, 2] + [0] * 16, 1: [1] + [0] * 17}


def test_model_on_the_hand_case():
    nf, send, recv = M.hand_case()
    assert len(send["seq"]) == 12 and len(recv["seq"]) == 8
    cnt, first, rs, flows, stats = M.model(nf, send, recv)
    assert cnt.tolist() == [0, 2, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert first.tolist() == [N, 0, 1, N, N, N, N, N, 4, N, N, N]
    assert rs.tolist() == [1, 2, N, 1, 8, N, N, 2]
    for f, want in HAND_FLOWS.items():
        assert {k: int(flows[f][k]) for k in want} == want, f
        assert flows[f]["loss_run_hist"].tolist() == HAND_HIST[f], f
    assert {k: int(stats[0][k]) for k in stats.dtype.names} == dict(
        send_skipped=1, recv_skipped=1, recv_unmatched=2, send_dup=1)
    # sent - delivered is the loss; the runs account for all of it
    for f in range(nf):
        assert int(flows[f]["sent"] - flows[f]["delivered"]) == (6, 1)[f]


def test_model_without_the_time_stamps():
    nf, send, recv = M.hand_case()
    cnt, first, rs, flows, stats = M.model(nf, send, recv, no_time=True)
    # recv 6 differs from send 2 in the stamp alone
    assert rs.tolist() == [1, 2, N, 1, 8, N, 2, 2] and cnt[2] == 3
    assert int(flows[1]["rx_dup"]) == 2 and int(flows[1]["rx_orphan"]) == 0
    assert int(stats[0]["recv_unmatched"]) == 1


def test_model_empty_sides():
    nf, send, recv = M.hand_case()
    none_s = M.cols(M.SEND_COLS, [])
    none_r = M.cols(M.RECV_COLS, [])
    cnt, first, rs, flows, stats = M.model(nf, send, none_r)
    assert not cnt.any() and (first == N).all() and len(rs) == 0
    assert flows["lost_head"].tolist() == flows["sent"].tolist() == [8, 2]
    assert flows["loss_runs"].tolist() == [1, 1] and flows["lost_tail"].tolist() == [0, 0]
    assert flows["lat_min"].tolist() == [2**63 - 1] * 2 and flows["lat_max"].tolist() == [-2**63] * 2
    assert flows[0]["loss_run_hist"].tolist() == [0, 0, 0, 1] + [0] * 14
    cnt, first, rs, flows, stats = M.model(nf, none_s, recv)
    assert (rs == N).all() and flows["rx_orphan"].tolist() == [4, 3]
    assert int(stats[0]["recv_unmatched"]) == 7 and not flows["sent"].any()


def test_layout_matches_header_and_symbols(tmp_path):
    import mgen_amd
    from mgen_amd import FLOW_MATCH_DTYPE, MATCH_STATS_DTYPE
    for s in ("mgenx_match_side", "mgenx_msg_match"):
        assert s in mgen_amd.EXPORTED_SYMBOLS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %zu %d %u %d\\n", sizeof(struct mgenx_flow_match), '
             'sizeof(struct mgenx_match_stats), MGENX_ABI_VERSION, MGENX_MATCH_NONE, '
             'MGENX_MATCH_NO_TIME);']
    for st, name, dt in (("flow", "mgenx_flow_match", FLOW_MATCH_DTYPE),
                         ("stats", "mgenx_match_stats", MATCH_STATS_DTYPE)):
        for f in dt.names:
            lines.append(f'printf("{st} {f} %zu\\n", offsetof(struct {name}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["256", "32", "1", str(0xFFFFFFFF), "1"]
    assert mgen_amd.MATCH_NONE == 0xFFFFFFFF == M.NONE and mgen_amd.MATCH_NO_TIME == 1
    assert FLOW_MATCH_DTYPE.itemsize == 256 == M.FLOW.itemsize
    assert MATCH_STATS_DTYPE.itemsize == 32 == M.STATS.itemsize
    assert FLOW_MATCH_DTYPE["loss_run_hist"].shape == (18,) == M.FLOW["loss_run_hist"].shape
    mine = {"flow": (FLOW_MATCH_DTYPE, M.FLOW), "stats": (MATCH_STATS_DTYPE, M.STATS)}
    seen = 0
    for line in out[1:]:
        if line:
            st, name, off = line.split()
            assert mine[st][0].fields[name][1] == int(off) == mine[st][1].fields[name][1], line
            seen += 1
    assert seen == len(M.FLOW.names) + len(M.STATS.names)


def test_bad_arguments_are_rejected_without_hip():
    from mgen_amd import load
    L = load()
    one = ctypes.c_void_p(16)     # a non-null pointer that is never followed
    assert L.mgenx_match_side(None, one, one, one, 4, 3, one, one, None) == -1
    send, recv, outs = (one,) * 5, (one,) * 6, (one,) * 5
    assert L.mgenx_msg_match(None, *send, 4, *recv, 4, 2, 0, *outs, None) == -1


def test_format_match_on_a_hand_made_array():
    from mgen_amd import FLOW_MATCH_DTYPE, REPORT_KEY_DTYPE
    from mgen_amd.match import format_match
    keys = np.zeros(3, REPORT_KEY_DTYPE)
    for f, fid in enumerate((7, 4000000000, 9)):
        keys[f]["flow_id"] = fid
        keys[f]["src"]["port"] = 5001
        keys[f]["dst"]["len"] = 4
        keys[f]["dst"]["port"] = 5000
        keys[f]["dst"]["addr"][:4] = (10, 0, 0, 9)
    keys[1]["dst"]["len"] = 16
    keys[1]["dst"]["addr"][:] = [0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1]
    flows = np.zeros(3, FLOW_MATCH_DTYPE)
    flows["lat_min"] = 2**63 - 1
    flows["lat_max"] = -2**63
    for k, v in dict(sent=8, delivered=2, rx_dup=1, rx_orphan=1, lost_head=1, lost_tail=2,
                     loss_runs=3, loss_run_max=3, lat_sum=651, lat_min=-50, lat_max=700).items():
        flows[0][k] = v
    for k, v in dict(sent=2**40, delivered=2**40, lat_sum=-3 * 2**40 + 1, lat_min=-7,
                     lat_max=2**53 + 1).items():
        flows[1][k] = v
    flows[2]["sent"] = flows[2]["lost_head"] = flows[2]["loss_run_max"] = 5
    flows[2]["loss_runs"] = 1
    assert format_match(keys, flows) == (
        "# flow dst sent delivered lost lost_head lost_tail rx_dup orphans loss_runs longest_run "
        "lat_mean lat_min lat_max\n"
        "7 10.0.0.9/5000 8 2 6 1 2 1 1 3 3 325 -50 700\n"
        "4000000000 2001:db8::1/5000 1099511627776 1099511627776 0 0 0 0 0 0 0 -3 -7 "
        "9007199254740993\n"
        "9 10.0.0.9/5000 5 0 5 5 0 0 0 1 5 - - -\n")
    assert format_match(keys[:0], flows[:0]) == (
        "# flow dst sent delivered lost lost_head lost_tail rx_dup orphans loss_runs longest_run "
        "lat_mean lat_min lat_max\n")
