"""The timeline of mgenx_msg_match_ex without a GPU: the serial model (tests/match_timeline_ref.py)
on the case worked by hand, the ABI layout against a C probe, argument checks, and the two
formatters of mgen_amd.match_series on hand-made arrays."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_timeline_ref as TL  # noqa: E402
import msg_match_ref as M  # noqa: E402

N = M.NONE
MAX, MIN = 2**63 - 1, -2**63
FIELDS = ("sent", "sent_bytes", "delivered", "delivered_bytes", "rx_dup", "lat_sum", "lat_min",
          "lat_max")
EMPTY = (0, 0, 0, 0, 0, 0, MAX, MIN)
US = 10**9           # the hand case's t_sec in microseconds


def cell(c):
    return tuple(int(c[k]) for k in FIELDS)


def run_tuples(runs):
    return [(int(r["flow_idx"]), int(r["length"]), int(r["first_send"]), int(r["last_send"]),
             int(r["flags"])) for r in runs]


def test_model_on_the_hand_case():
    nf, send, recv = M.hand_case()
    base, owner, bins, outside, runs = TL.model(nf, send, recv, 1_000_000_100, 250, 3, 1)
    assert owner.tolist() == [0, 1, 2, 3, 4, N, 6, 1, 8, 9, 10, 11]
    # flow 0: owners 0 1 3 (100 200 300 us) | 4 6 (400 500) | 8 10 11 (600 700 800)
    assert cell(bins[0][0]) == (3, 192, 1, 64, 1, 700, 700, 700)
    assert cell(bins[0][1]) == (2, 128, 0, 0, 0, 0, MAX, MIN)
    assert cell(bins[0][2]) == (3, 256, 1, 128, 0, -50, -50, -50)
    # flow 1: owner 2 (250 us, delivered twice) | - | owner 9 (650 us)
    assert cell(bins[1][0]) == (1, 100, 1, 100, 1, 999800, 999800, 999800)
    assert cell(bins[1][1]) == EMPTY
    assert cell(bins[1][2]) == (1, 100, 0, 0, 0, 0, MAX, MIN)
    assert outside.tolist() == [0, 0]
    assert run_tuples(runs) == [(0, 1, 0, 0, TL.HEAD), (0, 3, 3, 6, 0), (0, 2, 10, 11, TL.TAIL),
                                (1, 1, 9, 9, TL.TAIL)]
    usec = [int(x) for x in send["t_usec"]]
    assert runs["t_first_us"].tolist() == [US + usec[i] for i in (0, 3, 10, 9)]
    assert runs["t_last_us"].tolist() == [US + usec[i] for i in (0, 6, 11, 9)]
    assert not runs["rsv"].any()
    # the bins sum to the flow totals, and the count of runs is the flows' loss_runs
    flows = base[3]
    for f in range(nf):
        for k in ("sent", "sent_bytes", "delivered", "delivered_bytes", "rx_dup", "lat_sum"):
            assert int(bins[f][k].sum()) == int(flows[f][k]), (f, k)
        assert int(bins[f]["lat_min"].min()) == int(flows[f]["lat_min"])
        assert int(bins[f]["lat_max"].max()) == int(flows[f]["lat_max"])
    assert len(runs) == int(flows["loss_runs"].sum())


def test_model_fewer_windows_and_longer_runs():
    nf, send, recv = M.hand_case()
    _, _, bins, outside, runs = TL.model(nf, send, recv, 1_000_000_100, 250, 2, 2)
    assert outside.tolist() == [3, 1] and bins.shape == (2, 2)
    assert cell(bins[0][0]) == (3, 192, 1, 64, 1, 700, 700, 700)
    assert run_tuples(runs) == [(0, 3, 3, 6, 0), (0, 2, 10, 11, TL.TAIL)]
    # min_run 0 is taken as 1; no windows: no series
    _, _, bins, outside, runs = TL.model(nf, send, recv, 0, 1, 0, 0)
    assert bins.shape == (2, 0) and outside.tolist() == [0, 0] and len(runs) == 4


def test_model_never_delivered_and_negative_floor():
    nf, send, recv = M.hand_case()
    none_r = M.cols(M.RECV_COLS, [])
    _, _, bins, outside, runs = TL.model(nf, send, none_r, 1_000_000_101, 1000, 1, 1)
    assert run_tuples(runs) == [(0, 8, 0, 11, TL.HEAD | TL.TAIL), (1, 2, 2, 9, TL.HEAD | TL.TAIL)]
    assert outside.tolist() == [1, 0]            # send 0 is 1 us before t0: floor -1
    assert cell(bins[0][0]) == (7, 6 * 64 + 128, 0, 0, 0, 0, MAX, MIN)


def test_layout_matches_header_and_symbols(tmp_path):
    import mgen_amd
    from mgen_amd import LOSS_RUN_DTYPE, MATCH_BIN_DTYPE, MatchTimeline
    assert "mgenx_msg_match_ex" in mgen_amd.EXPORTED_SYMBOLS
    host = ("t0_us", "width_us", "n_bins", "min_run", "dev_bins", "dev_outside", "dev_runs",
            "run_cap", "dev_n_runs", "dev_send_owner")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgenx.h"', 'int main(){',
             'printf("%zu %zu %zu %d %d %d\\n", sizeof(struct mgenx_match_bin), '
             'sizeof(struct mgenx_loss_run), sizeof(mgenx_match_timeline), MGENX_ABI_VERSION, '
             'MGENX_RUN_HEAD, MGENX_RUN_TAIL);']
    for st, name, names in (("bin", "struct mgenx_match_bin", MATCH_BIN_DTYPE.names),
                            ("run", "struct mgenx_loss_run", LOSS_RUN_DTYPE.names),
                            ("tl", "mgenx_match_timeline", host)):
        for f in names:
            lines.append(f'printf("{st} {f} %zu\\n", offsetof({name}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["64", "40", str(ctypes.sizeof(MatchTimeline)), "1", "1", "2"]
    assert mgen_amd.RUN_HEAD == 1 == TL.HEAD and mgen_amd.RUN_TAIL == 2 == TL.TAIL
    assert MATCH_BIN_DTYPE.itemsize == 64 == TL.BIN.itemsize
    assert LOSS_RUN_DTYPE.itemsize == 40 == TL.RUN.itemsize
    assert [n for n, _ in MatchTimeline._fields_] == list(host)
    seen = 0
    for line in out[1:]:
        if not line:
            continue
        st, name, off = line.split()
        if st == "tl":
            assert getattr(MatchTimeline, name).offset == int(off), line
        else:
            mine, ref = {"bin": (MATCH_BIN_DTYPE, TL.BIN), "run": (LOSS_RUN_DTYPE, TL.RUN)}[st]
            assert mine.fields[name][1] == int(off) == ref.fields[name][1], line
        seen += 1
    assert seen == len(TL.BIN.names) + len(TL.RUN.names) + len(host)


def test_bad_arguments_are_rejected_without_hip():
    from mgen_amd import MatchTimeline, load
    L = load()
    one = ctypes.c_void_p(16)     # a non-null pointer that is never followed
    send, recv, outs = (one,) * 5, (one,) * 6, (one,) * 5
    tl = MatchTimeline(t0_us=0, width_us=1, n_bins=1, dev_bins=16, dev_outside=16)
    assert L.mgenx_msg_match_ex(None, *send, 4, *recv, 4, 2, 0, *outs, ctypes.byref(tl),
                                None) == -1


def _keys():
    from mgen_amd import REPORT_KEY_DTYPE
    keys = np.zeros(2, REPORT_KEY_DTYPE)
    for f, fid in enumerate((7, 4000000000)):
        keys[f]["flow_id"] = fid
        keys[f]["src"]["port"] = 5001
        keys[f]["dst"]["len"] = 4
        keys[f]["dst"]["port"] = 5000
        keys[f]["dst"]["addr"][:4] = (10, 0, 0, 9)
    keys[1]["dst"]["len"] = 16
    keys[1]["dst"]["addr"][:] = [0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1]
    return keys


def test_format_match_series_on_a_hand_made_array():
    from mgen_amd import MATCH_BIN_DTYPE
    from mgen_amd.match_series import format_match_series
    bins = np.zeros((2, 3), MATCH_BIN_DTYPE)
    bins["lat_min"], bins["lat_max"] = MAX, MIN
    for k, v in zip(FIELDS, (3, 192, 1, 64, 1, 700, 700, 700)):
        bins[0][0][k] = v
    for k, v in zip(FIELDS, (2, 128, 0, 0, 0, 0, MAX, MIN)):
        bins[0][2][k] = v
    for k, v in zip(FIELDS, (2**40, 2**50, 2**40, 2**50, 0, -3 * 2**40 + 1, -7, 2**53 + 1)):
        bins[1][1][k] = v
    hdr = ("# bin_start_us sent sent_bytes delivered delivered_bytes lost rx_dup lat_min lat_max "
           "lat_sum\n")
    assert format_match_series(_keys(), bins, -100, 2**33) == (
        "# flow>7 src>-/5001 dst>10.0.0.9/5000\n" + hdr +
        "-100 3 192 1 64 2 1 700 700 700\n"
        "17179869084 2 128 0 0 2 0 - - -\n"
        "\n\n"
        "# flow>4000000000 src>-/5001 dst>2001:db8::1/5000\n" + hdr +
        "8589934492 1099511627776 1125899906842624 1099511627776 1125899906842624 0 0 -7 "
        "9007199254740993 -3298534883327\n")
    assert format_match_series(_keys()[:0], bins[:0], 0, 1) == ""


def test_format_runs_on_a_hand_made_array():
    from mgen_amd import LOSS_RUN_DTYPE
    from mgen_amd.match_series import format_runs
    runs = np.zeros(3, LOSS_RUN_DTYPE)
    runs[0] = (0, 1, 0, 0, 1, 0, US + 100, US + 100)
    runs[1] = (0, 4000, 3, 4_000_000_000, 0, 0, US + 300, 2**53 + 1)
    runs[2] = (1, 2, 9, 11, 3, 0, -5, US)
    hdr = "# flow dst length first_send_us last_send_us first_line last_line head tail\n"
    assert format_runs(_keys(), runs) == (
        hdr +
        "7 10.0.0.9/5000 1 1000000100 1000000100 1 1 1 0\n"
        "7 10.0.0.9/5000 4000 1000000300 9007199254740993 4 4000000001 0 0\n"
        "4000000000 2001:db8::1/5000 2 -5 1000000000 10 12 1 1\n")
    assert format_runs(_keys(), runs[:0]) == hdr
