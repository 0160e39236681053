"""GPU, end to end: three tiny text logs through match_text_logs_multi with min_run / pairs and
through python -m mgen_amd.match_multi -r / -p, against numbers worked out by hand.

One flow of 12 messages, seq 0 .. 11, message i sent 100 i ms after T0 + 1 s; the sender's log
has a START line first, so message i is line i + 2 of it (1-based).
  receiver 0 misses messages 4 5 and 9;
  receiver 1 misses exactly what receiver 0 does;
  receiver 2 joins late (its first message is 3) and misses 5 and 7.
Runs: receivers 0 and 1 have {4 5} and {9}: 2 runs, the longest 2.  Receiver 2 has the head
{0 1 2}, {5} and {7}: 3 runs, the longest 3.
Pairs: the spans are 0 .. 11, 0 .. 11 and 3 .. 11.  (0, 1): 12 messages, each lost 3, both 3:
cond 1.  (0, 2) over 3 .. 11: 9 messages, receiver 0 lost 4 5 9, receiver 2 lost 5 7, both 5:
cond 1 / 3 for (0, 2) and 1 / 2 for (2, 0)."""
import pytest

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000
N = 12
DST = "224.225.1.2/5000"


def stamp(i):
    return (T0 + 1) * 10**6 + i * 100_000


def text_logs():
    send = ["%d.000000 START Mgen Version 5.02b\n" % T0]
    for i in range(N):
        t = stamp(i)
        send.append("%d.%06d SEND proto>UDP flow>1 seq>%d srcPort>5001 dst>%s size>64\n" % (
            t // 10**6, t % 10**6, i, DST))
    hears = [[i for i in range(N) if i not in (4, 5, 9)],
             [i for i in range(N) if i not in (4, 5, 9)],
             [i for i in range(3, N) if i not in (5, 7)]]
    recvs = []
    for r, got in enumerate(hears):
        lines = ["%d.000000 JOIN group>224.225.1.2\n" % T0]
        for i in got:
            t, rx = stamp(i), stamp(i) + 250 + 10 * r
            lines.append("%d.%06d RECV proto>UDP flow>1 seq>%d src>10.0.0.1/5001 dst>%s "
                         "sent>%d.%06d size>64 \n" % (rx // 10**6, rx % 10**6, i, DST,
                                                      t // 10**6, t % 10**6))
        recvs.append("".join(lines).encode())
    return "".join(send).encode(), recvs


def test_match_text_logs_multi_with_runs_and_pairs():
    from mgen_amd import match_text_logs_multi
    send, recvs = text_logs()
    plain = match_text_logs_multi(send, recvs)
    assert len(plain) == 6
    res = match_text_logs_multi(send, recvs, min_run=1, pairs=True)
    assert len(res) == 9
    for a, b in zip(plain, res[:6]):               # what stood there before is unchanged
        assert bytes(memoryview(a.tobytes() if hasattr(a, "tobytes") else bytes([a]))) == \
            bytes(memoryview(b.tobytes() if hasattr(b, "tobytes") else bytes([b])))
    keys, cells, fanout = res[0], res[1], res[2]
    rcv_runs, runs, pairs = res[6:]
    assert keys["flow_id"].tolist() == [1] and int(fanout[0]["sent"]) == N
    assert cells["lost_head"].tolist() == [[0, 0, 3]]
    assert rcv_runs.shape == (1, 3) and pairs.shape == (1, 3, 3)
    assert rcv_runs["loss_runs"].tolist() == [[2, 2, 3]]
    assert rcv_runs["loss_run_max"].tolist() == [[2, 2, 3]]
    assert rcv_runs["loss_run_hist"][0, 2].tolist() == [2, 1] + [0] * 16
    # by flow, last_send, rcv; first_send / last_send are 0-based lines of the sender's log
    rows = [(int(r["rcv"]), int(r["length"]), int(r["first_send"]), int(r["last_send"]),
             int(r["flags"]), int(r["t_first_us"]), int(r["t_last_us"])) for r in runs]
    assert rows == [
        (2, 3, 1, 3, 1, stamp(0), stamp(2)),
        (0, 2, 5, 6, 0, stamp(4), stamp(5)),
        (1, 2, 5, 6, 0, stamp(4), stamp(5)),
        (2, 1, 6, 6, 0, stamp(5), stamp(5)),
        (2, 1, 8, 8, 0, stamp(7), stamp(7)),
        (0, 1, 10, 10, 0, stamp(9), stamp(9)),
        (1, 1, 10, 10, 0, stamp(9), stamp(9)),
    ]
    as_tuples = [[tuple(int(v) for v in pairs[0, a, b]) for b in range(3)] for a in range(3)]
    assert as_tuples == [
        [(12, 3, 3, 3), (12, 3, 3, 3), (9, 3, 2, 1)],
        [(12, 3, 3, 3), (12, 3, 3, 3), (9, 3, 2, 1)],
        [(9, 2, 3, 1), (9, 2, 3, 1), (9, 2, 2, 2)],
    ]
    # each keyword alone appends its own results only
    only_runs = match_text_logs_multi(send, recvs, min_run=2)
    assert len(only_runs) == 8 and [int(r["length"]) for r in only_runs[7]] == [3, 2, 2]
    only_pairs = match_text_logs_multi(send, recvs, pairs=True, width_us=500_000)
    assert len(only_pairs) == 10 and only_pairs[9].tobytes() == pairs.tobytes()


def test_the_command_line_options(tmp_path, capsys):
    from mgen_amd.match_multi import main
    send, recvs = text_logs()
    paths = []
    for name, log in zip(("send", "r0", "r1", "r2"), [send] + recvs):
        (tmp_path / name).write_bytes(log)
        paths.append(str(tmp_path / name))
    capsys.readouterr()
    assert main(paths) == 0
    plain = capsys.readouterr().out
    assert "loss_runs" not in plain and "lost_both" not in plain

    assert main(["-p"] + paths) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)                  # -p only appends
    assert out[len(plain):].split("\n") == [
        "", "",
        "# flow dst a b span lost_a lost_b lost_both cond",
        "1 %s 0 1 12 3 3 3 1.000000" % DST,
        "1 %s 0 2 9 3 2 1 0.333333" % DST,
        "1 %s 1 0 12 3 3 3 1.000000" % DST,
        "1 %s 1 2 9 3 2 1 0.333333" % DST,
        "1 %s 2 0 9 2 3 1 0.500000" % DST,
        "1 %s 2 1 9 2 3 1 0.500000" % DST,
        ""]

    assert main(["-r", "2"] + paths) == 0
    out = capsys.readouterr().out.split("\n")
    was = plain.split("\n")
    assert out[0] == was[0] + " loss_runs longest_run"
    assert [o[len(w):] for o, w in zip(out[1:4], was[1:4])] == [" 2 2", " 2 2", " 3 3"]
    assert out[4:len(was) - 1] == was[4:-1]       # the reach histogram as before
    assert out[len(was) - 1:] == [
        "", "",
        "# flow dst rcv length first_line last_line t_first_us t_last_us head tail",
        "1 %s 0 2 6 7 %d %d 0 0" % (DST, stamp(4), stamp(5)),
        "1 %s 1 2 6 7 %d %d 0 0" % (DST, stamp(4), stamp(5)),
        "1 %s 2 3 2 4 %d %d 1 0" % (DST, stamp(0), stamp(2)),
        ""]

    assert main(["-n", "-r", "1", "-p"] + paths) == 0
    out = capsys.readouterr().out
    assert out.count("\n1 %s 2 1 " % DST) == 3    # receiver 2: two short runs, one pair row
    assert main(["-r", "x"] + paths) == 2 and main(["-r"]) == 2
