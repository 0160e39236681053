"""The crafted binary log records (binlog_cases) on the CPU: the plain-Python model
(binlog_parse_ref) against the oracle's text route, record by record with the exceptions
written out by name; what the corpus must reach (a field on each side of byte 128, the chunk
lengths, the four phases of the payload start); and the product decoder
(mgenx_binlogparse.hpp) as a sanitized host program, whole view and split view, over the
corpus and over a "record" at every byte offset of a log."""
import binlog_cases as C
import binlog_parse_ref as M
import binlog_util as B
import logparse_ref as R
from test_binlog_parse_cpu import LOG_EPOCH, _host_rows, _same


def _malformed_by_design(name):
    """The records the contract calls MALFORMED: stored messages Unpack rejects (version,
    destination type, fewer than 28 bytes), address lengths that do not fit their type, and the
    record longer than the reference's read buffer."""
    part = name.split(":")
    return (part[0] in ("reject", "mismatch", "too_long") or
            (part[0] == "cut" and int(part[2]) < 28))


def test_crafted_model_matches_the_text_route(oracle):
    """parse_record == logparse_ref.parse_line over the oracle's epoch conversion of the same
    records, field for field except ttl (the converter prints its flush flag there).  The text
    route may refuse only the tx_usec >= 10^6 records; the model may call MALFORMED only the
    named rejects, the named mismatches (their lines print "(invalid)"), the cuts below 28
    bytes and the TOO_LONG record, which also stops the converter's walk."""
    crafted = C.crafted()
    text, st, n = oracle.convert_binary_log(B.binlog([r for _, r in crafted]), opts=LOG_EPOCH)
    assert st == M.BINLOG_TOO_LONG and n == len(crafted) - 1
    lines = [ln for ln in R.split_lines(text) if b" REPORT " not in ln]
    assert len(lines) == n
    bad = []
    for (name, rec), line in zip(crafted, lines):
        want, got = R.parse_line(line), M.parse_record(rec)
        assert got["event"] == want["event"] == rec[0], name
        assert (got["status"] == R.MALFORMED) == _malformed_by_design(name), name
        if got["status"] == R.MALFORMED:
            if name.startswith("mismatch"):
                assert b"(invalid)" in line, (name, line)
            continue
        if want["status"] != R.OK:
            assert name.startswith("tx_usec>=1e6"), (name, line)
            assert got["tx_usec"] == 2_000_000 or got["rx_usec"] == 2_000_000, name
            continue
        if rec[0] == R.RECV:
            assert want["ttl"] == 0 and want["present"] & R.HAS_TTL, name
            want["ttl"] = -1
            want["present"] &= ~R.HAS_TTL
        diff = _same(got, want)
        if diff:
            bad.append((name, diff))
    assert not bad, (len(bad), bad[:40])
    last, rec = crafted[-1]
    got = M.parse_record(rec)
    assert last == "too_long:1029" and (got["status"], got["event"]) == (R.MALFORMED, 1)
    assert sum(name.startswith("tx_usec>=1e6") for name, _ in crafted) == 2


def test_cut_destination_keeps_its_declared_length():
    """A destination cut by the end of the stored message (lengths 28 .. 39 of an IPv6 one):
    length 16, the bytes present, zero fill -- RECV, TCP SEND and UDP SEND."""
    by_name = dict(C.crafted())
    whole = M.parse_record(by_name["cut:recv6:116"])["dst"]
    assert whole[:2] == (2, 16) and 0 not in whole[3]
    for kind in ("recv6", "send_tcp", "send_udp"):
        for c in range(28, 41):
            r = M.parse_record(by_name[f"cut:{kind}:{c}"])
            have = min(c - 24, 16)
            assert r["status"] == R.OK, (kind, c)
            assert r["dst"] == (2, 16, whole[2], whole[3][:have] + bytes(16 - have)), (kind, c)
            assert r["host"] == R.NO_ADDR and not r["present"] & R.HAS_HOST


def test_crafted_corpus_covers_its_points():
    crafted = C.crafted()
    parsed = {name: M.parse_record(rec) for name, rec in crafted}
    # record offset 128 on every trailer byte, for each record kind
    hit = {kind: set() for kind in C.KINDS}
    plen_past = data_across = False
    for name, rec in crafted:
        lay = C.layout(rec)
        if lay is None or parsed[name]["status"] != R.OK:
            continue
        mo, D, H, T = lay
        kind = ("recv4" if rec[15] == 4 else "recv6") if rec[0] == 1 else \
            ("send_tcp" if rec[1] == 2 else "send_udp")
        if T <= 128 < T + C.TRAILER:
            assert rec[mo + 26 + D] not in (1, 2), name      # only an unknown host type gets here
            hit[kind].add(128 - T)
            body = rec[T:T + C.TRAILER]
            assert 0 not in body[:13] and 0 not in body[14:] and len(set(body)) == 16, name
        if T + 14 >= 128 and parsed[name]["data"]:
            plen_past = True
        if parsed[name]["data"]:
            start = mo + (T + C.TRAILER - mo) // 4 * 4
            assert rec[start:start + len(parsed[name]["data"])] == parsed[name]["data"], name
            if start < 128 < start + len(parsed[name]["data"]):
                data_across = True
    assert all(hit[kind] == set(range(16)) for kind in C.KINDS), hit
    assert plen_past and data_across
    # whole records of 16 k and 16 k +- 1 bytes, each OK; the short end; the largest record
    lengths = {len(rec) for name, rec in crafted if parsed[name]["status"] == R.OK}
    assert set(C.CHUNK_LENGTHS) <= lengths and {12, 1028} <= lengths
    assert {0, 1, 15} <= {n % 16 for n in lengths}
    assert any(12 <= len(rec) <= 60 and rec[0] not in (1, 3) for _, rec in crafted)
    big = parsed["largest:1028"]
    assert len(big["data"]) == 1028 - C.RECV_FULL and big["present"] & R.HAS_DATA
    # The payload starts at the word-floored end of plen, counted from the message's start.
    # The message itself starts at a multiple of 4 (16 + 4 or 16 + 16, or 4 / 8 in a SEND), so
    # the start's own low bits are always 0; what varies is how far before the end of plen it
    # lies.  H = 0 .. 3 share every byte up to the host length and show all four distances.
    phases = {}
    for H in (0, 1, 2, 3):
        rec = dict(crafted)[f"phase:recv4:H{H}"]
        mo, D, h, T = C.layout(rec)
        assert h == H and rec[4:mo + 27 + D] == dict(crafted)["phase:recv4:H0"][4:mo + 27 + D]
        data = parsed[f"phase:recv4:H{H}"]["data"]
        start = rec.index(data[:16], mo)
        assert rec[start:start + len(data)] == data and len(data) == 0x0102
        phases[H] = T + C.TRAILER - start
    assert sorted(phases.values()) == [0, 1, 2, 3], phases
    assert parsed["phase:recv4:H255"]["status"] == R.OK and parsed["phase:recv4:H255"]["data"]
    # the SEND size rules
    assert parsed["value:tcp_len:65536"]["size"] == 65536
    assert parsed["value:tcp_len:4294967295"]["size"] == 0xFFFFFFFF


def _check_rows(pieces, rows):
    assert len(rows) == len(pieces)
    ok = 0
    for k, (rec, got) in enumerate(zip(pieces, rows)):
        want = M.parse_record(rec)
        assert (got["walk"], got["step"]) == M.walk_step(rec), k
        if want["status"] == R.OK:
            ok += 1
            diff = _same(got, want)
            assert diff is None, (k, diff)
        else:
            assert got["status"] == R.MALFORMED and got["event"] == want["event"], k
    return ok


def test_host_decoder_on_crafted_records(tmp_path):
    """The product decoder under ASan / UBSan over the crafted records, whole view and split
    view (the program exits non-zero when the two differ), against the model."""
    pieces = [rec for _, rec in C.crafted()]
    ok = _check_rows(pieces, _host_rows(tmp_path, pieces))
    assert ok == sum(M.parse_record(p)["status"] == R.OK for p in pieces) > 300


def test_host_decoder_at_every_offset(tmp_path):
    """A "record" at every byte offset of a log, each with the bytes the contract says it owns:
    thousands of garbage headers, overlapping and cut records."""
    buf, offs, _ = C.edge_log()
    pieces = [C.owned(buf, at) for at in range(len(buf) + 1)]
    assert all(pieces[at] == buf[at:at + len(pieces[at])] for at in offs)
    ok = _check_rows(pieces, _host_rows(tmp_path, pieces))
    true_ok = sum(M.parse_record(pieces[at])["status"] == R.OK for at in set(offs))
    assert ok > true_ok > 100        # the true records and some the garbage happens to form
