"""Binary log ingest on the CPU side (include/mgenx.h, mgenx_binlog_parse): the plain-Python
model (binlog_parse_ref) against the text grammar checker over the oracle's conversion of the
same records, the product decoder and the record walk's stop rule (mgenx_binlogparse.hpp) as a
sanitized host program against the model, and the C entry points' argument checks."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import binlog_parse_ref as M
import binlog_util as B
import logparse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "binlog_parse_host")
LOG_EPOCH = 0x1
FIELDS = ("event", "status", "protocol", "present", "rx_sec", "rx_usec", "tx_sec", "tx_usec",
          "flow", "seq", "size", "ttl", "flags", "err", "gps", "lat_raw", "lon_raw", "alt")
EINVAL = -1


def tcp_send_cuts(oracle):
    """TCP SEND records whose stored message is cut right after the destination address, inside
    the host fields, inside the GPS fields, and whole (test_convert_tcp_send_bounded_at_the_
    record's records)."""
    m = oracle.make_msg(msg_len=300, flow_id=5, seq=77, tx_sec=1_700_000_000, tx_usec=5,
                        host=("4", bytes([10, 1, 2, 3]), 6000))
    full = oracle.udp_pack(m, checksum=False)
    parts = []
    for cut in (28, 30, 32, 36, 40, 60, len(full)):
        body = struct.pack(">I", 300) + full[:cut]
        parts.append(struct.pack(">BBH", 3, 2, len(body)) + body)
    return parts


def rejected_records(oracle):
    """RECV records whose stored message is shorter than a header and SEND records with a bad
    version / destination type / 12 bytes (test_convert_logs_rejected_stored_messages' corpus):
    (records, how many of the first are RECV)."""
    from streams import golden
    ADDR_DTYPE = oracle.ADDR_DTYPE
    gold = golden()
    f = gold["unpack_fields_udp"]
    short = np.nonzero((f["err"] == 0) & (f["hdr_len"].astype(int) + f["payload_len"] < 28))[0]
    assert short.size > 5
    src = np.zeros(short.size, ADDR_DTYPE)
    src["type"], src["len"], src["port"] = 1, 4, 4321
    src["addr"][:, :4] = [192, 168, 1, 7]
    rx_s = np.full(short.size, 1_700_000_123, np.uint32)
    rx_u = np.arange(short.size, dtype=np.uint32) * 11
    recs = oracle.log_recv_binary(f[short], gold["unpack_slab"], gold["unpack_offs"][short], src,
                                  rx_s, rx_u, protocol=1)
    out = M.split_records(bytes(recs), 0)
    assert len(out) == short.size
    for proto, body in ((1, bytes([0, 64, 3]) + bytes(61)),
                        (2, struct.pack(">I", 9000) + bytes([0, 64, 2, 4]) + bytes(16) +
                         bytes([0, 0, 9, 4]) + bytes(40)),
                        (3, bytes(12))):
        out.append(struct.pack(">BBH", 3, proto, len(body)) + body)
    return out, int(short.size)


@pytest.fixture(scope="module")
def corpus(oracle):
    """The records every route agrees on: RECV (IPv4 / IPv6 sources, every protocol), SEND (UDP,
    SINK and TCP, whole and cut), every other event, RECV with MGEN_DATA reports."""
    rng = np.random.default_rng(21)
    return (B.recv_records(oracle, n=400) + B.send_records(oracle, n=200) + B.events(rng) +
            B.data_recv_records(oracle, n=60) + tcp_send_cuts(oracle))


def _same(got, want, skip=()):
    for k in want:
        if k in skip or k == "kind":
            continue
        if got[k] != want[k]:
            return f"{k}: {got[k]!r} != {want[k]!r}"
    return None


def test_model_matches_the_text_route(oracle, corpus):
    """The model == logparse_ref.parse_line over the oracle's epoch conversion, field for field
    except ttl (the converter prints its flush flag there)."""
    text, st, n = oracle.convert_binary_log(B.binlog(corpus), opts=LOG_EPOCH)
    assert st == 0 and n == len(corpus)
    lines = [ln for ln in R.split_lines(text) if b" REPORT " not in ln]
    assert len(lines) == len(corpus)
    seen = set()
    rejected = 0
    for k, (rec, line) in enumerate(zip(corpus, lines)):
        want = R.parse_line(line)
        got = M.parse_record(rec)
        if rec[0] == 1 and len(rec) - 16 - rec[15] < 28:
            # a golden-matrix message whose stored bytes (header + payload) are fewer than a
            # header: Unpack rejects it, the converter logs a fresh MgenMsg (the contract's
            # "rejected message"); every other record of the corpus is compared in full
            assert got["status"] == R.MALFORMED and got["event"] == 1 == want["event"], k
            assert b" flow>0 seq>0 " in line
            rejected += 1
            continue
        assert want["status"] == R.OK, (k, line)
        assert want["event"] != R.RECV or (want["ttl"] == 0 and want["present"] & R.HAS_TTL)
        want["ttl"] = -1
        want["present"] &= ~R.HAS_TTL
        bad = _same(got, want)
        assert bad is None, (k, bad, line)
        seen.add(want["event"])
    assert seen == set(range(1, 17)) - {2} and rejected < 40
    # the corpus reaches the optional fields
    recs = [M.parse_record(r) for r in corpus]
    for bit in (R.HAS_HOST, R.HAS_GPS, R.HAS_DATA, R.HAS_FLAGS):
        assert any(r["present"] & bit for r in recs), bit
    assert any(r["src"][0] == 2 for r in recs) and any(r["protocol"] == 2 for r in recs)


def test_model_exceptions(oracle):
    """What the contract decides from the bytes where the text route differs."""
    recs, n_recv = rejected_records(oracle)
    for k, rec in enumerate(recs):
        r = M.parse_record(rec)
        assert r["status"] == R.MALFORMED and r["event"] == (1 if k < n_recv else 3), k
    good = bytearray(B.recv_records(oracle, n=1)[0])
    mo = 16 + good[15]
    base = M.parse_record(bytes(good))
    assert base["status"] == R.OK and base["err"] == 0 and base["ttl"] == -1
    big = bytearray(good)
    big[mo + 16:mo + 20] = struct.pack(">I", 2_000_000)     # tx_usec the text grammar refuses
    r = M.parse_record(bytes(big))
    assert r["status"] == R.OK and r["tx_usec"] == 2_000_000
    bad_src = bytearray(good)
    bad_src[14] = 3 - bad_src[14]                           # the other type with this length
    assert M.parse_record(bytes(bad_src))["status"] == R.MALFORMED
    st = M.parse_record(B.start(7, 3_000_000))
    assert st["status"] == R.OK and (st["rx_sec"], st["rx_usec"]) == (7, 3_000_000)
    assert st["err"] == R.ERROR_NOT_RECV and st["protocol"] == 0
    send = M.parse_record(tcp_send_cuts(oracle)[-1])
    assert send["src"] == R.NO_ADDR and send["size"] == 300 and send["tx_sec"] == 0
    assert (send["rx_sec"], send["rx_usec"]) == (1_700_000_000, 5) and send["err"] == 0x20


def _host_rows(tmp_path, pieces):
    if not os.path.exists(HOST):      # as the other tests/cpp programs: built on demand
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/binlog_parse_host"], check=True)
    assert os.path.exists(HOST), "tests/cpp/binlog_parse_host not built (make all)"
    p = tmp_path / "pieces.bin"
    p.write_bytes(b"".join(struct.pack("<I", len(x)) + x for x in pieces))
    r = subprocess.run([HOST, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]        # a sanitizer report exits non-zero
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    out = []
    for row in r.stdout.splitlines():
        t = row.split(" ")
        d = dict(walk=int(t[0]), step=int(t[1]))
        d.update(zip(FIELDS, map(int, t[2:20])))
        for k, name in enumerate(("src", "dst", "host")):
            a = t[21 + k].split(":")
            d[name] = (int(a[0]), int(a[1]), int(a[2]), bytes.fromhex(a[3]))
        d["data"] = b"" if t[24] == "-" else bytes.fromhex(t[24])
        out.append(d)
    return out


def test_host_decoder_matches_the_model(oracle, corpus, tmp_path):
    """mgenx_binlogparse.hpp under ASan / UBSan, each record in an allocation of exactly its own
    bytes: the corpus, the rejected stored messages, records short for their type, cut records,
    and the stops of the record walk."""
    from test_binlog_cpu import short_for_type_cases
    stops = [struct.pack(">BBH", 2, 0, 20) + bytes(20), B.ev_time(40, 1, 1),
             struct.pack(">BBH", 8, 0, 1025) + bytes(1025), B.stop(5, 5)[:-2], b"\x08", b""]
    badaddr = bytearray(B.conn(10, 1, 1, bytes(4), 1, 1, 1))
    badaddr[14] = 7
    recv = corpus[0]
    cuts = [recv[:k] for k in (3, 4, 11, 16, 20, len(recv) - 1)]
    pieces = (list(corpus) + rejected_records(oracle)[0] +
              [rec for _, rec in short_for_type_cases()] + stops + [bytes(badaddr)] + cuts)
    rows = _host_rows(tmp_path, pieces)
    assert len(rows) == len(pieces)
    verdicts = set()
    for k, (rec, got) in enumerate(zip(pieces, rows)):
        want = M.parse_record(rec)
        walk, step = M.walk_step(rec)
        assert (got["walk"], got["step"]) == (walk, step), k
        verdicts.add(walk)
        if want["status"] == R.OK:
            bad = _same(got, want)
            assert bad is None, (k, bad)
        else:
            assert got["status"] == R.MALFORMED and got["event"] == want["event"], k
    assert verdicts == {M.WALK_NEXT, M.WALK_END, M.BINLOG_TOO_LONG, M.BINLOG_EVENT, M.BINLOG_SHORT}


def test_walk_rule_matches_the_host_index(oracle):
    """The model's walk rule chained over whole logs == mgenx_binlog_index (status, count,
    consumed), on the stop cases of test_binlog_cpu."""
    import mgen_amd
    from test_binlog_cpu import short_for_type_cases
    parts = [B.start(1, 2), B.listen(1, 3, 1, 7)] + B.recv_records(oracle, n=5)
    bads = [rec for _, rec in short_for_type_cases()] + [
        struct.pack(">BBH", 2, 0, 20) + bytes(20), B.ev_time(40, 1, 1),
        struct.pack(">BBH", 8, 0, 1025) + bytes(1025), B.stop(5, 5)[:-2], b"", b"\x01\x02\x03"]
    for bad in bads:
        log = B.binlog(parts + [bad])
        offs, info = mgen_amd.binlog_index(log)
        at, n, st = len(B.HEADER), 0, M.WALK_NEXT
        while True:
            st, step = M.walk_step(log[at:at + 1028], len(log) - at)
            if st != M.WALK_NEXT:
                break
            assert offs[n] == at
            n, at = n + 1, at + step
        assert (n, at) == (info.n_records, info.consumed)
        assert info.status == (0 if st == M.WALK_END else st)


def test_entry_points_reject_null_arguments():
    import mgen_amd
    L = mgen_amd.load()
    info = mgen_amd.BinlogInfo()
    buf = (ctypes.c_uint8 * 8)()
    assert L.mgenx_binlog_header(None, 8, ctypes.byref(info)) == EINVAL
    assert L.mgenx_binlog_header(buf, 8, None) == EINVAL
    out = mgen_amd.LogparseOut()
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: the checks come first
    assert L.mgenx_binlog_parse(None, fake, 8, fake, 1, 0, ctypes.byref(out), None) == EINVAL
    assert L.mgenx_binlog_parse(fake, fake, 8, fake, 1, 0, None, None) == EINVAL
    assert L.mgenx_binlog_parse(fake, fake, 8, fake, 1, 0, ctypes.byref(out), None) == EINVAL
    out.event = out.status = 0x1000
    assert L.mgenx_binlog_parse(fake, None, 8, fake, 1, 0, ctypes.byref(out), None) == EINVAL
    assert L.mgenx_binlog_parse(fake, fake, 8, None, 1, 0, ctypes.byref(out), None) == EINVAL
    assert L.mgenx_binlog_parse(fake, fake, 8, fake, 1, 1, ctypes.byref(out), None) == EINVAL
    out.payload_cap = 4
    assert L.mgenx_binlog_parse(fake, fake, 8, fake, 1, 0, ctypes.byref(out), None) == EINVAL
    out.payload_cap, out.payload = 0, 0x1000
    assert L.mgenx_binlog_parse(fake, fake, 8, fake, 1, 0, ctypes.byref(out), None) == EINVAL


def test_binlog_header_rules():
    """mgenx_binlog_header reproduces test_binlog_cpu.test_header_rules' table."""
    import mgen_amd
    for hdr, ok in [(B.HEADER, True), (b"mgen version=4.2 type=binary_log\n\0", True),
                    (b"mgen version=3.0 type=binary_log\n\0", False),
                    (b"mgen version=5.1.1 type=text_log\n\0", False),
                    (b"MGEN version=5 type=binary_log\n\0", False),
                    (b"mgen type=binary_log\n\0", False), (b"mgen version=5 type=binary_log", False)]:
        log = hdr + B.start(1, 1)
        info = mgen_amd.binlog_header(log)
        _, full = mgen_amd.binlog_index(log)
        assert (info.status == 0) == ok == (full.status == 0), hdr
        assert info.status in (0, 1) and info.n_records == 0
        assert mgen_amd.is_binary_log(log) == ok
        if ok:
            assert info.consumed == len(hdr) and info.version == full.version
    assert not mgen_amd.is_binary_log(b"") and not mgen_amd.is_binary_log(b"12.000001 START\n")
