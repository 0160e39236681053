"""CPU: the text log ingest's line grammar.  (a) the plain-Python checker (tests/
logparse_ref.py) reads back every field of the oracle's RECV / RERR lines over the golden
unpack matrix, which proves the checker against reference-pinned data; (b) the product's
per-line parser (mgen_amd/csrc/mgenx_logparse.hpp), built as a stand-alone host program under
the address and undefined-behaviour sanitizers, agrees with the checker field for field; (c)
the reference manual's own lines give hand-written values; (d) the C entry points reject null
arguments without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logparse_corpus as C   # noqa: E402
import logparse_ref as R      # noqa: E402

HOST = os.path.join(ROOT, "tests", "cpp", "logparse_host")
FIELDS = ("event", "status", "protocol", "present", "kind", "rx_sec", "rx_usec", "tx_sec",
          "tx_usec", "flow", "seq", "size", "ttl", "flags", "err", "gps", "lat_raw", "lon_raw",
          "alt")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "udp_matrix.npz"),
                        allow_pickle=False))


@pytest.fixture(scope="module")
def matrix_text(oracle, gold):
    """[(oracle text, expected per-line fields)] for the four (mode, opts, protocol) rows."""
    out = []
    for mode, opts, proto in C.MATRIX_ROWS:
        src, rx_sec, rx_usec, ttl = C.matrix_inputs(oracle, gold, opts)
        f = gold[f"unpack_fields_{mode}"]
        text = oracle.log_recv_text(f, gold["unpack_slab"], gold["unpack_offs"], src, rx_sec,
                                    rx_usec, protocol=proto, ttl=ttl, opts=opts)
        want = C.expect_from_fields(f, gold["unpack_slab"], gold["unpack_offs"], src, rx_sec,
                                    rx_usec, ttl, proto, opts)
        out.append((text, want))
    return out


def _same(got, want, i, line=b""):
    if want["status"] != R.OK:
        assert got["status"] == R.MALFORMED, (i, line)
        return
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, (i, line, diff)


def test_checker_reads_back_oracle_lines(matrix_text):
    n_bad = n_data = n_v6 = 0
    for text, want in matrix_text:
        lines = R.split_lines(text)
        assert len(lines) == len(want)
        for i, (line, w) in enumerate(zip(lines, want)):
            _same(R.parse_line(line), w, i, line)
            wide_usec = w["event"] == 1 and w["tx_usec"] > 999999
            assert (w["status"] == R.MALFORMED) == (b"(invalid)" in line or wide_usec), line
            n_bad += w["status"]
            n_data += bool(w["data"])
            n_v6 += w["src"][0] == 2
    assert n_bad > 0 and n_data > 100 and n_v6 > 1000     # the corpus exercises data> and IPv6 sources


def _host_parse(tmp_path, buf):
    if not os.path.exists(HOST):      # as the other tests/cpp programs: built on demand
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/logparse_host"], check=True)
    assert os.path.exists(HOST), "tests/cpp/logparse_host not built (make all)"
    p = tmp_path / "log.txt"
    p.write_bytes(buf)
    r = subprocess.run([HOST, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]        # a sanitizer report exits non-zero
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    out = []
    for row in r.stdout.splitlines():
        t = row.split(" ")
        d = dict(zip(FIELDS, map(int, t[:19])))
        for k, name in enumerate(("src", "dst", "host")):
            a = t[20 + k].split(":")
            d[name] = (int(a[0]), int(a[1]), int(a[2]), bytes.fromhex(a[3]))
        d["data"] = b"" if t[23] == "-" else bytes.fromhex(t[23])
        d["data_len"] = int(t[19])
        out.append(d)
    return out


def test_host_parser_matches_checker(tmp_path, matrix_text):
    corpora = [t for t, _ in matrix_text] + [C.doc_lines(), C.hostile_corpus()]
    for buf in corpora:
        got = _host_parse(tmp_path, buf)
        lines = R.split_lines(buf)
        assert len(got) == len(lines)
        for i, (g, line) in enumerate(zip(got, lines)):
            w = R.parse_line(line)
            assert (g["event"], g["status"]) == (w["event"], w["status"]), (i, line[:200])
            if w["status"] == R.OK:
                _same(g, w, i, line[:200])
                assert g["data_len"] == len(w["data"])


def test_hostile_corpus_has_both_verdicts():
    ref = R.parse_log(C.hostile_corpus())
    ok = sum(r["status"] == R.OK for r in ref)
    assert ok > 100 and len(ref) - ok > 500


def test_doc_lines_hand_written_values():
    got = R.parse_log(C.doc_lines())
    assert len(got) == len(C.DOC_EXPECT) == 5
    for i, (g, w) in enumerate(zip(got, C.DOC_EXPECT)):
        assert g["status"] == R.OK
        diff = {k: (g[k], w[k]) for k in w if g[k] != w[k]}
        assert not diff, (i, diff)
    assert [R.msg_len(g) for g in got] == [1024, 1024, 65535, 1024, 65535]
    # alt -999 from both spellings (doc/mgen.xml:2948 prints the 64-bit zero extension)
    assert got[0]["alt"] == got[2]["alt"] == -999


def test_new_entry_points_reject_null_arguments_without_gpu():
    import ctypes
    from mgen_amd import LogparseOut, load
    lib = load()
    assert lib.mgenx_text_index(None, None, 0, None, 0, None, None) == -1
    assert lib.mgenx_log_parse_text(None, None, 0, None, 0, 0, 0, None, None) == -1
    out = LogparseOut()
    assert lib.mgenx_log_parse_text(None, None, 0, None, 0, 0, 0, ctypes.byref(out), None) == -1
