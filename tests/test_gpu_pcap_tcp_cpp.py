"""mgenx::Pcap2Mgen with PcapOptions::tcp (include/mgenx_pcap.hpp): tests/cpp/pcap_tcp_host over
one mixed capture -- UDP flows with fragmented datagrams plus TCP connections -- gives the bytes
of the Python layer, which are the oracle's (tests/pcap_tcp_util.expected_log)."""
import os
import subprocess

import pytest

import pcap_tcp_util as T
import pcapng_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pcap_tcp_host")


@pytest.mark.gpu
def test_pcap_tcp_host_program(oracle, tmp_path):
    from mgen_amd import Engine
    from mgen_amd.pcap import Pcap2Mgen
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/pcap_tcp_host"], check=True)
    f, conns, whole = T.capture(oracle, seed=91, frag_mtu=1500)
    want, n_tcp, ref = T.expected_log(oracle, f, 1, conns, whole)
    assert n_tcp >= 30
    eng = Engine(0)
    try:
        py = Pcap2Mgen(eng, tcp=True, reassemble=True).run(f)
    finally:
        eng.close()
    s = ref.stats
    line = (f"pcap_tcp_host: {s['n_segments']} segments {s['n_streams']} streams "
            f"{s['n_pieces']} pieces {n_tcp} records\n")
    for name, data in (("x.pcap", f), ("x.pcapng", G.from_pcap(f, seed=3).file)):
        path = tmp_path / name
        path.write_bytes(data)
        r = subprocess.run([BIN, str(path), "reassemble"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == py and r.stdout == want
        assert r.stderr.decode() == line
