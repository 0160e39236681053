"""mgenx::MessageMatchMulti (include/mgenx.hpp): tests/cpp/msg_match_multi_host joins about 9000
sent messages in 4 flows with what 5 receivers logged of them through RunSeries and compares
cells, fanout, masks and bins with a serial loop written in the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "msg_match_multi_host")


@pytest.mark.gpu
def test_msg_match_multi_host_program():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/msg_match_multi_host"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msg_match_multi_host ok" in r.stdout
