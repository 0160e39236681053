"""mgenx::MessageMatchMulti::RunLoss (include/mgenx.hpp): tests/cpp/msg_match_multi_ex_host joins
a flow of 12 messages with what 3 receivers logged of it and compares the loss runs, their list
and the pair matrix with numbers worked out by hand in the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "msg_match_multi_ex_host")


@pytest.mark.gpu
def test_msg_match_multi_ex_host_program():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/msg_match_multi_ex_host"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msg_match_multi_ex_host ok" in r.stdout
