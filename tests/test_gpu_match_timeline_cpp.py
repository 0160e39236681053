"""mgenx::MessageMatch::RunTimeline (include/mgenx.hpp): tests/cpp/match_timeline_host joins about
9000 sent messages in 4 flows with what a receiver logged of them and compares the series per
send-time window, the list of loss runs and the owner column with a serial loop written in the
program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "match_timeline_host")


@pytest.mark.gpu
def test_match_timeline_host_program():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/match_timeline_host"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match_timeline_host ok" in r.stdout
