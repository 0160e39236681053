"""mgenx::FlowClock (include/mgenx.hpp): tests/cpp/flow_clock_host runs about 6000 records in 4
flows through one call, with and without MGENX_CLOCK_OFFSET_ONLY, and compares every output with
a serial monotone chain over __int128 written in the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "flow_clock_host")


@pytest.mark.gpu
def test_flow_clock_host_program():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/flow_clock_host"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flow_clock_host ok" in r.stdout
