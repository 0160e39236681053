"""mgenx::FlowSeriesQuantiles (include/mgenx.hpp): tests/cpp/flow_quant_host runs about 5000
records in 3 flows through one call and compares every window's percentiles with a serial loop
over std::sort written in the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "flow_quant_host")


@pytest.mark.gpu
def test_flow_quant_host_program():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/flow_quant_host"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flow_quant_host ok" in r.stdout
