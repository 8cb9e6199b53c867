"""The detector's host read-out under the address and undefined-behaviour sanitizers: tests/host_san/detector_main.cpp, a program
with its own main, is compiled together with fmpc_host.cpp and run over the list of lam.  Nothing is preloaded, nothing is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-sensorlessao_amd", "csrc")


def test_detector_read_host_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "detector_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(ROOT, "tests", "host_san", "detector_main.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "detector host ok" in lines and sum(ln.startswith("lam ") for ln in lines) == 11, r.stdout
