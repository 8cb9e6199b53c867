"""The science camera's host tables under the address and undefined-behaviour sanitizers: tests/host_san/science_main.cpp, a
program with its own main, is compiled together with fmpc_host.cpp and run over len in {64, 192}, every window and two samplings.
Nothing is preloaded, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-sensorlessao_amd", "csrc")


def test_science_tables_host_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "science_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(ROOT, "tests", "host_san", "science_main.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "science host ok" in lines and sum(ln.startswith("len ") for ln in lines) == 16, r.stdout
