"""The host side of the mirror of spline actuators under the address and undefined-behaviour sanitizers:
tests/host_san/dm_profile_main.cpp, a program with its own main over fmpc_dm_profile_oomao_host and fmpc_dm_profile_eval_host, is
compiled together with fmpc_host.cpp and run directly.  Nothing is preloaded, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-sensorlessao_amd", "csrc")


def test_dm_profile_host_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "dm_profile_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(ROOT, "tests", "host_san", "dm_profile_main.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "dm profile host ok" in lines and sum(ln.startswith("mech ") for ln in lines) == 5, r.stdout
    assert sum(ln.startswith("pieces ") for ln in lines) == 3, r.stdout
