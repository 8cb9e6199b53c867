"""The library's host-only builders under AddressSanitizer + UndefinedBehaviorSanitizer (sanitizers run on the CPU
build; GPU ASan is not available on the pool).  mpc-sensorlessao_amd/csrc/fmpc_host.cpp -- the iteration-invariant Y blocks and
their de-duplication, the twisted block factorisation in long double with its operator images and sweep schedules, the
least-recently-used cache of fmpc_solve_once -- is plain C++: tests/host_san/host_build_test.cpp links it with g++ and
checks numerically that the two sweeps, executed step by step from the schedules, reproduce a dense solve of Y."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-sensorlessao_amd", "csrc")


@pytest.fixture(scope="module")
def san_binary(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("host_san") / "host_build_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", os.path.join(ROOT, "tests", "host_san", "host_build_test.cpp"), os.path.join(CSRC, "fmpc_host.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 7, 8, 9, 30])
@pytest.mark.parametrize("has_xf", [0, 1])
def test_host_builders_under_asan_ubsan(san_binary, T, has_xf):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for var_order in ((2, 1) if T in (3, 30) else (2,)):
        r = subprocess.run([san_binary, "27", "144", str(T), str(has_xf), str(var_order), str(100 + T)], capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_api_host_math_under_asan_ubsan(tmp_path):
    """The host arithmetic the API files call in fmpc_host.cpp (tests/host_san/api_host_math_test.cpp): the constants of the bank's
    first-move builder against a long double restatement (L L', L y0 to 32 n 2^-53 of the largest entry; a singular matrix and a
    zero row of B refused), every entry of the dense form's operand images against the entry of J, A1, A2 its layout names (==, T = 2
    and 3, VAR(1) and VAR(2); a NaN refused), the bank's packed block descriptors against their table, and fmpc_host_spd_inverse
    (A inv = I to 64 n 2^-53 cond; a zero pivot refused)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path / "api_host_math_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", os.path.join(ROOT, "tests", "host_san", "api_host_math_test.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_host_model_under_asan_ubsan(tmp_path):
    """The host model of a handle (tests/host_san/model_build_test.cpp): fmpc_host_build_model on an integer-valued model (n = 3,
    m = 2, T = 4, VAR(1) and VAR(2), with and without xf and linear terms) -- transposes, doubled weights, midpoints, zeros for NULL
    q / r / qf, M1 / M2 against their recurrence, the presence pattern of the Y blocks, all by ==; fmpc_host_model_classify and
    the build refuse what fmpc_create refuses with FMPC_E_NOT_PD_PHI; fmpc_host_wave_cold at n = 27, m = 5 fills its layout with
    finite values and exactly symmetric G, Ma, Ma2."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path / "model_build_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", os.path.join(ROOT, "tests", "host_san", "model_build_test.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.fixture(scope="module")
def ramp_cold_binary(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("host_san_ramp") / "ramp_cold_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", os.path.join(ROOT, "tests", "host_san", "ramp_cold_test.cpp"), os.path.join(CSRC, "fmpc_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("cfg", ["8 5 6 0 1 1", "8 5 10 1 1 2", "5 8 4 0 1 3", "8 5 6 0 2 4", "6 4 1 0 1 5", "27 144 2 0 1 6", "27 144 3 1 2 7"])
def test_ramp_cold_form_builder_under_asan_ubsan(ramp_cold_binary, cfg):
    """fmpc_host_build_ramp_cold (the cold-start step with the ramp-rate rows as a constant KKT matrix plus a rank-m diagonal term,
    VAR_1/fast_mpc_ineq_const.m:58-76): the constants it builds, used exactly as the device kernel uses them, reproduce an
    independent dense solve of the full KKT system of each problem (long double) to 1e-11 -- VAR(1) and VAR(2), with and without
    terminal rows and disturbance, T = 1, and the AO sizes."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([ramp_cold_binary] + cfg.split(), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
