"""Host logic and the C-ABI library on a machine WITHOUT a GPU: the library loads, exports every
symbol include/fastmpc.h declares, validates arguments, and refuses to solve without a HIP device
(there is no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmpc_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(pkg._lib.SIGNATURES), (declared ^ set(pkg._lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.fmpc_version() == 100
    assert lib.fmpc_strerror(-8).decode().startswith("no HIP device")
    assert lib.fmpc_step_ld(5) == 5 and lib.fmpc_step_ld(0) == 1000


def test_status_codes_match_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    for name, val in re.findall(r"#define (FMPC_[EW]_[A-Z_]+|FMPC_OK)\s+(-?\d+)", hdr):
        assert getattr(pkg._lib, name) == int(val), name


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful without a GPU")
def test_no_cpu_fallback(pkg):
    md, data = pkg.synthetic.make_test_problem(8, 5, 10, seed=0)
    with pytest.raises(pkg.FastMPCError) as e:
        pkg.FastMPCHandle(md["A1"], md["A2"], md["B"], md["Q"], md["R"], md["Qf"], md["u_min"], md["u_max"],
                          md["x_min"], md["x_max"], 10)
    assert e.value.code in (pkg.FMPC_E_NO_DEVICE, pkg.FMPC_E_HIP)
    with pytest.raises(pkg.FastMPCError) as e2:
        pkg.FastMPCHandle(md["A1"], md["A2"], md["B"], md["Q"], md["R"], md["Qf"], md["u_min"], md["u_max"],
                          md["x_min"], md["x_max"], 10, device=-1)
    assert e2.value.code == pkg.FMPC_E_NO_DEVICE


def test_create_argument_checks(pkg):
    """Argument errors are reported before any device is touched."""
    lib = pkg.load()
    h = C.c_void_p()
    one = (C.c_double * 4)(1, 0, 0, 1)
    nul = None
    assert lib.fmpc_create(None, 2, 2, 1, 2, *([one] * 14), 0) == pkg.FMPC_E_NULL
    assert lib.fmpc_create(C.byref(h), 0, 2, 1, 2, *([one] * 14), 0) == pkg.FMPC_E_DIM
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 3, *([one] * 14), 0) == pkg.FMPC_E_DIM
    args = [one] * 14
    args[1] = nul                                     # A2 missing for VAR(2): fast_mpc_eq_const.m:21-22
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 2, *args, 0) == pkg.FMPC_E_NULL
    skewr = (C.c_double * 4)(1, 0.5, 0.25, 1)         # R not symmetric (dense symmetric positive definite R is solved)
    args = [one] * 14
    args[4] = skewr
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 2, *args, 0) == pkg.FMPC_E_NOT_PD_PHI
    indef = (C.c_double * 4)(1, 2, 2, 1)              # symmetric, positive diagonal, indefinite
    args = [one] * 14
    args[4] = indef
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 2, *args, 0) == pkg.FMPC_E_NOT_PD_PHI
    skew = (C.c_double * 4)(1, 0.5, 0.25, 1)          # Q not symmetric: chol(KKT_H) of the reference would not see a PD matrix
    args = [one] * 14
    args[3] = skew
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 2, *args, 0) == pkg.FMPC_E_NOT_PD_PHI
    neg = (C.c_double * 4)(-1, 0, 0, 1)               # Q not PD -> chol(KKT_H) would fail
    args = [one] * 14
    args[3] = neg
    assert lib.fmpc_create(C.byref(h), 2, 2, 1, 2, *args, 0) == pkg.FMPC_E_NOT_PD_PHI
    assert lib.fmpc_destroy(None) == pkg.FMPC_E_NULL
    assert lib.fmpc_solve(None, 1, *([None] * 5), 1, 0.01, *([None] * 5)) == pkg.FMPC_E_NULL
    # the later entry points refuse a NULL handle / NULL mandatory buffers the same way (no device needed to find out)
    assert lib.fmpc_solve_device(None, 1, *([None] * 5), 1, 0.01, *([None] * 5), None) == pkg.FMPC_E_NULL
    assert lib.fmpc_solve_u0_device(None, 1, *([None] * 5), 1, 0.01, *([None] * 6), None) == pkg.FMPC_E_NULL
    assert lib.fmpc_set_ramp(None, one, one) == pkg.FMPC_E_NULL
    # the entry points of round 2
    assert lib.fmpc_loop_step_device(None, 1, *([None] * 8), 1, 0.01, *([None] * 6), None) == pkg.FMPC_E_NULL
    assert lib.fmpc_set_dense_form(None, 1, -1) == pkg.FMPC_E_NULL
    assert lib.fmpc_last_dual_form(None) == pkg.FMPC_E_NULL
    assert lib.fmpc_set_precision(None, 0) == pkg.FMPC_E_NULL
    assert lib.fmpc_set_small_batch_kernel(None, 1) == pkg.FMPC_E_NULL
    assert lib.fmpc_solve_ramp(None, 1, *([None] * 6), 1, 0.01, *([None] * 5)) == pkg.FMPC_E_NULL
    assert lib.fmpc_solve_ramp_device(None, 1, *([None] * 6), 1, 0.01, *([None] * 5), None) == pkg.FMPC_E_NULL
    assert lib.fmpc_unpack_device(None, 1, None, None, None, None, None) == pkg.FMPC_E_NULL
    assert lib.fmpc_loop_inputs_device(None, 1, *([None] * 7), None) == pkg.FMPC_E_NULL
    assert lib.fmpc_last_dispatch(None, None, None) == pkg.FMPC_E_NULL


def test_estimator_create_refuses_a_mode_count_the_finish_kernel_cannot_serve(pkg):
    """fmpc_est_create, include/fastmpc.h: nx <= 1024 (one thread of the finish kernel per mode) and (d^2 + 16 nx) * 8 bytes of LDS
    <= 64 KiB -- FMPC_E_UNSUPPORTED before the device is touched (this box has none) and before the gain is computed (nx = 2000
    would be minutes of Jacobi sweeps); argument errors come first."""
    import time
    lib = pkg.load()
    h = C.c_void_p()
    buf = np.zeros(64 * 64)
    A = np.ones(2000)
    p_, a_ = buf.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p)
    t0 = time.perf_counter()
    for nx in (2000, 600):                             # d = 1, ndiv = 1, p = 1: 600 modes need 2 + 9600 doubles of LDS
        h.value = 1
        assert lib.fmpc_est_create(C.byref(h), 64, 32, 1, 1, p_, p_, 1.0, a_, p_, 1, nx, 0) == pkg.FMPC_E_UNSUPPORTED
        assert not h.value                             # no handle comes back
    assert time.perf_counter() - t0 < 1.0              # "at once": nothing was computed
    assert lib.fmpc_est_create(C.byref(h), 64, 0, 32, 1, p_, p_, 1.0, a_, p_, 1024, 449, 0) == pkg.FMPC_E_UNSUPPORTED   # d = 32: 448 is the last
    assert lib.fmpc_est_create(C.byref(h), 64, 32, 1, 1, None, p_, 1.0, a_, p_, 1, 2000, 0) == pkg.FMPC_E_NULL
    assert lib.fmpc_est_create(None, 64, 32, 1, 1, p_, p_, 1.0, a_, p_, 1, 2000, 0) == pkg.FMPC_E_NULL
    assert lib.fmpc_est_create(C.byref(h), 64, 32, 1, 1, p_, p_, 1.0, a_, p_, 2, 2000, 0) == pkg.FMPC_E_DIM               # p != ndiv d^2


def test_fast_mpc2_validation_mirrors_reference_errors(pkg):
    md, data = pkg.synthetic.make_test_problem(8, 5, 10, seed=0)
    mk = lambda **kw: pkg.Fast_MPC2(kw.get("Q", md["Q"]), md["R"], [], md["Qf"], kw.get("q", []), [], [], md["x_min"],
                                    md["x_max"], kw.get("umin", md["u_min"]), md["u_max"], [], [], 10,
                                    kw.get("x0", data["x0"][0]), data["x0_pre"][0], np.zeros(5), md["A1"],
                                    kw.get("A2", md["A2"]), md["B"], kw.get("w", data["w"][0]), [], kw.get("x_init", []))
    cases = [(dict(x_init=np.zeros(7)), "Initialization size mismatch"),
             (dict(q=np.zeros(3)), "Linear state cost"),
             (dict(umin=np.zeros(2)), "Check cotrol iequality"),
             (dict(A2=[]), "Define the state dynamics"),
             (dict(x0=np.zeros(3)), "equality state dynamics matrix size"),
             (dict(w=np.zeros(8)), "Index exceeds")]
    for kw, msg in cases:
        with pytest.raises(pkg.FastMPCError) as e:
            mk(**kw).mpc_fixed_log_newton(1, 0.01)
        assert msg in str(e.value), (msg, str(e.value))
    obj = mk()
    z0 = obj.initialize()
    assert z0.shape == (130,) and np.array_equal(z0, np.zeros(130))
    with pytest.raises(NotImplementedError):
        obj.matlab_solve()
    # VAR_1: the ramp rows need du_min, du_max (m each) and u_prev (VAR_1/fast_mpc_ineq_const.m:58-76)
    for du, up in (([], np.zeros(5)), (np.ones(4), np.zeros(5)), (np.ones(5), np.zeros(3))):
        v1 = pkg.Fast_MPC2_VAR1(md["Q"], md["R"], [], md["Qf"], [], [], [], md["x_min"], md["x_max"], md["u_min"], md["u_max"],
                                -np.asarray(du), du, 10, data["x0"][0], up, md["A1"], md["B"], data["w"][0], [], [])
        with pytest.raises(pkg.FastMPCError) as e:
            v1.mpc_fixed_log_newton(1, 0.01)
        assert e.value.code == pkg.FMPC_E_DIM


def test_deinterleave_and_shard_range(pkg):
    z = np.arange(3 * 5.0)
    U, X = pkg.deinterleave(z, 3, 2, 3)
    assert np.array_equal(U, [0, 1, 5, 6, 10, 11]) and np.array_equal(X, [2, 3, 4, 7, 8, 9, 12, 13, 14])
    got = [pkg.shard_range(10, 4, r) for r in range(4)]
    assert got == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert [pkg.shard_range(2, 4, r) for r in range(4)] == [(0, 1), (1, 2), (2, 2), (2, 2)]
    assert pkg.shard_range(4096, 8, 7) == (3584, 4096)


def test_synthetic_is_seeded_and_stable(pkg):
    a = pkg.synthetic.make_model(27, 144, 30); b = pkg.synthetic.make_model(27, 144, 30)
    assert all(np.array_equal(a[k], b[k]) for k in ("A1", "A2", "B"))
    comp = np.block([[a["A1"], a["A2"]], [np.eye(27), np.zeros((27, 27))]])
    assert np.max(np.abs(np.linalg.eigvals(comp))) < 0.999
    d = pkg.synthetic.make_replay_batch(a, r=0, steps=50)
    assert d["x0"].shape == (50, 27) and np.array_equal(d["x0"][:-1], d["x0_pre"][1:])
    assert abs(np.mean(np.linalg.norm(pkg.synthetic.make_realisation(a, 0, 500)[1:], axis=1)) - 3.0) < 1e-9
    assert [pkg.synthetic.radial_order(j) for j in (1, 2, 3, 4, 6, 7, 10, 11)] == [0, 1, 1, 2, 2, 3, 3, 4]


def test_plain_c_client_builds_against_the_header_and_library(pkg, tmp_path):
    """examples/c_client.c needs nothing but include/fastmpc.h and libfastmpc.so (no HIP, no torch): it compiles and links
    with gcc on a box without a GPU (tests/test_gpu_c_client.py runs it)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "mpc-sensorlessao_amd", "lib")
    exe = str(tmp_path / "c_client")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_client.c"),
                    "-o", exe, "-L" + lib_dir, "-lfastmpc", "-Wl,-rpath," + lib_dir, "-lm"], check=True)
    assert os.path.exists(exe)


@pytest.mark.parametrize("var_order,xf,lin", [(2, False, False), (2, True, True), (1, False, True), (1, True, False)])
def test_dense_builder_methods_of_the_class(pkg, var_order, xf, lin):
    """objective_function / inequality_const / equality_const of the drop-in class (VAR_2/Fast_MPC2.m:56-67; host-side
    numpy, the device never forms H, P, C) against the op-for-op restatement in oracle/dense_ref.py, VAR_2 and VAR_1
    (ramp rows on), with and without terminal rows and linear costs."""
    from oracle.dense_ref import DenseFastMPC
    rng = np.random.default_rng(7)
    n, m, T = 4, 3, 5
    A1 = rng.standard_normal((n, n)); A2 = rng.standard_normal((n, n)); B = rng.standard_normal((n, m))
    Q = np.diag(rng.random(n) + 1); R = np.diag(rng.random(m) + 1); Qf = np.diag(rng.random(n) + 2)
    q = rng.standard_normal(n) if lin else None; r = rng.standard_normal(m) if lin else None; qf = rng.standard_normal(n) if lin else None
    xmin, xmax, umin, umax = -np.ones(n), 2 * np.ones(n), -0.5 * np.ones(m), 0.7 * np.ones(m)
    dumin, dumax, uprev = -0.1 * np.ones(m), 0.2 * np.ones(m), 0.05 * rng.standard_normal(m)
    x0, x0p, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(T * n)
    xfv = rng.standard_normal(n) if xf else None
    if var_order == 2:
        mine = pkg.Fast_MPC2(Q, R, None, Qf, q, r, qf, xmin, xmax, umin, umax, dumin, dumax, T, x0, x0p, uprev, A1, A2, B, w, xfv, None)
        ref = DenseFastMPC(Q, R, None, Qf, q, r, qf, xmin, xmax, umin, umax, dumin, dumax, T, x0, x0p, uprev, A1, A2, B, w, xfv, None)
    else:
        mine = pkg.Fast_MPC2_VAR1(Q, R, None, Qf, q, r, qf, xmin, xmax, umin, umax, dumin, dumax, T, x0, uprev, A1, B, w, xfv, None)
        ref = DenseFastMPC.var1(Q, R, None, Qf, q, r, qf, xmin, xmax, umin, umax, dumin, dumax, T, x0, uprev, A1, B, w, xfv, None)
    for name in ("objective_function", "inequality_const", "equality_const"):
        Mm, vm = getattr(mine, name)()
        Mr, vr = getattr(ref, name)()
        assert Mm.shape == np.asarray(Mr).shape, name
        assert np.array_equal(Mm, np.asarray(Mr)), name
        assert np.array_equal(vm, np.asarray(vr).reshape(-1)), name
    assert np.array_equal(mine.initialize(), np.asarray(ref.initialize()).reshape(-1))
