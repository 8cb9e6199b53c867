"""The ramp-rate rows (VAR_1/fast_mpc_ineq_const.m:58-76) at the sizes and weights fmpc_newton_ramp does not take: n > 64,
B' beyond its LDS, dense Q / Qf / R (fast_mpc_objective.m:50-55).  They run on fmpc_newton_ramp_ws (FMPC_PATH_RAMP_WS).  Same
bar as tests/test_gpu_ramp.py against the dense oracle with ramp rows: 1e-9 relative on z, 1e-7 on nu, identical iteration
counts, status codes and (canonicalised) step lengths."""
import ctypes as C

import numpy as np
import pytest

from oracle.dense_ref import DenseFastMPC
from tests.util import canon_steps, handle_from_model, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _oracle(md, x0, x0_pre, w, u_prev, du_min, du_max, nw, k, nu0, x_init=None):
    m = md["m"]
    info = {}
    if md.get("var_order", 2) == 1:
        d = DenseFastMPC.var1(md["Q"], md["R"], None, md["Qf"], md.get("q"), md.get("r"), md.get("qf"), md["x_min"], md["x_max"],
                              md["u_min"], md["u_max"], du_min, du_max, md["T"], x0, u_prev, md["A1"], md["B"], w,
                              md.get("xf"), x_init, ramp=True)
    else:
        d = DenseFastMPC(md["Q"], md["R"], None, md["Qf"], md.get("q"), md.get("r"), md.get("qf"), md["x_min"], md["x_max"],
                         md["u_min"], md["u_max"], du_min, du_max, md["T"], x0, x0_pre, u_prev, md["A1"], md["A2"], md["B"], w,
                         md.get("xf"), x_init, ramp=True)
    assert d.inequality_const()[0].shape[0] == 4 * md["T"] * m
    z = d.mpc_fixed_log_newton(nw, k, nu0=nu0, info=info)
    return z, info


def _ramp_inputs(md, batch, seed, width=0.4):
    rng = np.random.default_rng(seed)
    m = md["m"]
    du_min = -width * (0.5 + rng.random(m)); du_max = width * (0.5 + rng.random(m))
    # the mid-box start has u_0 = umid: keep u_prev close enough for a positive first-stage ramp slack
    umid = 0.5 * (md["u_min"] + md["u_max"])
    u_prev = umid + 0.5 * (du_min + (du_max - du_min) * rng.random((batch, m)))
    return du_min, du_max, u_prev


def _spd(size, seed, scale=1.0):
    """Seeded dense SPD weight: scale (I + 0.3 sym(noise)), the noise normalised so that the spectrum stays in [0.5, 1.5] scale."""
    rng = np.random.default_rng(seed)
    N = rng.standard_normal((size, size)) / np.sqrt(size)
    M = scale * (np.eye(size) + 0.3 * 0.5 * (N + N.T))
    assert np.all(M == M.T) and np.linalg.eigvalsh(M).min() > 0.4 * scale
    return M


def _z_init(md, batch, u_prev, du_min, du_max, seed):
    """An explicit start (fast_mpc_init.m:12-15) with every ramp slack positive, built as tests/test_gpu_ramp.py builds its start."""
    n, m, T = md["n"], md["m"], md["T"]
    rng = np.random.default_rng(seed)
    s = n + m
    z_init = np.tile(np.concatenate([np.concatenate([0.2 * rng.standard_normal(m), rng.standard_normal(n)]) for _ in range(T)]),
                     (batch, 1))
    z_init[:, :m] = u_prev + 0.5 * (du_min + du_max)
    for j in range(1, T):
        z_init[:, s * j:s * j + m] = z_init[:, s * (j - 1):s * (j - 1) + m] + 0.25 * (du_min + du_max)
    return z_init


def _check(pkg, md, data, du_min, du_max, u_prev, nw, k=0.01, z_init=None, expect_path=None, probs=None, h=None):
    own = h is None
    if own:
        h = handle_from_model(pkg, md)
        h.set_ramp(du_min, du_max)
    x0p = data.get("x0_pre") if md.get("var_order", 2) == 2 else None
    z, info = h.solve(data["x0"], x0p, data["w"], z_init=z_init, nu0=data["nu0"], n_newton=nw, k=k, return_info=True,
                      u_prev=u_prev, check=False)
    if expect_path is not None:
        assert h.last_dispatch()[0] == expect_path
    batch = z.shape[0]
    for p in (range(batch) if probs is None else probs):
        zo, io = _oracle(md, data["x0"][p], None if x0p is None else x0p[p], data["w"][p], u_prev[p], du_min, du_max, nw or None, k,
                         data["nu0"][p], x_init=None if z_init is None else z_init[p])
        collapsed = bool((canon_steps(io["t"]) == 0).any())
        assert info["status"][p] == (pkg.FMPC_W_LINESEARCH if collapsed else 0), (p, info["status"][p])
        assert info["iters"][p] == io["iters"], (p, info["iters"][p], io["iters"])
        assert np.array_equal(canon_steps(info["step"][p][:io["iters"]]), canon_steps(io["t"][:io["iters"]]))
        assert rel_err(z[p], zo) <= TOL, (p, rel_err(z[p], zo))
        assert rel_err(info["nu"][p], io["nu"]) <= 1e-7, (p, rel_err(info["nu"][p], io["nu"]))
    if own:
        h.close()
    return z, info


@pytest.mark.parametrize("nw", [1, 5, 0])
def test_n_beyond_64_var1(pkg, gpu, nw):
    """n = 65 (radial order 10), diagonal weights: fmpc_set_ramp refused this size before the workspace kernel."""
    md, data = pkg.synthetic.make_test_problem(65, 12, 4, seed=21, var_order=1, batch=3)
    du_min, du_max, u_prev = _ramp_inputs(md, 3, 5)
    _check(pkg, md, data, du_min, du_max, u_prev, nw, expect_path=pkg.FMPC_PATH_RAMP_WS)


def test_n_beyond_64_var2_xf_warm_start(pkg, gpu):
    # (with the terminal rows the Schur complement needs n <= T m: (T + 1) n rows of C against T (n + m) columns)
    md, data = pkg.synthetic.make_test_problem(70, 30, 3, seed=22, var_order=2, xf=True, batch=3)
    du_min, du_max, u_prev = _ramp_inputs(md, 3, 6)
    zi = _z_init(md, 3, u_prev, du_min, du_max, 2)
    _check(pkg, md, data, du_min, du_max, u_prev, 3, z_init=zi, expect_path=pkg.FMPC_PATH_RAMP_WS)


@pytest.mark.parametrize("nw", [1, 5])
def test_lds_overflow_at_n_below_64(pkg, gpu, nw):
    """n = 60, m = 300: the m n doubles of B' alone exceed the LDS of fmpc_newton_ramp."""
    md, data = pkg.synthetic.make_test_problem(60, 300, 2, seed=23, var_order=1, batch=2)
    du_min, du_max, u_prev = _ramp_inputs(md, 2, 7)
    _check(pkg, md, data, du_min, du_max, u_prev, nw, expect_path=pkg.FMPC_PATH_RAMP_WS)


@pytest.mark.parametrize("n,m,T,var_order,xf,nw", [(8, 5, 6, 1, False, 4), (27, 20, 5, 2, False, 3)])
def test_dense_state_weights(pkg, gpu, n, m, T, var_order, xf, nw):
    md, data = pkg.synthetic.make_test_problem(n, m, T, seed=24 + n, var_order=var_order, xf=xf, batch=3)
    md["Q"] = _spd(n, 31); md["Qf"] = _spd(n, 32, 50.0)
    du_min, du_max, u_prev = _ramp_inputs(md, 3, 8)
    _check(pkg, md, data, du_min, du_max, u_prev, nw, expect_path=pkg.FMPC_PATH_RAMP_WS)


@pytest.mark.parametrize("n,m,T,var_order,xf,dense_q,nw", [(8, 5, 6, 1, False, False, 4), (12, 30, 4, 2, True, True, 3)])
def test_dense_input_weight(pkg, gpu, n, m, T, var_order, xf, dense_q, nw):
    """Dense R: the u-part of Phi is block-tridiagonal (block Cholesky over the stages); with dense Q, Qf as well."""
    md, data = pkg.synthetic.make_test_problem(n, m, T, seed=25 + n, var_order=var_order, xf=xf, batch=3)
    md["R"] = _spd(m, 33)
    if dense_q:
        md["Q"] = _spd(n, 34); md["Qf"] = _spd(n, 35, 50.0)
    du_min, du_max, u_prev = _ramp_inputs(md, 3, 9)
    _check(pkg, md, data, du_min, du_max, u_prev, nw, expect_path=pkg.FMPC_PATH_RAMP_WS)


@pytest.mark.parametrize("dense_r", [False, True])
def test_config0_shape_at_radial_order_10(pkg, gpu, dense_r):
    """BASELINE configs[0] shape (VAR(1), m = 144, T = 10) with n = 65 (radial order 10), budgets 1 and 5."""
    md = pkg.synthetic.make_model(65, 144, 10, var_order=1)
    if dense_r:
        md["R"] = _spd(144, 36)                                                  # (the model's R is I)
    data = pkg.synthetic.make_replay_batch(md, r=2, steps=3)
    data["nu0"] = data["nu0"][:, :650]
    data["w"] = np.zeros((3, 650))
    du = 0.2121 * np.ones(144)
    u_prev = 0.1 * np.random.default_rng(8).standard_normal((3, 144))
    h = handle_from_model(pkg, md)
    h.set_ramp(-du, du)
    for nw in (1, 5):
        _check(pkg, md, data, -du, du, u_prev, nw, expect_path=pkg.FMPC_PATH_RAMP_WS, h=h)
    h.close()


def test_entry_points(pkg, gpu):
    import torch
    n, m, T = 66, 10, 4
    md, data = pkg.synthetic.make_test_problem(n, m, T, seed=27, var_order=1, batch=3)
    du_min, du_max, u_prev = _ramp_inputs(md, 3, 10)
    lib = pkg.load()
    # fmpc_solve_once with var_order 1: ramp rows from du_min, du_max, u_prev
    zo, io = _oracle(md, data["x0"][0], None, data["w"][0], u_prev[0], du_min, du_max, 4, 0.01, data["nu0"][0])
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)
    P = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)
    keep = [cm(md["Q"]), cm(md["R"]), cm(md["Qf"]), md["x_min"], md["x_max"], md["u_min"], md["u_max"], du_min, du_max,
            data["x0"][0], u_prev[0], cm(md["A1"]), cm(md["B"]), data["w"][0], data["nu0"][0]]
    x_opt = np.empty(T * (n + m)); iters = C.c_int(0)
    rc = lib.fmpc_solve_once(n, m, T, 1, P(keep[0]), P(keep[1]), None, P(keep[2]), None, None, None, P(keep[3]), P(keep[4]),
                             P(keep[5]), P(keep[6]), P(keep[7]), P(keep[8]), P(keep[9]), None, P(keep[10]), P(keep[11]), None,
                             P(keep[12]), P(keep[13]), None, None, P(keep[14]), 4, 0.01, 0, P(x_opt), C.byref(iters))
    assert rc == 0 and iters.value == io["iters"] and rel_err(x_opt, zo) <= TOL
    # the class with a dense R (ramp rows on by default, as in the reference)
    R = _spd(m, 37)
    md_r = dict(md, R=R)
    args = (md["Q"], R, [], md["Qf"], [], [], [], md["x_min"], md["x_max"], md["u_min"], md["u_max"], du_min, du_max, T,
            data["x0"][1], u_prev[1], md["A1"], md["B"], data["w"][1], [], [])
    zo, io = _oracle(md_r, data["x0"][1], None, data["w"][1], u_prev[1], du_min, du_max, 1, 0.01, data["nu0"][1])
    z = pkg.Fast_MPC2_VAR1(*args).mpc_fixed_log_newton(1, 0.01, nu0=data["nu0"][1])
    assert rel_err(z, zo) <= TOL
    # first moves only on the device (z_out = NULL) == z[:, :m] of the host solve, from the cold start and with a budget
    h = handle_from_model(pkg, md)
    h.set_ramp(du_min, du_max)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for nw in (1, 3):
        z = h.solve(data["x0"], None, data["w"], nu0=data["nu0"], n_newton=nw, k=0.01, u_prev=u_prev)
        u0 = torch.empty((3, m), dtype=torch.float64, device=dev)
        zd, st, it = h.solve_device(t(data["x0"]), None, t(data["w"]), None, t(data["nu0"]), nw, 0.01, u_prev=t(u_prev), u0_out=u0,
                                    want_z=False)
        torch.cuda.synchronize()
        assert zd is None and h.last_dispatch()[0] == pkg.FMPC_PATH_RAMP_WS
        assert np.array_equal(u0.cpu().numpy(), z[:, :m]) and (st.cpu().numpy() == 0).all()
    h.close()


def test_batch_beyond_the_workgroups_in_flight(pkg, gpu):
    """More problems than workgroups in flight: every problem bitwise equal to the same problem solved alone."""
    batch = 300
    md, data = pkg.synthetic.make_test_problem(65, 12, 4, seed=28, var_order=1, batch=batch)
    du_min, du_max, u_prev = _ramp_inputs(md, batch, 11)
    h = handle_from_model(pkg, md)
    h.set_ramp(du_min, du_max)
    z, info = h.solve(data["x0"], None, data["w"], nu0=data["nu0"], n_newton=3, k=0.01, return_info=True, u_prev=u_prev)
    assert h.last_dispatch()[0] == pkg.FMPC_PATH_RAMP_WS
    for p in range(batch):
        z1, i1 = h.solve(data["x0"][p:p + 1], None, data["w"][p:p + 1], nu0=data["nu0"][p:p + 1], n_newton=3, k=0.01,
                         return_info=True, u_prev=u_prev[p:p + 1])
        assert np.array_equal(z1[0], z[p]) and np.array_equal(i1["nu"][0], info["nu"][p]), p
        assert i1["iters"][0] == info["iters"][p] and i1["status"][0] == info["status"][p]
    _check(pkg, md, data, du_min, du_max, u_prev, 3, probs=(0, 150, 299), h=h)
    h.close()


def test_lds_kernel_keeps_its_domain(pkg, gpu):
    """Sizes fmpc_newton_ramp takes keep FMPC_PATH_RAMP, and the cold start keeps its Woodbury form (dual form 5).  Forced onto
    the workspace kernel (fmpc_set_ramp_workspace) the same solves agree to rounding."""
    for (n, m, T) in ((8, 5, 6), (27, 144, 10)):
        if n == 27:
            md = pkg.synthetic.make_model(n, m, T, var_order=1)
            data = pkg.synthetic.make_replay_batch(md, r=3, steps=3)
            data["nu0"] = data["nu0"][:, :T * n]
            data["w"] = 0.01 * np.random.default_rng(1).standard_normal((3, T * n))
        else:
            md, data = pkg.synthetic.make_test_problem(n, m, T, seed=29, var_order=1, batch=3)
        du_min, du_max, u_prev = _ramp_inputs(md, 3, 12)
        h = handle_from_model(pkg, md)
        h.set_ramp(du_min, du_max)
        z, info = h.solve(data["x0"], None, data["w"], nu0=data["nu0"], n_newton=3, k=0.01, return_info=True, u_prev=u_prev)
        assert h.last_dispatch()[0] == pkg.FMPC_PATH_RAMP and h.last_dual_form() == 5
        h.set_ramp_workspace(True)
        zw, iw = h.solve(data["x0"], None, data["w"], nu0=data["nu0"], n_newton=3, k=0.01, return_info=True, u_prev=u_prev)
        assert h.last_dispatch()[0] == pkg.FMPC_PATH_RAMP_WS and h.last_dual_form() == 0
        assert np.array_equal(info["iters"], iw["iters"]) and np.array_equal(info["status"], iw["status"])
        assert np.array_equal(canon_steps(info["step"]), canon_steps(iw["step"]))
        assert max(rel_err(zw[p], z[p]) for p in range(3)) <= 1e-10
        h.set_ramp_workspace(False)
        h.solve(data["x0"], None, data["w"], nu0=data["nu0"], n_newton=1, k=0.01, u_prev=u_prev)
        assert h.last_dispatch()[0] == pkg.FMPC_PATH_RAMP and h.last_dual_form() == 5
        h.close()
