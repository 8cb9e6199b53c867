"""The per-problem-factor kernels on models whose per-index constants all differ (tests/hetero_model.py): distinct diagonals of
Q, Qf != Q and R, linear costs q, qf, r, per-actuator u_min != -u_max and an x box that is not centred.  Every kernel reads rl[c],
ql[r], qfl[r], Q2[r], Qf2[r], R2[q], umin[q], umax[q], umid[e], xmid[e - m] with index arithmetic of its own, and on the models of
synthetic.py (multiples of I, zero linear costs, one symmetric box) a wrong index, a dropped linear term or Qf2 taken for Q2
computes the same numbers.  tests/test_hetero_model_ref.py shows on the CPU that each such change moves the oracle's z by at least
1e-6 (measured >= 1.5e-5) on every problem of every case below; it also asserts what these cases can NOT see: qf and Qf when xf
fixes the terminal state, and the x box wherever the first step from the cold start is a full one -- xmid only sets the x rows of
the mid-box start, and a full Newton step removes them.  The tests named *_x_box_* are cold starts whose FIRST step backtracks
(t = 1/2 on every problem; found by a search on the CPU over narrow u boxes, k = 1, 10, 100 and, with ramp rows, u_prev next to
the ramp bounds): there rolling x_min or x_max moves z by 5e-2 and more.

Bars, the project's own for each kernel: against the oracle 1e-9 relative on z and 1e-7 on nu per problem, identical iterations,
status and (canonicalised) step lengths, on EVERY problem of these batches of 3 to 5; the fp32 factor unrefined 1e-4 and
iterations >= the oracle's (tests/test_gpu_tiled.py), with one refinement sweep the fp64 bars (tests/test_gpu_refine.py); two
forms of the library 1e-10 (the Woodbury cold step of the ramp rows against the general path, tests/test_gpu_ramp.py); closed loops
1e-8 over the fed-back steps.  Every case asserts the path that ran and prints it with its worst errors."""
import numpy as np
import pytest

from tests import hetero_model as H
from tests.util import canon_steps, handle_from_model, rel_err

pytestmark = pytest.mark.gpu
TOL_Z, TOL_NU, TOL32, TOL_FORMS, TOL_LOOP = 1e-9, 1e-7, 1e-4, 1e-10, 1e-8
PATHS = {0: "GENERIC", 1: "WAVE", 2: "SHARED", 3: "PANEL", 4: "RAMP", 5: "TILED", 6: "TILED_F32", 7: "RAMP_WS"}


def run(pkg, md, data, budget, k, z_init=None, prec=None, refine=None, ramp=None, u_prev=None, ramp_ws=False):
    """One host-entry solve on a fresh handle (the switches in the environment are read when it is created and at its first
    solve) -> results and what the handle reports about the kernel that ran."""
    h = handle_from_model(pkg, md)
    if prec is not None:
        h.set_precision(prec)
    if refine is not None:
        h.set_refinement(refine)
    if ramp is not None:
        h.set_ramp(*ramp)
    if ramp_ws:
        h.set_ramp_workspace(True)
    z, info = h.solve(data["x0"], data.get("x0_pre"), data.get("w"), z_init=z_init, nu0=data.get("nu0"), n_newton=budget, k=k,
                      return_info=True, check=False, u_prev=u_prev)
    res = dict(z=z, nu=info["nu"], st=info["status"], it=info["iters"], stp=info["step"], path=h.last_dispatch()[0], form=h.last_dual_form(),
               waves=h.last_tiled_wavefronts(), sweeps=h.last_refinement())
    h.close()
    return res


def check(res, ref, label, tol_z=TOL_Z, tol_nu=TOL_NU, same_iters=True):
    """Every problem against the oracle; the worst errors are printed before anything is asserted."""
    zo, nuo, ito, sto, steps = ref
    B = len(zo)
    ez = max(rel_err(res["z"][p], zo[p]) for p in range(B)); en = max(rel_err(res["nu"][p], nuo[p]) for p in range(B))
    print("%s: path %s, dual form %d, worst z %.2e nu %.2e, iterations %s (oracle %s)"
          % (label, PATHS[res["path"]], res["form"], ez, en, res["it"].tolist(), [int(i) for i in ito]))
    assert np.all(np.isfinite(res["z"])) and np.all(np.isfinite(res["nu"])), label
    assert np.array_equal(res["st"], sto), (label, res["st"], sto)
    if same_iters:
        assert np.array_equal(res["it"], ito), (label, res["it"], ito)
        for p in range(B):
            assert np.array_equal(canon_steps(res["stp"][p][:ito[p]]), canon_steps(steps[p][:ito[p]])), (label, p, res["stp"][p], steps[p])
    else:
        assert np.all(res["it"] >= ito), (label, res["it"], ito)
    assert ez <= tol_z and en <= tol_nu, (label, ez, en)
    return ez, en


def solver_case(pkg, name, budget, path, label, **kw):
    md, data, zi = H.build(name)
    res = run(pkg, md, data, budget, H.CASES[name]["k"], z_init=zi, **kw)
    assert res["path"] == path, (label, PATHS[res["path"]])
    check(res, H.oracle(name, budget), "%s %s budget %d" % (label, name, budget))
    return res


# ------------------------------------------------------------------------------------------------------------- tiled kernel, fp64
@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("name", ["8x5x10", "16x7x6", "20x33x5", "40x21x7", "50x30x4", "65x20x3", "79x40x3"])
def test_tiled_fp64_over_the_block_counts(pkg, gpu, monkeypatch, name, budget):
    """fmpc_newton_tiled<double> with NB = 1, 2, 2, 3, 4, 5, 5 blocks of 16 (FMPC_TILED=1): n a multiple of 16, m no multiple of
    16, both VAR orders, xf on (20, 33, 5) and (40, 21, 7); w and nu0 given, cold start (the kernel's own mid-box start)."""
    monkeypatch.setenv("FMPC_TILED", "1")
    solver_case(pkg, name, budget, pkg._lib.FMPC_PATH_TILED, "tiled fp64")


@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("waves", [2, 4])
def test_tiled_fp64_n27_two_and_four_wavefronts(pkg, gpu, monkeypatch, waves, budget):
    monkeypatch.setenv("FMPC_TILED", "1")
    monkeypatch.setenv("FMPC_TILED_NW", str(waves))
    res = solver_case(pkg, "27x144x6", budget, pkg._lib.FMPC_PATH_TILED, "tiled fp64, %d wavefronts" % waves)
    assert res["waves"] == waves, res["waves"]


def test_tiled_fp64_backtracking_from_a_start_inside_the_asymmetric_box(pkg, gpu, monkeypatch):
    """tests/test_gpu_parity.py::test_active_barrier_and_backtracking (|u| <= 0.3 before heterogeneous(), k = 10, budget 8) with z0
    drawn inside the asymmetric box: the slacks umax[q] - u and u - umin[q] of the line search, per actuator."""
    monkeypatch.setenv("FMPC_TILED", "1")
    res = solver_case(pkg, "backtrack", 8, pkg._lib.FMPC_PATH_TILED, "tiled fp64, backtracking")
    assert np.any((res["stp"] > 0) & (res["stp"] < 1)), "case must exercise backtracking"


@pytest.mark.parametrize("budget", [1, 3])
@pytest.mark.parametrize("kernel", ["tiled", "generic-lds", "generic-workspace"])
def test_x_box_first_step_backtracks(pkg, gpu, monkeypatch, kernel, budget):
    """(40, 21, 5) with |u| <= 0.3 before heterogeneous() and k = 100: the oracle's first step from the mid-box start takes t = 1/2
    on every problem, so xmid[e - m] stays in z; on the tiled kernel and both instances of the generic one."""
    monkeypatch.setenv({"tiled": "FMPC_TILED", "generic-lds": "FMPC_FORCE_GENERIC", "generic-workspace": "FMPC_GENERIC_BIG"}[kernel], "1")
    res = solver_case(pkg, "xbox-40x21x5", budget, pkg._lib.FMPC_PATH_TILED if kernel == "tiled" else pkg.FMPC_PATH_GENERIC, "x box, " + kernel)
    assert np.all((res["stp"][:, 0] > 0) & (res["stp"][:, 0] < 1))


@pytest.mark.parametrize("budget", [1, 3])
@pytest.mark.parametrize("kernel", ["wave", "tiled-2", "tiled-4", "generic-lds"])
def test_x_box_first_step_backtracks_n27(pkg, gpu, monkeypatch, kernel, budget):
    """n = 27: the dynamics of make_model under the demo weights with |u| <= 0.2 and k = 100 (with make_model's own Q = 1.5e4 I the
    first step is a full one down to a u box of 1e-3 of its width at every k tried).  The one-wavefront kernel factoring per
    problem (FMPC_NO_SHARED=1: FMPC_PATH_WAVE; the shared cold-start forms take t = 1 or hand the problem over), the tiled kernel
    with two and four wavefronts, the generic kernel."""
    if kernel == "wave":
        for v in ("FMPC_NO_PANEL", "FMPC_NO_SMALL_TILED", "FMPC_NO_SHARED"):
            monkeypatch.setenv(v, "1")
    elif kernel == "generic-lds":
        monkeypatch.setenv("FMPC_FORCE_GENERIC", "1")
    else:
        monkeypatch.setenv("FMPC_TILED", "1")
        monkeypatch.setenv("FMPC_TILED_NW", kernel[-1])
    path = {"wave": pkg.FMPC_PATH_WAVE, "generic-lds": pkg.FMPC_PATH_GENERIC}.get(kernel, pkg._lib.FMPC_PATH_TILED)
    res = solver_case(pkg, "xbox-27x144x6", budget, path, "x box, n = 27, " + kernel)
    assert np.all((res["stp"][:, 0] > 0) & (res["stp"][:, 0] < 1))
    assert not kernel.startswith("tiled") or res["waves"] == int(kernel[-1])


# ------------------------------------------------------------------------------------------------------------- generic kernel
@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("name", ["8x5x10", "27x144x6"])
def test_generic_kernel_lds_instance(pkg, gpu, monkeypatch, name, budget):
    """fmpc_newton_generic<false> (FMPC_FORCE_GENERIC=1: tiles in LDS)."""
    monkeypatch.setenv("FMPC_FORCE_GENERIC", "1")
    solver_case(pkg, name, budget, pkg.FMPC_PATH_GENERIC, "generic kernel, LDS instance")


@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("name", ["8x5x10", "20x33x5"])
def test_generic_kernel_workspace_instance_forced(pkg, gpu, monkeypatch, name, budget):
    """fmpc_newton_generic<true> (FMPC_GENERIC_BIG=1: tiles in the workspace) at sizes the other kernels take too; (20, 33, 5) has
    xf, at budget 1 as well."""
    monkeypatch.setenv("FMPC_GENERIC_BIG", "1")
    solver_case(pkg, name, budget, pkg.FMPC_PATH_GENERIC, "generic kernel, workspace instance (forced)")


@pytest.mark.parametrize("name,budget,prec", [("83x7x3", 1, None), ("83x7x3", 5, None), ("100x40x5", 3, None), ("100x40x5", 5, None),
                                              ("70x300x2", 1, "f64"), ("70x300x2", 5, "f64")])
def test_generic_kernel_workspace_instance_on_its_own_sizes(pkg, gpu, name, budget, prec):
    """n > 79, and n = 70 with m = 300 when fp64 is asked for: no other fp64 kernel takes these (tests/test_gpu_any_size.py)."""
    solver_case(pkg, name, budget, pkg.FMPC_PATH_GENERIC, "generic kernel, workspace instance", prec=prec)


# ------------------------------------------------------------------------------------------------------------- one-wavefront kernel
@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("mode", ["shared cold factor", "own factor", "explicit start"])
def test_one_wavefront_kernel_n27(pkg, gpu, monkeypatch, mode, budget):
    """fmpc_newton_wave (FMPC_NO_PANEL=1, FMPC_NO_SMALL_TILED=1) with w: from the cold start with the shared first factor
    (FMPC_PATH_SHARED), from the cold start factoring per problem (FMPC_NO_SHARED=1: the kernel's own mid-box start), and from an
    explicit start inside the box."""
    monkeypatch.setenv("FMPC_NO_PANEL", "1")
    monkeypatch.setenv("FMPC_NO_SMALL_TILED", "1")
    if mode == "own factor":
        monkeypatch.setenv("FMPC_NO_SHARED", "1")
    name = "27x144x6-start" if mode == "explicit start" else "27x144x6"
    solver_case(pkg, name, budget, pkg.FMPC_PATH_SHARED if mode == "shared cold factor" else pkg.FMPC_PATH_WAVE, "one-wavefront kernel, " + mode)


# ------------------------------------------------------------------------------------------------------------- fp32 factor
@pytest.mark.parametrize("budget", [2, 5])
@pytest.mark.parametrize("name", ["33x20x6", "65x20x4", "83x40x4"])
def test_fp32_factor_unrefined(pkg, gpu, name, budget):
    """fmpc_newton_tiled<float> with 3, 5 and 6 blocks: 1e-4 on z and at least the oracle's iterations, after two steps and more
    (tests/hetero_model.py says why not after one).  This bar is wider than what rolling u_min or u_max moves (5e-5 .. 3e-4): the
    constants of this instance are held to 1e-9 by the refined solves below, which read them through the same code."""
    md, data, zi = H.build(name)
    res = run(pkg, md, data, budget, H.CASES[name]["k"], prec="f32", refine=0)
    assert res["path"] == pkg._lib.FMPC_PATH_TILED_F32 and res["sweeps"] == 0, (PATHS[res["path"]], res["sweeps"])
    check(res, H.oracle(name, budget), "fp32 factor %s budget %d" % (name, budget), tol_z=TOL32, tol_nu=np.inf, same_iters=False)


@pytest.mark.parametrize("budget", [2, 5])
@pytest.mark.parametrize("name", ["33x20x6", "65x20x4", "83x40x4"])
def test_fp32_factor_with_one_refinement_sweep(pkg, gpu, name, budget):
    md, data, zi = H.build(name)
    res = run(pkg, md, data, budget, H.CASES[name]["k"], prec="f32", refine=1)
    assert res["path"] == pkg._lib.FMPC_PATH_TILED_F32 and res["sweeps"] == 1, (PATHS[res["path"]], res["sweeps"])
    check(res, H.oracle(name, budget), "fp32 factor, one sweep, %s budget %d" % (name, budget))


# ------------------------------------------------------------------------------------------------------------- dense weights
@pytest.mark.parametrize("budget", [1, 5])
@pytest.mark.parametrize("name", ["8x5x10-Q", "8x5x10-R", "40x21x5-Q", "40x21x5-R"])
def test_dense_weights_with_linear_costs_on_the_tiled_kernel(pkg, gpu, name, budget):
    solver_case(pkg, name, budget, pkg._lib.FMPC_PATH_TILED, "tiled fp64, dense weight")


@pytest.mark.parametrize("budget", [1, 5])
def test_dense_weights_with_linear_costs_on_the_workspace_instance(pkg, gpu, monkeypatch, budget):
    monkeypatch.setenv("FMPC_GENERIC_BIG", "1")
    solver_case(pkg, "8x5x6-QR", budget, pkg.FMPC_PATH_GENERIC, "generic kernel, workspace instance, dense Q, Qf, R")


# ------------------------------------------------------------------------------------------------------------- ramp-rate rows
def ramp_ref(name, budget):
    ref = H.ramp_oracle(name, budget)
    steps = [r[3][:r[2]] for r in ref]
    status = np.array([1 if (canon_steps(s) == 0).any() else 0 for s in steps])
    return np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref]), status, steps


@pytest.mark.parametrize("budget", H.RAMP_BUDGETS)
@pytest.mark.parametrize("name", ["8x5x6-var1", "8x5x6-var2-xf", "20x33x5", "27x144x4-var2-xf"])
def test_ramp_rows_woodbury_cold_step_and_lds_kernel(pkg, gpu, monkeypatch, name, budget):
    """The sizes of fmpc_newton_ramp, u_prev placed around umid != 0.  The default handle takes the cold step in its Woodbury form
    (fmpc_ramp_cold, dual form 5: its constant is built by fmpc_ensure_ramp_cold from umid, r, R, the box) and continues with
    fmpc_newton_ramp; under FMPC_NO_RAMP_COLD=1 fmpc_newton_ramp takes every step from its own mid-box start (dual form 0).  Both
    against the dense oracle with ramp rows, and against each other at 1e-10 as in tests/test_gpu_ramp.py."""
    md, data, du_min, du_max, u_prev = H.build_ramp(name)
    ref = ramp_ref(name, budget)
    monkeypatch.delenv("FMPC_NO_RAMP_COLD", raising=False)
    a = run(pkg, md, data, budget, H.RAMP_K, ramp=(du_min, du_max), u_prev=u_prev)
    monkeypatch.setenv("FMPC_NO_RAMP_COLD", "1")
    b = run(pkg, md, data, budget, H.RAMP_K, ramp=(du_min, du_max), u_prev=u_prev)
    assert a["path"] == pkg.FMPC_PATH_RAMP and a["form"] == 5, (PATHS[a["path"]], a["form"])
    assert b["path"] == pkg.FMPC_PATH_RAMP and b["form"] == 0, (PATHS[b["path"]], b["form"])
    check(a, ref, "ramp rows, Woodbury cold step, %s budget %d" % (name, budget))
    check(b, ref, "ramp rows, LDS kernel, %s budget %d" % (name, budget))
    assert np.array_equal(a["it"], b["it"]) and np.array_equal(a["st"], b["st"]) and np.array_equal(canon_steps(a["stp"]), canon_steps(b["stp"]))
    ez = max(rel_err(a["z"][p], b["z"][p]) for p in range(H.RAMP_BATCH))
    print("Woodbury cold step vs general path: z %.2e" % ez)
    assert ez <= TOL_FORMS


@pytest.mark.parametrize("budget", H.RAMP_BUDGETS)
def test_ramp_rows_workspace_kernel(pkg, gpu, budget):
    """fmpc_newton_ramp_ws at n = 65 (tests/test_gpu_ramp_any_size.py::test_n_beyond_64_var1 with T = 3)."""
    md, data, du_min, du_max, u_prev = H.build_ramp("65x12x3")
    res = run(pkg, md, data, budget, H.RAMP_K, ramp=(du_min, du_max), u_prev=u_prev)
    assert res["path"] == pkg.FMPC_PATH_RAMP_WS, PATHS[res["path"]]
    check(res, ramp_ref("65x12x3", budget), "ramp rows, workspace kernel, budget %d" % budget)


@pytest.mark.parametrize("budget", H.RAMP_BUDGETS)
@pytest.mark.parametrize("kernel", ["woodbury", "lds", "workspace"])
def test_x_box_first_step_backtracks_with_ramp_rows(pkg, gpu, monkeypatch, kernel, budget):
    """(8, 5, 6) VAR(1) with |u| <= 0.3 before heterogeneous(), k = 10 and u_prev up to 0.9 of the way to the ramp bounds (the recipe
    of tests/test_gpu_ramp.py::test_ramp_cold_start_woodbury_form): t = 1/2 in the first step of every problem.  The Woodbury cold
    step, fmpc_newton_ramp from its own start (FMPC_NO_RAMP_COLD=1) and fmpc_newton_ramp_ws (fmpc_set_ramp_workspace)."""
    name = "xbox-8x5x6"
    md, data, du_min, du_max, u_prev = H.build_ramp(name)
    if kernel == "lds":
        monkeypatch.setenv("FMPC_NO_RAMP_COLD", "1")
    else:
        monkeypatch.delenv("FMPC_NO_RAMP_COLD", raising=False)
    res = run(pkg, md, data, budget, H.RAMP_CASES[name]["k"], ramp=(du_min, du_max), u_prev=u_prev, ramp_ws=kernel == "workspace")
    want = {"woodbury": (pkg.FMPC_PATH_RAMP, 5), "lds": (pkg.FMPC_PATH_RAMP, 0), "workspace": (pkg.FMPC_PATH_RAMP_WS, 0)}[kernel]
    assert (res["path"], res["form"]) == want, (PATHS[res["path"]], res["form"])
    check(res, ramp_ref(name, budget), "x box, ramp rows, %s, budget %d" % (kernel, budget))
    assert np.all((res["stp"][:, 0] > 0) & (res["stp"][:, 0] < 1))


# ------------------------------------------------------------------------------------------------------------- model bank
@pytest.mark.parametrize("budget", H.BANK_BUDGETS)
@pytest.mark.parametrize("name", list(H.BANK_CASES))
def test_model_bank(pkg, gpu, name, budget):
    """Three VAR models on one heterogeneous set of constants (a bank holds A1, A2 only: weights, costs and bounds are the handle's),
    five problems on models [0, 1, 2, 1, 0], through the entry of tests/test_gpu_bank.py; every problem against its own model's
    oracle.  The x box is NOT covered for the bank's instances of the tiled kernel: that entry solves at k = 1e-2, where no first
    step backtracked in the search (u boxes down to |u| <= 0.03, x0 up to 30 x); the bank instances share the start-point code of
    the tiled kernel's other instances, which test_x_box_first_step_backtracks covers."""
    import torch
    from tests import test_gpu_bank as TB
    assert TB.K == H.BANK_K
    base, models, per, data = H.build_bank(name)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*TB.stack_models(models))
    assert h.model_bank_count == 3
    model_of = torch.tensor(H.BANK_MODEL_OF, dtype=torch.int32, device=gpu)
    out = TB.bank_solve(h, TB.dev_data(data), budget, model_of=model_of)
    path = h.last_dispatch()[0]
    h.close()
    res = dict(z=out["z"], nu=out["nu"], st=out["status"], it=out["iters"], stp=out["step"], path=path, form=0)
    assert path == pkg._lib.FMPC_PATH_TILED, PATHS[path]
    check(res, H.bank_oracle(name, budget), "model bank %s budget %d" % (name, budget))
    assert np.array_equal(out["u0"], out["z"][:, :base["m"]])


# ------------------------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize("ramp", [False, True])
def test_closed_loop_away_from_n27(pkg, gpu, ramp):
    """ClosedLoop at (8, 5, 6), 4 fed-back steps, 3 realisations, one Newton step per solve, against oracle.closed_loop_ref: without
    ramp rows (VAR(2), the tiled kernel) and with them (VAR(1), every step the Woodbury cold step around umid != 0)."""
    import torch
    vo = 1 if ramp else 2
    md, a, du = H.build_loop(vo)
    refs = H.loop_oracle(ramp, vo)
    h = handle_from_model(pkg, md)
    if ramp:
        h.set_ramp(*du)
    loop = pkg.ClosedLoop(h, H.LOOP_R, n_newton=1, k=H.LOOP_K, ramp=ramp)
    U0, X0 = loop.run(torch.from_numpy(np.ascontiguousarray(a)).to(gpu))
    torch.cuda.synchronize()
    U0, X0 = U0.cpu().numpy(), X0.cpu().numpy()
    path, form = h.last_dispatch()[0], h.last_dual_form()
    status = loop.status.cpu().numpy()
    h.close()
    eu = max(rel_err(U0[:, r], refs[r]["u0"]) for r in range(H.LOOP_R)); ex = max(rel_err(X0[:, r], refs[r]["x0"]) for r in range(H.LOOP_R))
    print("closed loop, ramp=%s: path %s, dual form %d, worst u0 %.2e x0 %.2e" % (ramp, PATHS[path], form, eu, ex))
    assert (path, form) == ((pkg.FMPC_PATH_RAMP, 5) if ramp else (pkg._lib.FMPC_PATH_TILED, 0)), (PATHS[path], form)
    assert int(np.abs(status).sum()) == 0 and all((r["status"] == 0).all() for r in refs)
    assert eu <= TOL_LOOP and ex <= TOL_LOOP, (eu, ex)
