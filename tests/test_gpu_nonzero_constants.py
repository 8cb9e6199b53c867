"""Every shared-factor cold-start form of the n = 27 path on a model whose constants do not vanish (tests/nonzero_model.py: linear
costs q, r, qf and a box that is not centred on zero, so umid, xmid, cu, c2, u0c, zc, nuc, e, e0 and ep are all non-zero; the CPU
side of these inputs is pinned by tests/test_nonzero_model_ref.py).  The forms are affine maps of the data with a constant part:
with synthetic.make_model that part is zero, and a wrong constant column of an operand image, a dropped e0 or a sign on ep passes
every other GPU test of these kernels.

Bars (the project's own): against the structured oracle 1e-9 relative on z and on the first moves and 1e-7 on nu, per problem,
with identical iterations, status and step lengths, on EVERY problem of these small batches; between two forms of the library
1e-11, or bit equality where the existing test of that pair demands it; closed loops against oracle.closed_loop 1e-8 over the
fed-back steps.  Every cold case asserts the form that ran (last_dispatch, last_dual_form) and that no problem was handed to the
exact path: a pass through the exact path proves nothing about the form."""
import functools
import importlib
import os

import numpy as np
import pytest

from oracle.closed_loop_ref import closed_loop
from tests.nonzero_model import K_BAR, nonzero_data, nonzero_model, oracle_decision_ratio, scale_box
from tests.test_gpu_stretch import bracket
from tests.util import banded_from_model, canon_steps, handle_from_model, oracle_batch, rel_err

pkg = importlib.import_module("mpc-sensorlessao_amd")

pytestmark = pytest.mark.gpu
TOL_Z, TOL_NU, TOL_FORMS, TOL_LOOP = 1e-9, 1e-7, 1e-11, 1e-8
M = 144

# (T, batch, xf, nu0, var_order): T = 17 is the first horizon at which a stage (16) starts on a tile boundary, and its 17 stage
# offsets 171 j mod 16 give most alignments of a u tile; T = 1, 2 have no or few u tiles and a partial last tile; batch 65 crosses
# a group of 64 problems, batch 17 leaves a ragged column tile
AFFINE_CASES = [(1, 5, True, True, 2), (2, 33, False, True, 2), (3, 17, False, False, 2), (10, 65, True, True, 2), (10, 40, False, True, 1),
                (17, 20, False, False, 2)]


@functools.lru_cache(maxsize=None)
def case(T, batch, xf, nu0, var_order, w=False, m=M, box=1.0, spread=False, n_newton=1):
    """Model, data and the oracle's (z, nu, iters, status, steps) of EVERY problem; computed once per shape and shared (read only)."""
    md = nonzero_model(pkg, T, var_order=var_order, xf=xf, m=m)
    if box != 1.0:
        md = scale_box(md, box)
    data = nonzero_data(pkg, md, batch, nu0=nu0, w=w, scale=np.linspace(0.05, 5.0, batch) if spread else None)
    return md, data, oracle_batch(md, data, n_newton, K_BAR)


def env_handle(md, **env):
    """A handle created with the given switches set (they are read at create time)."""
    for k_, v in env.items():
        os.environ[k_] = v
    try:
        return handle_from_model(pkg, md)
    finally:
        for k_ in env:
            del os.environ[k_]


def to_dev(data, dev):
    import torch
    return {k_: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)) for k_, v in data.items()}


def run_dev(h, t, dev, want_nu=False, want_z=True, pad=0, n_newton=1):
    """One solve_device call into poisoned outputs -> dict of host arrays + (path, handed) and the dual form."""
    import torch
    batch = t["x0"].shape[0]
    big = torch.full((batch, h.nz + pad), -7.0, dtype=torch.float64, device=dev) if want_z else None
    z = None if big is None else (big[:, :h.nz] if pad else big)
    u0 = torch.full((batch, h.m), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((batch,), -99, dtype=torch.int32, device=dev); it = torch.full((batch,), -99, dtype=torch.int32, device=dev)
    stp = torch.full((batch, pkg._lib.load().fmpc_step_ld(n_newton)), float("nan"), dtype=torch.float64, device=dev)
    nu = torch.full((batch, h.nu_len), float("nan"), dtype=torch.float64, device=dev) if want_nu else None
    h.solve_device(t["x0"], t["x0_pre"], t["w"], None, t["nu0"], n_newton, K_BAR, z_out=z, nu_out=nu, status=st, iters=it, step=stp, u0_out=u0,
                   want_z=want_z)
    torch.cuda.synchronize()
    if pad and want_z:
        assert bool((big[:, h.nz:] == -7.0).all()), "something was written between the rows"
    return dict(z=None if z is None else z.cpu().numpy(), u0=u0.cpu().numpy(), st=st.cpu().numpy(), it=it.cpu().numpy(), stp=stp.cpu().numpy(),
                nu=None if nu is None else nu.cpu().numpy(), dispatch=h.last_dispatch(), form=h.last_dual_form())


def check_oracle(res, ref, label, m=M):
    """Every problem against the oracle: z, first moves, nu (where present), iterations, status, step lengths."""
    zo, nuo, ito, sto, steps = ref
    B = zo.shape[0]
    worst = {}
    if res.get("z") is not None:
        assert np.all(np.isfinite(res["z"]))
        worst["z"] = max(rel_err(res["z"][p], zo[p]) for p in range(B))
    if res.get("u0") is not None:
        worst["u0"] = max(rel_err(res["u0"][p], zo[p, :m]) for p in range(B))
    if res.get("nu") is not None:
        worst["nu"] = max(rel_err(res["nu"][p], nuo[p]) for p in range(B))
    print("%s vs oracle: %s" % (label, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert np.array_equal(res["it"], ito) and np.array_equal(res["st"], sto), (label, res["it"], ito, res["st"], sto)
    for p in range(B):
        assert np.array_equal(canon_steps(res["stp"][p, :ito[p]]), canon_steps(steps[p][:ito[p]])), (label, p, res["stp"][p], steps[p])
    assert worst.get("z", 0.0) <= TOL_Z and worst.get("u0", 0.0) <= TOL_Z and worst.get("nu", 0.0) <= TOL_NU, (label, worst)


def check_forms(a, b, label, keys=("z", "nu")):
    """Two forms of the library on the same batch: identical decisions, results within 1e-11 per problem."""
    assert np.array_equal(a["st"], b["st"]) and np.array_equal(a["it"], b["it"]) and np.array_equal(a["stp"], b["stp"]), label
    for key in keys:
        if a.get(key) is None or b.get(key) is None:
            continue
        worst = max(rel_err(a[key][p], b[key][p]) for p in range(a[key].shape[0]))
        print("%s: %s %.2e" % (label, key, worst))
        assert worst <= TOL_FORMS, (label, key, worst)


ALL_BY_THE_FORM = (pkg.FMPC_PATH_PANEL, 0)             # the panel path's kernels produced every result: nothing handed over


def affine_calls(h, t, dev, label):
    """The calls of the affine form that write z: z alone, z with nu+, first moves only.  Each asserts that the affine form ran
    and handed nothing over; z must not change by a bit when nu+ is requested, and u0_out is z[:, :m]."""
    a = run_dev(h, t, dev)
    n_ = run_dev(h, t, dev, want_nu=True)
    f = run_dev(h, t, dev, want_z=False)
    for r_ in (a, n_, f):
        assert r_["dispatch"] == ALL_BY_THE_FORM and r_["form"] == 2, (label, r_["dispatch"], r_["form"])
    assert np.array_equal(n_["z"], a["z"]) and np.array_equal(n_["u0"], a["u0"]), label + ": z changes when nu+ is requested"
    assert np.array_equal(a["u0"], a["z"][:, :M]), label
    return a, n_, f


@pytest.mark.parametrize("T,batch,xf,nu0,var_order", AFFINE_CASES)
def test_affine_step_u_rows_through_nu(gpu, monkeypatch, T, batch, xf, nu0, var_order):
    """(a) fmpc_cold_nu, the default of every call that writes z."""
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    md, data, ref = case(T, batch, xf, nu0, var_order)
    h = handle_from_model(pkg, md)
    a, n_, f = affine_calls(h, to_dev(data, gpu), gpu, "affine (nu)")
    check_oracle(a, ref, "affine (nu) T=%d batch=%d" % (T, batch))
    check_oracle(n_, ref, "affine (nu), nu+ requested")
    check_oracle(f, ref, "first moves only")
    h.close()


@pytest.mark.parametrize("T,batch,xf,nu0,var_order", AFFINE_CASES)
def test_affine_step_direct_product_and_first_moves_only(gpu, monkeypatch, T, batch, xf, nu0, var_order):
    """(b) FMPC_AFFINE_DIRECT=1 (fmpc_cold_affine<true, ..>: every tile one product over d) and z_out = NULL
    (fmpc_cold_affine<false, false>), against the oracle and against (a) under the relations of tests/test_gpu_affine_nu.py:
    decisions, stage-0 rows and first moves bit for bit, nu+ bit for bit (its rows are direct tiles in both), the rest 1e-11."""
    md, data, ref = case(T, batch, xf, nu0, var_order)
    h = handle_from_model(pkg, md)
    t = to_dev(data, gpu)
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    a, an, af = affine_calls(h, t, gpu, "affine (nu)")
    monkeypatch.setenv("FMPC_AFFINE_DIRECT", "1")
    d, dn, df = affine_calls(h, t, gpu, "affine (direct)")
    monkeypatch.delenv("FMPC_AFFINE_DIRECT")
    check_oracle(d, ref, "affine (direct) T=%d batch=%d" % (T, batch))
    check_oracle(dn, ref, "affine (direct), nu+ requested")
    check_oracle(df, ref, "affine, first moves only")
    check_forms(a, d, "u rows through nu+ vs direct product", keys=("z",))
    assert np.array_equal(a["z"][:, :M], d["z"][:, :M]) and np.array_equal(a["u0"], d["u0"])
    assert np.array_equal(an["nu"], dn["nu"])
    assert T == 1 or not np.array_equal(a["z"], d["z"]), "the switch did not select another kernel"
    for r_ in (af, df):
        assert np.array_equal(r_["u0"], a["u0"]) and np.array_equal(r_["st"], a["st"]) and np.array_equal(r_["it"], a["it"])
    h.close()


def test_affine_step_padded_rows(gpu, monkeypatch):
    """(c) T = 3, batch 37: rows at a distance of N_z + 6 = 519 doubles (ordinary stores) and of 528 = 33 * 16 (whole cache lines: the
    kernel instances with non-temporal stores), both kernels.  Bit for bit the contiguous rows; the pad untouched (run_dev)."""
    md, data, ref = case(3, 37, False, True, 2)
    h = handle_from_model(pkg, md)
    t = to_dev(data, gpu)
    assert h.nz + 6 == 519 and (h.nz + 15) % 16 == 0
    for direct in (False, True):
        if direct:
            monkeypatch.setenv("FMPC_AFFINE_DIRECT", "1")
        else:
            monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
        c = run_dev(h, t, gpu)
        check_oracle(c, ref, "contiguous rows, direct=%s" % direct)
        for pad in (6, 15):
            for want_nu in (False, True):
                p = run_dev(h, t, gpu, pad=pad, want_nu=want_nu)
                assert p["dispatch"] == ALL_BY_THE_FORM and p["form"] == 2
                assert np.array_equal(p["z"], c["z"]) and np.array_equal(p["u0"], c["u0"]) and np.array_equal(p["st"], c["st"]), (direct, pad, want_nu)
                check_oracle(p, ref, "padded rows +%d, direct=%s, nu=%s" % (pad, direct, want_nu))
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    h.close()


def host_solve(h, data, n_newton=1):
    z, info = h.solve(data["x0"], data["x0_pre"], data["w"], nu0=data["nu0"], n_newton=n_newton, k=K_BAR, return_info=True)
    return dict(z=z, u0=z[:, :h.m], nu=info["nu"], st=info["status"], it=info["iters"], stp=info["step"], dispatch=h.last_dispatch(), form=h.last_dual_form(),
                cont=continuation_count(h))


def continuation_count(h):
    """Length of the continuation list of the last panel-path solve with a budget > 1 (test entry of the library, not in the header)."""
    import ctypes as C
    fn = h._lib.fmpc_debug_continuation_count
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]; fn.restype = C.c_int
    cnt = C.c_int(-1)
    assert fn(h._h, C.byref(cnt)) == 0
    return cnt.value


def bit_equal_problems(a, b, keys=("z", "nu")):
    return np.array([all(np.array_equal(a[k_][p], b[k_][p]) for k_ in keys) for p in range(a["z"].shape[0])])


DENSE_CASES = ([(T, b, xf, nu0, vo, False, M) for (T, b, xf, nu0, vo) in AFFINE_CASES if T in (1, 3, 10)]
               + [(T, b, xf, True, vo, True, M) for (T, b) in ((3, 20), (8, 16), (10, 33)) for vo in (1, 2) for xf in (False, True)]
               + [(3, 20, False, True, 2, False, 97), (3, 20, True, True, 2, True, 97)])        # partial last column block of B'


@pytest.mark.parametrize("T,batch,xf,nu0,var_order,w,m", DENSE_CASES)
def test_three_kernel_form_and_sweeps_form(gpu, T, batch, xf, nu0, var_order, w, m):
    """(d) fmpc_cold_inv[_rg] + fmpc_cold_dz (FMPC_NO_AFFINE=1: dual form 1) and fmpc_cold_panel + fmpc_cold_dz (FMPC_NO_INV=1: the
    sweeps, dual form 0), without w and with w = 0.05 randn: each against the oracle, and against each other at 1e-11."""
    md, data, ref = case(T, batch, xf, nu0, var_order, w=w, m=m)
    h3 = env_handle(md, FMPC_NO_AFFINE="1")
    hs = env_handle(md, FMPC_NO_INV="1")
    r3 = host_solve(h3, data)
    rs = host_solve(hs, data)
    assert r3["dispatch"] == ALL_BY_THE_FORM and r3["form"] == 1, (r3["dispatch"], r3["form"])
    assert rs["dispatch"] == ALL_BY_THE_FORM and rs["form"] == 0, (rs["dispatch"], rs["form"])
    check_oracle(r3, ref, "three-kernel form", m=m)
    check_oracle(rs, ref, "sweeps form", m=m)
    check_forms(r3, rs, "three-kernel form vs sweeps")
    if not w:
        # the default handle takes the affine form for these solves: the same step once more, through the host entry
        h = handle_from_model(pkg, md)
        ra = host_solve(h, data)
        assert ra["dispatch"] == ALL_BY_THE_FORM and ra["form"] == 2
        check_oracle(ra, ref, "affine form (host entry)", m=m)
        check_forms(ra, r3, "affine form vs three-kernel form")
        h.close()
    h3.close(); hs.close()


@pytest.mark.parametrize("T,batch,nu0,var_order,m", [(3, 17, False, 2, M), (10, 40, True, 1, M), (2, 33, True, 2, M), (3, 20, True, 2, 97)])
def test_dual_solve_fused_into_dz(gpu, T, batch, nu0, var_order, m):
    """(d) the variant tests/test_gpu_dense_form.py::test_dual_solve_fused_into_dz selects (FMPC_FUSE_DZ=1 with FMPC_NO_AFFINE=1:
    d_z computes nu+ itself from [x0; x0_pre] and nuc), against the oracle and the unfused three-kernel form."""
    md, data, ref = case(T, batch, False, nu0, var_order, m=m)
    hf = env_handle(md, FMPC_NO_AFFINE="1", FMPC_FUSE_DZ="1")
    hu = env_handle(md, FMPC_NO_AFFINE="1")
    rf = host_solve(hf, data)
    ru = host_solve(hu, data)
    assert rf["dispatch"] == ALL_BY_THE_FORM and rf["form"] == 1 and ru["dispatch"] == ALL_BY_THE_FORM and ru["form"] == 1
    check_oracle(rf, ref, "dual solve fused into d_z", m=m)
    check_forms(rf, ru, "fused vs unfused d_z")
    # (both report dual form 1: that the switch selected another kernel shows in the rounding -- nu+ is summed inside d_z)
    assert not (np.array_equal(rf["z"], ru["z"]) and np.array_equal(rf["nu"], ru["nu"])), "FMPC_FUSE_DZ=1 did not select another kernel"
    hf.close(); hu.close()


@pytest.mark.parametrize("box,spread", [(1.0, False), (0.002, False), (300.0, False), (2e-6, True)])
@pytest.mark.parametrize("w", [False, True])
def test_newton_budget_three(gpu, w, box, spread):
    """(e) n_newton = 3 at k = 1e-2, T = 10, batch 20: the panel step (fmpc_cold_dz in its next-exit-test variant, the only
    consumer of the tables [c2 | 2R | hp | hm] with c2 = 2R umid + r) decides, compacts, and the tiled kernel continues from the
    iterate it leaves.  Against the oracle at budget 3 (z, nu, iterations, status, all recorded steps) and the exact path
    (FMPC_NO_PANEL=1) at 1e-11.  Four boxes, the asymmetry kept in each:
    x 1      every problem goes on after the panel step (the oracle takes 2 iterations);
    x 0.002  a box as tight as the symmetric model's hand-over tests use.  In this model it hands nothing over: |xmid| ~ 65 puts 2 Q xmid ~ 2e6
             per stage into the dual residual of the start, rho^2 ~ 1e13, and ||e||^2 <= 0.5 rho^2 holds until the box is some 1e-6 wide;
    x 300    the residual after the first step is 1.7e-7 on the oracle, a factor 6 under the exit test's 1e-6, so every problem
             stops after ONE step -- decided from the d_z kernel's residual sums, i.e. from c2 (= 2R umid + r ~ 7000 here): with a
             wrong c2 the problems go to the continuation, which ends them with the same result (the list length tells);
    x 2e-6   with the data scaled by linspace(0.05, 5, 20), the scale chosen on the CPU at which the oracle backtracks in the
             first step (t = 0.5 on the 6 largest problems): those, and every problem whose ||e||^2 / rho^2 on the oracle is above
             0.5, have to be handed over.  Here the continuation's kernel matters (barrier curvature k / s^2 ~ 1e10 against 2R = 2),
             so the comparison with the exact path is made with the continuation on the exact path's own kernel
             (FMPC_NO_SMALL_TILED=1): the handed-over problems are then redone from the cold start by that kernel and must equal
             the exact path bit for bit, as tests/test_gpu_panel.py demands at budget 1, and every other problem meets 1e-11.
             The default continuation (tiled kernel) against that one: 1e-10 on z, the bar of this pair in
             tests/test_gpu_dense_form.py::test_budget_continuation_on_the_tiled_kernel_with_handed_over_problems."""
    md, data, ref = case(10, 20, False, True, 2, w=w, box=box, spread=spread, n_newton=3)
    h = handle_from_model(pkg, md)
    hx = env_handle(md, FMPC_NO_PANEL="1")
    r = host_solve(h, data, n_newton=3)
    rx = host_solve(hx, data, n_newton=3)
    path, handed = r["dispatch"]
    print("budget 3, w=%s, box x %g: iterations %s, %d handed over" % (w, box, r["it"].tolist(), handed))
    assert path == pkg.FMPC_PATH_PANEL and r["form"] >= 1 and rx["dispatch"][0] != pkg.FMPC_PATH_PANEL
    if box in (1.0, 0.002):
        assert handed == 0 and ref[2].min() >= 2, "no problem goes on after the panel step: the case does not test the continuation"
        assert r["cont"] == 20, r["cont"]
    if box == 300.0:
        assert handed == 0 and ref[2].max() == 1, "problems go on after the panel step: the case does not test the exit decision"
        # ... and the panel step itself has to see that: ||r_d(z+, nu+)||^2 = 2.8e-14 on the oracle against the 0.996e-12 its exit
        # decision asks for.  (The continuation would evaluate the exit test exactly and hide a wrong residual sum.)
        assert r["cont"] == 0, "%d problems went to the continuation" % r["cont"]
    if spread:
        unclear = oracle_decision_ratio(banded_from_model(md), data) > 0.5
        assert sum(1 for s_ in ref[4] if s_[0] < 1.0) >= 3, "the oracle does not backtrack in the first step"
        assert 20 > handed >= max(int(unclear.sum()), 3), (handed, int(unclear.sum()))
    check_oracle(r, ref, "budget 3 (panel step + continuation)")
    check_oracle(rx, ref, "budget 3 (exact path)")
    assert np.array_equal(r["st"], rx["st"]) and np.array_equal(r["it"], rx["it"]) and np.array_equal(r["stp"], rx["stp"])
    if spread:
        hw = env_handle(md, FMPC_NO_SMALL_TILED="1")
        rw = host_solve(hw, data, n_newton=3)
        hw.close()
        assert rw["dispatch"] == r["dispatch"] and rw["form"] == r["form"] and rw["cont"] == r["cont"]
        check_oracle(rw, ref, "budget 3 (panel step + one-wavefront continuation)")
        same = bit_equal_problems(rw, rx)
        print("budget 3: %d problems equal the exact path bit for bit, %d handed over" % (int(same.sum()), handed))
        assert int(same.sum()) == handed, (int(same.sum()), handed)
        # (the existing test of the tiled / one-wavefront pair bounds z alone; nu of both is held to the oracle above)
        pairs = ((rw, rx, TOL_FORMS, "one-wavefront continuation vs exact path", ("z", "nu")), (r, rw, 1e-10, "tiled vs one-wavefront continuation", ("z",)))
    else:
        pairs = ((r, rx, TOL_FORMS, "vs exact path", ("z", "nu")),)
    for a_, b_, tol, label, keys in pairs:
        assert np.array_equal(a_["st"], b_["st"]) and np.array_equal(a_["it"], b_["it"]) and np.array_equal(a_["stp"], b_["stp"]), label
        for key in keys:
            worst = max(rel_err(a_[key][p], b_[key][p]) for p in range(20))
            print("budget 3 %s: %s %.2e" % (label, key, worst))
            assert worst <= tol, (label, key, worst)
    h.close(); hx.close()


LOOP_STEPS, LOOP_T, LOOP_RMAX = 6, 10, 70


@functools.lru_cache(maxsize=None)
def loop_case(var_order):
    """Turbulence of LOOP_RMAX realisations, nu0 per step, and the oracle loop of realisations 0, 1, 2 (a batch of R uses the
    first R realisations: the oracle loops are shared)."""
    md = nonzero_model(pkg, LOOP_T, var_order=var_order)
    a = np.stack([pkg.synthetic.make_realisation(md, r=r, steps=LOOP_STEPS)[1:LOOP_STEPS + 1] for r in range(LOOP_RMAX)], axis=1)
    nu0 = np.random.default_rng(1).random((LOOP_STEPS, LOOP_RMAX, LOOP_T * 27))
    refs = [closed_loop(md, a[:, r], 1, K_BAR, nu0=nu0[:, r]) for r in range(3)]
    return md, a, nu0, refs


@pytest.mark.parametrize("R,var_order,mode,form", [(5, 2, "step", 1), (40, 2, "step", 1), (40, 1, "step", 1), (70, 2, "step", 4), (70, 2, "nofuse", 3),
                                                   (7, 2, "recorded", 1)])
def test_first_move_forms_in_the_closed_loop(gpu, monkeypatch, R, var_order, mode, form):
    """(f) ClosedLoop(keep_z=False), 6 fed-back steps at T = 10: fmpc_first_move / fmpc_loop_step27 (R <= 64), fmpc_loop_u0 fused
    (dual form 4) and with FMPC_NO_LOOP_FUSE=1 (3), fmpc_first_move_run (run_recorded): u0 = u0c + K0 d and the decision from
    d'E d + 2 e'd + e0 and d'Ep d - 2 ep'd + ep0, whose constants u0c, e, e0, ep vanish in the symmetric model."""
    import torch
    md, a, nu0, refs = loop_case(var_order)
    at = torch.from_numpy(np.ascontiguousarray(a[:, :R])).to(gpu)
    nt = torch.from_numpy(np.ascontiguousarray(nu0[:, :R])).to(gpu)
    h1 = handle_from_model(pkg, md)
    h2 = env_handle(md, FMPC_NO_LOOP_FUSE="1") if mode == "nofuse" else handle_from_model(pkg, md)
    la = pkg.ClosedLoop(h1, R, n_newton=1, k=K_BAR)
    lb = pkg.ClosedLoop(h2, R, n_newton=1, k=K_BAR, keep_z=False)
    Ua, Xa = la.run(at, nt)
    torch.cuda.synchronize()
    assert h1.last_dispatch() == ALL_BY_THE_FORM
    if mode == "recorded":
        Ub, Xb = lb.run_recorded(at, nt)
        torch.cuda.synchronize()
    else:
        Ub = torch.empty_like(Ua); Xb = torch.empty_like(Xa)
        for s in range(LOOP_STEPS):
            Ub[s].copy_(lb.step(at[s], nt[s])); Xb[s].copy_(lb.x0)
            torch.cuda.synchronize()
            assert h2.last_dispatch() == ALL_BY_THE_FORM, (s, h2.last_dispatch())
    assert lb.z is None and h2.last_dispatch() == ALL_BY_THE_FORM and h2.last_dual_form() == form, (h2.last_dispatch(), h2.last_dual_form())
    assert int(la.status.abs().sum()) == 0 and int(lb.status.abs().sum()) == 0 and torch.equal(la.iters, lb.iters)
    Ua, Xa, Ub, Xb = (x.cpu().numpy() for x in (Ua, Xa, Ub, Xb))
    eu, ex, ew = rel_err(Ub, Ua), rel_err(Xb, Xa), rel_err(lb.w.cpu().numpy(), la.w.cpu().numpy())
    print("first moves only vs the loop that keeps z: u0 %.2e, x0 %.2e, w %.2e" % (eu, ex, ew))
    assert max(eu, ex, ew) <= TOL_FORMS
    for r in range(3):
        ref = refs[r]
        assert (ref["status"] == 0).all()
        for name, U, X in (("keeps z", Ua, Xa), ("first moves only", Ub, Xb)):
            eu, ex = rel_err(U[:, r], ref["u0"]), rel_err(X[:, r], ref["x0"])
            print("realisation %d, %s vs oracle loop: u0 %.2e, x0 %.2e" % (r, name, eu, ex))
            assert eu <= TOL_LOOP and ex <= TOL_LOOP
    h1.close(); h2.close()


def test_first_move_decision_forms_with_nonzero_constants(gpu):
    """(f) The two quadratic forms the first-move kernel decides on, ||e||^2 = d'E d + 2 e'd + e0 and ||r_p||^2 = d'Ep d - 2 ep'd + ep0,
    against the same sums of the oracle's Newton step, realisation by realisation over fed-back steps, with the bars of
    tests/test_gpu_closed_loop.py::test_first_move_decision_forms_against_the_oracle.  The trajectories cannot see these constants
    (the decision is clear by orders of magnitude); here e0 is most of ||e||^2 and ep0 most of ||r_p||^2."""
    import ctypes as C
    import torch
    md, a, _, _ = loop_case(2)
    R, steps = 4, 4
    at = torch.from_numpy(np.ascontiguousarray(a[:steps, :R])).to(gpu)
    h = handle_from_model(pkg, md)
    forms = torch.zeros((R, 3), dtype=torch.float64, device=gpu)
    fn = h._lib.fmpc_debug_first_move_forms
    fn.argtypes = [C.c_void_p, C.c_void_p]; fn.restype = C.c_int
    assert fn(h._h, C.c_void_p(forms.data_ptr())) == 0
    lp = pkg.ClosedLoop(h, R, n_newton=1, k=K_BAR, keep_z=False)
    orc = banded_from_model(md)
    worst_e, worst_p = 0.0, 0.0
    for s_ in range(steps):
        lp.step(at[s_])
        torch.cuda.synchronize()
        assert h.last_dispatch() == ALL_BY_THE_FORM and h.last_dual_form() == 1
        f = forms.cpu().numpy()
        x0, x0p, w = lp.x0.cpu().numpy(), lp.x0_pre.cpu().numpy(), lp.w.cpu().numpy()
        for r in range(R):
            info = {}
            orc.solve(x0[r], x0p[r], w[r], 1, K_BAR, info=info)
            eps2, rp2 = info["eps2"][0], info["rp2"][0]
            guard = 1e-9 * (eps2 + rp2 + 1.0)
            assert f[r, 0] >= eps2 - guard and f[r, 1] <= rp2 + guard, (s_, r, f[r], eps2, rp2)
            worst_e = max(worst_e, abs(f[r, 0] - eps2) / (eps2 + 1e-30)); worst_p = max(worst_p, abs(f[r, 1] - rp2) / (rp2 + 1e-30))
            assert f[r, 2] <= info["rho2"][0] * (1 + 1e-9)
    assert fn(h._h, None) == 0
    print("decision forms vs the oracle's sums: ||e||^2 %.2e, ||r_p||^2 %.2e" % (worst_e, worst_p))
    assert worst_e <= 1e-6 and worst_p <= 1e-6, (worst_e, worst_p)
    h.close()


def test_chain_of_three_steps_in_lanes(gpu, monkeypatch):
    """(g) K = 3 affine steps at T = 3, batch 20, onto distinct buffers inside a stretch bracket (the entry of
    tests/test_gpu_stretch_lanes.py::test_distinct_buffers_run_in_lanes): bit for bit the three eager calls; the last step
    against the oracle."""
    import torch
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    monkeypatch.delenv("FMPC_STRETCH_LANES", raising=False)
    K, batch = 3, 20
    md = nonzero_model(pkg, 3)
    h = handle_from_model(pkg, md)
    datas = [nonzero_data(pkg, md, batch, nu0=True, seed=30 + i) for i in range(K)]
    for i, d in enumerate(datas):
        d["x0"] = d["x0"] * (1.0 + 0.1 * i); d["x0_pre"] = d["x0_pre"] * (1.0 + 0.1 * i)
    sets = []
    for d in datas:
        s = to_dev(d, gpu)
        s.update(z=torch.full((batch, h.nz), -3.0, dtype=torch.float64, device=gpu), nu=torch.full((batch, h.nu_len), -5.0, dtype=torch.float64, device=gpu),
                 u0=torch.zeros((batch, h.m), dtype=torch.float64, device=gpu), st=torch.full((batch,), -9, dtype=torch.int32, device=gpu),
                 it=torch.full((batch,), -9, dtype=torch.int32, device=gpu), stp=torch.zeros((batch, 1), dtype=torch.float64, device=gpu))
        sets.append(s)
    outs = ("z", "nu", "u0", "st", "it", "stp")

    def solve(s):
        h.solve_device(s["x0"], s["x0_pre"], None, None, s["nu0"], 1, K_BAR, z_out=s["z"], nu_out=s["nu"], status=s["st"], iters=s["it"], step=s["stp"],
                       u0_out=s["u0"])

    for s in sets:
        solve(s)
        torch.cuda.synchronize()
        assert h.last_dispatch() == ALL_BY_THE_FORM and h.last_dual_form() == 2
    eager = [{k_: s[k_].clone() for k_ in outs} for s in sets]
    for s in sets:
        for k_, v in (("z", -3.0), ("nu", -5.0), ("u0", 0.0), ("st", -9), ("it", -9), ("stp", 0.0)):
            s[k_].fill_(v)
    with bracket(pkg):
        for s in sets:
            solve(s)
    torch.cuda.synchronize()
    assert h.last_stretch()[0] == K, h.last_stretch()
    assert h.last_dispatch()[1] == 0
    for i, (s, e) in enumerate(zip(sets, eager)):
        for k_ in outs:
            assert torch.equal(s[k_], e[k_]), (i, k_)
    last = sets[-1]
    res = dict(z=last["z"].cpu().numpy(), u0=last["u0"].cpu().numpy(), nu=last["nu"].cpu().numpy(), st=last["st"].cpu().numpy(), it=last["it"].cpu().numpy(),
               stp=last["stp"].cpu().numpy())
    check_oracle(res, oracle_batch(md, datas[-1], 1, K_BAR), "last step of the chain")
    h.close()


HAND_OVER_BOX = 3e-6


def test_hand_over_with_nonzero_constants(gpu, monkeypatch):
    """(h) The (a) model at T = 10 with the box scaled (the asymmetry kept) and the data scaled by linspace(0.05, 5, 40).  At a box
    scaled by 0.002 nothing is flagged in this model and the oracle does not backtrack, nor at any scale down to 1e-5: |xmid| ~ 65
    puts 2 Q xmid ~ 2e6 per stage into the dual residual of the start, rho^2 ~ 1e13 dominates ||e||^2, and the full step removes
    it, so t = 1 keeps being accepted.  Scale chosen on the CPU: 3e-6, where the oracle's own ||e||^2 / rho^2 passes 0.5 inside
    the batch (flagged and accepted problems side by side) and the oracle backtracks on 6 of the 40 problems (t = 0.5; on 34 of
    40 at 1e-6, on none at 1e-5).  Every problem meets the oracle bars; the redone ones equal the exact path bit for bit, as
    tests/test_gpu_affine_nu.py::test_flagged_problems_end_with_the_exact_paths_z and tests/test_gpu_panel.py demand."""
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    md, data, ref = case(10, 40, True, True, 2, box=HAND_OVER_BOX, spread=True)
    t_or = np.array([s[0] for s in ref[4]])
    print("box x %g: the oracle backtracks on %d of 40 problems" % (HAND_OVER_BOX, int((t_or < 1.0).sum())))
    assert (t_or < 1.0).sum() >= 3
    h = handle_from_model(pkg, md)
    hx = env_handle(md, FMPC_NO_PANEL="1")
    t = to_dev(data, gpu)
    a = run_dev(h, t, gpu)
    n_ = run_dev(h, t, gpu, want_nu=True)
    f = run_dev(h, t, gpu, want_z=False)
    x = run_dev(hx, t, gpu, want_nu=True)
    path, handed = a["dispatch"]
    print("box x %g: %d of 40 problems handed to the exact path" % (HAND_OVER_BOX, handed))
    assert path == pkg.FMPC_PATH_PANEL and a["form"] == 2 and x["dispatch"][0] != pkg.FMPC_PATH_PANEL
    unclear = oracle_decision_ratio(banded_from_model(md), data) > 0.5
    assert 3 <= int(unclear.sum()) <= handed < 40, (int(unclear.sum()), handed)
    assert n_["dispatch"] == a["dispatch"] and f["dispatch"] == a["dispatch"]
    check_oracle(a, ref, "hand-over, z")
    check_oracle(n_, ref, "hand-over, z and nu+")
    check_oracle(f, ref, "hand-over, first moves only")
    check_oracle(x, ref, "exact path")
    assert np.array_equal(n_["z"], a["z"]) and np.array_equal(a["u0"], a["z"][:, :M]) and np.array_equal(f["u0"], a["u0"])
    redone = a["stp"][:, 0] != 1.0                  # certainly handed over: the affine kernel only ever accepts t = 1
    assert redone.sum() >= 3
    assert np.array_equal(a["z"][redone], x["z"][redone]) and np.array_equal(n_["nu"][redone], x["nu"][redone])
    # every problem the exact path redid, those it ended with t = 1 too: as many problems equal the exact path bit for bit as
    # were handed over (the affine product of an accepted problem differs from it in rounding)
    same = bit_equal_problems(n_, x)
    print("%d problems equal the exact path bit for bit, %d handed over" % (int(same.sum()), handed))
    assert int(same.sum()) == handed and bool(same[redone].all()), (int(same.sum()), handed)
    assert np.array_equal(a["stp"], x["stp"]) and np.array_equal(a["st"], x["st"])
    check_forms(n_, x, "affine form with hand-over vs exact path")
    h.close(); hx.close()
