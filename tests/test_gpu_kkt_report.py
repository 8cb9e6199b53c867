"""GPU tests of the KKT report (fmpc_kkt_report_device, its bank and host forms; include/fastmpc.h): the panel kernel (n <= 32,
diagonal weights, box rows), the any-size kernel (n > 32, dense Q, Qf, R, ramp rows, the bank) against a float64 numpy function that
builds H, g, P, h, C, b per problem with oracle.dense_ref.DenseFastMPC and evaluates the six definitions literally -- nothing
about the solver is assumed.  Inputs are seeded, of order 1.
Tolerances (a residual norm is a difference of large terms, so the bar is relative to the terms, computed from the same dense
matrices):  rd, rp, nr: 1e-12 (||2Hz|| + ||g|| + k ||P'd|| + ||C'nu|| + ||Cz|| + ||b||);  cost: 1e-12 (|z'Hz| + |g'z|);
barrier: 1e-12 sum |log s_i|;  min_slack: 1e-14 max |h|;  flags exactly -- every reference nr, rp is asserted to be a factor 10
away from the exit thresholds and every reference min_slack 1e-3 away from 0, so the flags cannot hinge on rounding."""
import ctypes as C

import numpy as np
import pytest

from oracle.dense_ref import DenseFastMPC
from tests.util import handle_from_model

pytestmark = pytest.mark.gpu

K = 1e-2
GUARD = 64                                   # doubles of NaN either side of a padded array
RD, RP, NR, COST, BARRIER, MIN_SLACK = range(6)


def _spd(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return scale * (G @ G.T / n + np.eye(n))


def make_model(pkg, n, m, T, var_order=2, dense=False, xf=False, seed=3, bounds=1.0):
    """The shared synthetic dynamics with weights, linear terms and bounds of order 1 (times `bounds`) that tell every entry apart."""
    md = pkg.synthetic.make_model(n, m, T, var_order=var_order)
    rng = np.random.default_rng(seed)
    if dense:
        md["Q"] = _spd(n, 1); md["Qf"] = _spd(n, 2, 2.0); md["R"] = _spd(m, 7)
    else:
        md["Q"] = np.diag(1.0 + rng.random(n)); md["Qf"] = np.diag(2.0 * (1.0 + rng.random(n))); md["R"] = np.diag(1.0 + rng.random(m))
    md["q"] = rng.standard_normal(n); md["r"] = rng.standard_normal(m); md["qf"] = rng.standard_normal(n)
    md["u_min"] = -bounds * (1.0 + rng.random(m)); md["u_max"] = bounds * (1.0 + rng.random(m))
    if xf:
        md["xf"] = rng.standard_normal(n)
    return md


@pytest.fixture(scope="module")
def models(pkg, gpu):
    cache = {}

    def get(n, m, T, var_order=2, dense=False, xf=False, bounds=1.0):
        key = (n, m, T, var_order, dense, xf, bounds)
        if key not in cache:
            md = make_model(pkg, n, m, T, var_order, dense, xf, bounds=bounds)
            cache[key] = (md, handle_from_model(pkg, md))
        return cache[key]

    yield get
    for _, h in cache.values():
        h.close()


def make_inputs(md, R, seed, with_pre=True, with_w=True, ramp=None):
    """x0, x0_pre, w, a strictly feasible z (every box slack >= 0.1 (u_max - u_min); with ramp = (du_min, du_max) every ramp slack
    as well) and nu, all of order 1.  Also u_prev with ramp."""
    n, m, T = md["n"], md["m"], md["T"]
    rng = np.random.default_rng(seed)
    nu_len = n * (T + (1 if md.get("xf") is not None else 0))
    x0 = rng.standard_normal((R, n))
    x0_pre = rng.standard_normal((R, n)) if with_pre else None
    w = rng.standard_normal((R, T * n)) if with_w else None
    Z = np.empty((R, T, m + n))
    span = md["u_max"] - md["u_min"]
    Z[:, :, :m] = md["u_min"] + span * rng.uniform(0.1, 0.9, (R, T, m))
    Z[:, :, m:] = rng.standard_normal((R, T, n))
    u_prev = None
    if ramp is not None:
        du_min, du_max = ramp                                       # a walk whose steps keep 0.1 of the ramp range on either side
        u_prev = md["u_min"] + span * rng.uniform(0.4, 0.6, (R, m))
        prev = u_prev
        for j in range(T):
            step = du_min + (du_max - du_min) * rng.uniform(0.1, 0.9, (R, m))
            Z[:, j, :m] = np.clip(prev + step, md["u_min"] + 0.1 * span, md["u_max"] - 0.1 * span)
            prev = Z[:, j, :m]
    nu = rng.standard_normal((R, nu_len))
    return dict(x0=x0, x0_pre=x0_pre, w=w, z=Z.reshape(R, -1).copy(), nu=nu, u_prev=u_prev)


def dense_problem(md, x0, x0_pre, w, u_prev=None, ramp=None, A1=None, A2=None):
    """H, g, P, h, C, b of one problem from the restated reference (w = None: zeros(T n), the documented superset of quirk D7)."""
    n, m, T = md["n"], md["m"], md["T"]
    A1 = md["A1"] if A1 is None else A1
    A2 = md["A2"] if A2 is None else A2
    w = np.zeros(T * n) if w is None else w
    common = (md["Q"], md["R"], None, md["Qf"], md["q"], md["r"], md["qf"], md["x_min"], md["x_max"], md["u_min"], md["u_max"])
    if md["var_order"] == 2:
        d = DenseFastMPC(*common, None, None, T, x0, np.zeros(n) if x0_pre is None else x0_pre, np.zeros(m), A1, A2, md["B"], w,
                         md.get("xf"), None)
    elif ramp is not None:
        d = DenseFastMPC.var1(*common, ramp[0], ramp[1], T, x0, u_prev, A1, md["B"], w, md.get("xf"), None, ramp=True)
    else:
        d = DenseFastMPC.var1(*common, np.zeros(m), np.zeros(m), T, x0, np.zeros(m), A1, md["B"], w, md.get("xf"), None, ramp=False)
    H, g = d.objective_function()
    P, h = d.inequality_const()
    Cm, b = d.equality_const()
    return H, g, P, h, Cm, b


def kkt_ref(md, inp, k=K, with_nu=True, ramp=None, models_of=None):
    """The six definitions, literally, per problem.  Returns report (R, 6), flags (R,), tol (R, 6): the bar of every field."""
    R = inp["x0"].shape[0]
    rep = np.empty((R, 6)); flags = np.zeros(R, dtype=np.int32); tol = np.empty((R, 6))
    for p in range(R):
        if models_of is not None and models_of[p] is None:                  # outside the bank
            rep[p] = np.nan; tol[p] = 0.0
            continue
        A1, A2 = (None, None) if models_of is None else models_of[p]
        H, g, P, h, Cm, b = dense_problem(md, inp["x0"][p], None if inp["x0_pre"] is None else inp["x0_pre"][p],
                                          None if inp["w"] is None else inp["w"][p],
                                          None if inp["u_prev"] is None or ramp is None else inp["u_prev"][p], ramp, A1, A2)
        z = inp["z"][p]
        nu = inp["nu"][p] if with_nu else np.zeros(b.shape[0])
        s = h - P @ z
        with np.errstate(divide="ignore", invalid="ignore"):
            d = 1.0 / s
            logs = np.log(s)
        Hz2, kPd, Cnu, Cz = 2.0 * (H @ z), k * (P.T @ d), Cm.T @ nu, Cm @ z
        r_d = Hz2 + g + kPd + Cnu
        r_p = Cz - b
        rd, rp = np.linalg.norm(r_d), np.linalg.norm(r_p)
        nr = np.linalg.norm(np.concatenate([r_d, r_p]))
        zHz, gz = z @ H @ z, g @ z
        outside = s.min() <= 0.0
        rep[p] = [rd, rp, nr, zHz + gz, -logs.sum(), s.min()]
        scale = sum(np.linalg.norm(v) for v in (Hz2, g, kPd[np.isfinite(kPd)], Cnu, Cz, b))
        tol[p] = [1e-12 * scale] * 3 + [1e-12 * (abs(zHz) + abs(gz)), 1e-12 * np.abs(logs[np.isfinite(logs)]).sum(), 1e-14 * np.abs(h).max()]
        assert abs(s.min()) >= 1e-3, (p, s.min())                           # the flags cannot hinge on rounding
        if outside:
            rep[p, [RD, NR, BARRIER]] = np.nan
            flags[p] = 2
        elif not with_nu:
            rep[p, [RD, NR]] = np.nan
        else:
            assert not (1e-7 < nr < 1e-5) and not (1e-9 < rp < 1e-7), (p, nr, rp)
            flags[p] = 1 if (nr <= 1e-6 and rp <= 1e-8) else 0
    return rep, flags, tol


def compare(dev_rep, dev_flags, ref, what=""):
    rep, flags, tol = ref
    dev_rep = np.asarray(dev_rep); dev_flags = np.asarray(dev_flags)
    assert dev_rep.shape == rep.shape, what
    for p in range(rep.shape[0]):
        for f in range(6):
            if np.isnan(rep[p, f]):
                assert np.isnan(dev_rep[p, f]), (what, p, f, dev_rep[p, f])
            else:
                err = abs(dev_rep[p, f] - rep[p, f])
                assert err <= tol[p, f], (what, p, f, dev_rep[p, f], rep[p, f], err, tol[p, f])
    assert np.array_equal(dev_flags, flags), (what, dev_flags, flags)


def dev_call(h, gpu, inp, k=K, with_nu=True, bank=False, model_of=None, with_u_prev=False, pad=False):
    """The device call on copies of inp.  pad: z rows 16 ceil(N_z / 16) + 16 apart and report rows 8 apart, NaN in every padding
    and in GUARD doubles either side of both arrays; asserts that nothing outside the report rows was written."""
    import torch
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
    R, nz = inp["z"].shape
    x0, x0_pre, w, nu = t(inp["x0"]), t(inp["x0_pre"]), t(inp["w"]), t(inp["nu"]) if with_nu else None
    u_prev = t(inp["u_prev"]) if with_u_prev else None
    if not pad:
        z, out, flat = t(inp["z"]), None, None
    else:
        ldz, ldr = ((nz + 15) // 16) * 16 + 16, 8
        zbuf = torch.full((2 * GUARD + R * ldz,), float("nan"), dtype=torch.float64, device=gpu)
        z = zbuf[GUARD:GUARD + R * ldz].view(R, ldz)[:, :nz]
        z.copy_(t(inp["z"]))
        flat = torch.full((2 * GUARD + R * ldr,), float("nan"), dtype=torch.float64, device=gpu)
        out = flat[GUARD:GUARD + R * ldr].view(R, ldr)
    fn = h.kkt_report_bank_device if bank else h.kkt_report_device
    kw = dict(model_of=model_of) if bank else {}
    rep, flags = fn(x0, x0_pre, w, z=z, nu=nu, k=k, u_prev=u_prev, out=out, **kw)
    torch.cuda.synchronize()
    if pad:
        body = flat[GUARD:GUARD + R * 8].view(R, 8)
        assert torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[GUARD + R * 8:]).all() and torch.isnan(body[:, 6:]).all()
        assert rep.shape == (R, 6) and rep.data_ptr() == body.data_ptr()
    return rep.cpu().numpy(), flags.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- panel kernel
PANEL_SHAPES = [(27, 144, 3), (8, 5, 1), (8, 5, 2), (8, 5, 4), (32, 16, 3), (5, 33, 3)]


@pytest.mark.parametrize("n,m,T", PANEL_SHAPES)
@pytest.mark.parametrize("var_order,xf", [(2, False), (2, True), (1, False), (1, True)])
def test_panel_random_iterate(pkg, gpu, models, n, m, T, var_order, xf):
    """(a) a random strictly feasible z with a random nu, at ragged batches, x0_pre / w given or NULL, padded rows."""
    md, h = models(n, m, T, var_order, False, xf)
    for R, with_pre, with_w, pad in ((1, True, True, False), (16, False, True, True), (17, True, False, False), (33, False, False, True)):
        inp = make_inputs(md, R, seed=100 + R, with_pre=with_pre, with_w=with_w)
        ref = kkt_ref(md, inp)
        assert (ref[1] == 0).all() and (ref[0][:, NR] > 1e-5).all()
        compare(*dev_call(h, gpu, inp, pad=pad), ref, what=(R, with_pre, with_w, pad))


@pytest.mark.parametrize("n,m,T,var_order,xf", [(27, 144, 3, 2, False), (8, 5, 4, 2, True), (8, 5, 2, 1, False), (5, 33, 3, 2, False)])
def test_panel_infeasible_row_and_primal_only(pkg, gpu, models, n, m, T, var_order, xf):
    """(c) one problem with a u entry pushed past u_max: bit 1, NaN in rd, nr, barrier, the other rows bit for bit as before;
    (d) nu = None: rd and nr NaN, bit 0 clear, the rest computed."""
    md, h = models(n, m, T, var_order, False, xf)
    R, bad = 17, 5
    inp = make_inputs(md, R, seed=7)
    rep0, fl0 = dev_call(h, gpu, inp)
    compare(rep0, fl0, kkt_ref(md, inp))
    j, c = T - 1, m - 1
    inp2 = dict(inp, z=inp["z"].copy())
    inp2["z"][bad, j * (n + m) + c] = md["u_max"][c] + 0.5
    rep1, fl1 = dev_call(h, gpu, inp2)
    ref1 = kkt_ref(md, inp2)
    assert ref1[1][bad] == 2 and np.isnan(ref1[0][bad, [RD, NR, BARRIER]]).all() and abs(ref1[0][bad, MIN_SLACK] + 0.5) < 1e-12
    compare(rep1, fl1, ref1)
    keep = np.arange(R) != bad
    assert np.array_equal(rep1[keep], rep0[keep]) and np.array_equal(fl1[keep], fl0[keep])
    rep2, fl2 = dev_call(h, gpu, inp, with_nu=False)
    ref2 = kkt_ref(md, inp, with_nu=False)
    assert np.isnan(ref2[0][:, [RD, NR]]).all() and (ref2[1] == 0).all()
    compare(rep2, fl2, ref2)
    assert np.array_equal(rep2[:, [RP, COST, BARRIER, MIN_SLACK]], rep0[:, [RP, COST, BARRIER, MIN_SLACK]])


@pytest.mark.parametrize("n,m,T,var_order", [(27, 144, 3, 2), (8, 5, 4, 2), (8, 5, 4, 1)])
def test_solver_iterates(pkg, gpu, models, n, m, T, var_order):
    """(b) z_out, nu_out of solve_device with budgets 1 and 8 at k = 1e-2: the report agrees with the dense definitions at both, nr
    falls from budget 1 to budget 8, and where the solver stopped below its budget it took the reference's tolerance exit, so bit 0
    is set.  The bounds are 8 times those of the other tests: with them the reference's Newton steps from the mid-box start stay inside
    the box, budget 1 leaves nr in [1e-5, 1e-2] and budget 8 stops after two steps with nr <= 1e-8 (float64 numpy oracle on these
    seeds) -- kkt_ref asserts the factor 10 to the thresholds on what the device returns."""
    import torch
    md, h = models(n, m, T, var_order, False, False, bounds=8.0)
    R = 17
    inp = make_inputs(md, R, seed=31)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
    x0, x0_pre, w, nu0 = t(inp["x0"]), t(inp["x0_pre"]), t(inp["w"]), t(np.random.default_rng(32).random(inp["nu"].shape))
    if var_order == 1:
        x0_pre = None                                                   # (ignored by the report; the solve takes none)
    nrs = {}
    for budget in (1, 8):
        nu_out = torch.empty_like(nu0)
        z, status, iters = h.solve_device(x0, x0_pre, w, nu0=nu0, n_newton=budget, k=K, nu_out=nu_out)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() >= 0).all()
        rep, flags = h.kkt_report_device(x0, x0_pre, w, z=z, nu=nu_out, k=K)
        torch.cuda.synchronize()
        got = dict(inp, z=z.cpu().numpy(), nu=nu_out.cpu().numpy())
        rep, flags = rep.cpu().numpy(), flags.cpu().numpy()
        compare(rep, flags, kkt_ref(md, got), what=budget)
        early = iters.cpu().numpy() < budget
        assert (flags[early] & 1).all(), (budget, iters.cpu().numpy(), flags)
        nrs[budget] = rep[:, NR]
    assert (nrs[8] < nrs[1]).all(), nrs


def test_bitwise_repeat_and_graph_replay(pkg, gpu, models):
    """Two calls on the same inputs give the same bits; a call captured in a torch.cuda.graph after one eager warm-up (the panel
    kernel's scratch is sized there: nothing is allocated under capture) replays to the same bits."""
    import torch
    md, h = models(27, 144, 3, 2, False, False)
    R = 33
    inp = make_inputs(md, R, seed=9)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
    x0, x0_pre, w, z, nu = (t(inp[key]) for key in ("x0", "x0_pre", "w", "z", "nu"))
    out = torch.empty((R, 6), dtype=torch.float64, device=gpu); flags = torch.empty(R, dtype=torch.int32, device=gpu)
    h.kkt_report_device(x0, x0_pre, w, z=z, nu=nu, k=K, out=out, flags=flags)
    torch.cuda.synchronize()
    a, fa = out.clone(), flags.clone()
    compare(a.cpu().numpy(), fa.cpu().numpy(), kkt_ref(md, inp))
    out.fill_(float("nan")); flags.fill_(-1)
    h.kkt_report_device(x0, x0_pre, w, z=z, nu=nu, k=K, out=out, flags=flags)
    torch.cuda.synchronize()
    assert torch.equal(out, a) and torch.equal(flags, fa)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.kkt_report_device(x0, x0_pre, w, z=z, nu=nu, k=K, out=out, flags=flags)
    out.fill_(float("nan")); flags.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a) and torch.equal(flags, fa)


# ---------------------------------------------------------------------------------------------------- any-size kernel
@pytest.mark.parametrize("n,m,T,dense,xf", [(40, 12, 3, False, False), (40, 12, 3, False, True), (8, 5, 3, True, False), (8, 5, 3, True, True)])
def test_any_size_kernel(pkg, gpu, models, n, m, T, dense, xf):
    md, h = models(n, m, T, 2, dense, xf)
    for R, with_pre, with_w, pad in ((1, True, True, False), (17, False, False, True)):
        inp = make_inputs(md, R, seed=200 + R, with_pre=with_pre, with_w=with_w)
        compare(*dev_call(h, gpu, inp, pad=pad), kkt_ref(md, inp), what=(R, pad))
    inp = make_inputs(md, 5, seed=41)
    rep0, fl0 = dev_call(h, gpu, inp)
    inp["z"][2, m - 1] = md["u_max"][m - 1] + 0.5                       # (c) and (d) on this kernel
    rep1, fl1 = dev_call(h, gpu, inp)
    compare(rep1, fl1, kkt_ref(md, inp))
    keep = np.arange(5) != 2
    assert fl1[2] == 2 and np.array_equal(rep1[keep], rep0[keep])
    compare(*dev_call(h, gpu, inp, with_nu=False), kkt_ref(md, inp, with_nu=False))


def test_ramp_rows_var1(pkg, gpu):
    """VAR(1) (8, 5, 3) with set_ramp and u_prev, against DenseFastMPC.var1 with its ramp rows; u_prev without set_ramp is refused."""
    import torch
    md = make_model(pkg, 8, 5, 3, var_order=1)
    h = handle_from_model(pkg, md)
    try:
        rng = np.random.default_rng(5)
        ramp = (-(0.3 + 0.2 * rng.random(5)), 0.3 + 0.2 * rng.random(5))
        inp = make_inputs(md, 17, seed=51, ramp=ramp)
        with pytest.raises(pkg.FastMPCError) as e:
            dev_call(h, gpu, inp, with_u_prev=True)
        assert e.value.code == pkg.FMPC_E_UNSUPPORTED
        h.set_ramp(*ramp)
        ref = kkt_ref(md, inp, ramp=ramp)
        assert (ref[0][:, MIN_SLACK] > 1e-3).all()
        compare(*dev_call(h, gpu, inp, with_u_prev=True), ref)
        compare(*dev_call(h, gpu, inp), kkt_ref(md, inp))               # u_prev = NULL: box rows only (the panel kernel)
        inp["z"][3, 0] = inp["u_prev"][3, 0] + ramp[1][0] + 0.05        # a ramp row violated, every box row still satisfied
        assert inp["z"][3, 0] < md["u_max"][0] - 1e-3
        ref = kkt_ref(md, inp, ramp=ramp)
        assert ref[1][3] == 2
        compare(*dev_call(h, gpu, inp, with_u_prev=True), ref)
        # the host entry, and the one-problem class on top of it
        rep, fl = h.kkt_report(inp["x0"], None, inp["w"], z=inp["z"], nu=inp["nu"], k=K, u_prev=inp["u_prev"])
        compare(rep, fl, ref)
        obj = pkg.Fast_MPC2_VAR1(md["Q"], md["R"], None, md["Qf"], md["q"], md["r"], md["qf"], md["x_min"], md["x_max"], md["u_min"],
                                 md["u_max"], ramp[0], ramp[1], 3, inp["x0"][0], inp["u_prev"][0], md["A1"], md["B"], inp["w"][0], None, None)
        d = obj.kkt_report(inp["z"][0], inp["nu"][0], K)
        one = (ref[0][:1], ref[1][:1], ref[2][:1])
        compare(np.array([[d[name] for name in pkg.FMPC_KKT_FIELD_NAMES]]), np.array([int(d["converged"]) | 2 * int(d["infeasible"])]), one)
    finally:
        h.close()


def test_host_entry_and_class(pkg, gpu, models):
    """fmpc_kkt_report on numpy arrays and Fast_MPC2.kkt_report give the device call's report."""
    md, h = models(8, 5, 4, 2, False, True)
    inp = make_inputs(md, 5, seed=61)
    ref = kkt_ref(md, inp)
    compare(*h.kkt_report(inp["x0"], inp["x0_pre"], inp["w"], z=inp["z"], nu=inp["nu"], k=K), ref)
    row, fl = h.kkt_report(inp["x0"][0], inp["x0_pre"][0], inp["w"][0], z=inp["z"][0], nu=None, k=K)
    compare(row[None], np.array([fl]), tuple(v[:1] for v in kkt_ref(md, inp, with_nu=False)))
    obj = pkg.Fast_MPC2(md["Q"], md["R"], None, md["Qf"], md["q"], md["r"], md["qf"], md["x_min"], md["x_max"], md["u_min"], md["u_max"],
                        None, None, 4, inp["x0"][1], inp["x0_pre"][1], None, md["A1"], md["A2"], md["B"], inp["w"][1], md["xf"], None)
    d = obj.kkt_report(inp["z"][1], inp["nu"][1], K)
    assert set(d) == set(pkg.FMPC_KKT_FIELD_NAMES) | {"converged", "infeasible"}
    compare(np.array([[d[name] for name in pkg.FMPC_KKT_FIELD_NAMES]]), np.array([int(d["converged"]) | 2 * int(d["infeasible"])]),
            tuple(v[1:2] for v in ref))


def test_argument_rules_with_a_handle(pkg, gpu, models):
    """0 < ldz < N_z (the one rule that needs the handle) and the rules around it, on dummy pointers that are never read."""
    md, h = models(8, 5, 4, 2, False, False)
    lib, L = pkg.load(), pkg._lib
    P = C.c_void_p(0x1000)
    nz = 4 * 13

    def rep(batch=4, ldz=0, k=K, ldr=0, u_prev=None, z=P):
        return lib.fmpc_kkt_report_device(h._h, batch, P, None, None, u_prev, z, ldz, None, k, P, ldr, None, None)

    assert rep(ldz=nz - 1) == L.FMPC_E_DIM and rep(ldz=1) == L.FMPC_E_DIM
    assert rep(ldr=5) == L.FMPC_E_DIM and rep(k=0.0) == L.FMPC_E_DIM and rep(batch=-1) == L.FMPC_E_DIM
    assert rep(z=None) == L.FMPC_E_NULL
    assert rep(batch=0, ldz=nz + 3, ldr=8) == L.FMPC_OK
    assert rep(u_prev=P) == L.FMPC_E_UNSUPPORTED                        # no fmpc_set_ramp on this handle
    assert lib.fmpc_kkt_report_bank_device(h._h, 4, None, P, None, None, None, P, 0, None, K, P, 0, None, None) == L.FMPC_E_UNSUPPORTED   # no bank


# ---------------------------------------------------------------------------------------------------- bank
@pytest.mark.parametrize("n,m,T,var_order", [(27, 144, 2, 2), (8, 5, 3, 2), (8, 5, 3, 1)])
def test_bank(pkg, gpu, n, m, T, var_order):
    """Three models, model_of with repeats and one index outside the bank, against the dense reference built per problem with that
    problem's A1, A2; model_of = None takes model p; u_prev is refused."""
    import torch
    md = make_model(pkg, n, m, T, var_order=var_order)
    rng = np.random.default_rng(70)
    count = 3
    A1 = np.stack([md["A1"] + 0.05 * rng.standard_normal((n, n)) for _ in range(count)])
    A2 = np.stack([md["A2"] + 0.05 * rng.standard_normal((n, n)) for _ in range(count)]) if var_order == 2 else np.zeros((count, n, n))
    h = handle_from_model(pkg, md)
    try:
        h.set_model_bank(torch.from_numpy(A1).to(gpu), torch.from_numpy(A2).to(gpu) if var_order == 2 else None)
        mo = np.array([2, 0, 0, 1, 7, 2, 1], dtype=np.int32)
        inp = make_inputs(md, mo.size, seed=71)
        per = [(A1[i], A2[i]) if 0 <= i < count else None for i in mo]
        ref = kkt_ref(md, inp, models_of=per)
        assert np.isnan(ref[0][4]).all() and ref[1][4] == 0
        compare(*dev_call(h, gpu, inp, bank=True, model_of=torch.from_numpy(mo).to(gpu)), ref)
        compare(*dev_call(h, gpu, inp, bank=True, model_of=torch.from_numpy(mo).to(gpu), pad=True, with_nu=False),
                kkt_ref(md, inp, models_of=per, with_nu=False))
        inp3 = {key: (None if v is None else v[:count]) for key, v in inp.items()}
        compare(*dev_call(h, gpu, inp3, bank=True), kkt_ref(md, inp3, models_of=[(A1[i], A2[i]) for i in range(count)]))
        with pytest.raises(pkg.FastMPCError) as e:
            dev_call(h, gpu, inp, bank=True)                            # model_of = None with batch > count
        assert e.value.code == pkg.FMPC_E_UNSUPPORTED
    finally:
        h.close()
