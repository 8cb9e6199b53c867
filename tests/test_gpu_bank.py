"""Model bank on the GPU: one VAR model (A1, A2) per problem of a batched solve (fmpc_bank_set_device, fmpc_solve_bank_device,
fmpc_loop_inputs_bank_device).  The oracles are used one problem at a time with that problem's model.

Models are random per problem (synthetic.make_model with a seed per problem: spectral radius of the companion matrix < 1), the
seeds are fixed, and the oracle ends every problem of every case below with status 0 or FMPC_W_LINESEARCH (checked on the CPU
when the cases were chosen, asserted again here): no problem is excluded from any comparison.

Bars: against the oracle z <= 1e-9 relative, nu <= 1e-7, identical iterations, status and step record;
against the library's own per-model handles (constants built by different code: host, content-interned blocks there, the bank
kernel here) identical iterations, status and steps, z and nu within 1e-10 relative -- the bar tests/test_gpu_ramp.py uses for two
forms whose constants are built by different code."""
import importlib

import numpy as np
import pytest

from tests.util import banded_from_model, canon_steps, handle_from_model, rel_err

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib

pytestmark = pytest.mark.gpu

K = 1e-2
OK_STATUS = (_lib.FMPC_OK, _lib.FMPC_W_LINESEARCH)


def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def make_bank_case(n, m, T, batch, var_order=2, xf=False, seed0=100, with_w=False, dense=None):
    """Shared B, weights, bounds (the handle's); per problem its own A1, A2 and its own data."""
    base = pkg.synthetic.make_model(n, m, T, var_order=var_order)
    rng = np.random.default_rng(seed0)
    if xf:
        base["xf"] = 0.1 * rng.standard_normal(n)
    if dense == "Q":
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        base["Q"] = base["Q"] + 2e3 * (G @ G.T)
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        base["Qf"] = base["Qf"] + 2e3 * (G @ G.T)
    if dense == "R":
        G = rng.standard_normal((m, m)) / np.sqrt(m)
        base["R"] = base["R"] + 0.2 * (G @ G.T)
    models = []
    for p in range(batch):
        mp_ = pkg.synthetic.make_model(n, m, T, seed=seed0 + 1 + p, var_order=var_order)
        mdl = dict(base)
        mdl["A1"], mdl["A2"] = mp_["A1"], mp_["A2"]
        models.append(mdl)
    nb = T + (1 if xf else 0)
    x0 = np.empty((batch, n)); x0p = np.empty((batch, n))
    for p in range(batch):
        a = pkg.synthetic.make_realisation(models[p], r=seed0 + p, steps=1, burn_in=50)
        x0[p], x0p[p] = a[1], a[0]
    data = dict(x0=x0, x0_pre=x0p, w=(0.05 * rng.standard_normal((batch, T * n)) if with_w else None),
                nu0=rng.random((batch, nb * n)))
    return base, models, data


def oracle_per_model(models, data, n_newton, z_init=None):
    B = len(models)
    z, nu, it, st, steps = [], [], np.zeros(B, dtype=int), np.zeros(B, dtype=int), []
    for p, mdl in enumerate(models):
        info = {}
        zz, nn, i_, s_ = banded_from_model(mdl).solve(data["x0"][p], data["x0_pre"][p], None if data["w"] is None else data["w"][p],
                                                      n_newton, K, z_init=None if z_init is None else z_init[p],
                                                      nu0=data["nu0"][p], info=info)
        z.append(zz); nu.append(nn); it[p], st[p] = i_, s_; steps.append(info.get("t", []))
    return np.array(z), np.array(nu), it, st, steps


def stack_models(models, var_order=2):
    torch, dev = torch_dev()
    A1 = torch.from_numpy(np.stack([m_["A1"] for m_ in models])).to(dev)
    A2 = torch.from_numpy(np.stack([m_["A2"] for m_ in models])).to(dev) if var_order == 2 else None
    return A1, A2


def dev_data(data):
    torch, dev = torch_dev()
    return {k_: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)) for k_, v in data.items()}


def bank_solve(h, d, n_newton, model_of=None, z_init=None, use_nu0=True, want_z=True):
    torch, dev = torch_dev()
    batch = d["x0"].shape[0]
    sld = h._lib.fmpc_step_ld(n_newton)
    nu = torch.full((batch, h.nu_len), 7.0, dtype=torch.float64, device=dev)
    step = torch.full((batch, sld), 7.0, dtype=torch.float64, device=dev)
    u0 = torch.full((batch, h.m), 7.0, dtype=torch.float64, device=dev)
    st = torch.full((batch,), 77, dtype=torch.int32, device=dev)
    it = torch.full((batch,), 77, dtype=torch.int32, device=dev)
    z = torch.full((batch, h.nz), 7.0, dtype=torch.float64, device=dev) if want_z else None
    z, st, it = h.solve_bank_device(d["x0"], d["x0_pre"], d["w"], z_init, d["nu0"] if use_nu0 else None, n_newton, K,
                                    model_of=model_of, z_out=z, nu_out=nu, status=st, iters=it, step=step, u0_out=u0, want_z=want_z)
    torch.cuda.synchronize()
    return dict(z=None if z is None else z.cpu().numpy(), nu=nu.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy(),
                step=step.cpu().numpy(), u0=u0.cpu().numpy())


def check_vs_oracle(out, ora, n_newton, ztol=1e-9, nutol=1e-7):
    zo, nuo, ito, sto, stepso = ora
    assert all(s_ in OK_STATUS for s_ in sto), sto                      # the cases were chosen so: nothing is excluded
    assert np.array_equal(out["iters"], ito), (out["iters"], ito)
    assert np.array_equal(out["status"], sto), (out["status"], sto)
    ez = max(rel_err(out["z"][p], zo[p]) for p in range(len(ito)))
    en = max(rel_err(out["nu"][p], nuo[p]) for p in range(len(ito)))
    print(f"bank vs oracle: z {ez:.2e} nu {en:.2e}")
    assert ez <= ztol and en <= nutol, (ez, en)
    for p in range(len(ito)):
        t = canon_steps(out["step"][p][:ito[p]])
        assert np.array_equal(t, canon_steps(stepso[p])), (p, t, stepso[p])
        assert np.array_equal(out["u0"][p], out["z"][p][:out["u0"].shape[1]])


def per_model_handles(models, data, n_newton, prec=None, refine=0, z_init=None):
    """The same batch solved the only way the library had: one handle per model, forced onto the tiled kernel."""
    torch, dev = torch_dev()
    d = dev_data(data)
    res = dict(z=[], nu=[], status=[], iters=[], step=[])
    for p, mdl in enumerate(models):
        h = handle_from_model(pkg, mdl)
        if prec:
            h.set_precision(prec); h.set_refinement(refine)
        h.set_small_batch_kernel(2)
        sl = slice(p, p + 1)
        sld = h._lib.fmpc_step_ld(n_newton)
        nu = torch.empty((1, h.nu_len), dtype=torch.float64, device=dev)
        step = torch.empty((1, sld), dtype=torch.float64, device=dev)
        # an explicit start keeps the solve on the per-problem-factor path (no shared cold-start factor)
        zi = z_init[sl].contiguous() if z_init is not None else cold_start(mdl).to(dev)
        z, st, it = h.solve_device(d["x0"][sl].contiguous(), d["x0_pre"][sl].contiguous(), None if d["w"] is None else d["w"][sl].contiguous(),
                                   zi, d["nu0"][sl].contiguous(), n_newton, K, nu_out=nu, step=step)
        torch.cuda.synchronize()
        assert h.last_dispatch()[0] in (_lib.FMPC_PATH_TILED, _lib.FMPC_PATH_TILED_F32), h.last_dispatch()
        res["z"].append(z.cpu().numpy()[0]); res["nu"].append(nu.cpu().numpy()[0]); res["status"].append(int(st.cpu()[0]))
        res["iters"].append(int(it.cpu()[0])); res["step"].append(step.cpu().numpy()[0])
        h.close()
    return {k_: np.array(v) for k_, v in res.items()}


def cold_start(mdl):
    """The mid-box start the library takes without z_init (fast_mpc_init.m:19-20), as an explicit start."""
    import torch
    T = mdl["T"]
    s = np.concatenate([(mdl["u_min"] + mdl["u_max"]) / 2, (mdl["x_min"] + mdl["x_max"]) / 2])
    return torch.from_numpy(np.tile(s, T)[None, :].copy())


def check_vs_library(out, ref, tol=1e-10):
    assert np.array_equal(out["iters"], ref["iters"]) and np.array_equal(out["status"], ref["status"])
    ez = max(rel_err(out["z"][p], ref["z"][p]) for p in range(len(ref["iters"])))
    en = max(rel_err(out["nu"][p], ref["nu"][p]) for p in range(len(ref["iters"])))
    print(f"bank vs per-model handles: z {ez:.2e} nu {en:.2e}")
    assert ez <= tol and en <= tol, (ez, en)
    for p in range(len(ref["iters"])):
        assert np.array_equal(canon_steps(out["step"][p][:ref["iters"][p]]), canon_steps(ref["step"][p][:ref["iters"][p]]))
    return ez, en


# ---------------------------------------------------------------------------------------------------------------- 3: oracle
@pytest.mark.parametrize("n,m,T,batch,var_order,xf", [
    (27, 144, 30, 64, 2, False), (8, 5, 10, 33, 2, True), (40, 30, 10, 48, 2, False), (65, 144, 12, 6, 2, False),
    (27, 144, 10, 32, 1, False)])
@pytest.mark.parametrize("budget", [1, 5])
def test_bank_parity_with_oracle(n, m, T, batch, var_order, xf, budget):
    base, models, data = make_bank_case(n, m, T, batch, var_order=var_order, xf=xf)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models, var_order))
    assert h.model_bank_count == batch
    out = bank_solve(h, dev_data(data), budget)
    assert h.last_dispatch()[0] == _lib.FMPC_PATH_TILED
    check_vs_oracle(out, oracle_per_model(models, data, budget), budget)
    h.close()


def test_bank_explicit_start_with_w():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(8, 5, 10, 17, with_w=True, seed0=300)
    rng = np.random.default_rng(7)
    zi = np.tile(np.concatenate([np.zeros(5), np.zeros(8)]), 10)[None, :] + 0.3 * rng.standard_normal((17, 130))
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    out = bank_solve(h, dev_data(data), 5, z_init=torch.from_numpy(zi).to(dev))
    check_vs_oracle(out, oracle_per_model(models, data, 5, z_init=zi), 5)
    h.close()


@pytest.mark.parametrize("dense", ["Q", "R"])
def test_bank_dense_weights(dense):
    base, models, data = make_bank_case(8, 5, 6, 9, dense=dense, seed0=400)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    out = bank_solve(h, dev_data(data), 5)
    check_vs_oracle(out, oracle_per_model(models, data, 5), 5)
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 4, 5: the library
@pytest.mark.parametrize("n,m,T,batch", [(27, 144, 30, 12), (8, 5, 10, 12), (40, 30, 10, 8), (65, 144, 12, 4)])
def test_bank_equals_per_model_handles(n, m, T, batch):
    base, models, data = make_bank_case(n, m, T, batch)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    out = bank_solve(h, dev_data(data), 5)
    check_vs_library(out, per_model_handles(models, data, 5))
    h.close()


def test_bank_of_the_handles_own_model():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(27, 144, 10, 16)
    own = [dict(base) for _ in range(16)]
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(own))
    d = dev_data(data)
    zi = cold_start(base).to(dev).repeat(16, 1).contiguous()
    out = bank_solve(h, d, 5, z_init=zi)
    # the shared-model solve, forced onto the tiled kernel (an explicit start: per-problem factor)
    h.set_small_batch_kernel(2)
    sld = h._lib.fmpc_step_ld(5)
    nu = torch.empty((16, h.nu_len), dtype=torch.float64, device=dev); step = torch.empty((16, sld), dtype=torch.float64, device=dev)
    u0 = torch.empty((16, h.m), dtype=torch.float64, device=dev)
    z, st, it = h.solve_device(d["x0"], d["x0_pre"], None, zi, d["nu0"], 5, K, nu_out=nu, step=step, u0_out=u0)
    torch.cuda.synchronize()
    assert h.last_dispatch()[0] == _lib.FMPC_PATH_TILED
    ref = dict(z=z.cpu().numpy(), nu=nu.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy(), step=step.cpu().numpy())
    check_vs_library(out, ref)
    h.close()


def test_bank_first_moves_only():
    """z_out == NULL (want_z=False): the iterate lives in the handle's scratch; u0, nu, status, iterations and steps are bitwise those of
    the full solve."""
    base, models, data = make_bank_case(8, 5, 10, 21, with_w=True, seed0=350)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    d = dev_data(data)
    full = bank_solve(h, d, 5)
    first = bank_solve(h, d, 5, want_z=False)
    assert first["z"] is None
    for key in ("u0", "nu", "status", "iters", "step"):
        assert np.array_equal(first[key], full[key]), key
    assert np.array_equal(full["u0"], full["z"][:, :5])
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 6: indexing
def test_bank_model_of_permutation_and_range():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(8, 5, 10, 24, with_w=True, seed0=500)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    d = dev_data(data)
    ref = bank_solve(h, d, 5)
    perm = np.random.default_rng(3).permutation(24)
    dp = {k_: (None if v is None else v[torch.from_numpy(perm).to(dev)].contiguous()) for k_, v in d.items()}
    mo = torch.from_numpy(perm.astype(np.int32)).to(dev)
    out = bank_solve(h, dp, 5, model_of=mo)
    for key in ("z", "nu", "status", "iters", "step", "u0"):
        assert np.array_equal(out[key], ref[key][perm]), key
    # one index outside the bank: that problem FMPC_E_DIM, iters 0, outputs untouched; all others bitwise as without it
    bad = perm.astype(np.int32).copy(); bad[5] = 24
    outb = bank_solve(h, dp, 5, model_of=torch.from_numpy(bad).to(dev))
    assert outb["status"][5] == _lib.FMPC_E_DIM and outb["iters"][5] == 0
    assert np.all(outb["z"][5] == 7.0) and np.all(outb["nu"][5] == 7.0) and np.all(outb["u0"][5] == 7.0)
    keep = np.arange(24) != 5
    for key in ("z", "nu", "status", "iters", "step", "u0"):
        assert np.array_equal(outb[key][keep], out[key][keep]), key
    bad[5] = -1
    outb = bank_solve(h, dp, 5, model_of=torch.from_numpy(bad).to(dev))
    assert outb["status"][5] == _lib.FMPC_E_DIM and np.array_equal(outb["z"][keep], out["z"][keep])
    h.close()


def test_bank_model_of_repeats():
    torch, dev = torch_dev()
    nprob = 2000
    base, models, _ = make_bank_case(8, 5, 10, 4, seed0=600)
    rng = np.random.default_rng(11)
    data = dict(x0=0.5 * rng.standard_normal((nprob, 8)), x0_pre=0.5 * rng.standard_normal((nprob, 8)), w=None,
                nu0=rng.random((nprob, 80)))
    mo = rng.integers(0, 4, nprob).astype(np.int32)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    d = dev_data(data)
    out = bank_solve(h, d, 3, model_of=torch.from_numpy(mo).to(dev))
    assert all(s_ in OK_STATUS for s_ in out["status"])
    for j in range(4):
        idx = np.nonzero(mo == j)[0]
        ti = torch.from_numpy(idx).to(dev)
        dj = {k_: (None if v is None else v[ti].contiguous()) for k_, v in d.items()}
        sub = bank_solve(h, dj, 3, model_of=torch.full((len(idx),), j, dtype=torch.int32, device=dev))
        for key in ("z", "nu", "status", "iters", "step", "u0"):
            assert np.array_equal(sub[key], out[key][idx]), (j, key)
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 7: fp32 factor
@pytest.mark.parametrize("sweeps", [0, 1])
def test_bank_fp32_factor(sweeps):
    """The bars of tests/test_gpu_refine.py for the same sweeps.  One sweep (_compare_refined there): status, iteration counts and the
    canonicalised step record equal to the oracle's, z within 1e-9 relative (TOL64), nu within 1e-7.  No refinement: iters >= oracle and
    z within 1e-4.
    Against per-model handles in the same arithmetic: iterations, status and steps identical.  The two builders' fp64 blocks differ in
    their last bits, so a few entries of the fp32 images of Y differ by one fp32 ulp -- a perturbation of the size of the fp32 factor's
    own rounding.  With one sweep both sides are within 1e-9 (z) and 1e-7 (nu) of the oracle, so they are within 2e-9 and 2e-7 of each
    other; without refinement nothing tighter than the bar of the unrefined factor against the oracle follows: 1e-4."""
    base, models, data = make_bank_case(65, 144, 12, 6)
    h = handle_from_model(pkg, base)
    h.set_precision("f32"); h.set_refinement(sweeps)
    h.set_model_bank(*stack_models(models))
    out = bank_solve(h, dev_data(data), 5)
    assert h.last_dispatch()[0] == _lib.FMPC_PATH_TILED_F32 and h.last_refinement() == sweeps
    zo, nuo, ito, sto, stepso = oracle_per_model(models, data, 5)
    assert all(s_ in OK_STATUS for s_ in sto)
    ez = [rel_err(out["z"][p], zo[p]) for p in range(6)]
    en = [rel_err(out["nu"][p], nuo[p]) for p in range(6)]
    print(f"fp32 factor, {sweeps} sweeps: z {max(ez):.2e} nu {max(en):.2e}, iters {out['iters'].tolist()} oracle {ito.tolist()}")
    if sweeps:
        assert np.array_equal(out["status"], sto), (out["status"], sto)
        assert np.array_equal(out["iters"], ito), (out["iters"], ito)
        for p in range(6):
            assert ez[p] <= 1e-9, (p, ez[p])
            assert en[p] <= 1e-7, (p, en[p])
            t = canon_steps(out["step"][p][:ito[p]])
            assert np.allclose(t, canon_steps(stepso[p]), rtol=0, atol=0), (p, t, stepso[p])
    else:
        assert np.all(out["iters"] >= ito), (out["iters"], ito)
        assert max(ez) <= 1e-4, ez
    # and the same arithmetic through per-model handles
    ref = per_model_handles(models, data, 5, prec="f32", refine=sweeps)
    assert np.array_equal(out["iters"], ref["iters"]) and np.array_equal(out["status"], ref["status"])
    el = max(rel_err(out["z"][p], ref["z"][p]) for p in range(6))
    eln = max(rel_err(out["nu"][p], ref["nu"][p]) for p in range(6))
    print(f"fp32 factor, {sweeps} sweeps, bank vs per-model handles: z {el:.2e} nu {eln:.2e}")
    for p in range(6):
        assert np.array_equal(canon_steps(out["step"][p][:ref["iters"][p]]), canon_steps(ref["step"][p][:ref["iters"][p]]))
    assert el <= (2e-9 if sweeps else 1e-4) and eln <= (2e-7 if sweeps else 1e-4), (el, eln)
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 8: round trip
def test_bank_from_identified_models():
    torch, dev = torch_dev()
    n, m, T, batch = 8, 5, 10, 6
    base, models, data = make_bank_case(n, m, T, batch, seed0=700)
    series = np.stack([pkg.synthetic.make_realisation(models[p], r=40 + p, steps=399, burn_in=100) for p in range(batch)])   # (batch, 400, n)
    A1, A2 = pkg.identify_var2_device(torch.from_numpy(series).to(dev), 300)[:2]
    assert tuple(A1.stride()) == (n * n, 1, n)                          # passed by pointer, no copy
    h = handle_from_model(pkg, base)
    h.set_model_bank(A1, A2)
    out = bank_solve(h, dev_data(data), 5)
    ident = []
    for p in range(batch):
        mdl = dict(base); mdl["A1"], mdl["A2"] = A1[p].cpu().numpy(), A2[p].cpu().numpy()
        ident.append(mdl)
    check_vs_library(out, per_model_handles(ident, data, 5))
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 9: loop inputs
@pytest.mark.parametrize("n,m,T,var_order", [(27, 144, 30, 2), (8, 5, 10, 2), (40, 30, 10, 1)])
def test_bank_loop_inputs(n, m, T, var_order):
    from oracle.closed_loop_ref import design_matrices
    torch, dev = torch_dev()
    batch = 9
    base, models, _ = make_bank_case(n, m, T, batch, var_order=var_order, seed0=800)
    rng = np.random.default_rng(5)
    a = rng.standard_normal((batch, n)); xl = rng.standard_normal((batch, n))
    u1 = rng.standard_normal((batch, m)); u2 = rng.standard_normal((batch, m))
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models, var_order))
    t = lambda v: torch.from_numpy(v).to(dev)
    for use1, use2, usel in ((True, True, True), (True, False, True), (False, False, False), (False, True, True)):
        x0 = torch.full((batch, n), 7.0, dtype=torch.float64, device=dev); x0p = torch.full_like(x0, 7.0)
        w = torch.full((batch, T * n), 7.0, dtype=torch.float64, device=dev)
        h.loop_inputs_bank(t(a), t(xl) if usel else None, t(u1) if use1 else None, t(u2) if use2 else None, x0, x0p, w)
        torch.cuda.synchronize()
        for p, mdl in enumerate(models):
            M1, M2 = design_matrices(mdl["A1"], mdl["A2"] if var_order == 2 else np.zeros((n, n)), T)
            v1 = mdl["B"] @ u1[p] if use1 else np.zeros(n); v2 = mdl["B"] @ u2[p] if use2 else np.zeros(n)
            wr = -(M1 @ v1) - (M2 @ v2)
            scale = max(np.max(np.abs(wr)), 1e-300)
            assert np.max(np.abs(w[p].cpu().numpy() - wr)) <= 1e-12 * scale, (p, use1, use2)
            assert np.allclose(x0[p].cpu().numpy(), a[p] + v1, rtol=0, atol=1e-13 * max(1.0, np.max(np.abs(a[p] + v1))))
            assert np.array_equal(x0p[p].cpu().numpy(), xl[p] if usel else np.zeros(n))
    # against fmpc_loop_inputs_device of per-model handles, and x0 aliasing x0_last
    x0 = t(xl).clone(); x0p = torch.empty_like(x0); w = torch.empty((batch, T * n), dtype=torch.float64, device=dev)
    h.loop_inputs_bank(t(a), x0, t(u1), t(u2), x0, x0p, w)
    torch.cuda.synchronize()
    assert np.array_equal(x0p.cpu().numpy(), xl)
    for p, mdl in enumerate(models):
        hp = handle_from_model(pkg, mdl)
        x0r = torch.empty((1, n), dtype=torch.float64, device=dev); x0pr = torch.empty_like(x0r)
        wr = torch.empty((1, T * n), dtype=torch.float64, device=dev)
        hp.loop_inputs_device(t(a[p:p + 1]), t(xl[p:p + 1]), t(u1[p:p + 1]), t(u2[p:p + 1]), x0r, x0pr, wr)
        torch.cuda.synchronize()
        scale = float(wr.abs().max())
        assert float((w[p] - wr[0]).abs().max()) <= 1e-12 * scale
        assert float((x0[p] - x0r[0]).abs().max()) <= 1e-13 * max(1.0, float(x0r.abs().max()))
        hp.close()
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 10: errors
def test_bank_unsupported_cases_enqueue_nothing():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(8, 5, 10, 6, seed0=900)
    d = dev_data(data)

    def expect_unsupported(h, dd=d, **kw):
        z = torch.full((dd["x0"].shape[0], h.nz), 7.0, dtype=torch.float64, device=dev)
        st = torch.full((dd["x0"].shape[0],), 77, dtype=torch.int32, device=dev)
        with pytest.raises(pkg.FastMPCError) as e:
            h.solve_bank_device(dd["x0"], dd["x0_pre"], None, None, dd["nu0"], 5, K, z_out=z, status=st, **kw)
        torch.cuda.synchronize()
        assert e.value.code == _lib.FMPC_E_UNSUPPORTED
        assert bool((z == 7.0).all()) and bool((st == 77).all())

    h = handle_from_model(pkg, base)
    expect_unsupported(h)                                               # no bank
    w = torch.full((6, 80), 7.0, dtype=torch.float64, device=dev)
    with pytest.raises(pkg.FastMPCError) as e:
        h.loop_inputs_bank(d["x0"], None, None, None, torch.empty_like(d["x0"]), torch.empty_like(d["x0"]), w)
    assert e.value.code == _lib.FMPC_E_UNSUPPORTED and bool((w == 7.0).all())
    h.set_model_bank(*stack_models(models[:4]))
    expect_unsupported(h)                                               # model_of None with batch > count
    h.set_model_bank(*stack_models(models))
    h.set_z_ld(h.nz + 6)
    expect_unsupported(h)                                               # padded z rows
    h.set_z_ld(0)
    h.set_precision("f32")
    expect_unsupported(h)                                               # the bank was built for the other arithmetic
    h.set_precision("f64")
    h.release_model_bank()
    assert h.model_bank_count == 0
    expect_unsupported(h)
    h.set_ramp(-0.5 * np.ones(5), 0.5 * np.ones(5))                     # ramp rows: no bank form
    with pytest.raises(pkg.FastMPCError) as e:
        h.set_model_bank(*stack_models(models))
    assert e.value.code == _lib.FMPC_E_UNSUPPORTED and h.model_bank_count == 0
    h.close()
    # no fp64 tiled instance: n > 79
    big = pkg.synthetic.make_model(84, 8, 3)
    hb = handle_from_model(pkg, big)
    A = torch.zeros((2, 84, 84), dtype=torch.float64, device=dev)
    with pytest.raises(pkg.FastMPCError) as e:
        hb.set_model_bank(A, A)
    assert e.value.code == _lib.FMPC_E_UNSUPPORTED
    hb.close()


def test_existing_entry_points_ignore_the_bank():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(27, 144, 10, 8, seed0=950)
    d = dev_data(data)

    def run(h):
        outs = []
        for budget, zi in ((1, None), (5, None), (5, cold_start(base).to(dev).repeat(8, 1).contiguous())):
            nu = torch.empty((8, h.nu_len), dtype=torch.float64, device=dev)
            u0 = torch.empty((8, h.m), dtype=torch.float64, device=dev)
            z, st, it = h.solve_device(d["x0"], d["x0_pre"], None, zi, d["nu0"], budget, K, nu_out=nu, u0_out=u0)
            torch.cuda.synchronize()
            outs += [z.cpu().numpy(), nu.cpu().numpy(), u0.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()]
        x0 = torch.empty((8, 27), dtype=torch.float64, device=dev); x0p = torch.empty_like(x0)
        w = torch.empty((8, 270), dtype=torch.float64, device=dev)
        h.loop_inputs_device(d["x0"], d["x0_pre"], torch.from_numpy(outs[2]).to(dev), None, x0, x0p, w)
        torch.cuda.synchronize()
        return outs + [x0.cpu().numpy(), w.cpu().numpy()]

    h0 = handle_from_model(pkg, base)
    plain = run(h0)
    h0.close()
    h1 = handle_from_model(pkg, base)
    h1.set_model_bank(*stack_models(models))
    bank_solve(h1, d, 2)
    banked = run(h1)
    h1.close()
    for a_, b_ in zip(plain, banked):
        assert np.array_equal(a_, b_)


# ---------------------------------------------------------------------------------------------------------------- 11: graphs
def test_bank_solve_in_a_graph():
    torch, dev = torch_dev()
    base, models, data = make_bank_case(8, 5, 10, 12, seed0=1000)
    d = dev_data(data)
    h = handle_from_model(pkg, base)
    A1, A2 = stack_models(models)
    h.set_model_bank(A1, A2)
    eager = bank_solve(h, d, 5)
    z = torch.zeros((12, h.nz), dtype=torch.float64, device=dev); nu = torch.zeros((12, h.nu_len), dtype=torch.float64, device=dev)
    st = torch.zeros(12, dtype=torch.int32, device=dev); it = torch.zeros(12, dtype=torch.int32, device=dev)
    Ab = torch.cat([A1, A1]); Bb = torch.cat([A2, A2])
    torch.cuda.synchronize()
    gen0 = h._lib.fmpc_alloc_generation()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin()
        h.solve_bank_device(d["x0"], d["x0_pre"], None, None, d["nu0"], 5, K, z_out=z, nu_out=nu, status=st, iters=it)
        # growing the bank while the stream is being captured: refused, the capture stays intact
        with pytest.raises(pkg.FastMPCError) as e:
            h.set_model_bank(Ab, Bb)
        assert e.value.code == _lib.FMPC_E_ALLOC
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    assert h._lib.fmpc_alloc_generation() == gen0                        # nothing was allocated by the recorded solve
    assert h.model_bank_count == 12                                      # and the refused call left the bank as it was
    for _ in range(3):
        z.zero_(); nu.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(z.cpu().numpy(), eager["z"]) and np.array_equal(nu.cpu().numpy(), eager["nu"])
        assert np.array_equal(st.cpu().numpy(), eager["status"]) and np.array_equal(it.cpu().numpy(), eager["iters"])
    h.close()
