"""Per-model first-move form of the bank's cold-start loop step (fmpc_bank_first_move_device; fmpc_bank_first_build_k,
fmpc_first_move_bank): parity with the stored-factor path of the same handle and with the per-model oracle, the hand-over to the
exact path, indexing, lifetime and refusals, HIP graphs, loop_run_bank."""
import importlib

import numpy as np
import pytest

from tests.util import canon_steps, handle_from_model, rel_err
from tests.test_gpu_bank import K, make_bank_case, oracle_per_model, stack_models, torch_dev

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib

pytestmark = pytest.mark.gpu

N, M, T = 27, 144, 30
KEYS = ("u0", "x0", "x0_pre", "w", "status", "iters", "step")


def loop_case(R, steps, seed0, scale=1.0, tweak=None):
    base, models, _ = make_bank_case(N, M, T, R, seed0=seed0)
    if tweak:
        tweak(base)
        for mdl in models:
            a1, a2 = mdl["A1"], mdl["A2"]
            mdl.update(base); mdl["A1"], mdl["A2"] = a1, a2
    a = np.stack([pkg.synthetic.make_realisation(models[r], r=seed0 + r, steps=steps, burn_in=50)[1:steps + 1] for r in range(R)], axis=1)
    return base, models, np.ascontiguousarray(np.reshape(scale, (1, -1, 1)) * a)       # a: (steps, R, n)


def nonvanishing(base):
    """q, r != 0 and asymmetric input bounds: u0c, e, e0 and cu are all non-zero."""
    rng = np.random.default_rng(7)
    base["r"] = 0.05 * rng.standard_normal(M)
    base["q"] = 0.05 * rng.standard_normal(N); base["qf"] = 0.05 * rng.standard_normal(N)
    base["u_max"] = np.asarray(base["u_max"], dtype=float) * (1.0 + 0.5 * rng.random(M))
    base["u_min"] = np.asarray(base["u_min"], dtype=float) * (1.0 + 0.1 * rng.random(M))


def tight(base):
    base["u_max"] = 0.005 * np.asarray(base["u_max"], dtype=float); base["u_min"] = 0.005 * np.asarray(base["u_min"], dtype=float)


def banked(base, models, form=False):
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    h.prefactor_model_bank(K)
    if form:
        h.first_move_model_bank(K)
    return h


def run_steps(h, a, model_of=None, nu0=None, n_newton=1, k=K, fill=0.0, want_z=False, dims=(N, M, T), path=_lib.FMPC_PATH_TILED):
    """steps consecutive loop_step_bank calls with the first moves fed back; every output of every step."""
    torch, dev = torch_dev()
    steps, R, _ = a.shape
    N, M, T = dims
    f64 = dict(dtype=torch.float64, device=dev)
    ta = torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # a[:, perm] comes out of numpy with the permuted axis outermost
    mo = None if model_of is None else torch.from_numpy(np.asarray(model_of, dtype=np.int32)).to(dev)
    tnu = None if nu0 is None else torch.from_numpy(nu0).to(dev)
    x0 = torch.zeros((R, N), **f64); x0p = torch.zeros((R, N), **f64); w = torch.zeros((R, T * N), **f64)
    U = torch.full((steps, R, M), fill, **f64)
    out = {k_: [] for k_ in KEYS}
    took, handed = [], []
    for s in range(steps):
        st = torch.full((R,), -77, dtype=torch.int32, device=dev); it = torch.full((R,), -77, dtype=torch.int32, device=dev)
        sp = torch.full((R, _lib.load().fmpc_step_ld(n_newton)), -5.0, **f64)
        z = torch.zeros((R, h.nz), **f64) if want_z else None
        h.loop_step_bank(ta[s], x0 if s >= 1 else None, U[s - 1] if s >= 1 else None, U[s - 2] if s >= 2 else None, x0, x0p, w,
                         None if tnu is None else tnu[s], n_newton, k, model_of=mo, z_out=z, status=st, iters=it, step=sp, u0_out=U[s])
        torch.cuda.synchronize()
        took.append(h.last_bank_first_move()); handed.append(h.last_dispatch()[1])
        assert h.last_dispatch()[0] == path
        for k_, v in zip(KEYS, (U[s], x0, x0p, w, st, it, sp)):
            out[k_].append(v.cpu().numpy().copy())
    res = {k_: np.stack(v) for k_, v in out.items()}
    res["took"], res["handed"] = took, handed
    return res


def close(on, off, tol):
    for k_ in ("u0", "x0", "x0_pre", "w"):
        d = rel_err(on[k_], off[k_])                                    # relative Frobenius norm, as in tests/test_gpu_closed_loop.py
        print(f"  {k_}: {d:.2e}")
        assert d <= tol, (k_, d)
    assert np.array_equal(on["status"], off["status"]) and np.array_equal(on["iters"], off["iters"])
    for s in range(on["step"].shape[0]):
        assert np.array_equal(canon_steps(on["step"][s]), canon_steps(off["step"][s]))


def oracle_last(models, res, nu0=None):
    """The per-model oracle on the inputs of the last step: first moves and step lengths."""
    nb = T
    data = dict(x0=res["x0"][-1], x0_pre=res["x0_pre"][-1], w=res["w"][-1],
                nu0=np.zeros((len(models), nb * N)) if nu0 is None else nu0[-1])
    z, _, it, st, steps = oracle_per_model(models, data, 1)
    return z[:, :M], np.array([s_[0] if len(s_) else 1.0 for s_ in steps]), st


def three_way(base, models, a, nu0, max_handed):
    h = banked(base, models)
    off = run_steps(h, a, nu0=nu0)
    assert not any(off["took"])
    h.first_move_model_bank(K)
    assert h.bank_first_move_count == len(models)
    on = run_steps(h, a, nu0=nu0)
    assert all(on["took"])
    print("handed over per step:", on["handed"])
    assert max(on["handed"]) <= max_handed
    close(on, off, 1e-11)
    u_or, t_or, st_or = oracle_last(models, off, nu0)
    assert np.all(t_or == 1.0) and np.all(st_or == 0), t_or
    err = rel_err(on["u0"][-1], u_or)
    print(f"first moves against the per-model oracle: {err:.2e}")
    assert err <= 1e-9, err
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 1, 2: parity
@pytest.mark.parametrize("with_nu0", [False, True])
def test_parity_three_ways(with_nu0):
    R, steps = 24, 4
    base, models, a = loop_case(R, steps, 1300)
    nu0 = np.random.default_rng(5).random((steps, R, T * N)) if with_nu0 else None
    three_way(base, models, a, nu0, R // 4)


def test_parity_nonvanishing_constants():
    R, steps = 24, 4
    base, models, a = loop_case(R, steps, 1700, tweak=nonvanishing)
    three_way(base, models, a, None, R // 4)


# ---------------------------------------------------------------------------------------------------------------- 3: hand-over
def test_hand_over_really_happens():
    R, steps = 24, 3
    base, models, a = loop_case(R, steps, 1900, scale=np.where(np.arange(R) % 2 == 0, 10.0, 1.0), tweak=tight)   # every other one pushed into its bounds
    h = banked(base, models)
    off = run_steps(h, a)
    h.first_move_model_bank(K)
    on = run_steps(h, a)
    assert all(on["took"])
    _, t_or, _ = oracle_last(models, off)
    back = t_or < 1.0
    print("oracle backtracks on", int(back.sum()), "of", R, "; handed over per step:", on["handed"])
    assert back.any()
    assert on["handed"][-1] >= int(back.sum())
    assert np.all(off["step"][-1][back, 0] < 1.0) and np.all(on["step"][-1][back, 0] < 1.0)     # none accepted with t = 1
    close(on, off, 1e-10)
    # the hand-over count belongs to the form's dispatch: a bank solve behind it reports none
    torch, dev = torch_dev()
    d = {k_: torch.from_numpy(np.ascontiguousarray(off[k_][-1])).to(dev) for k_ in ("x0", "x0_pre", "w")}
    h.solve_bank_device(d["x0"], d["x0_pre"], d["w"], None, None, 1, K)
    torch.cuda.synchronize()
    assert h.last_dispatch() == (_lib.FMPC_PATH_TILED, 0) and h.last_bank_first_move()
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 4: indexing
def test_indexing():
    torch, dev = torch_dev()
    R, steps = 8, 3
    base, models, a = loop_case(R, steps, 2100)
    h = banked(base, models, form=True)
    ref = run_steps(h, a)
    perm = np.random.default_rng(3).permutation(R)
    got = run_steps(h, a[:, perm], model_of=perm)
    assert all(got["took"])
    for k_ in KEYS:
        assert np.array_equal(got[k_], ref[k_][:, perm]), k_
    # many realisations on few models: no dependence on the batch position
    mo = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1], dtype=np.int32)
    many = run_steps(h, a[:, mo], model_of=mo)
    for k_ in KEYS:
        assert np.array_equal(many[k_], ref[k_][:, mo]), k_
    # an index out of range: FMPC_E_DIM, that realisation's outputs unwritten, the others unchanged
    bad = np.arange(R, dtype=np.int32); bad[2] = R + 5
    one = run_steps(h, a[:1], model_of=bad, fill=-9.0)
    assert one["status"][0][2] == _lib.FMPC_E_DIM and np.all(one["u0"][0][2] == -9.0) and np.all(one["step"][0][2] == -5.0)
    keep = np.arange(R) != 2
    for k_ in KEYS:
        assert np.array_equal(one[k_][0][keep], ref[k_][0][keep]), k_
    h.close()
    # a model with a failed factor: the exact path's results
    nan_models = [dict(mdl) for mdl in models]
    nan_models[3]["A1"] = nan_models[3]["A1"].copy(); nan_models[3]["A1"][0, 0] = np.nan
    h2 = banked(base, nan_models)
    off = run_steps(h2, a[:2])
    h2.first_move_model_bank(K)
    assert h2.bank_first_move_count == R - 1
    on = run_steps(h2, a[:2])
    assert all(on["took"]) and min(on["handed"]) >= 1
    assert np.array_equal(on["status"], off["status"]) and np.array_equal(on["iters"], off["iters"])
    ok = np.arange(R) != 3
    assert np.max(np.abs(on["u0"][:, ok] - off["u0"][:, ok])) <= 1e-11
    assert np.array_equal(np.isnan(on["u0"]), np.isnan(off["u0"]))
    h2.close()


# ---------------------------------------------------------------------------------------------------------------- 5: lifetime, refusals
def test_lifetime_and_fallbacks():
    R, steps = 6, 2
    base, models, a = loop_case(R, steps, 2300)
    h = handle_from_model(pkg, base)
    h.set_model_bank(*stack_models(models))
    off_ns = run_steps(h, a)                                            # the exact path without a stored factor
    h.prefactor_model_bank(K)
    off = run_steps(h, a)
    off2 = run_steps(h, a, n_newton=2)
    offk = run_steps(h, a, k=2 * K)
    offz = run_steps(h, a, want_z=True)
    h.first_move_model_bank(K)
    on = run_steps(h, a)
    h.release_bank_prefactor()                                          # the operands are the form's own memory
    again = run_steps(h, a)
    assert all(again["took"]) and h.bank_first_move_count == R
    # a realisation that was accepted at every step is bitwise what it was; one that was handed over now goes through the exact
    # path without a store: library against library, 1e-10, identical status, iterations and steps
    differs = [p for p in range(R) if not all(np.array_equal(again[k_][:, p], on[k_][:, p]) for k_ in KEYS)]
    print("handed over per step after the release:", again["handed"], "; realisations that differ:", differs)
    assert len(differs) <= sum(again["handed"])
    for p in differs:
        for k_ in ("u0", "x0", "x0_pre", "w"):
            assert rel_err(again[k_][:, p], off_ns[k_][:, p]) <= 1e-10, (p, k_)
        assert np.array_equal(again["status"][:, p], off_ns["status"][:, p]) and np.array_equal(again["iters"][:, p], off_ns["iters"][:, p])
        assert np.array_equal(canon_steps(again["step"][:, p]), canon_steps(off_ns["step"][:, p]))
    h.prefactor_model_bank(K)
    for kw, ref in ((dict(n_newton=2), off2), (dict(k=2 * K), offk), (dict(want_z=True), offz)):
        got = run_steps(h, a, **kw)
        assert not any(got["took"])
        for k_ in KEYS:
            assert np.array_equal(got[k_], ref[k_]), (kw, k_)
    # what drops the form: the next step is bitwise the form-off step
    h.set_precision("f32"); h.set_precision("f64")
    assert h.bank_first_move_count == 0
    h.set_model_bank(*stack_models(models)); h.prefactor_model_bank(K)
    got = run_steps(h, a)
    assert not any(got["took"])
    for k_ in KEYS:
        assert np.array_equal(got[k_], off[k_]), k_
    h.first_move_model_bank(K)
    assert h.bank_first_move_count == R
    h.set_model_bank(*stack_models(models))
    assert h.bank_first_move_count == 0
    h.prefactor_model_bank(K)
    got = run_steps(h, a)                                               # the form is not rebuilt: the form-off step
    assert not any(got["took"])
    for k_ in KEYS:
        assert np.array_equal(got[k_], off[k_]), k_
    h.first_move_model_bank(K)
    h.release_bank_first_move()
    assert h.bank_first_move_count == 0 and not any(run_steps(h, a)["took"])
    h.first_move_model_bank(K)
    h.release_model_bank()
    assert h.bank_first_move_count == 0
    h.close()


def test_refusals_enqueue_nothing():
    """Every FMPC_E_UNSUPPORTED case of the builder: the code, count 0, and the bank loop step behind the refused call is bitwise the
    step in front of it (every output filled with a sentinel first) and does not take the form: nothing was built, nothing ran."""
    torch, dev = torch_dev()
    R = 4
    base, models, a = loop_case(R, 2, 2500)
    lib = _lib.load()
    rng = np.random.default_rng(11)

    def refused(h, a_=None, dims=(N, M, T), path=_lib.FMPC_PATH_TILED):
        before = None if a_ is None else run_steps(h, a_, fill=-9.0, dims=dims, path=path)
        with pytest.raises(pkg.FastMPCError) as e:
            h.first_move_model_bank(K)
        assert e.value.code == _lib.FMPC_E_UNSUPPORTED
        assert h.bank_first_move_count == 0 and not h.last_bank_first_move()
        if a_ is not None:
            after = run_steps(h, a_, fill=-9.0, dims=dims, path=path)
            assert not any(after["took"])
            for k_ in KEYS:
                assert np.array_equal(after[k_], before[k_], equal_nan=True), k_

    def unsupported(fn, *args):
        with pytest.raises(pkg.FastMPCError) as e:
            fn(*args)
        assert e.value.code == _lib.FMPC_E_UNSUPPORTED

    h = handle_from_model(pkg, base)
    refused(h)                                                          # no bank
    h.set_model_bank(*stack_models(models))
    refused(h, a)                                                       # no stored factor
    h.prefactor_model_bank(2 * K)
    refused(h, a)                                                       # ... at this k
    h.prefactor_model_bank(K)
    h.set_ramp(-0.5 * np.ones(M), 0.5 * np.ones(M))
    refused(h)                                                          # ramp-rate rows (the bank's calls refuse them too: no step)
    h.close()
    h = handle_from_model(pkg, base)
    h.set_precision("f32"); h.set_model_bank(*stack_models(models)); h.prefactor_model_bank(K)
    refused(h, a, path=_lib.FMPC_PATH_TILED_F32)                        # fp32 factor
    h.close()
    d8 = (8, 5, 10)
    b8, m8, _ = make_bank_case(*d8, R, seed0=2600)
    h = handle_from_model(pkg, b8); h.set_model_bank(*stack_models(m8)); h.prefactor_model_bank(K)
    refused(h, 0.3 * rng.standard_normal((2, R, 8)), d8)                # a size the first-move kernel does not take
    h.close()
    # dense weights at the kernel's own size (a short horizon keeps the dense-R step quick): refused for the weights alone
    dd = (N, M, 10)
    ad = 0.3 * rng.standard_normal((2, R, N))
    bR, mR, _ = make_bank_case(*dd, R, seed0=2650, dense="R")
    h = handle_from_model(pkg, bR); h.set_model_bank(*stack_models(mR))
    unsupported(h.prefactor_model_bank, K)                              # (a dense R has no stored factor either)
    refused(h, ad, dd)                                                  # dense R
    h.close()
    bQ, mQ, _ = make_bank_case(*dd, R, seed0=2660, dense="Q")
    h = handle_from_model(pkg, bQ); h.set_model_bank(*stack_models(mQ)); h.prefactor_model_bank(K)
    refused(h, ad, dd)                                                  # dense Q, Qf
    h.close()
    assert lib.fmpc_bank_first_move_device(None, K, None) == _lib.FMPC_E_NULL


# ---------------------------------------------------------------------------------------------------------------- 6: graph
def test_form_steps_in_a_graph():
    torch, dev = torch_dev()
    R, steps = 12, 3
    base, models, a = loop_case(R, steps, 2700)
    h = banked(base, models, form=True)
    f64 = dict(dtype=torch.float64, device=dev)
    ta = torch.from_numpy(a).to(dev)

    def buffers():
        return dict(x0=torch.zeros((R, N), **f64), x0_pre=torch.zeros((R, N), **f64), w=torch.zeros((R, T * N), **f64),
                    U=torch.zeros((steps, R, M), **f64), st=torch.zeros(R, dtype=torch.int32, device=dev),
                    it=torch.zeros(R, dtype=torch.int32, device=dev))

    def call(b):
        for s in range(steps):
            h.loop_step_bank(ta[s], b["x0"] if s >= 1 else None, b["U"][s - 1] if s >= 1 else None, b["U"][s - 2] if s >= 2 else None,
                             b["x0"], b["x0_pre"], b["w"], None, 1, K, status=b["st"], iters=b["it"], u0_out=b["U"][s])

    e = buffers()
    call(e)
    torch.cuda.synchronize()
    assert h.last_bank_first_move()
    eager = {k_: v.cpu().numpy() for k_, v in e.items()}
    b = buffers()
    gen0 = h._lib.fmpc_alloc_generation()
    g = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        g.capture_begin()
        call(b)
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s_)
    assert h._lib.fmpc_alloc_generation() == gen0 and h.last_bank_first_move()
    for _ in range(3):
        for v in b.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k_, v in b.items():
            assert np.array_equal(v.cpu().numpy(), eager[k_]), k_
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 7: loop_run_bank
def test_loop_run_bank_takes_the_form():
    torch, dev = torch_dev()
    R, steps = 6, 8
    base, models, a = loop_case(R, steps, 2900)
    h = banked(base, models)
    ta = torch.from_numpy(a).to(dev)
    loop = pkg.ClosedLoop(h, R, n_newton=1, k=K, keep_z=False, bank=True)
    U_off, X_off = [t.cpu().numpy() for t in loop.run_recorded(ta)]
    assert not h.last_bank_first_move()
    h.first_move_model_bank(K)
    loop = pkg.ClosedLoop(h, R, n_newton=1, k=K, keep_z=False, bank=True)
    U_on, X_on = [t.cpu().numpy() for t in loop.run_recorded(ta)]
    torch.cuda.synchronize()
    assert h.last_bank_first_move()
    step = run_steps(h, a)
    assert np.array_equal(step["u0"], U_on) and np.array_equal(step["x0"], X_on)
    assert np.max(np.abs(U_on - U_off)) <= 1e-11 * max(1.0, np.max(np.abs(U_off))) and np.max(np.abs(X_on - X_off)) <= 1e-11 * max(1.0, np.max(np.abs(X_off)))
    h.close()
