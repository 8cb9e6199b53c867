"""VAR(1) / VAR(2) identification at any solver size (fmpc_var_fit_device) and the validation of a model
(fmpc_var_validate_device) vs the numpy restatement of README.md:116-153 (tests/var_fit_ref.py) on the synthetic series.

Tolerance of the fit, per series and per matrix: ||A_j - ref||_F / ||ref||_F <= 1e-14 cond_2(AA'AA), floor 1e-12, with
cond <= 1e9 asserted.  The normal equations square the conditioning and the reference solves them that way; two fp64 CPU
evaluations of them (numpy.linalg.solve; 16-row chunked Gram sums + a Cholesky solve) differ by about 1e-17 cond on these
inputs, so the bar leaves a factor of several hundred over a correct fp64 implementation, while a wrong index or an fp32
accumulation is orders of magnitude beyond it.  rmse, rrmse: 1e-11 relative (fp64 spread between summation orders
<= 3.3e-13 at n = 111)."""
import functools

import numpy as np
import pytest
import torch

from tests.var_fit_ref import identify_var, validate_var

pytestmark = pytest.mark.gpu

# (n, order, num_train, batch): the sizes the issue names, then tails of rows = num_train - order with rows % 16 in {0, 1, 15}
CASES = [(33, 2, 200, 3), (16, 1, 100, 2), (27, 1, 300, 2), (48, 2, 300, 2), (40, 1, 200, 3), (65, 2, 400, 2), (111, 2, 600, 2),
         (224, 1, 700, 1), (5, 1, 40, 1),
         (5, 1, 49, 1), (5, 1, 50, 1), (20, 1, 64, 2), (33, 2, 210, 1), (33, 2, 211, 1), (33, 2, 225, 2)]
COUNTS = (3, 37, 50)


@functools.lru_cache(maxsize=None)
def case_data(pkg, n, order, num_train, batch):
    """Series and the restatement's models, conds and validation figures of a case: computed once, shared, read-only."""
    model = pkg.synthetic.make_model(n, 16, 4, var_order=order)
    series = np.stack([pkg.synthetic.make_realisation(model, r=b + 1, steps=num_train + 60) for b in range(batch)])
    refs = [identify_var(series[b], num_train, order) for b in range(batch)]
    val = {cnt: [validate_var(series[b], refs[b][0], num_train, cnt) for b in range(batch)] for cnt in COUNTS}
    series.setflags(write=False)
    return model, series, refs, val


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def fit(pkg, t, order, num_train, **kw):
    A1, A2, st = pkg.identify_var_device(t, order=order, num_train=num_train, **kw)
    torch.cuda.synchronize()
    return A1, A2, st


def same(x, y):
    return all((a is None and b is None) or torch.equal(a, b) for a, b in zip(x, y))


# ------------------------------------------------------------------------------------------------------------ 1: the restatement
@pytest.mark.parametrize("n,order,num_train,batch", CASES)
def test_fit_matches_numpy_restatement(pkg, gpu, n, order, num_train, batch):
    _, series, refs, _ = case_data(pkg, n, order, num_train, batch)
    A1, A2, st = fit(pkg, torch.from_numpy(series).to(gpu), order, num_train)
    assert int(st.abs().sum()) == 0
    assert (A2 is None) == (order == 1)
    assert tuple(A1.stride()) == (n * n, 1, n)
    for b in range(batch):
        ref, cond = refs[b]
        assert cond <= 1e9, cond
        bar = max(1e-14 * cond, 1e-12)
        for j, A in enumerate((A1, A2)[:order]):
            e = rel(A[b].cpu().numpy(), ref[j])
            print(f"fit ({n}, {order}, {num_train}) series {b} A{j + 1}: {e:.2e} (cond {cond:.2e}, bar {bar:.2e})")
            assert e <= bar, (b, j, e, cond)
    a1, a2, s1 = fit(pkg, torch.from_numpy(series[0]).to(gpu), order, num_train)        # single-series form
    assert torch.equal(a1, A1[0]) and (order == 1 or torch.equal(a2, A2[0])) and int(s1) == 0


# ------------------------------------------------------------------------------------------------------------ 2: recovery
def test_fit_recovers_the_generating_model(pkg, gpu):
    model = pkg.synthetic.make_model(40, 16, 4, var_order=1)
    series = pkg.synthetic.make_realisation(model, r=3, steps=19999)
    A, A2, st = fit(pkg, torch.from_numpy(series).to(gpu), 1, None)
    assert int(st) == 0 and A2 is None
    assert rel(A.cpu().numpy(), model["A1"]) < 0.1


# ------------------------------------------------------------------------------------------------------------ 3: the old entry
@pytest.mark.parametrize("n,num_train,batch", [(27, 1000, 3), (32, 300, 2)])
def test_order2_small_n_is_the_old_kernel(pkg, gpu, n, num_train, batch):
    model = pkg.synthetic.make_model(n, 16, 4)
    series = np.stack([pkg.synthetic.make_realisation(model, r=b + 1, steps=num_train + 60) for b in range(batch)])
    t = torch.from_numpy(series).to(gpu)
    old = pkg.identify_var2_device(t, num_train=num_train)
    new = fit(pkg, t, 2, num_train)
    assert same(old, new)
    assert pkg.var_fit_workspace_bytes(n, 2, batch) == 0                      # no workspace there, NULL accepted (above)


# ------------------------------------------------------------------------------------------------------------ 4: slots
def test_slots_and_batch_position(pkg, gpu):
    n, order, num_train, batch = 33, 2, 200, 5
    _, series, _, _ = case_data(pkg, n, order, num_train, batch)
    t = torch.from_numpy(series).to(gpu)
    full = fit(pkg, t, order, num_train)
    slot = pkg.var_fit_workspace_bytes(n, order, 1)
    assert slot >= 8 * ((2 * n) ** 2 + 2 * n * n) and pkg.var_fit_workspace_bytes(n, order, batch) == batch * slot
    two = fit(pkg, t, order, num_train, workspace=torch.empty(2 * slot, dtype=torch.uint8, device=gpu))
    assert same(full, two)
    one = fit(pkg, t[3:4].contiguous(), order, num_train)
    assert torch.equal(one[0][0], full[0][3]) and torch.equal(one[1][0], full[1][3])
    assert same(full, fit(pkg, t, order, num_train))


# ------------------------------------------------------------------------------------------------------------ 5: status
@pytest.mark.parametrize("bad", ["zero", "nan"])
def test_bad_series_is_reported_alone(pkg, gpu, bad):
    n, order, num_train, batch = 33, 2, 200, 3
    _, series, _, _ = case_data(pkg, n, order, num_train, batch)
    s4 = np.concatenate([series[:1], series[:1], series[1:]])               # good, BAD, good, good
    if bad == "zero":
        s4[1] = 0.0
    else:
        s4[1, 77, 5] = np.nan
    good = fit(pkg, torch.from_numpy(series).to(gpu), order, num_train)
    A1 = torch.full((4, n, n), 7.0, dtype=torch.float64, device=gpu); A2 = torch.full_like(A1, 7.0)
    st = torch.full((4,), 77, dtype=torch.int32, device=gpu)
    out = (A1.transpose(1, 2), A2.transpose(1, 2), st)
    r1, r2, rs = fit(pkg, torch.from_numpy(s4).to(gpu), order, num_train, out=out)
    assert rs.cpu().tolist() == [0, pkg.FMPC_E_NOT_PD_SCHUR, 0, 0]
    assert bool((A1[1] == 7.0).all()) and bool((A2[1] == 7.0).all())         # the sentinel stays
    keep = [0, 2, 3]
    assert torch.equal(r1[keep], good[0]) and torch.equal(r2[keep], good[1])


# ------------------------------------------------------------------------------------------------------------ 6: validation
@pytest.mark.parametrize("n,order,num_train,batch", CASES[:9])
def test_validation_matches_numpy_restatement(pkg, gpu, n, order, num_train, batch):
    _, series, refs, val = case_data(pkg, n, order, num_train, batch)
    t = torch.from_numpy(series).to(gpu)
    # the restatement's own model: the fit's conditioning stays out of it
    A = [torch.from_numpy(np.stack([refs[b][0][j] for b in range(batch)])).to(gpu) for j in range(order)]
    for cnt in COUNTS:
        rmse, rrmse = pkg.validate_var_device(t, A[0], A[1] if order == 2 else None, first=num_train, count=cnt)
        torch.cuda.synchronize()
        assert tuple(rmse.shape) == (batch, n) and tuple(rrmse.shape) == (batch, n)
        for b in range(batch):
            e1 = float(np.max(np.abs(rmse[b].cpu().numpy() - val[cnt][b][0]) / val[cnt][b][0]))
            e2 = float(np.max(np.abs(rrmse[b].cpu().numpy() - val[cnt][b][1]) / val[cnt][b][1]))
            print(f"validate ({n}, {order}, {num_train}) count {cnt} series {b}: rmse {e1:.2e} rrmse {e2:.2e}")
            assert e1 <= 1e-11 and e2 <= 1e-11, (cnt, b, e1, e2)
    only, none = pkg.validate_var_device(t, A[0], A[1] if order == 2 else None, first=num_train, count=37, want_rrmse=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(only, pkg.validate_var_device(t, A[0], A[1] if order == 2 else None, first=num_train, count=37)[0])


def test_validation_constant_column(pkg, gpu):
    n, order, num_train, batch = 33, 2, 200, 3
    _, series, refs, _ = case_data(pkg, n, order, num_train, batch)
    s = series.copy()
    s[1, num_train:num_train + 37, 4] = 0.25                                 # mode 4 of series 1 constant over the stretch
    A = [torch.from_numpy(np.stack([refs[b][0][j] for b in range(batch)])).to(gpu) for j in range(order)]
    rmse, rrmse = pkg.validate_var_device(torch.from_numpy(s).to(gpu), A[0], A[1], first=num_train, count=37)
    torch.cuda.synchronize()
    fin = torch.isfinite(rrmse).cpu().numpy()
    want = np.ones((batch, n), dtype=bool); want[1, 4] = False
    assert np.array_equal(fin, want) and bool(torch.isfinite(rmse).all())
    r0, rr0 = validate_var(s[1], refs[1][0], num_train, 37)
    assert np.max(np.abs(rmse[1].cpu().numpy() - r0) / r0) <= 1e-11


# ------------------------------------------------------------------------------------------------------------ 7: into the bank
@pytest.mark.parametrize("n,m,T,var_order", [(8, 5, 10, 1), (40, 30, 10, 2)])
def test_bank_from_models_of_the_new_entry(pkg, gpu, n, m, T, var_order):
    from tests.test_gpu_bank import bank_solve, check_vs_library, dev_data, make_bank_case, per_model_handles
    from tests.util import handle_from_model
    batch = 6
    base, models, data = make_bank_case(n, m, T, batch, var_order=var_order, seed0=700)
    series = np.stack([pkg.synthetic.make_realisation(models[p], r=40 + p, steps=399, burn_in=100) for p in range(batch)])
    A1, A2, st = fit(pkg, torch.from_numpy(series).to(gpu), var_order, 300)
    assert int(st.abs().sum()) == 0 and tuple(A1.stride()) == (n * n, 1, n)    # passed by pointer, no copy
    h = handle_from_model(pkg, base)
    h.set_model_bank(A1, A2)
    out = bank_solve(h, dev_data(data), 5)
    ident = []
    for p in range(batch):
        mdl = dict(base)
        mdl["A1"] = A1[p].cpu().numpy()
        mdl["A2"] = A2[p].cpu().numpy() if var_order == 2 else np.zeros((n, n))
        ident.append(mdl)
    check_vs_library(out, per_model_handles(ident, data, 5))
    h.close()


# ------------------------------------------------------------------------------------------------------------ 8: graph
def test_fit_and_validation_in_a_graph(pkg, gpu):
    n, order, num_train, batch = 33, 2, 200, 3
    _, series, _, _ = case_data(pkg, n, order, num_train, batch)
    t = torch.from_numpy(series).to(gpu)
    ws = torch.empty(pkg.var_fit_workspace_bytes(n, order, batch), dtype=torch.uint8, device=gpu)
    eager = fit(pkg, t, order, num_train, workspace=ws)
    ev = pkg.validate_var_device(t, eager[0], eager[1], first=num_train, count=37)
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(x) for x in eager)
    ov = tuple(torch.empty_like(x) for x in ev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin()
        pkg.identify_var_device(t, order=order, num_train=num_train, workspace=ws, out=out)
        pkg.validate_var_device(t, out[0], out[1], first=num_train, count=37, out=ov)
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        for x in out + ov:
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same(out, eager) and same(ov, ev)


# ------------------------------------------------------------------------------------------------------------ 9: errors
def test_errors_write_nothing(pkg, gpu):
    L = pkg._lib

    def fit_rc(n, order, num_train, ns, ws_bytes=None):
        t = torch.ones((1, ns, n), dtype=torch.float64, device=gpu)
        A1 = torch.full((1, n, n), 7.0, dtype=torch.float64, device=gpu); A2 = torch.full_like(A1, 7.0)
        st = torch.full((1,), 77, dtype=torch.int32, device=gpu)
        ws = None if ws_bytes is None else torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
        with pytest.raises(pkg.FastMPCError) as e:
            pkg.identify_var_device(t, order=order, num_train=num_train, workspace=ws, out=(A1.transpose(1, 2), A2.transpose(1, 2), st))
        torch.cuda.synchronize()
        assert bool((A1 == 7.0).all()) and bool((A2 == 7.0).all()) and int(st[0]) == 77
        return e.value.code

    assert fit_rc(113, 2, 400, 400, ws_bytes=1 << 20) == L.FMPC_E_UNSUPPORTED     # p = 226
    assert fit_rc(33, 3, 200, 200, ws_bytes=1 << 20) == L.FMPC_E_DIM
    assert fit_rc(33, 2, 67, 200) == L.FMPC_E_DIM                                 # 65 rows, 66 unknowns
    assert fit_rc(33, 2, 200, 150) == L.FMPC_E_DIM                                # num_samples < num_train
    assert fit_rc(33, 2, 200, 200, ws_bytes=pkg.var_fit_workspace_bytes(33, 2, 1) - 8) == L.FMPC_E_DIM

    def val_rc(n, first, count, ns, two=True):
        t = torch.ones((1, ns, n), dtype=torch.float64, device=gpu)
        A = torch.zeros((1, n, n), dtype=torch.float64, device=gpu)
        r = torch.full((1, n), 7.0, dtype=torch.float64, device=gpu); rr = torch.full_like(r, 7.0)
        with pytest.raises(pkg.FastMPCError) as e:
            pkg.validate_var_device(t, A, A if two else None, first=first, count=count, out=(r, rr))
        torch.cuda.synchronize()
        assert bool((r == 7.0).all()) and bool((rr == 7.0).all())
        return e.value.code

    assert val_rc(33, 1, 10, 100) == L.FMPC_E_DIM                                 # first < order
    assert val_rc(33, 0, 10, 100, two=False) == L.FMPC_E_DIM
    assert val_rc(33, 95, 6, 100) == L.FMPC_E_DIM                                 # first + count > num_samples
    assert val_rc(113, 10, 10, 100) == L.FMPC_E_UNSUPPORTED
