"""GPU tests of the closed-loop records with the model bank (fmpc_loop_records_bank_device / fmpc_loop_records_run_bank_device): the
chain + panel kernels (n <= 32, diagonal weights), the any-size kernel (n > 32 or dense Q, Qf, R) and the stretch call, where problem
p predicts with model model_of[p].  Reference: float64 numpy with oracle.closed_loop_ref.design_matrices PER MODEL and the
records_ref / stretch_ref formulas of tests/test_gpu_loop_records.py (helpers copied from there), on seeded inputs of order 1; models
from synthetic.make_model(..., seed=...) per problem as in tests/test_gpu_bank.py::make_bank_case (companion spectral radius < 1).
Tolerance: tests.util.rel_err <= 1e-12 on every output, the project's bar for the records and the loop inputs.  The device computes
the prediction as the model's free response, numpy through M1, M2: two orderings of the same sum, which on a CPU differ by at most
1.3e-14 over 40 seeded models at each size used here; every test asserts that difference <= 1e-13 on its own inputs first."""

import numpy as np
import pytest

from oracle.closed_loop_ref import design_matrices
from tests.util import handle_from_model, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12
ORDER_TOL = 1e-13                            # recursion against M1, M2 in numpy
VOLTS = (0.047275, 2.709264, 1.0)            # coeff_a, coeff_b (README.md:350), unit_change
GUARD = 64                                   # doubles of NaN either side of every output
ALL = ("Xp", "xerr", "J", "du", "uv")
NAN = float("nan")


def _spd(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return scale * (G @ G.T / n + np.eye(n))


def make_base(pkg, n, m, T, var_order=2, dense=False, qscale=1.5e4):
    """The shared synthetic model with weights that tell Q, Qf and the entries of R apart (B, weights, bounds: the handle's)."""
    md = pkg.synthetic.make_model(n, m, T, var_order=var_order)
    rng = np.random.default_rng(11)
    if dense:
        md["Q"] = _spd(n, 1, qscale); md["Qf"] = _spd(n, 2, 2.0 * qscale); md["R"] = _spd(m, 7)
    else:
        md["Q"] = np.diag(qscale * (1.0 + rng.random(n))); md["Qf"] = np.diag(2.0 * qscale * (1.0 + rng.random(n)))
        md["R"] = np.diag(1.0 + rng.random(m))
    return md


class Bank:
    """A handle with a bank of `count` seeded models, and per model A1, A2, M1, M2 in numpy."""

    def __init__(self, pkg, dev, n, m, T, count, var_order=2, dense=False, qscale=1.5e4, prec=None, own=False):
        import torch
        self.md = make_base(pkg, n, m, T, var_order, dense, qscale)
        self.models = []
        for j in range(count):
            mj = dict(self.md)
            if not own:                      # own: every model of the bank is the handle's
                src = pkg.synthetic.make_model(n, m, T, seed=101 + j, var_order=var_order)
                mj["A1"], mj["A2"] = src["A1"], src["A2"]
            self.models.append(mj)
        self.A1 = np.stack([mj["A1"] for mj in self.models]); self.A2 = np.stack([mj["A2"] for mj in self.models])
        if var_order == 1:
            assert not self.A2.any()
        MM = [design_matrices(mj["A1"], mj["A2"], T) for mj in self.models]
        self.M1 = np.stack([a for a, _ in MM]); self.M2 = np.stack([b for _, b in MM])
        self.count, self.var_order = count, var_order
        self.h = handle_from_model(pkg, self.md)
        if prec is not None:
            self.h.set_precision(prec)
        self.h.set_model_bank(torch.from_numpy(self.A1).to(dev), torch.from_numpy(self.A2).to(dev) if var_order == 2 else None)


@pytest.fixture(scope="module")
def banks(pkg, gpu):
    cache = {}

    def get(n, m, T, count, var_order=2, dense=False, qscale=1.5e4):
        key = (n, m, T, count, var_order, dense, qscale)
        if key not in cache:
            cache[key] = Bank(pkg, gpu, n, m, T, count, var_order, dense, qscale)
        return cache[key]

    yield get
    for b in cache.values():
        b.h.close()


def model_pattern(R, count):
    """Model indices with repeats and not sorted."""
    return ((7 * np.arange(R) + 3) % count).astype(np.int32)


def volts_ref(u, volts=VOLTS):
    a, b, uc = volts
    return np.sign(u) * (-b + np.sqrt(b * b + 4.0 * a * np.abs(u) * uc)) / (2.0 * a)


def records_ref(bk, mo, x0, x0_pre, w, U, u1, with_J):
    """The definitions with M1, M2 of model mo[p], in float64 numpy; asserts that the free-response recursion gives the same Xp to
    ORDER_TOL.  U: (R, stages, m).  Returns Xp (R, stages, n), xerr (R, stages), J (R,) or None, du, uv."""
    md = bk.md
    n, T, B = md["n"], md["T"], md["B"]
    R, S = U.shape[0], U.shape[1]
    x0_pre = np.zeros((R, n)) if x0_pre is None else x0_pre
    w = np.zeros((R, T * n)) if w is None else w
    Xp = np.empty((R, S, n)); Xc = np.empty((R, S, n))
    for p in range(R):
        M1, M2, A1, A2 = bk.M1[mo[p]], bk.M2[mo[p]], bk.A1[mo[p]], bk.A2[mo[p]]
        p1, p2 = x0[p], x0_pre[p]
        for i in range(S):
            blk = slice(i * n, (i + 1) * n)
            Xp[p, i] = M1[blk] @ x0[p] + M2[blk] @ x0_pre[p] + w[p, blk] + B @ U[p, i]
            p1, p2 = A1 @ p1 + A2 @ p2, p1
            Xc[p, i] = p1 + w[p, blk] + B @ U[p, i]
    order = rel_err(Xc, Xp)
    print(f"  recursion vs M1, M2 in numpy: {order:.2e}")
    assert order <= ORDER_TOL, order
    xerr = np.linalg.norm(Xp, axis=2)
    J = None
    if with_J:
        assert S == T
        J = np.einsum("ria,ab,rib->r", Xp[:, :T - 1], md["Q"], Xp[:, :T - 1]) + np.einsum("ra,ab,rb->r", Xp[:, T - 1], md["Qf"], Xp[:, T - 1]) \
            + np.einsum("ric,cd,rid->r", U, md["R"], U)
    du = U[:, 0] - (0.0 if u1 is None else u1)
    return Xp, xerr, J, du, volts_ref(U[:, 0])


def make_inputs(md, R, seed, ldu_pad=0, first_moves=False):
    """Seeded inputs of order 1; u as a solve's z (rows ldu = T (n + m) + ldu_pad apart, NaN in the padding, the x entries of z random
    too), or as the first moves (R, m).  One entry of u_0 is exactly 0."""
    n, m, T = md["n"], md["m"], md["T"]
    rng = np.random.default_rng(seed)
    x0, x0_pre, w, u1 = rng.standard_normal((R, n)), rng.standard_normal((R, n)), rng.standard_normal((R, T * n)), rng.standard_normal((R, m))
    if first_moves:
        ubuf = rng.standard_normal((R, m))
        ubuf[0, 0] = 0.0
        return x0, x0_pre, w, u1, ubuf, ubuf[:, None, :].copy()
    nz = T * (n + m)
    ubuf = np.full((R, nz + ldu_pad), np.nan)
    ubuf[:, :nz] = rng.standard_normal((R, nz))
    ubuf[0, 0] = 0.0
    U = ubuf[:, :nz].reshape(R, T, n + m)[:, :, :m].copy()
    return x0, x0_pre, w, u1, ubuf, U


class Outputs:
    """The outputs between NaN guard regions, NaN-filled."""
    SIZES = {"Xp": lambda n, m, S: S * n, "xerr": lambda n, m, S: S, "J": lambda n, m, S: 1, "du": lambda n, m, S: m, "uv": lambda n, m, S: m}

    def __init__(self, torch, dev, R, n, m, S, names):
        self.bufs, self.views, self.R = {}, {}, R
        for k in names:
            cnt = R * self.SIZES[k](n, m, S)
            b = torch.full((GUARD + cnt + GUARD,), NAN, dtype=torch.float64, device=dev)
            self.bufs[k] = b
            self.views[k] = b[GUARD:GUARD + cnt]

    def get(self, k):
        return self.views.get(k)

    def check_guards(self, skip=()):
        """Guards intact; the rows of the problems in `skip` still NaN, no NaN elsewhere."""
        for k, b in self.bufs.items():
            assert bool(b[:GUARD].isnan().all()) and bool(b[-GUARD:].isnan().all()), f"{k}: guard overwritten"
            rows = self.views[k].view(self.R, -1).isnan()
            for p in range(self.R):
                assert bool(rows[p].all()) if p in skip else not bool(rows[p].any()), (k, p)


def tdev(torch, dev, v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def call(torch, bk, dev, inp, mo, S, names, nulls=(), h=None, shared=False):
    """One fmpc_loop_records_bank_device call on `inp` (shared: fmpc_loop_records_device); returns the Outputs."""
    md = bk.md
    n, m = md["n"], md["m"]
    x0, x0_pre, w, u1, ubuf, _ = inp
    t = lambda v: tdev(torch, dev, v)
    out = Outputs(torch, dev, x0.shape[0], n, m, S, names)
    tu = t(ubuf)
    h = bk.h if h is None else h
    args = (t(x0), None if "x0_pre" in nulls else t(x0_pre), None if "w" in nulls else t(w), tu, None if "u1" in nulls else t(u1))
    kw = dict(stages=S, ldu=tu.stride(0), stage_stride=n + m, volts=VOLTS, Xp=out.get("Xp"), xerr=out.get("xerr"), J=out.get("J"),
              du=out.get("du"), uv=out.get("uv"))
    if shared:
        h.loop_records_device(*args, **kw)
    else:
        h.loop_records_bank_device(*args, model_of=t(mo), **kw)
    torch.cuda.synchronize()
    return out


def compare(bk, mo, inp, out, S, nulls=(), skip=()):
    x0, x0_pre, w, u1, _, U = inp
    R, n = x0.shape[0], bk.md["n"]
    mo = np.arange(R) if mo is None else mo
    keep = np.array([p for p in range(R) if p not in skip])
    moc = np.where(np.isin(np.arange(R), keep), mo, 0)
    Xp, xerr, J, du, uv = records_ref(bk, moc, x0, None if "x0_pre" in nulls else x0_pre, None if "w" in nulls else w, U[:, :S],
                                      None if "u1" in nulls else u1, "J" in out.views)
    ref = {"Xp": Xp.reshape(R, S * n), "xerr": xerr, "J": J, "du": du, "uv": uv}
    out.check_guards(skip)
    for k, v in out.views.items():
        got = v.cpu().numpy().reshape(R, -1)[keep]
        err = rel_err(got, ref[k].reshape(R, -1)[keep])
        print(f"  {k}: rel err {err:.2e}")
        assert err <= TOL, (k, err)
    if "uv" in out.views and 0 not in skip:
        assert float(out.views["uv"][0]) == 0.0                       # u = 0.0 exactly gives 0.0 V


CASES = [
    # n, m, T, count, var_order, dense, batch, ldu_pad, model_of given
    pytest.param(27, 144, 30, 5, 2, False, 33, 0, True, id="panel-two-panels-and-a-ragged-third"),
    pytest.param(27, 144, 30, 5, 2, False, 33, 24, True, id="panel-padded-rows-of-z"),
    pytest.param(27, 97, 6, 3, 2, False, 5, 0, True, id="panel-m-not-a-multiple-of-4"),
    pytest.param(8, 5, 6, 3, 2, False, 1, 0, True, id="panel-n-below-16-one-problem"),
    pytest.param(8, 5, 6, 3, 2, False, 17, 0, True, id="panel-n-below-16"),
    pytest.param(8, 5, 6, 3, 1, False, 3, 0, True, id="panel-var1-no-A2"),
    pytest.param(16, 5, 3, 3, 2, False, 17, 0, True, id="panel-n-16-one-row-tile"),
    pytest.param(17, 5, 3, 3, 2, False, 17, 0, True, id="panel-n-17-second-row-tile"),
    pytest.param(32, 20, 3, 3, 2, False, 3, 0, True, id="panel-n-32-the-limit"),
    pytest.param(32, 20, 3, 3, 1, False, 3, 0, True, id="panel-n-32-var1-no-A2"),
    pytest.param(8, 5, 6, 3, 2, True, 3, 0, True, id="any-size-dense-weights"),
    pytest.param(40, 30, 4, 3, 2, False, 3, 0, True, id="any-size-n-above-32"),
    pytest.param(27, 144, 30, 5, 2, False, 5, 0, False, id="model-of-null-batch-equals-count"),
    pytest.param(40, 30, 4, 3, 2, False, 3, 0, False, id="any-size-model-of-null"),
]


@pytest.mark.parametrize("n,m,T,count,var_order,dense,R,ldu_pad,given", CASES)
def test_full_horizon_records_against_numpy(pkg, gpu, banks, n, m, T, count, var_order, dense, R, ldu_pad, given):
    """u passed as z with stage_stride = n + m, all five outputs, every code path."""
    import torch
    bk = banks(n, m, T, count, var_order, dense)
    mo = model_pattern(R, count) if given else None
    inp = make_inputs(bk.md, R, seed=5, ldu_pad=ldu_pad)
    out = call(torch, bk, gpu, inp, mo, T, ALL)
    compare(bk, mo, inp, out, T)


@pytest.mark.parametrize("key,R", [((27, 144, 30), 33), ((40, 30, 4), 3)])
def test_bank_of_the_handles_own_model_agrees_with_the_shared_call(pkg, gpu, key, R):
    """Every model of the bank is the handle's: the bank call agrees with fmpc_loop_records_device, and that call returns the same
    bits before and after (the bank leaves it alone)."""
    import torch
    bk = Bank(pkg, gpu, *key, 3, own=True)
    mo = model_pattern(R, 3)
    inp = make_inputs(bk.md, R, seed=9)
    T = key[2]
    before = call(torch, bk, gpu, inp, None, T, ALL, shared=True)
    bank = call(torch, bk, gpu, inp, mo, T, ALL)
    after = call(torch, bk, gpu, inp, None, T, ALL, shared=True)
    compare(bk, mo, inp, bank, T)
    for k in ALL:
        assert torch.equal(before.views[k], after.views[k]), k
        err = rel_err(bank.views[k].cpu().numpy(), before.views[k].cpu().numpy())
        print(f"  {k}: bank vs shared {err:.2e}")
        assert err <= TOL, (k, err)
    bk.h.close()


@pytest.mark.parametrize("key,count,R", [((27, 144, 30), 5, 33), ((40, 30, 4), 3, 4)])
def test_model_index_outside_the_bank_leaves_the_problem_alone(pkg, gpu, banks, key, count, R):
    import torch
    bk = banks(*key, count)
    mo = model_pattern(R, count)
    mo[1], mo[R - 2] = -1, count
    inp = make_inputs(bk.md, R, seed=10)
    out = call(torch, bk, gpu, inp, mo, key[2], ALL)
    compare(bk, mo, inp, out, key[2], skip=(1, R - 2))


def test_unsupported_without_a_bank_and_with_too_few_models(pkg, gpu, banks):
    """FMPC_E_UNSUPPORTED, outputs untouched: no bank; model_of NULL with batch > count."""
    import torch
    bk = banks(8, 5, 6, 3)
    n, m, T, R = 8, 5, 6, 4
    inp = make_inputs(bk.md, R, seed=12)
    hn = handle_from_model(pkg, bk.md)                                # no bank
    for h, mo in ((hn, model_pattern(R, 3)), (bk.h, None)):
        t = lambda v: tdev(torch, gpu, v)
        out = Outputs(torch, gpu, R, n, m, T, ALL)
        tu = t(inp[4])
        with pytest.raises(pkg.FastMPCError) as ei:
            h.loop_records_bank_device(t(inp[0]), t(inp[1]), t(inp[2]), tu, t(inp[3]), stages=T, ldu=tu.stride(0), stage_stride=n + m,
                                       volts=VOLTS, model_of=t(mo), **{k: out.get(k) for k in ALL})
        assert ei.value.code == pkg._lib.FMPC_E_UNSUPPORTED
        X0, U0 = t(np.zeros((2, R, n))), t(np.zeros((2, R, m)))
        so = {k: torch.full((2 * R * c,), NAN, dtype=torch.float64, device=gpu) for k, c in (("Xp0", n), ("xerr0", 1), ("dU", m), ("Uv", m))}
        with pytest.raises(pkg.FastMPCError) as ei:
            h.loop_records_run_bank_device(X0, U0, volts=VOLTS, model_of=t(mo), **so)
        assert ei.value.code == pkg._lib.FMPC_E_UNSUPPORTED
        torch.cuda.synchronize()
        out.check_guards(skip=range(R))
        assert all(bool(v.isnan().all()) for v in so.values())
    hn.close()


@pytest.mark.parametrize("key,count,R", [((27, 144, 30), 5, 33), ((40, 30, 4), 3, 3)])
def test_first_moves_only_and_null_inputs(pkg, gpu, banks, key, count, R):
    """stages = 1, u = u0 with ldu = m, J = NULL; then x0_pre = w = u1 = NULL over the full horizon: zeros."""
    import torch
    bk = banks(*key, count)
    mo = model_pattern(R, count)
    inp = make_inputs(bk.md, R, seed=6, first_moves=True)
    names = ("Xp", "xerr", "du", "uv")
    compare(bk, mo, inp, call(torch, bk, gpu, inp, mo, 1, names), 1)
    nulls = ("x0_pre", "w", "u1")
    compare(bk, mo, inp, call(torch, bk, gpu, inp, mo, 1, names, nulls=nulls), 1, nulls=nulls)
    inp = make_inputs(bk.md, R, seed=7)
    compare(bk, mo, inp, call(torch, bk, gpu, inp, mo, key[2], ALL, nulls=nulls), key[2], nulls=nulls)


@pytest.mark.parametrize("key,dense,R", [((27, 144, 30), False, 33), ((8, 5, 6), True, 3)])
def test_each_output_alone_and_twice_give_the_same_bits(pkg, gpu, banks, key, dense, R):
    import torch
    bk = banks(*key, 5 if key[0] == 27 else 3, 2, dense)
    T = key[2]
    mo = model_pattern(R, bk.count)
    inp = make_inputs(bk.md, R, seed=8)
    full = call(torch, bk, gpu, inp, mo, T, ALL)
    again = call(torch, bk, gpu, inp, mo, T, ALL)
    full.check_guards()
    for k in ALL:
        assert torch.equal(full.views[k], again.views[k]), k
    for k in ALL:
        alone = call(torch, bk, gpu, inp, mo, T, (k,))
        alone.check_guards()
        assert torch.equal(alone.views[k], full.views[k]), k


def test_fp32_factor_bank_gives_the_bits_of_the_fp64_bank(pkg, gpu, banks):
    """The records read the bank's fp64 images: FMPC_PREC_F32_MIXED, then set_model_bank, changes nothing."""
    import torch
    key, R, steps = (27, 144, 10), 19, 5
    b64 = banks(*key, 4)
    b32 = Bank(pkg, gpu, *key, 4, prec="f32")
    mo = model_pattern(R, 4)
    inp = make_inputs(b64.md, R, seed=13)
    o64 = call(torch, b64, gpu, inp, mo, key[2], ALL)
    o32 = call(torch, b32, gpu, inp, mo, key[2], ALL)
    compare(b64, mo, inp, o64, key[2])
    for k in ALL:
        assert torch.equal(o64.views[k], o32.views[k]), k
    rng = np.random.default_rng(14)
    X0, U0 = tdev(torch, gpu, rng.standard_normal((steps, R, 27))), tdev(torch, gpu, rng.standard_normal((steps, R, 144)))
    s64 = pkg.LoopRecords(b64.h, R, volts=VOLTS).stretch(X0, U0, model_of=tdev(torch, gpu, mo), bank=True)
    s32 = pkg.LoopRecords(b32.h, R, volts=VOLTS).stretch(X0, U0, model_of=tdev(torch, gpu, mo), bank=True)
    torch.cuda.synchronize()
    for k in ("Xp0", "xerr0", "dU", "Uv"):
        assert torch.equal(s64[k], s32[k]), k
    b32.h.close()


def stretch_ref(bk, mo, X0, U0, x0_before=None, ub1=None, ub2=None):
    """The stretch call's definitions on X0 (steps, R, n), U0 (steps, R, m) with A1, A2 of model mo[p]."""
    B = bk.md["B"]
    steps, R, n = X0.shape
    m = U0.shape[2]
    z = lambda v, c: np.zeros((R, c)) if v is None else v
    A1, A2 = bk.A1[mo], bk.A2[mo]                                      # (R, n, n)
    Xp0 = np.empty_like(X0); dU = np.empty_like(U0)
    for s in range(steps):
        xpre = X0[s - 1] if s >= 1 else z(x0_before, n)
        u1 = U0[s - 1] if s >= 1 else z(ub1, m)
        u2 = U0[s - 2] if s >= 2 else (z(ub1, m) if s == 1 else z(ub2, m))
        w0 = -np.einsum("rab,rb->ra", A1, u1 @ B.T) - np.einsum("rab,rb->ra", A2, u2 @ B.T)
        Xp0[s] = np.einsum("rab,rb->ra", A1, X0[s]) + np.einsum("rab,rb->ra", A2, xpre) + w0 + U0[s] @ B.T
        dU[s] = U0[s] - u1
    return Xp0, np.linalg.norm(Xp0, axis=2), dU, volts_ref(U0)


STRETCH = [
    # n, m, T, count, var_order, batch, steps, the state before the stretch given
    pytest.param(27, 144, 10, 4, 2, 3, 5, True, id="panel-one-ragged-tile"),
    pytest.param(8, 5, 6, 3, 2, 3, 19, False, id="panel-ragged-second-tile-null-before"),
    pytest.param(8, 5, 6, 3, 2, 3, 19, True, id="panel-ragged-second-tile"),
    pytest.param(8, 5, 6, 3, 1, 2, 3, True, id="panel-var1-no-A2"),
    pytest.param(17, 5, 3, 3, 2, 3, 19, True, id="panel-n-17-ragged-second-tile"),
    pytest.param(32, 20, 3, 3, 2, 2, 3, False, id="panel-n-32-null-before"),
    pytest.param(40, 30, 4, 3, 2, 2, 3, False, id="any-size-null-before"),
    pytest.param(40, 30, 4, 3, 2, 2, 3, True, id="any-size"),
]


@pytest.mark.parametrize("n,m,T,count,var_order,R,steps,before", STRETCH)
def test_stretch_against_numpy_and_the_one_timestep_call(pkg, gpu, banks, n, m, T, count, var_order, R, steps, before):
    """fmpc_loop_records_run_bank_device on seeded X0, U0 of order 1: against numpy, and step by step against
    fmpc_loop_records_bank_device with stages = 1 on x0 = X0[s], x0_pre = X0[s-1] and w of fmpc_loop_inputs_bank_device."""
    import torch
    bk = banks(n, m, T, count, var_order)
    h = bk.h
    mo = model_pattern(R, count)
    mo[0] = count - 1
    rng = np.random.default_rng(30)
    X0, U0 = rng.standard_normal((steps, R, n)), rng.standard_normal((steps, R, m))
    U0[0, 0, 0] = 0.0
    bef = (rng.standard_normal((R, n)), rng.standard_normal((R, m)), rng.standard_normal((R, m))) if before else (None, None, None)
    t = lambda v: tdev(torch, gpu, v)
    tX, tU, tb, tmo = t(X0), t(U0), [t(v) for v in bef], t(mo)
    sizes = {"Xp0": n, "xerr0": 1, "dU": m, "Uv": m}
    bufs = {k: torch.full((GUARD + steps * R * c + GUARD,), NAN, dtype=torch.float64, device=gpu) for k, c in sizes.items()}
    views = {k: b[GUARD:-GUARD] for k, b in bufs.items()}
    h.loop_records_run_bank_device(tX, tU, *tb, volts=VOLTS, model_of=tmo, **views)
    torch.cuda.synchronize()
    # numpy's reference adds w_0 = -A1 B u[s-1] - A2 B u[s-2]; the device multiplies the corrected states: the same sum in two orders
    Bt = bk.md["B"].T
    zz = lambda v, c: np.zeros((R, c)) if v is None else v
    mv = lambda A, x: np.einsum("rab,rb->ra", A[mo], x)
    chain = np.empty_like(X0)
    for s in range(steps):
        u1 = U0[s - 1] if s >= 1 else zz(bef[1], m)
        u2 = U0[s - 2] if s >= 2 else zz(bef[1] if s == 1 else bef[2], m)
        xpre = X0[s - 1] if s >= 1 else zz(bef[0], n)
        chain[s] = mv(bk.A1, X0[s] - u1 @ Bt) + mv(bk.A2, xpre - u2 @ Bt) + U0[s] @ Bt
    ref = dict(zip(sizes, stretch_ref(bk, mo, X0, U0, *bef)))
    order = rel_err(chain, ref["Xp0"])
    print(f"  corrected-state form vs w form in numpy: {order:.2e}")
    assert order <= ORDER_TOL
    for k, b in bufs.items():
        assert bool(b[:GUARD].isnan().all()) and bool(b[-GUARD:].isnan().all()) and not bool(views[k].isnan().any()), k
        err = rel_err(views[k].cpu().numpy().reshape(ref[k].shape), ref[k])
        print(f"  {k}: stretch vs numpy {err:.2e}")
        assert err <= TOL, (k, err)
    assert float(views["Uv"][0]) == 0.0
    # step by step through the one-timestep call
    zeros_a = torch.zeros((R, n), dtype=torch.float64, device=gpu)
    sx, sxp, sw = (torch.empty((R, c), dtype=torch.float64, device=gpu) for c in (n, n, T * n))
    for s in range(steps):
        u1 = tU[s - 1] if s >= 1 else tb[1]
        u2 = tU[s - 2] if s >= 2 else (tb[1] if s == 1 else tb[2])
        xpre = tX[s - 1] if s >= 1 else tb[0]
        h.loop_inputs_bank(zeros_a, None, u1, u2, sx, sxp, sw, model_of=tmo)                  # w = -M1 B u1 - M2 B u2 of the models
        o = {k: torch.full((R * c,), NAN, dtype=torch.float64, device=gpu) for k, c in (("Xp", n), ("xerr", 1), ("du", m), ("uv", m))}
        h.loop_records_bank_device(tX[s], xpre, sw, tU[s], u1, stages=1, ldu=m, volts=VOLTS, model_of=tmo, **o)
        torch.cuda.synchronize()
        for ks, k1 in (("Xp0", "Xp"), ("xerr0", "xerr"), ("dU", "du"), ("Uv", "uv")):
            got = views[ks].view(steps, -1)[s].cpu().numpy()
            err = rel_err(got, o[k1].cpu().numpy())
            assert err <= TOL, (s, ks, err)


def test_captured_graph_with_both_calls_replays_on_changed_inputs(pkg, gpu, banks):
    """Both bank calls in one captured graph after a warm run (RecordedSolves runs its function once eagerly: weights, cost scratch and
    workspace exist, nothing is allocated under capture), replayed three times on changed inputs."""
    import torch
    n, m, T, R, steps = 27, 144, 30, 33, 5
    bk = banks(n, m, T, 5)
    h = bk.h
    mo = model_pattern(R, 5)
    t = lambda v: tdev(torch, gpu, v)
    tmo = t(mo)
    inp = make_inputs(bk.md, R, seed=20)
    tin = [t(v) for v in inp[:5]]
    out = Outputs(torch, gpu, R, n, m, T, ALL)
    tX, tU = torch.zeros((steps, R, n), dtype=torch.float64, device=gpu), torch.zeros((steps, R, m), dtype=torch.float64, device=gpu)
    sizes = {"Xp0": n, "xerr0": 1, "dU": m, "Uv": m}
    so = {k: torch.full((steps * R * c,), NAN, dtype=torch.float64, device=gpu) for k, c in sizes.items()}

    def record():
        h.loop_records_bank_device(tin[0], tin[1], tin[2], tin[4], tin[3], stages=T, ldu=tin[4].stride(0), stage_stride=n + m, volts=VOLTS,
                                   model_of=tmo, **{k: out.get(k) for k in ALL})
        h.loop_records_run_bank_device(tX, tU, volts=VOLTS, model_of=tmo, **so)

    rec = pkg.RecordedSolves(record)
    assert rec.valid()
    for rep in range(3):
        inp = make_inputs(bk.md, R, seed=21 + rep)
        rng = np.random.default_rng(40 + rep)
        X0, U0 = rng.standard_normal((steps, R, n)), rng.standard_normal((steps, R, m))
        for dst, src in zip(tin + [tX, tU], list(inp[:5]) + [X0, U0]):
            dst.copy_(t(src))
        for v in list(out.views.values()) + list(so.values()):
            v.fill_(NAN)
        rec.replay()
        torch.cuda.synchronize()
        compare(bk, mo, inp, out, T)
        ref = dict(zip(sizes, stretch_ref(bk, mo, X0, U0)))
        for k in sizes:
            err = rel_err(so[k].cpu().numpy().reshape(ref[k].shape), ref[k])
            assert err <= TOL, (rep, k, err)


def test_closed_loop_on_the_bank_records(pkg, gpu):
    """ClosedLoop(bank=True, model_of=...) at (27, 144, 10), 8 realisations, 4 steps: .records(rec) after each step against per-model
    ClosedLoops on per-model handles; run_recorded(a, records=rec): X0, U0 equal a run without records, the records equal numpy's.
    Both raised ValueError before the bank had a records form.  (Weights of the order of R, as in
    tests/test_gpu_loop_records.py::test_stretch_against_steps_and_numpy: the loop drives Xp towards zero with Q = 1.5e4 I.)"""
    import torch
    n, m, T, R, steps, count = 27, 144, 10, 8, 4, 3
    bk = Bank(pkg, gpu, n, m, T, count, qscale=1.0)
    h = bk.h
    mo = model_pattern(R, count)
    tmo = tdev(torch, gpu, mo)
    a = np.stack([pkg.synthetic.make_realisation(bk.models[mo[r]], r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)   # (steps, R, n)
    ta = tdev(torch, gpu, a)
    keys = ("Xp", "xerr", "J", "du", "uv")
    loop = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=True, bank=True, model_of=tmo)
    rec = pkg.LoopRecords(h, R, volts=VOLTS)
    got = {k: [] for k in keys}
    for s in range(steps):
        loop.step(ta[s])
        o = loop.records(rec)
        assert o["Xp"].shape == (R, T, n) and o["J"].shape == (R,) and torch.equal(o["x_prev"], o["Xp"][:, 0])
        for k in keys:
            got[k].append(o[k].clone())
    torch.cuda.synchronize()
    got = {k: torch.stack(v).cpu().numpy() for k, v in got.items()}                 # (steps, R, ...)
    for j in range(count):
        mine = np.nonzero(mo == j)[0]
        tmine = torch.from_numpy(mine).to(gpu)
        hj = handle_from_model(pkg, bk.models[j])
        lj = pkg.ClosedLoop(hj, len(mine), n_newton=1, k=1e-2, keep_z=True)
        rj = pkg.LoopRecords(hj, len(mine), volts=VOLTS)
        for s in range(steps):
            lj.step(ta[s][tmine].contiguous())
            oj = lj.records(rj)
            torch.cuda.synchronize()
            for k in keys:
                err = rel_err(got[k][s][mine], oj[k].cpu().numpy())
                print(f"  model {j} step {s} {k}: bank loop vs per-model loop {err:.2e}")
                assert err <= TOL, (j, s, k, err)
        hj.close()
    # a recorded stretch with its records
    plain = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=False, bank=True, model_of=tmo)
    U0p, X0p = plain.run_recorded(ta)
    lr = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=False, bank=True, model_of=tmo)
    U0, X0, rs = lr.run_recorded(ta, records=pkg.LoopRecords(h, R, volts=VOLTS))
    torch.cuda.synchronize()
    assert torch.equal(U0, U0p) and torch.equal(X0, X0p)
    ref = dict(zip(("Xp0", "xerr0", "dU", "Uv"), stretch_ref(bk, mo, X0.cpu().numpy(), U0.cpu().numpy())))
    for k, v in ref.items():
        err = rel_err(rs[k].cpu().numpy(), v)
        print(f"  {k}: stretch records of the bank loop vs numpy {err:.2e}")
        assert err <= TOL, (k, err)
    h.close()
