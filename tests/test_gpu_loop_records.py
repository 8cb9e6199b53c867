"""GPU tests of the closed-loop records (fmpc_loop_records_device / fmpc_loop_records_run_device; README.md:576-622): the panel
kernel (n <= 32, diagonal weights), the any-size kernel (n > 32 or dense Q, Qf, R) and the stretch call against a float64 numpy
restatement of the definitions in include/fastmpc.h, on seeded random inputs of order 1 -- nothing about the solver is assumed.
Tolerance: tests.util.rel_err <= 1e-12 on every output, the bar of the loop-inputs kernel (tests/test_gpu_closed_loop.py:36): the
sums here have the same length, at most m + 2 n terms."""
import ctypes as C

import numpy as np
import pytest

from oracle.closed_loop_ref import design_matrices
from tests.util import handle_from_model, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12
VOLTS = (0.047275, 2.709264, 1.0)            # coeff_a, coeff_b (README.md:350), unit_change
GUARD = 64                                   # doubles of NaN either side of every output


def _spd(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return scale * (G @ G.T / n + np.eye(n))


def make_model(pkg, n, m, T, var_order=2, dense=False, qscale=1.5e4):
    """The shared synthetic model with weights that tell Q, Qf and the entries of R apart."""
    md = pkg.synthetic.make_model(n, m, T, var_order=var_order)
    rng = np.random.default_rng(11)
    if dense:
        md["Q"] = _spd(n, 1, qscale); md["Qf"] = _spd(n, 2, 2.0 * qscale); md["R"] = _spd(m, 7)
    else:
        md["Q"] = np.diag(qscale * (1.0 + rng.random(n))); md["Qf"] = np.diag(2.0 * qscale * (1.0 + rng.random(n)))
        md["R"] = np.diag(1.0 + rng.random(m))
    return md


@pytest.fixture(scope="module")
def models(pkg, gpu):
    """(n, m, T, var_order, dense) -> (model, handle, M1, M2): built once per module."""
    cache = {}

    def get(n, m, T, var_order=2, dense=False, qscale=1.5e4):
        key = (n, m, T, var_order, dense, qscale)
        if key not in cache:
            md = make_model(pkg, n, m, T, var_order, dense, qscale)
            M1, M2 = design_matrices(md["A1"], md["A2"], T)
            cache[key] = (md, handle_from_model(pkg, md), M1, M2)
        return cache[key]

    yield get
    for _, h, _, _ in cache.values():
        h.close()


def volts_ref(u, volts=VOLTS):
    a, b, uc = volts
    return np.sign(u) * (-b + np.sqrt(b * b + 4.0 * a * np.abs(u) * uc)) / (2.0 * a)


def records_ref(md, M1, M2, x0, x0_pre, w, U, u1, with_J):
    """The definitions, in float64 numpy.  U: (R, stages, m).  Returns Xp (R, stages, n), xerr (R, stages), J (R,) or None, du, uv."""
    n, m, T, B = md["n"], md["m"], md["T"], md["B"]
    R, S = U.shape[0], U.shape[1]
    x0_pre = np.zeros((R, n)) if x0_pre is None else x0_pre
    w = np.zeros((R, T * n)) if w is None else w
    Xp = np.empty((R, S, n))
    for i in range(S):
        blk = slice(i * n, (i + 1) * n)
        Xp[:, i] = x0 @ M1[blk].T + x0_pre @ M2[blk].T + w[:, blk] + U[:, i] @ B.T
    xerr = np.linalg.norm(Xp, axis=2)
    J = None
    if with_J:
        assert S == T
        J = np.einsum("ria,ab,rib->r", Xp[:, :T - 1], md["Q"], Xp[:, :T - 1]) + np.einsum("ra,ab,rb->r", Xp[:, T - 1], md["Qf"], Xp[:, T - 1]) \
            + np.einsum("ric,cd,rid->r", U, md["R"], U)
    du = U[:, 0] - (0.0 if u1 is None else u1)
    return Xp, xerr, J, du, volts_ref(U[:, 0])


def make_inputs(md, R, seed, ldu_pad=0, first_moves=False):
    """Seeded inputs of order 1; u as a solve's z (rows ldu = T (n + m) + ldu_pad apart, NaN in the padding and -- so that a read of
    the wrong entries shows -- the x entries of z random too), or as the first moves (R, m).  One entry of u_0 is exactly 0."""
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
    """The five outputs between NaN guard regions."""
    SIZES = {"Xp": lambda n, m, S: S * n, "xerr": lambda n, m, S: S, "J": lambda n, m, S: 1, "du": lambda n, m, S: m, "uv": lambda n, m, S: m}

    def __init__(self, torch, dev, R, n, m, S, names):
        self.bufs, self.views = {}, {}
        for k in names:
            cnt = R * self.SIZES[k](n, m, S)
            b = torch.full((GUARD + cnt + GUARD,), float("nan"), dtype=torch.float64, device=dev)
            self.bufs[k] = b
            self.views[k] = b[GUARD:GUARD + cnt]

    def get(self, k):
        return self.views.get(k)

    def check_guards(self):
        for k, b in self.bufs.items():
            assert bool(b[:GUARD].isnan().all()) and bool(b[-GUARD:].isnan().all()), f"{k}: guard overwritten"
            assert not bool(self.views[k].isnan().any()), f"{k}: NaN in the payload"


def call(torch, h, dev, md, inp, S, names, nulls=(), ldu=None):
    """One fmpc_loop_records_device call on `inp`; returns the Outputs."""
    n, m = md["n"], md["m"]
    x0, x0_pre, w, u1, ubuf, _ = inp
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    R = x0.shape[0]
    out = Outputs(torch, dev, R, n, m, S, names)
    tu = t(ubuf)
    h.loop_records_device(t(x0), None if "x0_pre" in nulls else t(x0_pre), None if "w" in nulls else t(w), tu,
                          None if "u1" in nulls else t(u1), stages=S, ldu=tu.stride(0) if ldu is None else ldu,
                          stage_stride=n + m, volts=VOLTS, Xp=out.get("Xp"), xerr=out.get("xerr"), J=out.get("J"), du=out.get("du"), uv=out.get("uv"))
    torch.cuda.synchronize()
    return out


def compare(md, M1, M2, inp, out, S, nulls=()):
    x0, x0_pre, w, u1, _, U = inp
    R, n, m = x0.shape[0], md["n"], md["m"]
    with_J = "J" in out.views
    Xp, xerr, J, du, uv = records_ref(md, M1, M2, x0, None if "x0_pre" in nulls else x0_pre, None if "w" in nulls else w, U[:, :S],
                                      None if "u1" in nulls else u1, with_J)
    ref = {"Xp": Xp.reshape(R, S * n), "xerr": xerr, "J": J, "du": du, "uv": uv}
    out.check_guards()
    for k, v in out.views.items():
        got = v.cpu().numpy().reshape(ref[k].shape)
        err = rel_err(got, ref[k])
        print(f"  {k}: rel err {err:.2e}")
        assert err <= TOL, (k, err)
    if "uv" in out.views:
        assert float(out.views["uv"][0]) == 0.0                       # u = 0.0 exactly gives 0.0 V


ALL = ("Xp", "xerr", "J", "du", "uv")

CASES = [
    # n, m, T, var_order, dense, batch, ldu_pad
    pytest.param(27, 144, 30, 2, False, 33, 0, id="panel-two-panels-and-a-ragged-third"),
    pytest.param(27, 144, 30, 2, False, 33, 24, id="panel-padded-rows-of-z"),
    pytest.param(27, 97, 6, 2, False, 5, 0, id="panel-m-not-a-multiple-of-4"),
    pytest.param(8, 5, 6, 2, False, 1, 0, id="panel-n-below-16-one-problem"),
    pytest.param(8, 5, 6, 2, False, 17, 0, id="panel-n-below-16"),
    pytest.param(8, 5, 6, 1, False, 3, 0, id="panel-var1"),
    pytest.param(16, 5, 3, 2, False, 17, 0, id="panel-n-16-one-row-tile"),
    pytest.param(17, 5, 3, 2, False, 17, 0, id="panel-n-17-second-row-tile"),
    pytest.param(32, 20, 3, 2, False, 3, 0, id="panel-n-32-the-limit"),
    pytest.param(8, 5, 6, 2, True, 3, 0, id="any-size-dense-weights"),
    pytest.param(40, 30, 4, 2, False, 3, 0, id="any-size-n-above-32"),
]


@pytest.mark.parametrize("n,m,T,var_order,dense,R,ldu_pad", CASES)
def test_full_horizon_records_against_numpy(pkg, gpu, models, n, m, T, var_order, dense, R, ldu_pad):
    """u passed as z with stage_stride = n + m, all outputs, every code path of the table in the issue."""
    import torch
    md, h, M1, M2 = models(n, m, T, var_order, dense)
    if var_order == 1:
        assert not M2.any()
    inp = make_inputs(md, R, seed=5, ldu_pad=ldu_pad)
    out = call(torch, h, gpu, md, inp, T, ALL)
    compare(md, M1, M2, inp, out, T)


def test_first_moves_only(pkg, gpu, models):
    """stages = 1, u an m x batch array, J = NULL."""
    import torch
    md, h, M1, M2 = models(27, 144, 30)
    inp = make_inputs(md, 33, seed=6, first_moves=True)
    out = call(torch, h, gpu, md, inp, 1, ("Xp", "xerr", "du", "uv"))
    compare(md, M1, M2, inp, out, 1)


@pytest.mark.parametrize("key", [(27, 144, 30, 2, False), (40, 30, 4, 2, False)])
def test_null_inputs(pkg, gpu, models, key):
    """x0_pre = NULL, w = NULL, u1 = NULL: zeros."""
    import torch
    md, h, M1, M2 = models(*key)
    inp = make_inputs(md, 33 if key[0] == 27 else 3, seed=7)
    nulls = ("x0_pre", "w", "u1")
    out = call(torch, h, gpu, md, inp, md["T"], ALL, nulls=nulls)
    compare(md, M1, M2, inp, out, md["T"], nulls=nulls)


@pytest.mark.parametrize("key", [(27, 144, 30, 2, False), (8, 5, 6, 2, True)])
def test_each_output_alone_and_twice_give_the_same_bits(pkg, gpu, models, key):
    import torch
    md, h, M1, M2 = models(*key)
    T = md["T"]
    inp = make_inputs(md, 33 if key[0] == 27 else 3, seed=8)
    full = call(torch, h, gpu, md, inp, T, ALL)
    again = call(torch, h, gpu, md, inp, T, ALL)
    for k in ALL:
        assert torch.equal(full.views[k], again.views[k]), k
    for k in ALL:
        alone = call(torch, h, gpu, md, inp, T, (k,))
        alone.check_guards()
        assert torch.equal(alone.views[k], full.views[k]), k


def test_argument_rules_with_a_handle(pkg, gpu, models):
    """The rules that need the handle's m and T, answered before the device is touched (dummy pointers: never read)."""
    md, h, _, _ = models(8, 5, 6)
    n, m, T = 8, 5, 6
    lib, L = pkg.load(), pkg._lib
    P = C.c_void_p(0x1000)
    a, b, uc = VOLTS

    def rec(batch=4, stages=T, x0=P, u=P, ldu=T * (n + m), ss=n + m, Xp=P, J=P, uv=P, ca=a):
        return lib.fmpc_loop_records_device(h._h, batch, stages, x0, None, None, u, ldu, ss, None, ca, b, uc, Xp, None, J, None, uv, None)

    assert rec(stages=T - 1) == L.FMPC_E_DIM and rec(stages=1, ldu=m) == L.FMPC_E_DIM          # J with stages != T
    assert rec(stages=T + 1, J=None, ldu=1 << 20) == L.FMPC_E_DIM                              # stages outside [1, T]
    assert rec(ldu=(T - 1) * (n + m) + m - 1) == L.FMPC_E_DIM
    assert rec(stages=1, J=None, ldu=m - 1) == L.FMPC_E_DIM
    assert rec(ss=m - 1, ldu=1 << 20) == L.FMPC_E_DIM
    assert rec(ca=0.0) == L.FMPC_E_DIM and rec(ca=float("nan")) == L.FMPC_E_DIM
    assert rec(x0=None) == L.FMPC_E_NULL and rec(u=None) == L.FMPC_E_NULL
    assert rec(Xp=None, J=None, uv=None) == L.FMPC_OK                                          # nothing asked for
    assert rec(batch=0) == L.FMPC_OK
    assert rec(Xp=None, J=None, uv=None, ldu=3) == L.FMPC_E_DIM                                # the rules come first


def stretch_ref(md, X0, U0, x0_before=None, ub1=None, ub2=None):
    """The stretch call's definitions on a run's X0 (steps, R, n), U0 (steps, R, m)."""
    A1, A2, B = md["A1"], md["A2"], md["B"]
    steps, R, n = X0.shape
    m = U0.shape[2]
    z = lambda v, c: np.zeros((R, c)) if v is None else v
    Xp0 = np.empty_like(X0); dU = np.empty_like(U0)
    for s in range(steps):
        xpre = X0[s - 1] if s >= 1 else z(x0_before, n)
        u1 = U0[s - 1] if s >= 1 else z(ub1, m)
        u2 = U0[s - 2] if s >= 2 else (z(ub1, m) if s == 1 else z(ub2, m))
        w0 = -(u1 @ B.T) @ A1.T - (u2 @ B.T) @ A2.T
        Xp0[s] = X0[s] @ A1.T + xpre @ A2.T + w0 + U0[s] @ B.T
        dU[s] = U0[s] - u1
    return Xp0, np.linalg.norm(Xp0, axis=2), dU, volts_ref(U0)


@pytest.mark.parametrize("n,m,T,R,steps", [(27, 144, 10, 3, 5), (8, 5, 6, 2, 4), (17, 5, 3, 3, 19)])
def test_stretch_against_steps_and_numpy(pkg, gpu, models, n, m, T, R, steps):
    """ClosedLoop.run_recorded(a, records=rec) against per-step ClosedLoop.step + records(rec) on a second loop with keep_z=True
    (stage 0 of its full-horizon call), both against numpy on that run's X0, U0; a stretch continued from a non-empty state.

    The loop runs with state weights of the order of R (Q ~ I, not 1.5e4 I).  A loop that works well drives X_predicted towards
    zero, and the 1e-12 bar is one for sums whose result is of the order of their terms (the seeded inputs of the other tests):
    with Q = 1.5e4 I at (27, 144, 10) the CPU oracle loop gives ||Xp0|| = 3.3e-3 from terms of norm 30, where float64 numpy is
    itself 7.7e-13 away from the same formula in extended precision (two float64 evaluations then differ by about 2e-12: measured
    here 2.2e-12 stretch vs steps, 2.0e-12 stretch vs numpy, 1.5e-12 steps vs numpy).  With Q ~ I the same loop leaves
    ||Xp0|| = 3.4 and float64 numpy is 1e-15 from extended precision, so 1e-12 tests the kernels and not the cancellation."""
    import torch
    md, h, M1, M2 = models(n, m, T, qscale=1.0)
    a = np.stack([pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)   # (steps, R, n)
    ta = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    keys = ("Xp0", "xerr0", "dU", "Uv")
    # one stretch
    loop = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=False)
    U0, X0, rs = loop.run_recorded(ta, records=pkg.LoopRecords(h, R, volts=VOLTS))
    torch.cuda.synchronize()
    one = {k: rs[k].cpu().numpy() for k in keys}
    # step by step, full horizon from z
    loop2 = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=True)
    rec2 = pkg.LoopRecords(h, R, volts=VOLTS)
    st = {k: [] for k in keys}
    for s in range(steps):
        loop2.step(ta[s])
        o = loop2.records(rec2)
        assert o["Xp"].shape == (R, T, n) and o["J"].shape == (R,) and torch.equal(o["x_prev"], o["Xp"][:, 0])
        for k, v in zip(keys, (o["Xp"][:, 0], o["xerr"][:, 0], o["du"], o["uv"])):
            st[k].append(v.clone())
    torch.cuda.synchronize()
    st = {k: torch.stack(v).cpu().numpy() for k, v in st.items()}
    ref = dict(zip(keys, stretch_ref(md, X0.cpu().numpy(), U0.cpu().numpy())))
    for k in keys:
        e1, e2, e3 = rel_err(one[k], st[k]), rel_err(one[k], ref[k]), rel_err(st[k], ref[k])
        print(f"  {k}: stretch vs steps {e1:.2e}, stretch vs numpy {e2:.2e}, steps vs numpy {e3:.2e}")
        assert e1 <= TOL and e2 <= TOL and e3 <= TOL, (k, e1, e2, e3)
    # two steps, then the others from the state they leave
    loop3 = pkg.ClosedLoop(h, R, n_newton=1, k=1e-2, keep_z=False)
    rec3 = pkg.LoopRecords(h, R, volts=VOLTS)
    first = {k: v.clone() for k, v in loop3.run_recorded(ta[:2].contiguous(), records=rec3)[2].items()}
    second = loop3.run_recorded(ta[2:].contiguous(), records=rec3)[2]
    torch.cuda.synchronize()
    for k in keys:
        both = torch.cat([first[k], second[k]]).cpu().numpy()
        e = rel_err(both, one[k])
        print(f"  {k}: 2 + {steps - 2} steps vs {steps}: {e:.2e}")
        assert e <= TOL, (k, e)


def test_first_move_records_of_a_loop_without_z(pkg, gpu, models):
    """ClosedLoop without z: records(rec) passes the newest first move with stages = 1 and agrees with the full-horizon call's stage 0."""
    import torch
    md, h, M1, M2 = models(8, 5, 6, qscale=1.0)                     # (weights as in test_stretch_against_steps_and_numpy)
    R, steps = 2, 3
    a = np.stack([pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    ta = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    la, lb = pkg.ClosedLoop(h, R, keep_z=False), pkg.ClosedLoop(h, R, keep_z=True)
    ra, rb = pkg.LoopRecords(h, R, volts=VOLTS), pkg.LoopRecords(h, R, volts=VOLTS)
    for s in range(steps):
        la.step(ta[s]); lb.step(ta[s])
        oa, ob = la.records(ra), lb.records(rb)
        torch.cuda.synchronize()
        assert "J" not in oa and oa["Xp"].shape == (R, 1, 8)
        for ka, va, vb in (("Xp", oa["Xp"][:, 0], ob["Xp"][:, 0]), ("xerr", oa["xerr"][:, 0], ob["xerr"][:, 0]), ("du", oa["du"], ob["du"]),
                           ("uv", oa["uv"], ob["uv"])):
            assert rel_err(va.cpu().numpy(), vb.cpu().numpy()) <= TOL, (s, ka)


def test_captured_graph_replays_on_changed_inputs(pkg, gpu, models):
    """fmpc_loop_records_device captured in a torch.cuda.graph after a warm call (RecordedSolves runs it once eagerly: the weights are
    uploaded and the partial-cost buffer sized there, nothing is allocated under capture), replayed three times on changed inputs."""
    import torch
    md, h, M1, M2 = models(27, 144, 30)
    n, m, T, R = 27, 144, 30, 33
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
    inp = make_inputs(md, R, seed=20)
    tin = [t(v) for v in inp[:5]]
    out = Outputs(torch, gpu, R, n, m, T, ALL)

    def record():
        h.loop_records_device(tin[0], tin[1], tin[2], tin[4], tin[3], stages=T, ldu=tin[4].stride(0), stage_stride=n + m, volts=VOLTS,
                              Xp=out.get("Xp"), xerr=out.get("xerr"), J=out.get("J"), du=out.get("du"), uv=out.get("uv"))

    rec = pkg.RecordedSolves(record)
    assert rec.valid()
    for rep in range(3):
        inp = make_inputs(md, R, seed=21 + rep)
        for dst, src in zip(tin, inp[:5]):
            dst.copy_(t(src))
        for v in out.views.values():
            v.fill_(float("nan"))
        rec.replay()
        torch.cuda.synchronize()
        compare(md, M1, M2, inp, out, T)


def test_aoloop_records(pkg, gpu, models):
    """AOLoop.records(rec) after each step of the loop with its estimator: the stage-0 records of the loop's own x0 = ad_est,
    x0_pre, b_ref and newest first move, against numpy on copies of those buffers (weights as in the stretch test)."""
    import torch
    md, h, M1, M2 = models(27, 144, 10, qscale=1.0)
    R, steps, length = 2, 3, 64
    op = pkg.synthetic.estimator_optics(length)
    est = pkg.PhaseDiversityEstimator(op["pupil"], op["W"], op["zd_list"], op["dx"], op["range_min"] + 1, op["range_max"] + 1,
                                      op["A_s"], op["b_s"], AU=op["AU"])
    rng = np.random.default_rng(4)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    phase = np.tensordot(a, op["Z"][1:], axes=1) + 0.01 * rng.standard_normal((steps, R, length, length))
    loop = pkg.AOLoop(h, est, op["Z"][1:], R, n_newton=1, k=1e-2)
    rec = pkg.LoopRecords(h, R, volts=VOLTS)
    u_last = None
    for s in range(steps):
        u, x0 = loop.step(torch.from_numpy(np.ascontiguousarray(phase[s])).to(gpu))
        o = loop.records(rec)
        torch.cuda.synchronize()
        c = lambda v: v.cpu().numpy().copy()
        Xp, xerr, _, du, uv = records_ref(md, M1, M2, c(x0), c(loop.x0_pre), c(loop.w), c(u)[:, None, :], u_last, False)
        for k, got, ref in (("Xp", o["Xp"], Xp), ("xerr", o["xerr"], xerr), ("du", o["du"], du), ("uv", o["uv"], uv)):
            err = rel_err(c(got).reshape(ref.shape), ref)
            assert err <= TOL, (s, k, err)
        assert torch.equal(o["x_prev"], o["Xp"][:, 0])
        u_last = c(u)
    est.close()
