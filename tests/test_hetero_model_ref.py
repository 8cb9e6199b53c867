"""The inputs of tests/test_gpu_hetero_model.py on the CPU oracles.  For every (shape, budget, k) the GPU file runs:

  * the structured oracle agrees with the dense op-for-op oracle on the heterogeneous model, at the bar of
    tests/test_oracle_banded.py (1e-10 on z, 1e-9 on nu, the same iterations and step lengths); the cases with ramp-rate rows
    are solved by the dense oracle with ramp rows (the structured one has none);
  * every mutation of tests/hetero_model.py -- zero q, r, qf; Q, R, Qf, u_min, u_max rolled by one index; Qf = Q -- moves the
    oracle's z by at least 1e-6 relative on EVERY problem: 1000 times the 1e-9 bar of the GPU file, so a kernel with such a mistake
    cannot pass there.  (Measured when the cases were chosen: 1.5e-5 at the least, rolling u_min at (83, 7, 3); typically 1e-4 for
    the box and 1e-2 .. 1 for the weights and costs.)  A case that falls short is to be changed, never the floor;
  * the two things these cases cannot see are asserted as such, so that nobody takes them for covered: with xf the terminal
    state is fixed and qf, Qf do not matter (<= 1e-12), and the x box only sets the x rows of the mid-box start, which a full
    first Newton step (t = 1, asserted) removes again (<= 1e-12; an explicit start does not read the box at all).  The cases
    named xbox-* are the exception to the exception: cold starts whose first step backtracks on every problem (asserted), where
    rolling x_min or x_max has to pass the 1e-6 floor like every other mutation (measured: 5e-2 and more)."""
import numpy as np
import pytest

from tests import hetero_model as H
from tests.util import banded_from_model, canon_steps, dense_from_model, oracle_batch, rel_err

FLOOR, NOTHING = 1e-6, 1e-12
W_LINESEARCH = 1

SOLVER = [(name, b) for name, c in H.CASES.items() for b in c["budgets"]]
RAMP = [(name, b) for name in H.RAMP_CASES for b in H.RAMP_BUDGETS]
BANK = [(name, b) for name in H.BANK_CASES for b in H.BANK_BUDGETS]


@pytest.fixture(autouse=True, scope="module")
def one_blas_thread():
    """Small matrices: a BLAS thread pool only gets in the way (optional: without threadpoolctl the tests are merely slower)."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=1):
        yield


def _moved(z, zo):
    """Per problem the relative change of z; a mutated model on which the oracle's iterate is no longer finite (a rolled box
    can put u_prev outside the ramp interval of the mid-box start) has certainly moved."""
    out = []
    for p in range(len(zo)):
        e = rel_err(z[p], zo[p])
        out.append(e if np.isfinite(e) else np.inf)
    return np.array(out)


def _check_mutations(label, md, has_xf, first_steps_full, solve, zo, reads_box=True, sees_x_box=False):
    """solve(model) -> z of every problem.  Floors and the two exceptions.  sees_x_box: a case chosen because the first step of
    EVERY problem backtracks from the cold start -- there the x box is held to the floor like everything else."""
    for name, mm in H.mutations(md):
        ch = _moved(solve(mm), zo)
        print("%s, %s: z moves by %.1e .. %.1e" % (label, name, ch.min(), ch.max()))
        if has_xf and name in H.TERMINAL:
            assert ch.max() <= NOTHING, (label, name, ch)
        else:
            assert ch.min() >= FLOOR, (label, name, ch)
    assert sees_x_box or first_steps_full or not reads_box, "the first step backtracks: the x box can be seen here, assert a floor instead"
    for name, mm in H.x_box_mutations(md):
        ch = _moved(solve(mm), zo)
        print("%s, %s: z moves by %.1e .. %.1e" % (label, name, ch.min(), ch.max()))
        if sees_x_box:
            assert ch.min() >= FLOOR, (label, name, ch)
        else:
            assert ch.max() <= NOTHING, (label, name, ch)


def test_every_constant_differs_by_index():
    md, _, _ = H.build("8x5x10")
    for key in ("q", "r", "qf", "u_min", "u_max", "x_min", "x_max"):
        assert len(set(np.round(md[key], 12))) == len(md[key]), key
    for key in ("Q", "R", "Qf"):
        d = np.diag(md[key])
        assert len(set(np.round(d, 12))) == len(d) and np.all(d > 0), key
    assert not np.allclose(np.diag(md["Q"]), np.diag(md["Qf"]))
    umid = 0.5 * (md["u_min"] + md["u_max"]); xmid = 0.5 * (md["x_min"] + md["x_max"])
    assert np.all(np.abs(umid) > 0) and np.all(np.abs(xmid) > 0)
    assert np.all(md["u_min"] < 0) and np.all(md["u_max"] > 0)
    for dense in ("Q", "R", "QR"):
        mdd = H.heterogeneous(md, dense=dense)
        for key in ("Q", "Qf", "R"):
            M = mdd[key]
            assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() > 0
            assert (np.count_nonzero(M - np.diag(np.diag(M))) > 0) == (key[0] in dense)


@pytest.mark.parametrize("name,budget", SOLVER)
def test_banded_and_dense_oracles_agree(name, budget):
    md, data, zi = H.build(name)
    k = H.CASES[name]["k"]
    zo, nuo, ito, sto, steps = H.oracle(name, budget)
    assert all(s in (0, W_LINESEARCH) for s in sto), sto
    worst_z = worst_nu = 0.0
    for p in range(zo.shape[0]):
        d = dense_from_model(md, data["x0"][p], data["x0_pre"][p], data["w"][p], x_init=None if zi is None else zi[p])
        info = {}
        zd = d.mpc_fixed_log_newton(budget, k, nu0=data["nu0"][p], info=info)
        assert ito[p] == info["iters"] and np.array_equal(canon_steps(info.get("t", [])), canon_steps(steps[p])), (p, info.get("t"), steps[p])
        worst_z = max(worst_z, rel_err(zo[p], zd)); worst_nu = max(worst_nu, rel_err(nuo[p], info["nu"]))
    print("%s budget %d: banded vs dense z %.1e nu %.1e" % (name, budget, worst_z, worst_nu))
    assert worst_z <= 1e-10 and worst_nu <= 1e-9


@pytest.mark.parametrize("name,budget", SOLVER)
def test_solver_case_sees_every_mutation(name, budget):
    md, data, zi = H.build(name)
    c = H.CASES[name]
    zo, _, ito, sto, steps = H.oracle(name, budget)
    full = all(s[0] == 1.0 for s in steps)
    if name == "backtrack":
        assert any(0.0 < t < 1.0 for s in steps for t in s), "the case must backtrack"
    if c["sees_x_box"]:
        assert zi is None and all(0.0 < s[0] < 1.0 for s in steps) and all(st == 0 for st in sto), (steps, sto)
    _check_mutations("%s budget %d" % (name, budget), md, c["xf"], full, lambda mm: oracle_batch(mm, data, budget, c["k"], z_init=zi)[0], zo,
                     reads_box=zi is None, sees_x_box=c["sees_x_box"])


@pytest.mark.parametrize("name,budget", RAMP)
def test_ramp_case_sees_every_mutation(name, budget):
    md, data, du_min, du_max, u_prev = H.build_ramp(name)
    ref = H.ramp_oracle(name, budget)
    zo = [r[0] for r in ref]
    assert all(np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])) and r[2] == budget for r in ref)
    umid = 0.5 * (md["u_min"] + md["u_max"])
    assert np.all(umid != 0.0)              # (that it matters against the ramp interval: the floors of u_min, u_max below)
    full = all(r[3][0] == 1.0 for r in ref)
    c = H.RAMP_CASES[name]
    if c.get("sees_x_box"):
        assert all(0.0 < r[3][0] < 1.0 for r in ref), [r[3] for r in ref]
    _check_mutations("ramp %s budget %d" % (name, budget), md, c["xf"], full,
                     lambda mm: [r[0] for r in H.ramp_oracle_of(mm, data, du_min, du_max, u_prev, budget, c.get("k", H.RAMP_K))], zo,
                     sees_x_box=bool(c.get("sees_x_box")))


@pytest.mark.parametrize("name,budget", BANK)
def test_bank_case_sees_every_mutation(name, budget):
    base, models, per, data = H.build_bank(name)
    zo, _, ito, sto, steps = H.bank_oracle(name, budget)
    assert all(s == 0 for s in sto)
    assert len({id(mm) for mm in per}) == 3
    full = all(s[0] == 1.0 for s in steps)
    # a mutation of the shared constants, applied to every model of the bank
    def solve(mm):
        return H.bank_oracle_of([dict(mm, A1=mp_["A1"], A2=mp_["A2"]) for mp_ in per], data, budget)[0]
    _check_mutations("bank %s budget %d" % (name, budget), base, False, full, solve, zo)


@pytest.mark.parametrize("ramp", [False, True])
def test_closed_loop_case_sees_every_mutation(ramp):
    """The first moves of the fed-back steps, per realisation."""
    from oracle.closed_loop_ref import closed_loop
    vo = 1 if ramp else 2
    md, a, du = H.build_loop(vo)
    refs = H.loop_oracle(ramp, vo)
    assert all((r["status"] == 0).all() and np.all(np.isfinite(r["u0"])) for r in refs)
    assert all(np.all(r["u0"] > md["u_min"]) and np.all(r["u0"] < md["u_max"]) for r in refs), "a first move leaves the box"

    def solve(mm):
        return [closed_loop(mm, a[:, r], 1, H.LOOP_K, ramp=du if ramp else None)["u0"] for r in range(H.LOOP_R)]
    # (the loop's cold-start steps are full steps wherever the mutations of the x box change nothing: asserted by the bound itself)
    _check_mutations("closed loop, ramp=%s" % ramp, md, False, True, solve, [r["u0"] for r in refs])
