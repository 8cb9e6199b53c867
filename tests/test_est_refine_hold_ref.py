"""Pins tests/est_refine_hold_ref.py, the numpy restatement of the refinement with a held Jacobian and of the gain form that
tests/test_gpu_est_refine_hold.py judges the device by, to the convergence table the two forms were proposed with: the geometry,
seed and draws of tests/test_est_refine_ref.py (len 64, window (31, 17), diversities -3 / 0 / 3, 27 modes, noise-free, start the
linear estimate, SEED = 5, 6 draws), the worst relative error ||alpha_hat - alpha|| / ||alpha|| after the start and every
iteration.  Every entry above 1e-10 must land within a factor 4; refresh = 1 must be rr.refine exactly."""
import functools

import numpy as np
import pytest

from tests import est_refine_hold_ref as hr
from tests import est_refine_ref as rr
from tests.test_est_refine_ref import draws, geometry, maps

ONCE = 99                                                        # refresh >= iters: J built once, then held
# (norm, refresh): the start, then the error after iterations 1, 2, ..
TABLE = {
    (0.3, 1): [2.9e-2, 3.8e-4, 4.8e-8, 1.3e-14],
    (1.0, 1): [1.7e-1, 1.3e-2, 8.9e-5, 4.4e-9],
    (1.5, 1): [3.9e-1, 1.7e-1, 1.5e-2, 1.1e-4, 7.3e-9],
    (2.0, 1): [6.7e-1, 3.3e-1, 4.6e-2, 9.9e-4, 4.0e-7],
    (0.3, ONCE): [2.9e-2, 3.8e-4, 6.7e-6, 1.2e-7, 2.0e-9],
    (1.0, ONCE): [1.7e-1, 1.3e-2, 1.4e-3, 1.4e-4, 1.3e-5],
    (1.5, ONCE): [3.9e-1, 1.7e-1, 4.7e-2, 1.1e-2, 2.6e-3],
    (2.0, ONCE): [6.7e-1, 3.3e-1, 1.2e-1, 9.2e-2, 7.6e-2],
    (0.3, 0): [2.9e-2, 2.5e-3, 2.2e-4, 1.9e-5, 1.6e-6],
    (1.0, 0): [1.7e-1, 6.5e-2, 3.2e-2, 1.7e-2, 9.5e-3],
    (2.0, 3): [6.7e-1, 3.3e-1, 1.2e-1, 9.2e-2, 4.5e-3, 1.9e-4, 1.1e-5, 4.8e-11],
}


@functools.lru_cache(maxsize=None)
def inputs(norm):
    geom, Z, a = geometry(), maps()[1:], draws(norm)
    Y = rr.images(geom, Z, a)
    return geom, Z, a, Y, rr.linear_start(geom, Z, Y)


@functools.lru_cache(maxsize=None)
def run(norm, refresh, iters):
    geom, Z, a, Y, start = inputs(norm)
    out = hr.refine(geom, Z, Y, start, iters, refresh)
    return (np.linalg.norm(out["alphas"] - a[None], axis=2) / norm).max(axis=1), out


@pytest.mark.parametrize("norm,refresh", sorted(TABLE))
def test_the_convergence_table_is_reproduced(norm, refresh):
    want = TABLE[(norm, refresh)]
    err, out = run(norm, refresh, len(want) - 1)
    print(f"||alpha|| = {norm}, refresh {refresh}: " + " ".join(f"{e:.1e}" for e in err))
    for it, w in enumerate(want):
        if w > 1e-10:
            assert w / 4 <= err[it] <= 4 * w, (it, err[it], w)
        else:
            assert err[it] <= 1e-9, (it, err[it])
    assert np.all(out["status"] == 0) and np.all(out["info"][:, rr.ITERS] == len(want) - 1)


def test_refresh_three_reaches_nine_digits_in_four_iterations_at_one_radian():
    err, _ = run(1.0, 3, 4)
    assert 9.0e-9 / 4 <= err[4] <= 4 * 9.0e-9, err


def test_the_gain_form_stalls_at_one_and_a_half_radians_and_diverges_at_two():
    """The limits the header states: at ||alpha|| = 1.5 the error settles at 1e-1, at 2 it never gets below half the aberration
    and is at 0.61 after one and 0.81 after nine steps.  Nothing but COST against COST0 shows it: the cost of the worst draw is
    still above a tenth of its start after nine steps, where a converging run (0.3 rad) is more than six digits down."""
    stall, _ = run(1.5, 0, 9)
    assert np.all((1e-1 / 4 <= stall[5:]) & (stall[5:] <= 4e-1)) and stall[9] > 0.9 * stall[8], stall
    div, out = run(2.0, 0, 9)
    assert 0.61 / 4 <= div[1] <= 4 * 0.61 and 0.81 / 4 <= div[9] <= 4 * 0.81 and div[9] > div[5] and np.all(div > 0.5), div
    assert np.all(out["status"] == 0)                                                     # .. and no flag says so
    ratio = out["info"][:, rr.COST] / out["info"][:, rr.COST0]                            # (the cost need not even rise: it stays large)
    assert ratio.max() > 0.1 and run(0.3, 0, 9)[1]["info"][:, rr.COST].max() < 1e-6 * run(0.3, 0, 9)[1]["info"][:, rr.COST0].min(), ratio


@pytest.mark.parametrize("norm", [0.3, 2.0])
def test_refresh_one_is_the_gauss_newton_restatement_exactly(norm):
    geom, Z, _, Y, start = inputs(norm)
    for kw in (dict(), dict(damping=1e-3), dict(tol=1e-6)):
        want = rr.refine(geom, Z, Y[:2], start[:2], 3, **kw)
        got = hr.refine(geom, Z, Y[:2], start[:2], 3, 1, **kw)
        assert all(np.array_equal(want[k], got[k], equal_nan=True) for k in ("alphas", "info", "status")), kw


def test_the_first_iteration_is_full_whatever_the_schedule_and_the_gain_is_the_linear_estimators():
    geom, Z, a, Y, start = inputs(1.0)
    one = rr.refine(geom, Z, Y[:2], start[:2], 1)
    for refresh in (2, 3, ONCE):
        assert np.array_equal(hr.refine(geom, Z, Y[:2], start[:2], 1, refresh)["alphas"], one["alphas"])
    G = hr.gain(geom, Z)
    assert G.shape == (27, Y.shape[1])
    b_s = rr.image_model(geom, Z, np.zeros(27))[1]
    assert np.allclose((G @ (Y - b_s).T).T, start, rtol=0, atol=1e-12)
    # one gain step from zero is the linear estimate: y(0) = b_s
    out = hr.refine(geom, Z, Y[:2], np.zeros((2, 27)), 1, 0, G)
    assert np.allclose(out["alphas"][1], start[:2], rtol=0, atol=1e-12)


def test_the_contraction_condition_of_the_device_tests():
    """What the issue measured: a held J contracts by about 0.1 per iteration at 0.3 and 1 rad, the gain form by about 0.09 at
    0.3 rad; at 2 rad neither is below the 0.5 that a comparison with the device asks for."""
    geom, Z, a, Y, start = inputs(0.3)
    for norm, refresh, cap in ((0.3, ONCE, 0.15), (1.0, ONCE, 0.3), (0.3, 0, 0.2)):
        a = inputs(norm)[2]
        ratio = hr.contraction(run(norm, refresh, 4)[1]["alphas"], a, refresh)
        print(f"||alpha|| = {norm}, refresh {refresh}: worst ratio {ratio:.3f}")
        assert 0.0 < ratio <= cap, (norm, refresh, ratio)
    for refresh in (ONCE, 0):
        assert hr.contraction(run(2.0, refresh, 4 if refresh else 9)[1]["alphas"], inputs(2.0)[2], refresh) > 0.5


def test_tol_and_bad_input_freeze_a_row_in_both_forms():
    geom, Z, a, Y, start = inputs(0.3)
    for refresh in (ONCE, 0):
        out = hr.refine(geom, Z, Y[:3], start[:3], 9, refresh, tol=1e-4)
        it = out["info"][:, rr.ITERS].astype(int)
        assert np.all(out["status"] == rr.CONVERGED) and np.all(it < 9), (refresh, it)
        for b in range(3):
            assert np.array_equal(out["alphas"][it[b], b], out["alphas"][-1, b])
        Yb = Y[:3].copy(); Yb[2, 7] = np.nan
        sb = start[:3].copy(); sb[0] = 1e7 * a[0] / 0.3
        good = hr.refine(geom, Z, Y[:3], start[:3], 2, refresh)
        bad = hr.refine(geom, Z, Yb, sb, 2, refresh)
        assert bad["status"].tolist() == [rr.BAD_INPUT, 0, rr.BAD_INPUT]
        assert np.all(np.isnan(bad["alphas"][-1, [0, 2]])) and np.all(np.isnan(bad["info"][[0, 2], :2]))
        assert np.array_equal(bad["alphas"][:, 1], good["alphas"][:, 1]) and np.array_equal(bad["info"][1], good["info"][1])


def test_a_zero_column_fails_the_factorisation_but_not_the_gain_form():
    geom = geometry()
    Z = maps()[1:6].copy()
    Z[2] = 0.0
    a = draws(0.3, 2, 5)
    Y = rr.images(geom, Z, a)
    start = 0.9 * a
    held = hr.refine(geom, Z, Y, start, 3, 2)
    assert np.all(held["status"] == rr.FACTOR_FAILED) and np.array_equal(held["alphas"][-1], start)
    free = hr.refine(geom, Z, Y, start, 3, 0)
    assert np.all(free["status"] == 0) and np.all(free["info"][:, rr.ITERS] == 3) and np.all(free["alphas"][-1][:, 2] == start[:, 2])
    assert np.all(free["info"][:, rr.COST] < free["info"][:, rr.COST0])


def test_the_arguments_the_call_refuses_are_refused_here_too():
    geom, Z, _, Y, start = inputs(0.3)
    with pytest.raises(ValueError):
        hr.refine(geom, Z, Y[:1], start[:1], 1, -1)
    with pytest.raises(ValueError):
        hr.refine(geom, Z, Y[:1], start[:1], 1, 0, damping=1e-3)
