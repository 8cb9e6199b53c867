"""Pins tests/est_refine_ref.py, the numpy restatement of the Gauss-Newton refinement that tests/test_gpu_est_refine.py judges
the device by: len 64, the README's pupil, defocus diversities -3 / 0 / 3, the 27 modes of N = 6 without the piston, noise-free
images, the start the linear estimate.  TABLE is the measured convergence the refinement was proposed with (relative error
||alpha_hat - alpha|| / ||alpha||, worst of 6 draws, after 0..4 iterations); the draws here come from SEED and must land within
a factor 4 of it wherever it is above rounding level.  The caps are conditions: <= 1e-3 after 2 iterations at ||alpha|| = 1 and
<= 1e-5 after 4 at ||alpha|| = 2, and the draws must leave them a factor 5."""
import functools

import numpy as np
import pytest

from tests import est_refine_ref as rr
from tests import optics_ref as oref

L, SEED, DRAWS = 64, 5, 6
ZD = [-3.0, 0.0, 3.0]
TABLE = {0.3: [2.0e-2, 2.1e-4, 1.4e-8, 3e-14], 1.0: [1.5e-1, 1.4e-2, 1.1e-4, 7.5e-9, 5e-15], 2.0: [5.5e-1, 2.1e-1, 3.1e-2, 6.1e-4, 2.8e-7]}


@functools.lru_cache(maxsize=None)
def maps():
    Z = oref.zernike_grid(6, L)
    Z.setflags(write=False)
    return Z


def geometry(d=31, first=17, zd=ZD):
    return rr.readme_geom(L, d, first, zd, maps()[4])


def draws(norm, count=DRAWS, nmode=27):
    a = np.random.default_rng([SEED, int(10 * norm)]).standard_normal((count, nmode))
    return a * (norm / np.linalg.norm(a, axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def run(norm, d=31, first=17, ndiv=3, iters=4):
    geom = geometry(d, first, ZD[:ndiv])
    Z = maps()[1:]
    a = draws(norm)
    Y = rr.images(geom, Z, a)
    out = rr.refine(geom, Z, Y, rr.linear_start(geom, Z, Y), iters, want_cond=True)
    err = (np.linalg.norm(out["alphas"] - a[None], axis=2) / norm).max(axis=1)
    return err, out


@pytest.mark.parametrize("norm", [0.3, 1.0, 2.0])
def test_the_convergence_table_is_reproduced(norm):
    err, out = run(norm)
    print(f"||alpha|| = {norm}: " + " ".join(f"{e:.1e}" for e in err) + f"; cond(J'J) <= {out['cond']:.1e}")
    for it, want in enumerate(TABLE[norm]):
        if want > 1e-10:
            assert want / 4 <= err[it] <= 4 * want, (it, err[it], want)
        else:
            assert err[it] <= 1e-12, (it, err[it])
    assert out["cond"] <= 3.2e2                                  # the conditioning the device's tolerance is argued from
    assert np.all(out["status"] == 0) and np.all(out["info"][:, rr.ITERS] == 4)


def test_the_caps_hold_with_a_factor_five_to_spare():
    assert run(1.0)[0][2] * 5 <= 1e-3, run(1.0)[0][2]
    assert run(2.0)[0][4] * 5 <= 1e-5, run(2.0)[0][4]


@pytest.mark.parametrize("d,first", [(32, 16), (9, 28)])
def test_other_windows_behave_the_same(d, first):
    err, _ = run(1.0, d, first)
    print(f"window ({d}, {first}): " + " ".join(f"{e:.1e}" for e in err))
    for it, want in enumerate(TABLE[1.0][:4]):
        assert err[it] <= 4 * want, (it, err[it], want)


def test_one_diversity_converges_too():
    """One image (defocus -3) still determines the 27 modes: the linear start is poor (the proposal saw 0.46 at ||alpha|| = 1) and
    the iteration converges from it, every step closer, to the accuracy of the three-image case."""
    err, _ = run(1.0, ndiv=1, iters=6)
    print("one diversity: " + " ".join(f"{e:.1e}" for e in err))
    assert np.all(np.diff(err[:6]) < 0) and err[6] <= 1e-8, err


@pytest.mark.parametrize("norm", [0.3, 1.0, 2.0])
def test_the_cost_does_not_increase(norm):
    geom, Z, a = geometry(), maps()[1:], draws(norm, 2)
    Y = rr.images(geom, Z, a)
    start = rr.linear_start(geom, Z, Y)
    costs = np.stack([rr.refine(geom, Z, Y, start, it)["info"][:, rr.COST] for it in range(5)])
    floor = 1e-20 * np.sum(Y * Y, axis=1)                        # (costs at rounding level are not ordered)
    assert np.all(costs[1:] <= np.maximum(costs[:-1], floor)), costs
    out = rr.refine(geom, Z, Y, start, 2)
    assert np.allclose(out["info"][:, rr.COST0], costs[0], rtol=1e-12) and np.allclose(out["info"][:, rr.COST], costs[2], rtol=1e-12)


def test_noise_settles_at_its_floor_after_one_iteration():
    geom, Z, a = geometry(), maps()[1:], draws(1.0, 2)
    Y = rr.images(geom, Z, a)
    b_s = rr.image_model(geom, Z, np.zeros(27))[1]
    Y = Y + 0.01 * np.sqrt(np.mean(b_s ** 2)) * np.random.default_rng(SEED).standard_normal(Y.shape)
    out = rr.refine(geom, Z, Y, rr.linear_start(geom, Z, Y), 3)
    err = np.linalg.norm(out["alphas"] - a[None], axis=2).max(axis=1)
    print("noise of 1 % of rms(b_s): " + " ".join(f"{e:.1e}" for e in err))
    assert err[1] <= 4 * 1.9e-2 and abs(err[3] - err[1]) <= 0.5 * err[1], err      # the issue's floor: 1.9e-2


def test_tol_stops_a_realisation_and_counts_its_steps():
    geom, Z = geometry(), maps()[1:]
    a = np.stack([draws(0.3, 1)[0], draws(2.0, 1)[0]])
    Y = rr.images(geom, Z, a)
    start = rr.linear_start(geom, Z, Y)
    out = rr.refine(geom, Z, Y, start, 8, tol=1e-6)
    assert np.all(out["status"] == rr.CONVERGED)
    it = out["info"][:, rr.ITERS].astype(int)
    assert it[0] < it[1] < 8, it
    for b in range(2):                                           # alpha stops changing; the steps before are the free run's
        free = rr.refine(geom, Z, Y[b], start[b], int(it[b]))
        assert np.array_equal(out["alphas"][-1, b], free["alphas"][-1, 0]) and np.array_equal(out["alphas"][it[b], b], out["alphas"][-1, b])
        assert np.array_equal(out["info"][b, :3], free["info"][0, :3])


def test_a_zero_column_fails_the_factorisation_and_nothing_else():
    geom = geometry()
    Z = maps()[1:6].copy()
    Z[2] = 0.0                                                   # a map that vanishes in the pupil
    a = draws(0.3, 2, 5)
    Y = rr.images(geom, Z, a)
    start = 0.9 * a
    out = rr.refine(geom, Z, Y, start, 3)
    assert np.all(out["status"] == rr.FACTOR_FAILED) and np.all(out["info"][:, rr.ITERS] == 0)
    assert np.array_equal(out["alphas"][-1], start) and np.all(np.isfinite(out["info"]))
    assert np.array_equal(out["info"][:, rr.COST0], out["info"][:, rr.COST])
    damped = rr.refine(geom, Z, Y, start, 3, damping=1e-3)       # (the damping scales the diagonal: a zero stays a zero)
    assert np.all(damped["status"] == rr.FACTOR_FAILED)


def test_bad_input_stays_in_its_row():
    geom, Z, a = geometry(), maps()[1:], draws(0.3, 3)
    Y = rr.images(geom, Z, a)
    start = rr.linear_start(geom, Z, Y)
    good = rr.refine(geom, Z, Y, start, 2)
    Yb = Y.copy(); Yb[2, 7] = np.nan
    sb = start.copy(); sb[0] = 1e7 * a[0] / 0.3                  # pixels of 1e7 rad
    out = rr.refine(geom, Z, Yb, sb, 2)
    assert out["status"].tolist() == [rr.BAD_INPUT, 0, rr.BAD_INPUT]
    assert np.all(np.isnan(out["alphas"][-1, [0, 2]])) and np.all(np.isnan(out["info"][[0, 2], :2]))
    assert np.array_equal(out["alphas"][:, 1], good["alphas"][:, 1]) and np.array_equal(out["info"][1], good["info"][1])
    zero = rr.refine(geom, Z, Yb, sb, 0)                         # iters = 0: the costs and the status, alpha left alone
    assert zero["status"].tolist() == [rr.BAD_INPUT, 0, rr.BAD_INPUT] and np.array_equal(zero["alphas"][-1], sb)
    assert zero["info"][1, rr.COST0] == zero["info"][1, rr.COST] == good["info"][1, rr.COST0]
