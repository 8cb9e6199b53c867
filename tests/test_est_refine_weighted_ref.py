"""Pins tests/est_refine_weighted_ref.py, the numpy restatement of the refinement weighted by the detector's noise that
tests/test_gpu_est_refine_weighted.py judges the device by, and the claim the weighted fit was proposed with.  Setup: len 64, the
README's pupil, window (31, 17), defocus diversities -3 / 0 / 3, the 27 modes of N = 6 without the piston, the noise that of
`detector_read_host` on the exact images (seeded: the same on every run), gain = e- per call / sum(b_s), the start the linear
estimate of the noisy images, 5 iterations, floor 1.

The error table (rms of ||alpha_hat - alpha|| / ||alpha|| over 6 draws x 4 noise trials), as proposed and as SEED gives it:

    ||alpha||  e- per call  read noise   proposed: unweighted weighted ratio    here: unweighted weighted ratio
    0.3        1e4          0            1.26    0.548   2.30                   1.32    0.543   2.44
    0.3        1e6          0            0.116   0.0514  2.25                   0.124   0.0474  2.61
    0.3        1e6          2            0.137   0.0484  2.82                   0.123   0.0492  2.51
    0.3        1e8          0            0.0134  0.00473 2.84                   0.0124  0.00483 2.56
    1.0        1e4          0            0.296   0.156   1.90                   0.319   0.158   2.02
    1.0        1e4          2            0.275   0.207   1.33                   0.322   0.209   1.54
    1.0        1e6          2            0.0310  0.0146  2.12                   0.0308  0.0140  2.21
    1.0        1e8          2            0.00285 0.00140 2.04                   0.00306 0.00136 2.24

The conditions: weighted <= unweighted / 1.5 in the seven rows proposed with a ratio >= 1.9 -- the draws here leave them a factor
2.02 / 1.5 = 1.34 at the least -- and weighted <= unweighted in the row (1.0, 1e4, 2), which they leave a factor 1.54.

Goodness of fit (1e6 e-, read noise 2 e-, floor 0): chi^2 / (p - nmode) of the 6 draws lies within 6 sqrt(2 / (p - nmode)) = 0.159
of 1 (measured: 0.955 .. 1.031); the unweighted fit's residuals, weighted afterwards, give more (1.008 .. 1.098 times as much).

Sigma (10 modes, ||alpha|| = 0.3, 1e6 e-, read noise 2 e-, 128 noise draws of one alpha): the empirical rms error of every
coefficient over the predicted sigma (the mean over the draws) is 0.896 .. 1.067 here.  The relative standard error of an rms over
N draws is 1 / sqrt(2 N) = 0.0625: the assertion is 1 +- 4 of them, 0.75 .. 1.25.

COND is the largest cond(qe^2 J'WJ) of the cases the device is tested on (CASES below, and the table's 32): the device's
tolerance is argued from it."""
import functools

import numpy as np
import pytest

import importlib

from tests import est_refine_ref as rr
from tests import est_refine_weighted_ref as wr
from tests import optics_ref as oref

pkg = importlib.import_module("mpc-sensorlessao_amd")

L, SEED, DRAWS, TRIALS = 64, 5, 6, 4
ZD = [-3.0, 0.0, 3.0]
ONCE = 1000                                                      # refresh >= iters: J once
ROWS = [  # ||alpha||, e- per call, read noise, the proposal's ratio
    (0.3, 1e4, 0.0, 2.30), (0.3, 1e6, 0.0, 2.25), (0.3, 1e6, 2.0, 2.82), (0.3, 1e8, 0.0, 2.84),
    (1.0, 1e4, 0.0, 1.90), (1.0, 1e4, 2.0, 1.33), (1.0, 1e6, 2.0, 2.12), (1.0, 1e8, 2.0, 2.04),
]
# The cases of tests/test_gpu_est_refine_weighted.py: d, first, ndiv, nmode, refresh, detector.  5 realisations each, 3 iterations.
DETECTORS = dict(  # e- per call and the detector's other fields; floor
    photon=(1e5, dict(photon_noise=True), 1.0),
    read=(1e5, dict(photon_noise=False, read_noise=3.0), 0.0),
    both=(1e5, dict(photon_noise=True, read_noise=2.0, qe=0.7, background=5.0), 1.0),
)
NORMS = (0.3, 1.0, 0.1, 0.3, 1.0)
CASES = [
    (31, 17, 3, 27, 1, "photon"), (31, 17, 3, 27, 2, "both"), (31, 17, 3, 27, ONCE, "read"),
    (32, 16, 3, 27, 1, "both"),                                  # p = 3072, a multiple of 4
    (9, 28, 1, 1, 1, "photon"), (9, 28, 1, 1, 2, "read"),        # p = 81
    (31, 17, 3, 15, 1, "read"), (31, 17, 3, 16, 2, "photon"), (31, 17, 3, 17, 1, "both"),
    (31, 17, 3, 48, 1, "photon"), (31, 17, 3, 64, 1, "both"), (31, 17, 3, 64, ONCE, "photon"),
    (31, 17, 2, 27, 1, "photon"), (32, 16, 1, 16, ONCE, "both"), (9, 28, 2, 5, 2, "both"), (9, 28, 3, 15, 1, "read"),
]
COND = 2.3e2                                                     # see test_the_condition_number_the_device_is_judged_by


@functools.lru_cache(maxsize=None)
def maps(N=6):
    Z = oref.zernike_grid(N, L)
    Z.setflags(write=False)
    return Z


def select(nmode, Z6=None, Z10=None):
    """The maps of a mode count: 27 = N = 6 without the piston, 48 and 64 from N = 10, fewer from N = 6's third order on."""
    Z6, Z10 = maps(6) if Z6 is None else Z6, (maps(10) if nmode in (48, 64) else None) if Z10 is None else Z10
    return Z10[1:1 + nmode] if nmode in (48, 64) else Z6[1:28] if nmode == 27 else Z6[7:7 + nmode]


def geometry(d=31, first=17, ndiv=3):
    return rr.readme_geom(L, d, first, ZD[:ndiv], maps()[4])


def gain_of(geom, Z, electrons):
    """Photo-electrons per unit of Y_M that put `electrons` into all the windows of the unaberrated system."""
    return electrons / float(np.sum(rr.image_model(geom, Z, np.zeros(len(Z)))[1]))


def noisy_problem(geom, Z, norms, kind, seed=11):
    """(true alpha, noisy Y, linear start, detector dict, floor) of one realisation per entry of norms for a DETECTORS kind."""
    electrons, fields, floor = DETECTORS[kind]
    a = np.random.default_rng([seed, len(Z), len(norms)]).standard_normal((len(norms), len(Z)))
    a *= np.asarray(norms)[:, None] / np.linalg.norm(a, axis=1, keepdims=True)
    det = wr.detector(gain_of(geom, Z, electrons), **fields)
    noise = pkg.DetectorNoise(det["gain"], photon_noise=det["photon_noise"], read_noise=det["read_noise"], qe=det["qe"],
                              background=det["background"], seed=seed)
    Y = pkg.detector_read_host(rr.images(geom, Z, a), noise)
    return a, Y, rr.linear_start(geom, Z, Y), det, floor


@functools.lru_cache(maxsize=None)
def table_row(norm, electrons, read_noise):
    geom, Z = geometry(), maps()[1:]
    a = np.random.default_rng([SEED, int(10 * norm)]).standard_normal((DRAWS, 27))
    a *= norm / np.linalg.norm(a, axis=1, keepdims=True)
    Y0 = rr.images(geom, Z, a)
    gain = gain_of(geom, Z, electrons)
    eu, ew, cond = [], [], 0.0
    for t in range(TRIALS):
        Y = pkg.detector_read_host(Y0, pkg.DetectorNoise(gain, photon_noise=True, read_noise=read_noise, seed=SEED + 1000 * t), step=t)
        start = rr.linear_start(geom, Z, Y)
        u = rr.refine(geom, Z, Y, start, 5)
        w = wr.refine(geom, Z, Y, start, 5, wr.detector(gain, read_noise=read_noise), floor=1.0, want_cond=True)
        assert not u["status"].any() and not w["status"].any()
        eu.append(np.linalg.norm(u["alphas"][-1] - a, axis=1) / norm); ew.append(np.linalg.norm(w["alphas"][-1] - a, axis=1) / norm)
        cond = max(cond, w["cond"])
    return float(np.sqrt(np.mean(np.square(eu)))), float(np.sqrt(np.mean(np.square(ew)))), cond


@pytest.mark.parametrize("norm,electrons,read_noise,proposed", ROWS)
def test_weighting_halves_the_error(norm, electrons, read_noise, proposed):
    unweighted, weighted, cond = table_row(norm, electrons, read_noise)
    print(f"||alpha|| {norm}, {electrons:.0e} e-, read noise {read_noise}: unweighted {unweighted:.3g}, weighted {weighted:.3g}, "
          f"ratio {unweighted / weighted:.2f} (proposed {proposed}); cond {cond:.1f}")
    if proposed >= 1.9:
        assert weighted <= unweighted / 1.5, (unweighted, weighted)
        assert weighted * 1.3 <= unweighted / 1.5, "the margin the docstring states is gone: take more trials"
    else:
        assert weighted <= unweighted, (unweighted, weighted)
        assert weighted * 1.3 <= unweighted, "the margin the docstring states is gone: take more trials"
    assert cond <= COND


def test_chi2_is_a_goodness_of_fit_test():
    geom, Z = geometry(), maps()[1:]
    p, nmode = 3 * 31 * 31, 27
    a = np.random.default_rng([SEED, 3]).standard_normal((DRAWS, nmode))
    a *= 0.3 / np.linalg.norm(a, axis=1, keepdims=True)
    gain = gain_of(geom, Z, 1e6)
    det = wr.detector(gain, read_noise=2.0)
    Y = pkg.detector_read_host(rr.images(geom, Z, a), pkg.DetectorNoise(gain, photon_noise=True, read_noise=2.0, seed=SEED))
    start = rr.linear_start(geom, Z, Y)
    w = wr.refine(geom, Z, Y, start, 5, det, floor=0.0)
    u = rr.refine(geom, Z, Y, start, 5)
    reduced = w["info"][:, wr.COST] / (p - nmode)
    after = np.array([wr.chi2(Y[b], rr.image_model(geom, Z, u["alphas"][-1, b])[1], gain, det, 0.0)[0] for b in range(DRAWS)])
    print("chi^2 / (p - nmode):", reduced, "; the unweighted fit's, weighted afterwards, over it:", after / w["info"][:, wr.COST])
    assert np.all(np.abs(reduced - 1.0) <= 6.0 * np.sqrt(2.0 / (p - nmode))), reduced
    assert np.all(after > w["info"][:, wr.COST]), (after, w["info"][:, wr.COST])
    assert np.all(w["info"][:, wr.COST] < w["info"][:, wr.COST0])


def test_sigma_predicts_the_scatter_of_every_coefficient():
    N, nmode = 128, 10
    geom, Z = geometry(), maps()[1:1 + nmode]
    a = np.random.default_rng([SEED, 7]).standard_normal(nmode)
    a *= 0.3 / np.linalg.norm(a)
    gain = gain_of(geom, Z, 1e6)
    Y0 = np.repeat(rr.images(geom, Z, a), N, axis=0)
    Y = pkg.detector_read_host(Y0, pkg.DetectorNoise(gain, photon_noise=True, read_noise=2.0, seed=SEED + 1))     # row r: realisation r's draw
    out = wr.refine(geom, Z, Y, rr.linear_start(geom, Z, Y), 4, wr.detector(gain, read_noise=2.0), floor=1.0)
    assert not out["status"].any() and np.all(np.isfinite(out["sigma"]))
    ratio = np.sqrt(np.mean((out["alphas"][-1] - a) ** 2, axis=0)) / np.mean(out["sigma"], axis=0)
    print("rms error over predicted sigma, per coefficient:", ratio)
    assert np.all(np.abs(ratio - 1.0) <= 4.0 / np.sqrt(2.0 * N)), ratio
    assert np.all(np.std(out["sigma"], axis=0) <= 0.05 * np.mean(out["sigma"], axis=0))   # (the bound hardly depends on the draw)


def test_constant_weights_are_the_unweighted_fit():
    """photon_noise = 0, gain = qe = 1, read_noise = sigma: every w is 1 / sigma^2 and the iterates are rr.refine's, up to the
    rounding of the scaling by 1 / sigma, which cond(H) amplifies; chi^2 = cost / sigma^2."""
    geom, Z, sig = geometry(), maps()[1:], 3e-5
    a = np.random.default_rng([SEED, 9]).standard_normal((2, 27))
    a *= np.array([[0.3], [1.0]]) / np.linalg.norm(a, axis=1, keepdims=True)
    Y = rr.images(geom, Z, a) + sig * np.random.default_rng(SEED).standard_normal((2, 3 * 31 * 31))
    start = rr.linear_start(geom, Z, Y)
    u = rr.refine(geom, Z, Y, start, 4, want_cond=True)
    w = wr.refine(geom, Z, Y, start, 4, wr.detector(1.0, read_noise=sig, photon_noise=False), floor=0.0, want_cond=True)
    tol = 64.0 * np.finfo(float).eps * u["cond"]
    err = np.max(np.linalg.norm(w["alphas"] - u["alphas"], axis=2) / np.maximum(1.0, np.linalg.norm(u["alphas"], axis=2)))
    print(f"cond(H) {u['cond']:.1f} ({w['cond']:.1f} weighted), tolerance {tol:.1e}, the iterates differ by {err:.1e}")
    assert u["cond"] <= 3.2e2 and abs(w["cond"] / u["cond"] - 1.0) <= 1e-6
    assert err <= tol
    assert np.allclose(w["info"][:, :2], u["info"][:, :2] / sig ** 2, rtol=1e-9, atol=0.0)
    assert np.array_equal(w["info"][:, wr.ITERS], u["info"][:, rr.ITERS]) and np.array_equal(w["status"], u["status"])
    # sigma of constant weights: sig sqrt(diag((J'J)^-1)) at the last linearisation point
    J = rr.image_model(geom, Z, w["alphas"][-2, 0])[0]
    assert np.allclose(w["sigma"][0], sig * np.sqrt(np.diag(np.linalg.inv(J.T @ J))), rtol=1e-9)


def test_held_iterations_reweight_the_held_jacobian():
    geom, Z = geometry(), maps()[1:]
    a, Y, start, det, floor = noisy_problem(geom, Z, (0.3, 1.0), "photon")
    full = wr.refine(geom, Z, Y, start, 3, det, floor, refresh=1)
    held = wr.refine(geom, Z, Y, start, 3, det, floor, refresh=2)
    once = wr.refine(geom, Z, Y, start, 3, det, floor, refresh=ONCE)
    assert np.array_equal(full["alphas"][1], held["alphas"][1]) and np.array_equal(held["alphas"][1], once["alphas"][1])
    assert not np.array_equal(full["alphas"][2], held["alphas"][2]) and np.array_equal(held["alphas"][2], once["alphas"][2])
    assert not np.array_equal(held["alphas"][3], once["alphas"][3])
    # the held step by hand: the J of iteration 0, y and the weights of the current alpha
    J = rr.image_model(geom, Z, start[0])[0]
    y = rr.image_model(geom, Z, held["alphas"][1, 0])[1]
    w = wr.weights(y, det["gain"], det, floor)
    A = np.sqrt(w)[:, None] * J
    delta = np.linalg.solve(A.T @ A, A.T @ (np.sqrt(w) * (Y[0] - y)))
    assert np.allclose(held["alphas"][2, 0] - held["alphas"][1, 0], delta, rtol=1e-9, atol=1e-14)
    for out in (full, held, once):
        assert np.all(np.linalg.norm(out["alphas"][-1] - a, axis=1) < np.linalg.norm(start - a, axis=1))


def test_the_freeze_rules():
    geom, Z = geometry(), maps()[1:6]
    a, Y, start, det, floor = noisy_problem(geom, Z, (0.3, 0.3, 0.3, 0.3), "both")
    good = wr.refine(geom, Z, Y, start, 2, det, floor)
    assert not good["status"].any() and np.all(np.isfinite(good["sigma"]))
    Yb = Y.copy(); Yb[1, 7] = np.nan
    gains = np.array([det["gain"], det["gain"], -1.0, 0.0])
    out = wr.refine(geom, Z, Yb, start, 2, dict(det, gain=gains), floor)
    assert out["status"].tolist() == [0, wr.BAD_INPUT, wr.BAD_INPUT, wr.BAD_INPUT]
    assert np.all(np.isnan(out["alphas"][-1, 1:])) and np.all(np.isnan(out["info"][1:, :2])) and np.all(np.isnan(out["sigma"][1:]))
    assert np.array_equal(out["alphas"][:, 0], good["alphas"][:, 0]) and np.array_equal(out["info"][0], good["info"][0])
    assert np.array_equal(out["sigma"][0], good["sigma"][0])
    Zz = Z.copy(); Zz[2] = 0.0                                   # a map that vanishes: no factor, alpha stays, no sigma
    out = wr.refine(geom, Zz, Y, start, 2, det, floor)
    assert np.all(out["status"] == wr.FACTOR_FAILED) and np.array_equal(out["alphas"][-1], start) and np.all(np.isnan(out["sigma"]))
    assert np.all(np.isfinite(out["info"])) and np.array_equal(out["info"][:, wr.COST0], out["info"][:, wr.COST])
    tol = wr.refine(geom, Z, Y, start, 8, det, floor, tol=1e-3)  # a frozen realisation keeps the sigma of its last step
    assert np.all(tol["status"] == wr.CONVERGED) and np.all(tol["info"][:, wr.ITERS] < 8) and np.all(np.isfinite(tol["sigma"]))
    with pytest.raises(ValueError):
        wr.refine(geom, Z, Y, start, 2, det, floor, refresh=0)


@functools.lru_cache(maxsize=None)
def case_cond(d, first, ndiv, nmode, refresh, kind):
    geom, Z = geometry(d, first, ndiv), select(nmode)
    _, Y, start, det, floor = noisy_problem(geom, Z, NORMS, kind)
    return wr.refine(geom, Z, Y, start, 3, det, floor, refresh, want_cond=True)["cond"]


def test_the_condition_number_the_device_is_judged_by():
    """The largest cond(qe^2 J'WJ) over all the device's cases, held iterations included (measured: 2.27e2 for the 64 modes of
    N = 10 with both noises, 1.83e2 for 27 modes with read noise alone and J built once, <= 1.04e2 for the others) and the table's
    rows (32): below the 3.2e2 of the unweighted tests."""
    worst = {c: case_cond(*c) for c in CASES}                    # (every case: a held iteration weights the held J anew)
    for c, v in worst.items():
        print(c, f"{v:.2e}")
    assert max(worst.values()) <= COND and max(worst.values()) >= COND / 4
