"""Statistics of the atmosphere's process, taken from its numpy restatement (tests/atm_ref.py) -- they are the algorithm's, the
device computes the same lines.  W = 33, L0 / D = 42, r0 = 0.2 D, 4000 realisations, fixed seed: the structure function of the
windows over that of phaseStats.m:176-192 at separations of 1, 4, 16 and 32 pixels along x and along y, after the start-up and
after 240 steps of a wind of (0.8, 1.4) pixels (527 extrusions).

Bar: |ratio - 1| <= 4 standard errors + 0.05.  The standard error comes from the spread over the realisations; 0.05 is the
allowance for the bias of a stencil of a few lines.  Measured with the default stencil 1, 2, 4, 8, 16, 32 (seed 5, R = 4000): ratios
    separation        1 px            4 px            16 px           32 px          (x, y; standard errors 0.005, 0.008, 0.016, 0.020)
    start-up          1.002, 1.003    1.004, 1.006    0.995, 1.018    0.971, 1.019
    after 240 steps   0.999, 1.004    0.999, 1.007    1.001, 1.007    0.984, 1.014
so the bias stays below 0.03 where it can be told from the noise, and the allowance is kept at 0.05.
A stencil of the two nearest lines fails the same bar at 32 pixels along the wind: 0.823 after the start-up and 0.859 after 99
steps of one pixel along x (standard error 0.017, bar 0.117).  The whole file takes half a minute of CPU."""
import numpy as np
import pytest

from tests import atm_ref as ar

W, R, SEED = 33, 4000, 5
R0, L0, PITCH = 0.2, 42.0, 1.0 / (W - 2)
SEPS = (1, 4, 16, 32)
_CACHE = {}


def ratios(win):
    """{(axis, sep): (ratio, standard error)} of the structure function of windows (R, W, W) to theory."""
    out = {}
    for sep in SEPS:
        theory = ar.structure_function(np.array([sep * PITCH]), R0, L0)[0]
        for axis, name in ((2, "x"), (1, "y")):
            a = np.take(win, np.arange(sep, W), axis=axis) - np.take(win, np.arange(0, W - sep), axis=axis)
            per = (a ** 2).mean(axis=(1, 2)) / theory                     # one figure per realisation
            out[(name, sep)] = (float(per.mean()), float(per.std(ddof=1) / np.sqrt(per.size)))
    return out


def run(pkg, stencil, wind, steps):
    key = (tuple(stencil), wind, steps)
    if key not in _CACHE:
        ext = ar.extruders_lib(pkg, W, PITCH, R0, L0, list(stencil))
        ref = ar.AtmRef(W, stencil, ext, [1.0], [wind[0]], [wind[1]], R, ar.xi_lib(pkg, SEED, R, W))
        ref.reset()
        start = ratios(ref.win[0])
        ref.advance(steps)
        _CACHE[key] = (start, ratios(ref.win[0]), ref.e[0])
    return _CACHE[key]


@pytest.mark.parametrize("moment", ["start-up", "after 240 steps"])
def test_structure_function_of_the_default_stencil(pkg, moment):
    pytest.importorskip("scipy")
    start, end, e = run(pkg, ar.default_stencil(W), (0.8, 1.4), 240)
    assert e == W + ar.displacement(240, 0.8)[0] + ar.displacement(240, 1.4)[0] and e >= W + 527
    got = start if moment == "start-up" else end
    for key, (ratio, se) in got.items():
        print(f"default stencil, {moment}, {key}: ratio {ratio:.4f} s.e. {se:.4f}")
    for key, (ratio, se) in got.items():
        assert se < 0.03 and abs(ratio - 1.0) <= 4 * se + 0.05, (moment, key, ratio, se)


def test_two_line_stencil_fails_the_same_bar_along_the_wind(pkg):
    """The test can tell the difference: with the stencil {1, 2} the window loses the large scales along the wind."""
    pytest.importorskip("scipy")
    start, end, _ = run(pkg, [1, 2], (1.0, 0.0), 3 * W)
    for moment, got in (("start-up", start), ("after 99 steps along x", end)):
        ratio, se = got[("x", 32)]
        print(f"stencil 1, 2, {moment}, ('x', 32): ratio {ratio:.4f} s.e. {se:.4f}")
        assert se < 0.03 and abs(ratio - 1.0) > 4 * se + 0.05, (moment, ratio, se)
    ratio, se = end[("x", 1)]
    assert abs(ratio - 1.0) <= 4 * se + 0.05                              # (at one pixel it is as good as any)
