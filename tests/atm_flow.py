"""Frozen flow on the output of the atmosphere, from the formulas of include/fastmpc.h alone ("the content moves with the wind:
phi_l(x, y, t) = phi_l(x - vx t, y - vy t, 0)") -- no restatement of the extrusion or of the interpolation enters, so a sign or
an axis that the kernels and tests/atm_ref.py share the wrong way round shows here.

One layer, W = 18, out_len = W - 1 (the output step is one lattice pixel), no mask, pitch 1 and dt 1.  A provider is
`make(wind) -> (screens, vp)`: `screens(k)` gives the (batch, W - 1, W - 1) screens at step k (k never decreases), vp is the pair
of pixel steps the provider works with -- `formed(*speed_direction(*wind))` for one that goes through speeds and directions.  The
same checks run on the numpy restatement on the CPU (tests/test_atm_ref_flow.py) and on the device (tests/test_gpu_atm_shapes.py).

The pixel step of a wind is formed as speed cos(dir) and speed sin(dir), so only a wind along x (a signed speed towards 0) has
an exact one: cos and sin of a rounded multiple of pi / 2 or pi / 4 are a few 1e-17 off.  Where both components are exactly the
intended ones the shift is asserted bit for bit.  Where they are not, the formulas above still say where a pixel of the later
screen lies in the earlier one: eps pixels beside a pixel centre, eps = (s(k1) - s(k0)) + d - sign(v) (lines(k1) - lines(k0)) per
axis, a few 1e-15.  A bilinear surface moves by at most eps times the largest difference of two neighbours, <= 2 M eps with M the
largest |screen|; the coordinate fl(t + s) < 32 of either screen is rounded by <= 2^-49 = 8 eps_double per axis, and the
interpolation itself by a few eps_double M.  So the bound is (2 (|eps_x| + |eps_y|) + 80 * 2^-52) M, about 2e-14 M; a wrong
sign or a swapped axis is an error of the order of M."""
import math

import numpy as np

from tests import atm_ref as ar

W, STENCIL, BATCH, SEED = 18, [1, 2, 17], 17, 11
R0, L0 = 3.0, 600.0
K0, DELTA = 2 * W + 3, 4                                   # the origins of both rings have wrapped by K0
WINDS = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (1.0, -1.0), (0.5, -0.25), (-2.0, 1.0)]
EPS = 2.0 ** -52


def speed_direction(vx, vy):
    """A wind along x is a signed speed towards 0 (its pixel step is then exact); any other the usual modulus and angle."""
    return (vx, 0.0) if vy == 0.0 else (math.hypot(vx, vy), math.atan2(vy, vx))


def formed(speed, direction):
    """The pixel steps the library forms from a speed and a direction at pitch 1 and dt 1."""
    vpx, vpy = ar.pixels_per_step([speed], [direction], 1.0, 1.0)
    return float(vpx[0]), float(vpy[0])


def _offset(k, v):
    n, f = ar.displacement(k, v)
    return n, (1.0 - f if v > 0 else f)


def check_shift(s0, s1, k0, k1, wind, vp):
    """s1 (step k1) against s0 (step k0) moved by (dx, dy) = (k1 - k0) wind; vp: the pixel steps the provider works with.
    Returns whether the comparison was bit for bit."""
    n = s0.shape[-1]
    dx, dy = round((k1 - k0) * wind[0]), round((k1 - k0) * wind[1])
    assert (dx, dy) == ((k1 - k0) * wind[0], (k1 - k0) * wind[1])
    a = s1[:, max(dy, 0):n + min(dy, 0), max(dx, 0):n + min(dx, 0)]            # s1[:, y, x]
    b = s0[:, max(-dy, 0):n + min(-dy, 0), max(-dx, 0):n + min(-dx, 0)]        # s0[:, y - dy, x - dx]
    assert a.shape == b.shape and min(a.shape[1:]) >= 9 and max(a.shape[1:]) >= 13
    assert np.abs(a).max() > 0 and not np.array_equal(s0, s1)
    exact = tuple(vp) == tuple(wind)
    if exact:
        assert np.array_equal(a, b), (wind, float(np.abs(a - b).max()))
        return True
    eps = []
    for v, d in zip(vp, (dx, dy)):
        (n0, c0), (n1, c1) = _offset(k0, v), _offset(k1, v)
        eps.append(abs((c1 - c0) + d - (1 if v > 0 else -1) * (n1 - n0)) + 4 * EPS)
    assert max(eps) < 1e-13, (wind, vp, eps)                # the formed step is the intended one to rounding
    M = np.maximum(np.abs(s0).max(axis=(1, 2)), np.abs(s1).max(axis=(1, 2)))[:, None, None]
    err = np.abs(a - b)
    assert np.all(err <= (2 * sum(eps) + 80 * EPS) * M), (wind, float((err / M).max()))
    return False


def frozen_flow(make, need_exact=((1.0, 0.0), (-1.0, 0.0))):
    """Every wind of WINDS: the screens DELTA steps apart are each other's, moved by DELTA v.  Returns the winds that were
    compared bit for bit; those of need_exact must be among them."""
    exact = []
    for wind in WINDS:
        screens, vp = make(wind)
        s0 = np.array(screens(K0))
        s1 = np.array(screens(K0 + DELTA))
        if check_shift(s0, s1, K0, K0 + DELTA, wind, vp):
            exact.append(wind)
    assert set(need_exact) <= set(exact), exact
    return exact


def half_pixel(make):
    """Half a pixel of displacement is the mean of two neighbours, bit for bit: both sides are one rounding of the same exact
    value.  Unlike the whole-pixel shifts above this depends on the side the offset s of the output grid is taken from (a constant
    error of s moves both screens alike).  v = (0.5, 0) and (-0.5, 0) from an even k to k + 1: no line enters, a pixel becomes the
    mean of itself and its left (right) neighbour.  v = (0.5, -0.25) from a multiple of 4 to k + 2: one column enters, and a pixel
    becomes the mean of the one to its left and the one below that."""
    k = K0 + 1
    assert k % 4 == 0
    for wind, dk in (((0.5, 0.0), 1), ((-0.5, 0.0), 1), ((0.5, -0.25), 2)):
        screens, vp = make(wind)
        assert tuple(vp) == wind
        s0 = np.array(screens(k))
        s1 = np.array(screens(k + dk))
        assert np.abs(s0).max() > 0
        if wind == (0.5, 0.0):
            assert np.array_equal(s1[:, :, 1:], 0.5 * (s0[:, :, :-1] + s0[:, :, 1:]))
        elif wind == (-0.5, 0.0):
            assert np.array_equal(s1[:, :, :-1], 0.5 * (s0[:, :, :-1] + s0[:, :, 1:]))
        else:
            assert np.array_equal(s1[:, :-1, 1:], 0.5 * (s0[:, :-1, :-1] + s0[:, 1:, :-1]))
