"""tests/optics_ref.py against the reference's own model, tests/golden/model_approx_As_bs.npz (model_approx.mat, loaded at
README.md:294): zernfun's UNNORMALISED modes in zernmodfit's order on the grid x = (-N:2:N)/N, the pin-hole pupil of
README.md:383-391, defocus = mode index 4, zd_list = [-3 0 3], the window 241..271 (0-based) and AU = 1e12 reproduce A_s (all 28
columns, the piston included) and b_s to fp64 round-off.  This is the yardstick the GPU tests of the device optics lean on.

Measured: 1.2e-16 on b_s, <= 4.8e-16 per column 1..27 of its own norm.  Asserted: 1e-12 -- the round-off of two FFT
implementations with three orders of margin; a wrong mode order, sign, normalisation or orientation gives O(1).  The piston
column (norm 3e-2: the disk r <= 1 and the pin-hole differ at the rim) is judged relative to the largest column norm."""
import os

import numpy as np
import pytest

from tests import optics_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "model_approx_As_bs.npz")
TOL = 1e-12


@pytest.fixture(scope="module")
def rebuilt():
    g = oref.readme_geometry(512)
    Z = oref.zernike_grid(6, 512)
    A_s, b_s = oref.model(g["pupil"], Z[4], g["zd_list"], g["dx"], g["rmin"], g["rmax"], Z, g["AU"])
    v = np.load(FIX)
    return g, Z, A_s, b_s, v["A_s"], v["b_s"].reshape(-1)


def test_geometry_is_the_readmes(rebuilt):
    g, Z, *_ = rebuilt
    assert (g["rmin"], g["rmax"]) == (241, 271) and Z.shape == (28, 512, 512)      # 0-based: range_min:range_max = 242:272
    n, m = oref.zernike_modes(6)
    assert (n[4], m[4]) == (2, 0) and list(zip(n[:6], m[:6])) == [(0, 0), (1, -1), (1, 1), (2, -2), (2, 0), (2, 2)]


def test_b_s(rebuilt):
    *_, b_s, A_fix, b_fix = rebuilt
    err = np.linalg.norm(b_s - b_fix) / np.linalg.norm(b_fix)
    print("b_s relative error", err)
    assert err <= TOL, err


def test_A_s_every_column(rebuilt):
    _, _, A_s, _, A_fix, _ = rebuilt
    assert A_s.shape == A_fix.shape == (3 * 31 * 31, 28)
    norms = np.linalg.norm(A_fix, axis=0)
    errs = np.linalg.norm(A_s - A_fix, axis=0)
    print("A_s Frobenius", np.linalg.norm(A_s - A_fix) / np.linalg.norm(A_fix), "columns", (errs / norms).max(), "piston", errs[0] / norms.max())
    assert np.linalg.norm(A_s - A_fix) <= TOL * np.linalg.norm(A_fix)
    for j in range(1, 28):
        assert errs[j] <= TOL * norms[j], (j, errs[j] / norms[j])
    assert errs[0] <= TOL * norms.max(), errs[0] / norms.max()
    assert 1e-2 < norms[0] < 1e-1                                  # the piston column is a real signal, not round-off
