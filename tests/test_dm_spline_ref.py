"""tests/dm_spline_ref.py on its own: the properties of OOMAO's profile that the device tests lean on, and the tile counts of the
reference geometry that README.md and DESIGN.md quote."""
import importlib

import numpy as np
import pytest

from tests import dm_spline_ref as ref

MECHS = (0.1, 0.2, 0.3, 0.4, 0.5)
R_TABLE = {0.1: 2.077, 0.2: 2.577, 0.3: 2.968, 0.4: 3.333, 0.5: 3.752}
R_EXACT = {0.1: 2.07748492138267, 0.2: 2.576788878500312, 0.3: 2.9683604977434443, 0.4: 3.3333333333333335, 0.5: 3.7519542445997143}


@pytest.mark.parametrize("mech", MECHS)
def test_profile_properties(mech):
    b, c, R = ref.oomao_pp(mech)
    assert b.shape == (401,) and c.shape == (400, 4) and np.all(np.diff(b) > 0) and b[-1] == R and b[0] == -R and b[200] == 0.0
    assert round(R, 3) == R_TABLE[mech] and abs(R - R_EXACT[mech]) <= 1e-12
    f = lambda d: ref.pp_eval(b, c, np.array(d, dtype=np.float64))[0].astype(np.float64)
    # the y -> x spline is an interpolation, not an inverse: f(1) = mech only as well as it interpolates (1.2e-9 mech at worst)
    f01 = f([0.0, 1.0])
    assert abs(f01[0] - 1.0) <= 1e-8 and abs(f01[1] - mech) <= 1e-8, f01
    d = np.linspace(0.0, R, 5001)
    assert float(np.max(np.abs(f(d) - f(-d)))) <= 1e-14                                   # symmetric
    assert np.all(f([-R * (1 + 1e-15), R * (1 + 1e-15), -5.0, 5.0, np.nextafter(R, 9.0)]) == 0.0)   # exactly zero outside
    assert abs(f([R])[0]) <= 1e-15 and f([np.nextafter(R, 0.0)])[0] != 0.0                # closed on the right
    fd = f(d)
    assert np.all(np.diff(fd) <= 1e-15) and fd.min() >= -1e-15                            # 'monotonic'


def test_overshoot_has_no_scale_spline():
    bx, by = ref.bezier(ref.OVERSHOOT)
    assert by.min() < 0.0 and not np.all(np.diff(by) < 0)
    with pytest.raises(ValueError):
        ref.oomao_pp(0.1, ref.OVERSHOOT)


def test_pp_eval_scales():
    b, c = ref.asymmetric_pp()
    d = np.array([-1.6, -1.5, -0.25, 0.0, 0.5, 2.25, 2.3])
    f, S, D = ref.pp_eval(b, c, d)
    assert f[0] == 0 and f[-1] == 0 and S[0] == 0 and D[-1] == 0
    assert f[1] == c[0, 0] and f[2] == c[1, 0] and f[4] == c[2, 0]
    t = np.longdouble(1.75)
    assert abs(f[5] - (c[2, 0] + t * c[2, 1] + t * t * c[2, 2] + t ** 3 * c[2, 3])) <= 1e-18
    assert np.all(S[1:-1] >= np.abs(f[1:-1]))


@pytest.mark.parametrize("mech,lo,hi", [(0.1, 25, 25), (0.2, 25, 49), (0.3, 36, 49)])
def test_reference_geometry_tile_counts(mech, lo, hi):
    """512^2 pupil, 12 x 12 actuators, pitch 61.5 px: the actuators whose support meets a 64 x 64 tile."""
    g = importlib.import_module("mpc-sensorlessao_amd").reference_dm_geometry()
    _, _, R = ref.oomao_pp(mech)
    sets = ref.tile_sets(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], -R, R)
    assert len(sets) == 64
    n = [len(s) for s in sets]
    assert (min(n), max(n)) == (lo, hi), (min(n), max(n))
    assert all(np.all(np.diff(s) > 0) for s in sets)


def test_oomao_geometry_follows_the_maps():
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    valid = np.ones((5, 5), dtype=bool); valid[0, 0] = valid[4, 1] = False
    g = pkg.oomao_dm_geometry(5, 33, ratio_tel_dm=0.9, offset=(0.25, -0.5), valid=valid)
    r = ref.oomao_geometry(5, 33, 0.9, (0.25, -0.5), valid)
    for k in ("x", "y", "cx", "cy"):
        assert np.array_equal(g[k], r[k]), k
    assert g["pitch"] == 1.0 and g["cx"].shape == (23,)
    # actuator 0 is (i, j) = (1, 0): its row profile sits on yIF[1], its column profile on xIF[0]
    assert g["cy"][0] == -1.0 + 0.5 and g["cx"][0] == -2.0 - 0.25
