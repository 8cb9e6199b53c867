"""tests/atm_flow.py on the numpy restatement (tests/atm_ref.py, float64), on the CPU: the index logic of the frozen-flow checks is
validated before they judge the device (tests/test_gpu_atm_shapes.py), and the restatement itself is held to the header's
sentence.  Twice: with the intended pixel steps given exactly (all seven winds and the half-pixel identity hold bit for bit),
and with the steps formed from a speed and a direction as the library forms them."""
import numpy as np
import pytest

from tests import atm_flow as af
from tests import atm_ref as ar

_EXT = []


def provider(pkg, exact):
    if not _EXT:
        _EXT.append(ar.extruders_lib(pkg, af.W, 1.0, af.R0, af.L0, af.STENCIL))

    def make(wind):
        vp = tuple(wind) if exact else af.formed(*af.speed_direction(*wind))
        ref = ar.AtmRef(af.W, af.STENCIL, _EXT[0], [1.0], [vp[0]], [vp[1]], af.BATCH, ar.xi_lib(pkg, af.SEED, af.BATCH, af.W))
        ref.reset()

        def screens(k):
            assert k >= ref.k
            ref.advance(k - ref.k)
            return np.array(ref.screen(af.W - 1), dtype=np.float64)
        return screens, vp
    return make


def test_frozen_flow_with_exact_pixel_steps(pkg):
    assert af.frozen_flow(provider(pkg, True), need_exact=af.WINDS) == af.WINDS
    af.half_pixel(provider(pkg, True))


def test_frozen_flow_with_formed_pixel_steps(pkg):
    exact = af.frozen_flow(provider(pkg, False))
    print("compared bit for bit:", exact)
    af.half_pixel(provider(pkg, False))


def test_the_check_sees_a_wrong_sign(pkg):
    """The screens of the opposite wind fail the comparison: the check can tell."""
    make = provider(pkg, True)
    for wind in ((1.0, 0.0), (0.0, -1.0)):
        screens, _ = make((-wind[0], -wind[1]))
        s0, s1 = screens(af.K0), screens(af.K0 + af.DELTA)
        with pytest.raises(AssertionError):
            af.check_shift(s0, s1, af.K0, af.K0 + af.DELTA, wind, wind)
        vp = (wind[0] + 1e-17 * (wind[0] == 0), wind[1] + 1e-17 * (wind[1] == 0))       # the bounded form of the comparison
        with pytest.raises(AssertionError):
            af.check_shift(s0, s1, af.K0, af.K0 + af.DELTA, wind, vp)
