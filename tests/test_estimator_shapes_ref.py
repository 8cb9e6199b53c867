"""The reference the estimator's shape tests compare against (tests/estimator_shapes_ref.py) is itself checked here, without a
GPU: its FFT route against the partial DFT written out in long double, for every (len <= 128, pupil, diversities, window) that
tests/test_gpu_estimator_shapes.py uses, screens of 0.05 and 1.0 rad roughness.  Bar: 1e-12 relative in the 2-norm per case (an
FFT of 128 x 128 doubles against an 80-bit sum: a few 1e-16 expected, 3.0e-15 the worst measured)."""
import numpy as np
import pytest

from oracle import estimator_ref as er
from tests import estimator_shapes_ref as sr
from tests.util import rel_err


@pytest.fixture(scope="module")
def modes(pkg):
    return {length: pkg.synthetic.zernike_modes(length, 28) for length in (64, 128)}


@pytest.mark.parametrize("length", [64, 128])
def test_fft_route_against_the_long_double_partial_dft(modes, length):
    worst = 0.0
    for i, (ln, kind, zd, first, d) in enumerate(c for c in sr.cpu_cases() if c[0] == length):
        D = sr.shape_optics(ln, kind, zd, W=modes[ln][4])
        rng = np.random.default_rng(1000 * ln + i)
        for rough in (0.05, 1.0):
            scr = sr.rough_screens(rng, modes[ln][1:], 1, rough)[0]
            Y = sr.window_measurements(scr, D, first, d, sr.SCALE)
            Yl = sr.window_measurements_ld(scr, D, first, d, sr.SCALE)
            assert Y.shape == (len(zd) * d * d,) and Yl.dtype == np.longdouble
            e = float(np.linalg.norm(Y - Yl) / np.linalg.norm(Yl))
            worst = max(worst, e)
            assert e <= 1e-12, (ln, kind, zd, first, d, rough, e)
    print(f"len {length}: worst FFT against long double {worst:.2e}")


def test_the_general_reference_agrees_with_the_restatement_where_both_apply(pkg, modes):
    """Centred window + pin-hole disk + three diversities: oracle/estimator_ref.py computes the same Y_M; the disk is the reference's
    pupil pixel for pixel; W is mode 4."""
    for length in (64, 128):
        rmin, rmax = er.window_range(length, sr.DX)
        assert (rmin, rmax - rmin + 1) == sr.windows(length)[0]
        pupil = sr.shape_pupil(length, "disk")
        assert np.array_equal(pupil, er.pupil_mask(length, sr.DX))
        W = sr.diversity_mode(length)
        assert np.array_equal(W, modes[length][4])
        zd = (-3.0, 0.0, 3.0)
        scr = sr.rough_screens(np.random.default_rng(length), modes[length][1:], 1)[0]
        Y = sr.window_measurements(scr, sr.shape_optics(length, "disk", zd, W=W), rmin, rmax - rmin + 1, sr.SCALE)
        assert rel_err(Y, er.measurements(scr, pupil, W, zd, sr.DX, sr.AU)) <= 1e-14


def test_pupil_kinds_give_the_row_blocks_they_are_for():
    """Per block of 16 rows, the range of 4-column steps that see the pupil (what fmpc_est_create builds): empty blocks, blocks
    with fewer steps than the 4 / 8 / 16 wavefronts they are dealt to, full blocks."""
    def counts(pupil):
        length = pupil.shape[0]
        out = []
        for b in range(length // 16):
            q = np.nonzero(pupil[16 * b:16 * b + 16].reshape(16, length // 4, 4).any(axis=(0, 2)))[0]
            out.append(0 if q.size == 0 else int(q[-1] - q[0] + 1))
        return out
    for length in (64, 128):
        assert counts(sr.shape_pupil(length, "full")) == [length // 4] * (length // 16)
        rows = counts(sr.shape_pupil(length, "rows"))
        assert rows[0] == 0 and rows[-1] == 0 and rows[-2] == 0 and max(rows) > 0
        offc = counts(sr.shape_pupil(length, "offc"))
        assert 0 in offc and max(offc) >= length // 8
        disk, ann = sr.shape_pupil(length, "disk"), sr.shape_pupil(length, "annulus")
        assert ann.sum() < disk.sum() and ann[length // 2, length // 2] == 0 and counts(ann) == counts(disk)
        # fewer k-steps than the wavefronts of the workgroup (4 at len 64, 8 at len 128): only the spot has such a block at these sizes
        spot = counts(sr.shape_pupil(length, "spot"))
        assert sorted(spot)[-2:] == [0, 2]
        assert not any(0 < c < 4 for kind in sr.PUPIL_KINDS[:5] for c in counts(sr.shape_pupil(length, kind)))


def test_linear_model_and_the_window_list():
    rng = np.random.default_rng(0)
    A, b = sr.linear_model(rng, 3 * 31 * 31, 27, np.arange(3 * 31 * 31))
    assert A.shape == (2883, 27) and b.shape == (2883,) and b.dtype == np.float64
    A, b = sr.linear_model(rng, 3, 27, np.ones(3))                       # d = 1: fewer measurements than modes
    assert A.shape == (3, 27)
    x = sr.estimate(A, b, b + A @ np.ones(27))
    assert np.allclose(A @ x, A @ np.ones(27), rtol=1e-8)                # minimum-norm solution of a consistent system
    for length in (64, 128):
        for first, d in sr.windows(length):
            assert 0 <= first and first + d <= length and 1 <= d <= 32
        assert any(first == 0 for first, _ in sr.windows(length)) and any(first + d == length for first, d in sr.windows(length))
