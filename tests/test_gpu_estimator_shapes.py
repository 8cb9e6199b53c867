"""GPU tests of the estimator kernels over the space their C ABI accepts (fmpc_est_create: any window 1 <= d <= 32 at any `first`,
1 to 3 complex pupil planes of any shape, any nx the finish kernel serves; fmpc_phase_residual_device: any n <= 32, m, batch,
npx) -- tests/test_gpu_estimator.py runs one point of it (d = 31 centred, three diversities, nx = 27, the pin-hole disk).
Reference: tests/estimator_shapes_ref.py, the full FFT of README.md:461-472 for the ABI's own arguments (itself checked against a
long-double partial DFT to 1e-12, tests/test_estimator_shapes_ref.py) + numpy's minimum-norm least squares of the normal
equations.  Bars, the project's own for this operation (tests/test_gpu_estimator.py): 1e-10 relative on Y_M, 1e-8 on ad_est, per
screen; 1e-11 between two summation orders of the same screen; 1e-9 / 1e-7 for phases of thousands of turns.  Screens: 27 modes +
1 rad of pixel noise, so that every window -- the dark corners included -- carries halo energy and a relative bar means something.
Every test prints the worst figure it saw."""
import ctypes as C

import numpy as np
import pytest

from tests import estimator_shapes_ref as sr
from tests.util import rel_err

pytestmark = pytest.mark.gpu

FULL, TWO, ONE = (-3.0, 0.0, 3.0), (-2.0, 1.5), (0.0,)
_MODES = {}


def _modes(pkg, length):
    """zernike_modes(length, 28), built once per length for the module (512: a second)."""
    if length not in _MODES:
        _MODES[length] = pkg.synthetic.zernike_modes(length, 28)
    return _MODES[length]


def _build(pkg, length, kind, zd, first, d, nx, seed, A_s=None):
    """Handle + what the reference needs: D as the class builds it, a random well-conditioned A_s, b_s = Y_M of the zero screen."""
    Z = _modes(pkg, length)
    pupil, W = sr.shape_pupil(length, kind), Z[4]
    D = sr.shape_optics(length, kind, zd, W=W)
    b0 = sr.window_measurements(np.zeros((length, length)), D, first, d, sr.SCALE)
    if A_s is None:
        A_s, b_s = sr.linear_model(np.random.default_rng(seed), len(zd) * d * d, nx, b0)
    else:
        b_s = b0
    est = pkg.PhaseDiversityEstimator(pupil, W, zd, sr.DX, first + 1, first + d, A_s, b_s, AU=sr.AU)
    assert (est.len, est.d, est.ndiv, est.nx, est.p) == (length, d, len(zd), A_s.shape[1], len(zd) * d * d)
    return est, D, A_s, b_s


def _apply(est, scr, noise=None):
    import torch
    dev = torch.device("cuda:0")
    ad, Y = est.apply_device(torch.from_numpy(np.ascontiguousarray(scr)).to(dev), None if noise is None else torch.from_numpy(noise).to(dev),
                             want_Y=True)
    torch.cuda.synchronize()
    ad, Y = ad.cpu().numpy(), Y.cpu().numpy()
    assert ad.shape == (scr.shape[0], est.nx) and Y.shape == (scr.shape[0], est.p)
    return ad, Y


def _against_fft(ad, Y, scr, D, first, d, A_s, b_s, noise=None, which=None, ybar=1e-10, adbar=1e-8):
    """Per screen: Y_M against the FFT (by norm AND element by element, which also pins its length and column-major order), ad_est
    against least squares on the reference's Y_M.  Returns the worst (Y, ad) errors."""
    wy = wa = 0.0
    for b in (range(scr.shape[0]) if which is None else which):
        Yr = sr.window_measurements(scr[b], D, first, d, sr.SCALE)
        if noise is not None:
            Yr = Yr + noise[b]
        assert np.all(np.isfinite(Y[b])) and np.all(np.isfinite(ad[b]))
        ey, ea = rel_err(Y[b], Yr), rel_err(ad[b], sr.estimate(A_s, b_s, Yr))
        wy, wa = max(wy, ey), max(wa, ea)
        assert ey <= ybar, (b, ey)
        assert ea <= adbar, (b, ea)
        # element (u, v) of diversity k sits at k d^2 + v d + u: each entry within the same bar of the largest one ...
        assert np.max(np.abs(Y[b] - Yr)) <= ybar * np.max(np.abs(Yr)), b
        if d > 1:                                              # ... and the row-major order would not pass (the windows are not symmetric)
            Yt = Yr.reshape(-1, d, d).transpose(0, 2, 1).reshape(-1)
            assert rel_err(Yt, Yr) > 1e-3
    return wy, wa


# ---- a. windows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [64, 128])
@pytest.mark.parametrize("wi", range(7))
def test_windows_of_every_size_and_position(pkg, gpu, length, wi):
    """d = 31 centred, 32 (no padded column) at either corner, even d, d = 1, and windows whose frequencies first + j - len/2 are
    not symmetric about 0 (the DFT images of fmpc_host_estimator_dft_images at such a `first` have never met an FFT); len 64 takes
    the 4-wavefront PSF kernel, len 128 the 8-wavefront one.  Odd cases with noise."""
    first, d = sr.windows(length)[wi]
    est, D, A_s, b_s = _build(pkg, length, "disk", FULL, first, d, 27, seed=10 * length + wi)
    assert est.rank == min(27, est.p)
    rng = np.random.default_rng(77 * length + wi)
    scr = sr.rough_screens(rng, _modes(pkg, length)[1:], 3)
    noise = 1e-3 * np.abs(b_s).max() * rng.standard_normal((3, est.p)) if wi % 2 else None
    ad, Y = _apply(est, scr, noise)
    wy, wa = _against_fft(ad, Y, scr, D, first, d, A_s, b_s, noise)
    print(f"a. len {length} window ({first}, {d}){' + noise' if wi % 2 else ''}: Y {wy:.2e}  ad {wa:.2e}")
    est.close()


# ---- b. diversities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zd", [ONE, TWO, FULL], ids=["ndiv1", "ndiv2", "ndiv3"])
@pytest.mark.parametrize("first,d", [(5, 17), (49, 31)])
def test_one_two_and_three_diversities(pkg, gpu, zd, first, d):
    """ndiv < 3: the `k < P.ndiv` guards of the PSF kernel and its `k < P.ndiv ? k : 0` loads; the finish grid (batch, ndiv)."""
    est, D, A_s, b_s = _build(pkg, 128, "disk", zd, first, d, 27, seed=len(zd) * 100 + d)
    assert est.rank == 27
    scr = sr.rough_screens(np.random.default_rng(5 + len(zd)), _modes(pkg, 128)[1:], 3)
    ad, Y = _apply(est, scr)
    wy, wa = _against_fft(ad, Y, scr, D, first, d, A_s, b_s)
    print(f"b. ndiv {len(zd)} window ({first}, {d}): Y {wy:.2e}  ad {wa:.2e}")
    est.close()


# ---- c. pupils --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [128, 64])
@pytest.mark.parametrize("kind", sr.PUPIL_KINDS)
def test_pupils_that_are_not_the_centred_disk(pkg, gpu, length, kind):
    """The k-step range of every row block is dealt to NW x CS wavefronts by cnt wi / W: full blocks (cnt = len / 4), empty ones
    (`rows`, `offc`, `spot`), an off-centre and a hollow pupil, and -- `spot` -- a block of two k-steps for 4 (len 64) or 8 (len
    128) wavefronts, most of which get none.  Centred window and the corner (0, 32)."""
    wy = wa = 0.0
    for j, (first, d) in enumerate(((length // 2 - 15, 31), (0, 32))):
        est, D, A_s, b_s = _build(pkg, length, kind, FULL, first, d, 27, seed=length + j)
        scr = sr.rough_screens(np.random.default_rng(1000 * length + 10 * j + sr.PUPIL_KINDS.index(kind)), _modes(pkg, length)[1:], 2)
        if kind == "rows":                                     # (the reference itself sees light through what is left of the pupil)
            assert np.linalg.norm(sr.window_measurements(scr[0], D, first, d, sr.SCALE)) > 0.0 and np.count_nonzero(D) > 0
        ad, Y = _apply(est, scr)
        ey, ea = _against_fft(ad, Y, scr, D, first, d, A_s, b_s)
        wy, wa = max(wy, ey), max(wa, ea)
        est.close()
    print(f"c. len {length} pupil {kind}: Y {wy:.2e}  ad {wa:.2e}")


# ---- d. mode counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 8, 9, 10, 26, 28, 33, 64])
def test_mode_counts_around_the_row_blocks_of_the_finish_kernel(pkg, gpu, nx):
    """fmpc_est_finish takes the rows of G nine at a time (tail: j0 + jj < nx ? j0 + jj : j0) and writes share[tid] for tid < nx."""
    first, d = 49, 31
    est, D, A_s, b_s = _build(pkg, 128, "disk", FULL, first, d, nx, seed=nx)
    assert est.rank == nx
    scr = sr.rough_screens(np.random.default_rng(300 + nx), _modes(pkg, 128)[1:], 2)
    ad, Y = _apply(est, scr)
    wy, wa = _against_fft(ad, Y, scr, D, first, d, A_s, b_s)
    print(f"d. nx {nx}: Y {wy:.2e}  ad {wa:.2e}")
    est.close()


def test_rank_deficient_model_gives_the_minimum_norm_estimate(pkg, gpu):
    """nx = 10 with column 9 equal to column 8: rank 9, numpy's minimum-norm lstsq, and the two equal columns share their
    coefficient."""
    first, d = 49, 31
    A_s = np.random.default_rng(9).standard_normal((3 * d * d, 10))
    A_s[:, 9] = A_s[:, 8]
    est, D, A_s, b_s = _build(pkg, 128, "disk", FULL, first, d, 10, seed=0, A_s=A_s)
    assert est.rank == 9
    scr = sr.rough_screens(np.random.default_rng(310), _modes(pkg, 128)[1:], 2)
    ad, Y = _apply(est, scr)
    wy, wa = _against_fft(ad, Y, scr, D, first, d, A_s, b_s)
    for b in range(2):
        assert abs(ad[b, 8] - ad[b, 9]) <= 1e-9 * np.linalg.norm(ad[b])
    print(f"d. rank 9 of 10: Y {wy:.2e}  ad {wa:.2e}")
    est.close()


# ---- e. launch shapes at the reference's size --------------------------------------------------------------------------------
# fmpc_launch_estimator at len = 512 (32 row blocks), for `batch` screens of a handle with ndiv diversities and nx modes:
#   PSF kernel     wide (8 wavefronts) while batch * 32 < 512, i.e. batch <= 15, else narrow (4 wavefronts);
#                  columns split over two workgroups while nx <= 27 and batch * ndiv <= 12 (the workspace has room for that);
#   finish kernel  fmpc_est_finish_few (<2> behind the column split, else <1>) while nx <= 27 and batch * ndiv <= 64, else the
#                  general fmpc_est_finish.
#   ndiv 3, nx 27:  batch 1 .. 4   wide + split, few<2>      5 .. 15  wide, few<1>      16 .. 21  narrow, few<1>      22 ..  narrow, general
#   ndiv 1, nx 27:  batch 1 .. 12  wide + split, few<2>      13 .. 15 wide, few<1>
#   ndiv 3, nx 28:  batch 1 .. 15  wide, general             (neither the split nor the few-screen finish take nx > 27)
# The tests cannot see the shape; they see numbers: against the FFT, between shapes to 1e-11 (summation order), and bit for bit
# where the shape is the same.
@pytest.fixture(scope="module")
def ref512(pkg):
    Z = _modes(pkg, 512)
    scr = sr.rough_screens(np.random.default_rng(512), Z[1:], 22)
    return dict(scr=scr)


def test_launch_shapes_of_one_handle_at_len_512(pkg, gpu, ref512):
    """One handle, batches 1, 5, 15, 16, 21, 22, 1 of the same 22 screens in that order: every boundary of the table above, and a
    workspace (`part`, `shares`) grown and left dirty by 22 screens, whose layout differs from the split one, reused by a lone
    screen."""
    first, d, scr = 241, 31, ref512["scr"]
    est, D, A_s, b_s = _build(pkg, 512, "disk", FULL, first, d, 27, seed=512)
    order = [1, 5, 15, 16, 21, 22, 1]
    runs = [_apply(est, scr[:b]) for b in order]
    res = dict(zip(order[:-1], runs[:-1]))
    ad22, Y22 = res[22]
    wy, wa = _against_fft(ad22, Y22, scr, D, first, d, A_s, b_s, which=(0, 4, 21))
    ws = 0.0
    for b in order[:-1]:
        ad, Y = res[b]
        for i in range(b):
            ey, ea = rel_err(Y[i], Y22[i]), rel_err(ad[i], ad22[i])
            ws = max(ws, ey, ea)
            assert ey <= 1e-11 and ea <= 1e-11, (b, i, ey, ea)
    # the same launch shape: the same bits for the screens they share
    assert np.array_equal(res[5][0], res[15][0][:5]) and np.array_equal(res[5][1], res[15][1][:5])
    assert np.array_equal(res[16][0], res[21][0][:16]) and np.array_equal(res[16][1], res[21][1][:16])
    assert np.array_equal(runs[-1][0], runs[0][0]) and np.array_equal(runs[-1][1], runs[0][1])       # the dirty workspace does not show
    print(f"e. len 512, batches {order}: Y {wy:.2e}  ad {wa:.2e}  between launch shapes {ws:.2e}")
    est.close()


@pytest.mark.parametrize("zd,nx,batches", [(ONE, 27, (12, 13)), (FULL, 28, (1, 3))], ids=["ndiv1_split_boundary", "nx28_general_finish"])
def test_launch_shape_boundaries_of_other_handles_at_len_512(pkg, gpu, ref512, zd, nx, batches):
    """ndiv = 1: 12 screens is the last batch with the column split, 13 the first without.  nx = 28: the general finish behind the
    wide PSF kernel, for a lone screen too.  The first screen also stands last in every batch: same shape, same bits."""
    first, d, scr = 241, 31, ref512["scr"]
    est, D, A_s, b_s = _build(pkg, 512, "disk", zd, first, d, nx, seed=nx + len(zd))
    wy = wa = 0.0
    out = {}
    for b in batches:
        s = scr[:b].copy()
        s[b - 1] = scr[0]
        ad, Y = out[b] = _apply(est, s)
        ey, ea = _against_fft(ad, Y, s, D, first, d, A_s, b_s, which=(0,))
        wy, wa = max(wy, ey), max(wa, ea)
        assert np.array_equal(ad[b - 1], ad[0]) and np.array_equal(Y[b - 1], Y[0])
    (ad0, Y0), (ad1, Y1) = out[batches[0]], out[batches[1]]
    assert rel_err(Y0[0], Y1[0]) <= 1e-11 and rel_err(ad0[0], ad1[0]) <= 1e-11
    if nx == 28:                                               # batches 1 and 3 take the same shape
        assert np.array_equal(ad0[0], ad1[0]) and np.array_equal(Y0[0], Y1[0])
    print(f"e. len 512, ndiv {len(zd)}, nx {nx}, batches {batches}: Y {wy:.2e}  ad {wa:.2e}")
    est.close()


# ---- f. argument reduction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["seams", "cutoff"])
def test_argument_reduction_at_its_seams_and_under_its_cut_off(pkg, gpu, what):
    """fe_sincos reduces by pi/2 with k = rint(2 x / pi): phases at multiples of pi/4 give or take a few ulp (the odd multiples are
    where k changes, the even ones where the reduced argument or one of sin, cos vanishes), |j| up to 4000; and phases within one
    radian of the 1e6 cut-off, the largest k the three-part constant serves.  numpy's exp(1i x) is the reference; the bars are those
    of the existing large-phase test."""
    length, first, d = 64, 17, 31
    est, D, A_s, b_s = _build(pkg, length, "disk", FULL, first, d, 27, seed=64)
    rng = np.random.default_rng(8)
    if what == "seams":
        j = np.stack([rng.permutation(np.round(np.linspace(-4000, 4000, length * length))) for _ in range(2)])
        s = rng.integers(-1, 2, size=j.shape)
        assert set(np.unique(s)) == {-1, 0, 1} and j.min() == -4000 and j.max() == 4000
        scr = (j * (np.pi / 4) + s * 2.0 ** -50 * np.abs(j)).reshape(2, length, length)
    else:
        scr = (rng.choice([-1.0, 1.0], size=(2, length, length)) * rng.uniform(1e6 - 1, 1e6 - 1e-3, size=(2, length, length)))
        assert np.abs(scr).max() < 1e6 and np.abs(scr).min() >= 1e6 - 1
    ad, Y = _apply(est, scr)
    wy, wa = _against_fft(ad, Y, scr, D, first, d, A_s, b_s, ybar=1e-9, adbar=1e-7)
    print(f"f. {what}: Y {wy:.2e}  ad {wa:.2e}")
    est.close()


# ---- g. the residual screen -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,batch,npx", [(32, 150, 8, 256), (1, 1, 1, 1), (5, 13, 9, 300), (27, 144, 17, 255), (8, 5, 16, 257),
                                           (27, 144, 1, 64 * 64)])
def test_phase_residual_shapes(pkg, gpu, n, m, batch, npx):
    """out = phase + (u B') Z: n = 32 (every mode lane), m / 8 that is no multiple of the 6-wide inner block, m < 8 (empty eighths),
    full and partial groups of 8 screens, pixel counts around the workgroup's 256; u = NULL copies; the inputs stay as they were."""
    import torch
    from tests.util import handle_from_model
    md = pkg.synthetic.make_model(n, m, 4)
    h = handle_from_model(pkg, md)
    rng = np.random.default_rng(1000 * n + batch)
    phase = rng.standard_normal((batch, npx)); u = rng.standard_normal((batch, m)); Z = rng.standard_normal((n, npx))
    dev = torch.device("cuda:0")
    tp, tu, tz = (torch.from_numpy(a).to(dev) for a in (phase, u, Z))
    out = torch.full_like(tp, float("nan"))
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    assert h._lib.fmpc_phase_residual_device(h._h, batch, npx, vp(tp), vp(tu), vp(tz), vp(out), None) == 0
    torch.cuda.synchronize()
    e = rel_err(out.cpu().numpy(), phase + (u @ md["B"].T) @ Z)
    print(f"g. n {n} m {m} batch {batch} npx {npx}: {e:.2e}")
    assert e <= 1e-13, e
    out.fill_(float("nan"))
    assert h._lib.fmpc_phase_residual_device(h._h, batch, npx, vp(tp), None, None, vp(out), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), phase)
    assert np.array_equal(tp.cpu().numpy(), phase) and np.array_equal(tu.cpu().numpy(), u) and np.array_equal(tz.cpu().numpy(), Z)
    h.close()


def test_phase_residual_refuses_more_than_32_modes(pkg, gpu):
    """n = 40: FMPC_E_UNSUPPORTED (the kernel keeps B u in 32 lanes); nothing is launched, `out` stays as it was."""
    import torch
    from tests.util import handle_from_model
    h = handle_from_model(pkg, pkg.synthetic.make_model(40, 12, 4))
    dev = torch.device("cuda:0")
    tp = torch.zeros((2, 64), dtype=torch.float64, device=dev); tu = torch.zeros((2, 12), dtype=torch.float64, device=dev)
    tz = torch.zeros((40, 64), dtype=torch.float64, device=dev); out = torch.full_like(tp, 7.0)
    vp = lambda x: C.c_void_p(x.data_ptr())
    assert h._lib.fmpc_phase_residual_device(h._h, 2, 64, vp(tp), vp(tu), vp(tz), vp(out), None) == pkg.FMPC_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    h.close()
