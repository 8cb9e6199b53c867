"""The Shack-Hartmann sensor on the device (fmpc_sh_*, pkg.ShackHartmann) against the numpy restatement tests/shwfs_ref.py.

Shapes: (len, npl) = (64, 16), (64, 32), (128, 16), (128, 32) -- 2 x 2 up to 8 x 8 lenslets, both row-block counts of the kernel --
with pad 1, 2, 4 and s in {2, 8, 16, 32} (both column-tile counts), disk, off-centre, annulus and full pupils, the three threshold
modes.  Screens are modes plus 1 rad of per-pixel roughness, so every window carries light.

Bars (tests/shwfs_ref.py, measured and asserted on the CPU by tests/test_shwfs_ref.py): the restatement in double is within
5 ulp(1) of a lenslet's peak (frame) and 1.25 s ulp(1) pixels (slopes) of itself in long double; the device sums in another order
and has its own sincos, so its bars are 16 x these: 1.8e-14 of the peak, 4.4e-15 s pixels.  Everything called an equality is one
of bits (NaN where NaN)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import optics_ref as orf
from tests import shwfs_ref as sh

pytestmark = pytest.mark.gpu

MIN_LIGHT = 0.1                         # (partly lit lenslets are valid too)


@functools.lru_cache(maxsize=None)
def modes(length):
    Z = orf.zernike_grid(6, length)[1:]
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def pupil(length, kind):
    A = sh.make_pupil(length, kind)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def screens(length, batch, seed=0):
    s = sh.rough_screens(np.random.default_rng(1000 * length + batch + seed), modes(length), batch)
    s.setflags(write=False)
    return s


def dev(a, gpu):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(gpu)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=-7.25), torch.nan_to_num(b, nan=-7.25)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def rowmajor(frame):
    """A device frame (batch, nL s, nL s) [b, column, row] as numpy [b, row, column]."""
    return np.swapaxes(frame.cpu().numpy(), -1, -2)


def frame_error(got, want, nL, s):
    """Worst pixel error relative to its lenslet's own peak."""
    pk = want.reshape(nL, s, nL, s).max(axis=(1, 3))
    err = np.abs(got - want).reshape(nL, s, nL, s).max(axis=(1, 3)) / np.where(pk > 0, pk, 1.0)
    return float(err.max())


CASES = [(64, 16, 2, 16, "disk"), (64, 16, 1, 8, "offcentre"), (64, 16, 4, 32, "annulus"), (64, 16, 2, 2, "full"),
         (64, 32, 1, 32, "disk"), (64, 32, 2, 16, "annulus"), (64, 32, 4, 8, "offcentre"), (64, 32, 2, 2, "full"),
         (128, 16, 2, 16, "disk"), (128, 16, 2, 32, "offcentre"), (128, 16, 1, 16, "annulus"), (128, 16, 4, 8, "full"),
         (128, 32, 2, 32, "annulus"), (128, 32, 1, 16, "full"), (128, 32, 4, 2, "disk"), (128, 32, 2, 8, "offcentre")]


@pytest.mark.parametrize("length,npl,pad,s,kind", CASES)
def test_frame_and_slopes_against_the_reference(pkg, gpu, length, npl, pad, s, kind):
    A, phi, scale, batch = pupil(length, kind), screens(length, 3), 1.7, 3
    nL = length // npl
    sen = pkg.ShackHartmann(A, npl, pad=pad, spot=s, min_light=MIN_LIGHT, scale=scale)
    valid = sh.valid_mask(A, npl, MIN_LIGHT)
    assert (sen.len, sen.npl, sen.pad, sen.s, sen.nL, sen.nvalid) == (length, npl, pad, s, nL, int(valid.sum())) and np.array_equal(sen.valid, valid)
    d = dev(phi, gpu)
    frames = [sh.frame(A, phi[b], npl, pad, s, scale) for b in range(batch)]
    ref = np.linspace(0.0, 1.0, 2 * sen.nvalid)
    worst_f = worst_s = 0.0
    for thr, arg in (((sh.NONE, 0.0, 0.0), None), ((sh.FLOOR, 0.02 * frames[0].max(), 0.0), 0.02 * frames[0].max()), ((sh.FRACTION, 1e-6, 0.3), (1e-6, 0.3))):
        sen.set_threshold(arg)
        rc = sen._lib.fmpc_sh_set_reference_device(sen._h, C.c_void_p(dev(ref, gpu).data_ptr()), 0.75, None)
        torch.cuda.synchronize()
        assert rc == 0
        fr, sl, dk = sen.measure(d, want_frame=True, want_dark=True)
        assert fr.shape == (batch, nL * s, nL * s) and sl.shape == (batch, 2 * sen.nvalid) and dk.dtype == torch.int32
        fr, sl, dk = rowmajor(fr), sl.cpu().numpy(), dk.cpu().numpy()
        for b in range(batch):
            ws, wd = sh.slopes(frames[b], valid, s, thr, ref=ref, units=0.75)
            ef, es = frame_error(fr[b], frames[b], nL, s), float(np.abs(sl[b] - ws).max()) / 0.75
            worst_f, worst_s = max(worst_f, ef), max(worst_s, es)
            assert dk[b] == wd, (thr, b, dk[b], wd)
            assert ef <= sh.FRAME_BAR and es <= sh.slope_bar(s), (thr, b, ef, es)
    print("shwfs", (length, npl, pad, s, kind), "nvalid %d  frame %.2e (bar %.2e)  slopes %.2e px (bar %.2e)" % (sen.nvalid, worst_f, sh.FRAME_BAR, worst_s, sh.slope_bar(s)))
    sen.close()


def test_lenslets_without_light(pkg, gpu):
    """The caller's own mask with every lenslet valid on an off-centre disk: the dark corners are zeros in the frame, zero slopes,
    and counted."""
    length, npl, s = 128, 16, 16
    A = pupil(length, "offcentre")
    allv = np.ones((8, 8), dtype=bool)
    sen = pkg.ShackHartmann(A, npl, valid=allv)
    assert sen.nvalid == 64
    lit = (A.reshape(8, npl, 8, npl) > 0).any(axis=(1, 3))
    assert 0 < (~lit).sum() < 64
    fr, sl, dk = sen.measure(dev(screens(length, 2), gpu), want_frame=True, want_dark=True)
    fr, sl = rowmajor(fr), sl.cpu().numpy()
    for b in range(2):
        want_f = sh.frame(A, screens(length, 2)[b], npl, 2, s, 1.0)
        ws, wd = sh.slopes(want_f, allv, s)
        assert frame_error(fr[b], want_f, 8, s) <= sh.FRAME_BAR and np.abs(sl[b] - ws).max() <= sh.slope_bar(s)
        assert int(dk[b]) == wd == int((~lit).sum())
        dark_places = np.flatnonzero(~lit.ravel(order="F"))
        assert (sl[b][dark_places] == 0).all() and (sl[b][64 + dark_places] == 0).all()
        assert (fr[b].reshape(8, s, 8, s).transpose(0, 2, 1, 3)[~lit] == 0).all()         # [i, j, row, column] of the spots
    sen.close()


@pytest.mark.parametrize("npl,pad,s,thr", [(16, 2, 16, None), (16, 4, 32, (1e-6, 0.3)), (32, 1, 32, 0.01), (32, 2, 8, (0.0, 0.2))])
def test_bits_do_not_depend_on_batch_place_or_outputs(pkg, gpu, npl, pad, s, thr):
    length = 64
    A = pupil(length, "annulus")
    sen = pkg.ShackHartmann(A, npl, pad=pad, spot=s, min_light=MIN_LIGHT, threshold=thr)
    R = np.random.default_rng(5).standard_normal((27, 2 * sen.nvalid))
    sen.set_reconstructor(R)
    phi = dev(screens(length, 17), gpu)
    one = phi[4:5].contiguous()
    f1, s1, c1, d1 = sen.measure(one, want_frame=True, want_dark=True)
    for batch in (3, 17, 70):                                                          # the same screen at every place
        fb, sb, cb, db = sen.measure(one.expand(batch, length, length).contiguous(), want_frame=True, want_dark=True)
        for t1, tb in ((f1, fb), (s1, sb), (c1, cb), (d1, db)):
            assert torch.equal(tb, t1.expand_as(tb)), batch
    fm, sm, cm, dm = sen.measure(phi, want_frame=True, want_dark=True)                 # among other screens
    assert torch.equal(fm[4:5], f1) and torch.equal(sm[4:5], s1) and torch.equal(cm[4:5], c1) and torch.equal(dm[4:5], d1)
    # which outputs are asked for
    assert torch.equal(sen.measure(phi), sm)
    assert torch.equal(sen.coefficients(phi), cm)
    s2, c2 = sen.measure(phi, want_coef=True)
    assert torch.equal(s2, sm) and torch.equal(c2, cm)
    f2 = sen.measure(phi, want_frame=True, want_coef=False, want_slopes=False)
    assert torch.equal(f2, fm)
    # the slopes of the stored frame are the fused slopes; two calls in a row
    s3, c3, d3 = sen.slopes_from_frame(fm, want_coef=True, want_dark=True)
    assert torch.equal(s3, sm) and torch.equal(c3, cm) and torch.equal(d3, dm)
    padded = torch.zeros((17, fm[0].numel() + 5), dtype=torch.float64, device=gpu)     # frames ld doubles apart
    padded[:, :fm[0].numel()] = fm.reshape(17, -1)
    assert torch.equal(sen.slopes_from_frame(padded[:, :fm[0].numel()]), sm)
    fa, sa, ca, da = sen.measure(phi, want_frame=True, want_dark=True)
    assert torch.equal(fa, fm) and torch.equal(sa, sm) and torch.equal(ca, cm) and torch.equal(da, dm)
    sen.close()


@pytest.mark.parametrize("nmode", [1, 27, 32, 33, 64, 65, 128])
def test_coefficients_against_the_reference(pkg, gpu, nmode):
    length, npl, pad, s = 128, 16, 2, 16
    A, phi = pupil(length, "disk"), screens(length, 2)
    sen = pkg.ShackHartmann(A, npl, min_light=MIN_LIGHT)
    valid = sh.valid_mask(A, npl, MIN_LIGHT)
    R = np.random.default_rng(nmode).standard_normal((nmode, 2 * sen.nvalid))
    with pytest.raises(pkg.FastMPCError) as e:
        sen.coefficients(dev(phi, gpu))
    assert e.value.code == pkg.FMPC_E_UNSUPPORTED
    sen.set_reconstructor(R)
    assert sen.nmode == nmode
    sl, cf = sen.measure(dev(phi, gpu), want_coef=True)
    bar = sh.slope_bar(s) * np.linalg.norm(R, 1)
    for b in range(2):
        want = R @ sh.slopes(sh.frame(A, phi[b], npl, pad, s, 1.0), valid, s)[0]
        err = float(np.abs(cf[b].cpu().numpy() - want).max())
        print("coef nmode %d screen %d: %.2e (bar %.2e)" % (nmode, b, err, bar))
        assert err <= bar, (err, bar)
    if nmode == 128:
        with pytest.raises(pkg.FastMPCError) as e:
            sen.set_reconstructor(np.zeros((129, 2 * sen.nvalid)))
        assert e.value.code == pkg.FMPC_E_UNSUPPORTED and sen.nmode == 128
        sen.set_reconstructor(None)
        assert sen.nmode == 0
    sen.close()


def test_threshold_above_every_pixel(pkg, gpu):
    length, npl = 64, 16
    A = pupil(length, "disk")
    sen = pkg.ShackHartmann(A, npl, min_light=MIN_LIGHT)
    fr = sen.measure(dev(screens(length, 2), gpu), want_frame=True, want_slopes=False)
    sen.set_threshold(2.0 * float(fr.max()))
    sl, dk = sen.measure(dev(screens(length, 2), gpu), want_dark=True)
    assert not bool(sl.any()) and dk.tolist() == [sen.nvalid] * 2
    sen.set_threshold((2.0 * float(fr.max()), 0.1))
    sl, dk = sen.measure(dev(screens(length, 2), gpu), want_dark=True)
    assert not bool(sl.any()) and dk.tolist() == [sen.nvalid] * 2
    sen.close()


def test_a_screen_that_is_no_phase_screen(pkg, gpu):
    length, npl = 64, 16
    A = pupil(length, "disk")
    sen = pkg.ShackHartmann(A, npl, min_light=MIN_LIGHT, threshold=(0.0, 0.2))
    sen.set_reconstructor(np.random.default_rng(2).standard_normal((9, 2 * sen.nvalid)))
    phi = screens(length, 5).copy()
    clean = sen.measure(dev(phi, gpu), want_frame=True, want_dark=True)
    r, c = np.argwhere(A > 0)[37]
    assert A[r + 3, c] > 0
    phi[1, r, c] = np.nan
    phi[3, r + 3, c] = 1.0e6
    r0, c0 = np.argwhere(A == 0)[0]
    phi[2, r0, c0] = np.inf                                                            # no light there: never read into any arithmetic
    phi[4, r, c] = 999999.0                                                            # still a phase
    got = sen.measure(dev(phi, gpu), want_frame=True, want_dark=True)
    for b in (1, 3):
        assert bool(torch.isnan(got[0][b]).all()) and bool(torch.isnan(got[1][b]).all()) and bool(torch.isnan(got[2][b]).all()) and int(got[3][b]) == -1
    for b in (0, 2):
        assert all(torch.equal(g[b], k[b]) for g, k in zip(got, clean)), b
    assert bool(torch.isfinite(got[0][4]).all()) and bool(torch.isfinite(got[1][4]).all())
    # the same through a stored frame: the NaN frame gives NaN slopes, the others theirs
    sl, cf, dk = sen.slopes_from_frame(got[0], want_coef=True, want_dark=True)
    assert same(sl, got[1]) and same(cf, got[2]) and torch.equal(dk, got[3])
    sen.close()


def test_orientation_on_the_device(pkg, gpu):
    npl, pad, s, length = 16, 2, 16, 64
    sen = pkg.ShackHartmann(pupil(length, "full"), npl)
    ref = sen.set_reference()
    assert np.allclose(ref.cpu().numpy(), 7.5, atol=1e-12)
    col = np.broadcast_to(np.arange(length, dtype=np.float64), (length, length))
    for t, want in ((1.0, 0.96799), (0.25, 0.25328)):
        phi = 2 * np.pi * t * col / (pad * npl)
        sl = sen.measure(dev(np.stack([phi, phi.T]), gpu)).cpu().numpy()
        nv = sen.nvalid
        assert np.allclose(sl[0, :nv], want, atol=5e-6) and np.abs(sl[0, nv:]).max() <= 1e-12, sl[0]
        assert np.allclose(sl[1, nv:], want, atol=5e-6) and np.abs(sl[1, :nv]).max() <= 1e-12, sl[1]
    sen.close()


def test_calibrate_and_estimate_at_128_16(pkg, gpu):
    length, npl, pad, s, h = 128, 16, 2, 16, 0.05
    A, Z = pupil(length, "disk"), modes(length)
    sen = pkg.ShackHartmann(A, npl)
    valid = sh.valid_mask(A, npl)
    assert sen.nvalid == 52
    sen.set_reference()
    D, sv, rank = sen.calibrate(Z, h=h)
    Dr = sh.interaction(A, Z, npl, pad, s, valid, h=h)
    err = float(np.abs(D - Dr).max())
    print("D against the reference: %.2e (bar %.2e), cond %.2f" % (err, sh.slope_bar(s) / h, sv[0] / sv[-1]))
    assert D.shape == (104, 27) and rank == 27 and sen.nmode == 27 and err <= sh.slope_bar(s) / h
    rng = np.random.default_rng(8)
    al = rng.standard_normal((3, 27))
    al /= np.linalg.norm(al, axis=1, keepdims=True)                                     # 1 rad, in the span
    phi = np.tensordot(al, Z, axes=1)
    cf = sen.coefficients(dev(phi, gpu)).cpu().numpy()
    ref0 = sh.slopes(sh.frame(A, np.zeros((length, length)), npl, pad, s, 1.0), valid, s)[0]
    Rr = np.linalg.pinv(Dr)
    for b in range(3):
        e_dev = np.linalg.norm(cf[b] - al[b])
        e_ref = np.linalg.norm(Rr @ sh.slopes(sh.frame(A, phi[b], npl, pad, s, 1.0), valid, s, ref=ref0)[0] - al[b])
        print("estimate at 1 rad: device %.3e reference %.3e" % (e_dev, e_ref))
        assert e_dev <= 2 * e_ref, (e_dev, e_ref)
    sen.close()


def test_noisy_path_composes(pkg, gpu):
    """measure(frame) -> detector_read -> slopes_from_frame against the reference's slopes of the device-drawn noisy frame."""
    length, npl, pad, s = 64, 16, 2, 16
    A = pupil(length, "disk")
    valid = sh.valid_mask(A, npl, MIN_LIGHT)
    worst, least = 0.0, 1.0
    for thr, arg in (((sh.NONE, 0.0, 0.0), None), ((sh.FLOOR, 2.0, 0.0), 2.0), ((sh.FRACTION, 1.0, 0.1), (1.0, 0.1))):
        sen = pkg.ShackHartmann(A, npl, min_light=MIN_LIGHT, threshold=arg, scale=40.0)       # some 1e4 photo-electrons per full lenslet
        fr = sen.measure(dev(screens(length, 3), gpu), want_frame=True, want_slopes=False)
        det = pkg.DetectorNoise(gain=1.0, photon_noise=True, read_noise=0.5, seed=11)
        noisy = pkg.detector_read(fr.view(3, -1), det, step=2)
        assert not torch.equal(noisy, fr.view(3, -1))
        sl, dk = sen.slopes_from_frame(noisy, want_dark=True)
        nf = rowmajor(noisy.view(3, sen.frame_len, sen.frame_len))
        for b in range(3):
            ws, wd = sh.slopes(nf[b], valid, s, thr)
            mf = sh.centroids(np.maximum(nf[b], 0.0), valid, s, thr)[3]
            least = min(least, float(mf[mf > 0].min()))
            worst = max(worst, float(np.abs(sl[b].cpu().numpy() - ws).max()))
            assert int(dk[b]) == wd
        sen.close()
    print("noisy path: slopes %.2e px, bar %.2e / %.3f" % (worst, sh.slope_bar(s), least))
    assert worst <= sh.slope_bar(s) / least, (worst, least)


def test_measure_records_into_a_graph(pkg, gpu):
    length, npl = 64, 16
    sen = pkg.ShackHartmann(pupil(length, "annulus"), npl, min_light=MIN_LIGHT, threshold=(0.0, 0.1))
    sen.set_reconstructor(np.random.default_rng(3).standard_normal((9, 2 * sen.nvalid)))
    phi = dev(np.swapaxes(screens(length, 3), -1, -2), gpu)                             # column-major already: no copy in the call
    out = dict(frame=torch.zeros((3, sen.frame_len, sen.frame_len), dtype=torch.float64, device=gpu),
               slopes=torch.zeros((3, 2 * sen.nvalid), dtype=torch.float64, device=gpu),
               coef=torch.zeros((3, 9), dtype=torch.float64, device=gpu), dark=torch.zeros(3, dtype=torch.int32, device=gpu))
    run = lambda: sen.measure(phi, colmajor=True, out=out)
    for _ in range(3):
        run()                                                                          # eager, also the warm-up
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in out) and bool(out["slopes"].any())
    sen.close()


def test_argument_errors_with_a_sensor(pkg, gpu):
    lib = pkg.load()
    sen = pkg.ShackHartmann(pupil(64, "disk"), 16)
    E_NULL, E_DIM, E_UNS = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM, pkg.FMPC_E_UNSUPPORTED
    x = torch.zeros(64 * 64, dtype=torch.float64, device=gpu)
    px = C.c_void_p(x.data_ptr())
    assert lib.fmpc_sh_measure_device(sen._h, 1, None, px, None, None, None, None) == E_NULL
    assert lib.fmpc_sh_measure_device(sen._h, 1, px, None, None, None, None, None) == E_NULL
    assert lib.fmpc_sh_measure_device(sen._h, -1, px, px, None, None, None, None) == E_DIM
    assert lib.fmpc_sh_measure_device(sen._h, 1, px, None, None, px, None, None) == E_UNS           # coef without a reconstructor
    assert lib.fmpc_sh_measure_device(sen._h, 0, px, px, None, None, None, None) == 0
    assert lib.fmpc_sh_slopes_device(sen._h, 1, None, 0, px, None, None, None) == E_NULL
    assert lib.fmpc_sh_slopes_device(sen._h, 1, px, 0, None, None, None, None) == E_NULL
    assert lib.fmpc_sh_slopes_device(sen._h, 1, px, 64 * 64 - 1, px, None, None, None) == E_DIM
    assert lib.fmpc_sh_slopes_device(sen._h, 1, px, -1, px, None, None, None) == E_DIM
    assert lib.fmpc_sh_slopes_device(sen._h, 1, px, 0, None, px, None, None) == E_UNS
    for bad in ((3, 0.0, 0.0), (-1, 0.0, 0.0), (1, -1.0, 0.0), (1, float("nan"), 0.0), (2, 0.0, -0.5), (2, 0.0, float("inf"))):
        assert lib.fmpc_sh_set_threshold(sen._h, *bad) == E_DIM, bad
    assert lib.fmpc_sh_set_reference_device(sen._h, None, float("nan"), None) == E_DIM
    assert lib.fmpc_sh_set_reconstructor_device(sen._h, 0, px, None) == E_DIM
    assert lib.fmpc_sh_set_reconstructor_device(sen._h, 129, px, None) == E_UNS
    dims = [C.c_int() for _ in range(7)]
    assert lib.fmpc_sh_dims(sen._h, *[C.byref(d) for d in dims]) == 0
    assert [d.value for d in dims] == [64, 4, 16, 2, 16, sen.nvalid, 0]
    sen.close()
