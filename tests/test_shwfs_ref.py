"""The numpy restatement of the Shack-Hartmann sensor (tests/shwfs_ref.py) against what it restates: the partial-DFT spot
against OOMAO's literal FFT-phasor-crop sequence, its own rounding error against long double (the basis of the device bars), the
orientation of the slopes, the order of the valid list, and a modal reconstruction at (len, npl) = (128, 16)."""
import functools

import numpy as np
import pytest

from tests import optics_ref as orf
from tests import shwfs_ref as sh


@functools.lru_cache(maxsize=None)
def modes(length):
    Z = orf.zernike_grid(6, length)[1:]                                              # 27 modes, piston dropped
    Z.setflags(write=False)
    return Z


@pytest.mark.parametrize("npl,pad,s", sh.SPOT_CASES)
def test_partial_dft_is_the_literal_fft_phasor_crop(npl, pad, s):
    rng = np.random.default_rng(100 * npl + 10 * pad + s)
    amp, phi = 0.5 + rng.random((npl, npl)), rng.standard_normal((npl, npl))
    amp[0, :3] = 0.0
    a, b = sh.spot(amp, phi, pad, s, 1.3), sh.spot_fft(amp, phi, pad, s, 1.3)
    err = float(np.abs(a - b).max() / a.max())
    print("spot against fft", (npl, pad, s), "%.2e of the peak" % err)
    assert a.shape == (s, s) and err <= 1e-14, err


@pytest.mark.parametrize("npl,pad,s", sh.SPOT_CASES)
def test_rounding_error_of_the_double_reference(npl, pad, s):
    """Frame (relative to each lenslet's peak) and slopes (pixels) in double against long double, every threshold mode."""
    length = 4 * npl
    A = sh.make_pupil(length, "annulus")
    valid = sh.valid_mask(A, npl, 0.5)
    nL = length // npl
    phi = sh.rough_screens(np.random.default_rng(3), modes(length), 3)
    ef = es = 0.0
    for p in phi:
        f64, fld = sh.frame(A, p, npl, pad, s, 1.0), sh.frame(A, p, npl, pad, s, 1.0, sh.LD)
        pk = f64.reshape(nL, s, nL, s).max(axis=(1, 3))
        err = np.abs(f64 - fld.astype(np.float64)).reshape(nL, s, nL, s).max(axis=(1, 3)) / np.where(pk > 0, pk, 1.0)
        ef = max(ef, float(err.max()))
        for thr in ((sh.NONE, 0.0, 0.0), (sh.FLOOR, 0.02 * f64.max(), 0.0), (sh.FRACTION, 0.0, 0.3)):
            s64, d64 = sh.slopes(f64, valid, s, thr)
            sld, dld = sh.slopes(fld, valid, s, thr, dtype=sh.LD)
            assert d64 == dld
            es = max(es, float(np.abs(s64 - sld.astype(np.float64)).max()))
    print("double against long double", (npl, pad, s), "frame %.2e (pinned %.2e)  slopes %.2e px (pinned %.2e)" % (ef, sh.REF_FRAME_ERR, es, sh.ref_slope_err(s)))
    assert ef <= sh.REF_FRAME_ERR and es <= sh.ref_slope_err(s), (ef, es)


def tilt_slopes(t, transpose=False):
    npl, pad, s, length = 16, 2, 16, 64
    A = sh.make_pupil(length, "full")
    valid = sh.valid_mask(A, npl)
    col = np.broadcast_to(np.arange(length, dtype=np.float64), (length, length))
    phi = 2 * np.pi * t * col / (pad * npl)
    ref = sh.slopes(sh.frame(A, np.zeros((length, length)), npl, pad, s, 1.0), valid, s)[0]
    return sh.slopes(sh.frame(A, phi.T if transpose else phi, npl, pad, s, 1.0), valid, s, ref=ref)[0], int(valid.sum()), ref


def test_orientation_of_the_slopes():
    sl, nv, ref = tilt_slopes(1.0)
    assert nv == 16 and np.allclose(ref, 7.5, atol=1e-13)                            # a flat wavefront: centred between pixels
    assert np.allclose(sl[:nv], 0.96799, atol=5e-6) and np.abs(sl[nv:]).max() <= 1e-13, sl
    sl, nv, _ = tilt_slopes(1.0, transpose=True)
    assert np.allclose(sl[nv:], 0.96799, atol=5e-6) and np.abs(sl[:nv]).max() <= 1e-13, sl
    sl, nv, _ = tilt_slopes(0.25)
    assert np.allclose(sl[:nv], 0.25328, atol=5e-6) and np.abs(sl[nv:]).max() <= 1e-13, sl


def test_valid_list_of_an_off_centre_disk_is_column_major():
    A = sh.make_pupil(128, "offcentre")
    v = sh.valid_mask(A, 16)
    assert not np.array_equal(v, v.T) and not np.array_equal(v, v[::-1]) and not np.array_equal(v, v[:, ::-1])
    lst = sh.valid_list(v)
    want = [i + 8 * j for j in range(8) for i in range(8) if v[i, j]]                # validLenslet(:): i fastest
    assert lst.tolist() == want and len(want) == int(v.sum()) and 0 < len(want) < 64
    # the mask is the mean of amplitude^2, not of amplitude
    B = 0.7 * np.ones((32, 32))
    assert sh.valid_mask(B, 16, 0.5).sum() == 0 and sh.valid_mask(B, 16, 0.48).sum() == 4


def test_reconstruction_at_128_16():
    length, npl, pad, s = 128, 16, 2, 16
    A, Z = sh.make_pupil(length, "disk"), modes(length)
    valid = sh.valid_mask(A, npl)
    assert int(valid.sum()) == 52
    ref = sh.slopes(sh.frame(A, np.zeros((length, length)), npl, pad, s, 1.0), valid, s)[0]
    D = sh.interaction(A, Z, npl, pad, s, valid)
    sv = np.linalg.svd(D, compute_uv=False)
    print("cond(D) %.2f" % (sv[0] / sv[-1]))
    assert D.shape == (104, 27) and sv[0] / sv[-1] < 10
    R = np.linalg.pinv(D)
    rng = np.random.default_rng(8)
    al = rng.standard_normal(27)
    al *= 0.3 / np.linalg.norm(al)
    sl = sh.slopes(sh.frame(A, np.tensordot(al, Z, axes=1), npl, pad, s, 1.0), valid, s, ref=ref)[0]
    err = float(np.linalg.norm(R @ sl - al) / np.linalg.norm(al))
    print("modal estimate at 0.3 rad: %.2e" % err)
    assert err < 0.01, err
