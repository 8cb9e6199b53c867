"""tests/science_ref.py against itself and against the reference's own model: the centred-padded FFT and the long-double partial
DFT are the same image, and at the README geometry (pin-hole pupil, dx = 6.5e-6, AU = 1e12, len 512, d = 32, s = 1, a zero screen)
psf[1:, 1:] is the zero-diversity block of the reference's b_s (tests/golden/model_approx_As_bs.npz, entries 961:1922 reshaped
31 x 31 column-major).  Measured: 6e-16 between the two forms, 3e-17 against b_s.  Asserted: 1e-12, the bar of
tests/test_optics_ref_golden.py (round-off of two FFT implementations with three orders of margin; a wrong centre, sign,
orientation or padding gives O(1): padding after the shift, the reference's literal fft2(fftshift(P), res, res), is 0.52 off)."""
import os

import numpy as np
import pytest

from tests import optics_ref as oref
from tests import science_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "model_approx_As_bs.npz")
TOL = 1e-12


@pytest.mark.parametrize("length,d,s", [(64, 16, 1), (64, 64, 1), (128, 32, 2), (192, 48, 3)])
def test_fft_and_partial_dft_are_the_same_image(length, d, s):
    rng = np.random.default_rng(length + d)
    A = sr.make_pupil(length, rng)
    phi = sr.make_screens(length, 1, rng)[0]
    a = sr.image_fft(A, phi, d, s, 0.37)
    b = sr.image_dft(A, phi, d, s, 0.37)
    err = np.linalg.norm(a - b) / np.linalg.norm(b)
    print("fft vs partial dft", length, d, s, err)
    assert err <= TOL, err


def test_padding_after_the_shift_is_another_image():
    """What the header warns of: fft2(fftshift(P), res, res) with res = 2 len is not the sampled PSF."""
    length, d = 64, 32
    A = sr.make_pupil(length)
    P = A.astype(complex)
    I = np.fft.fftshift(np.fft.fft2(np.fft.fftshift(P), (2 * length, 2 * length)))
    lit = np.abs(I[length - d // 2:length + d // 2, length - d // 2:length + d // 2]) ** 2
    ref = sr.image_dft(A, np.zeros_like(A), d, 2, 1.0)
    assert np.linalg.norm(lit - ref) > 0.1 * np.linalg.norm(ref)


def test_reference_geometry_reproduces_the_b_s_block():
    g = oref.readme_geometry(512)
    scale = g["dx"] ** 4 * g["AU"]
    b = np.load(FIX)["b_s"].reshape(-1)[961:1922].reshape(31, 31, order="F")
    for img in (sr.image_fft(g["pupil"], np.zeros((512, 512)), 32, 1, scale), sr.image_dft(g["pupil"], np.zeros((512, 512)), 32, 1, scale)):
        err = np.linalg.norm(img[1:, 1:] - b) / np.linalg.norm(b)
        print("b_s block", err)
        assert err <= TOL, err
        assert abs(img[16, 16] - sr.sums(g["pupil"], scale)[2]) <= 1e-13 * img[16, 16]


def test_quality_and_summary_identities():
    """1 - S = sigma^2 + O(sigma^4) with amplitude weights; the whole DFT plane holds all the energy (Parseval)."""
    rng = np.random.default_rng(3)
    A = sr.make_pupil(64, rng)
    phi = 0.01 * rng.standard_normal((64, 64))
    q = sr.quality(A, phi)
    assert abs(float((1 - q[sr.STREHL]) / q[sr.RMS] ** 2) - 1) <= 1e-3
    img = sr.image_dft(A, phi, 64, 1, 2.5)
    out = sr.summary(img, 1, 32, A, 1, 2.5)
    assert abs(out[1] - 1) <= 1e-13 and abs(out[0] - float(q[sr.STREHL])) <= 1e-12
    assert np.all(np.diff(out[2:]) >= 0) and out[2] == pytest.approx(out[0] * sr.sums(A, 2.5)[2] / (2.5 * 64 ** 2 * sr.sums(A, 2.5)[1]), rel=1e-12)
