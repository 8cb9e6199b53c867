"""numpy restatement of the science camera (include/fastmpc.h: fmpc_sci_*): the image by the centred-padded FFT (integer
sampling) and by the long-double partial DFT (any sampling), the quality fields by long-double two-pass sums, the summary.
Arrays are indexed [row, column] / [u, v]; `colmajor` turns an image into the (d, d) array the device tensor is ([v, u])."""
import numpy as np

LD = np.longdouble
FIELDS = 6
MEAN, RMS, STREHL, MARECHAL, MIN, MAX = range(6)


def image_fft(pupil, phi, d, s, scale):
    """Integer s: the window around the centre of the DFT of the pupil field zero-padded ABOUT ITS CENTRE to s len."""
    length = pupil.shape[0]
    s = int(s)
    N = s * length
    P = pupil * np.exp(1j * np.where(pupil != 0, phi, 0.0))
    big = np.zeros((N, N), dtype=complex)
    o = N // 2 - length // 2
    big[o:o + length, o:o + length] = P
    I = np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(big)))
    c = N // 2
    return scale * np.abs(I[c - d // 2:c + d // 2, c - d // 2:c + d // 2]) ** 2


def dft_table(length, d, s):
    """F[y, j] = exp(-2 pi i (j - d/2)(y - len/2) / (s len)) in long double, the turn count reduced first."""
    n = np.outer(np.arange(length) - length // 2, np.arange(d) - d // 2).astype(LD)
    turn = n / (LD(s) * LD(length))
    turn = turn - np.rint(turn)
    ang = -(LD(2) * np.arccos(LD(-1))) * turn
    return np.cos(ang), np.sin(ang)


def image_dft(pupil, phi, d, s, scale):
    """Any s >= 1: I = F' P F in long double."""
    Fr, Fi = dft_table(pupil.shape[0], d, s)
    ph = np.where(pupil != 0, phi, 0.0).astype(LD)
    Pr, Pi = pupil.astype(LD) * np.cos(ph), pupil.astype(LD) * np.sin(ph)
    # T = P F
    Tr, Ti = Pr @ Fr - Pi @ Fi, Pr @ Fi + Pi @ Fr
    Or, Oi = Fr.T @ Tr - Fi.T @ Ti, Fr.T @ Ti + Fi.T @ Tr
    return (LD(scale) * (Or * Or + Oi * Oi)).astype(np.float64)


def quality(pupil, phi):
    """The six fields in long double, two passes."""
    m = pupil != 0
    a = pupil[m].astype(LD); p = phi[m].astype(LD)
    W = a.sum()
    mu = (a * p).sum() / W
    var = (a * (p - mu) ** 2).sum() / W
    S = ((a * np.cos(p)).sum() ** 2 + (a * np.sin(p)).sum() ** 2) / W ** 2
    return np.array([mu, np.sqrt(var), S, np.exp(-var), p.min(), p.max()], dtype=LD)


def sums(pupil, scale):
    a = pupil.astype(LD)
    return float(a.sum()), float((a * a).sum()), float(LD(scale) * a.sum() ** 2)


def summary(image, frames, nrad, pupil, s, scale):
    """image: (d, d) indexed [u, v].  Returns 2 + nrad values."""
    d = image.shape[0]
    sa, sa2, I0 = sums(pupil, scale)
    den = LD(frames) * LD(scale) * (LD(s) * pupil.shape[0]) ** 2 * LD(sa2)
    u = np.arange(d) - d // 2
    r2 = u[:, None] ** 2 + u[None, :] ** 2
    out = [LD(image[d // 2, d // 2]) / (LD(frames) * LD(I0)), image.astype(LD).sum() / den]
    for rho in range(nrad):
        out.append(image.astype(LD)[r2 <= rho * rho].sum() / den)
    return np.array(out, dtype=np.float64)


def colmajor(image):
    return np.ascontiguousarray(image.T)


def qranges(pupil):
    """Per row block of 16: [first, last + 1) of the k-steps (4 columns) with a pixel A != 0; (0, 0) for an empty block."""
    length = pupil.shape[0]
    qr = np.zeros((length // 16, 2), dtype=np.int32)
    for b in range(length // 16):
        cols = np.nonzero((pupil[16 * b:16 * b + 16] != 0).any(axis=0))[0]
        if cols.size:
            qr[b] = (cols[0] // 4, cols[-1] // 4 + 1)
    return qr


def make_pupil(length, rng=None):
    """A pupil that exercises the skipping: an annulus with the obstruction off centre, amplitude in [0.5, 1.5], rows
    [0, 16) and the leading columns empty."""
    rng = np.random.default_rng(5) if rng is None else rng
    y, x = np.mgrid[0:length, 0:length]
    cy, cx = length * 0.56, length * 0.58
    R = length * 0.38
    m = ((y - cy) ** 2 + (x - cx) ** 2 <= R * R) & ((y - cy - 0.1 * R) ** 2 + (x - cx + 0.15 * R) ** 2 > (0.3 * R) ** 2)
    m &= (y >= 16) & (x >= length // 8)
    return np.where(m, 0.5 + rng.random((length, length)), 0.0)


def make_screens(length, batch, rng, noise=0.5):
    y, x = np.mgrid[0:length, 0:length] / float(length) - 0.5
    out = np.empty((batch, length, length))
    for b in range(batch):
        c = rng.standard_normal(5)
        out[b] = noise * rng.standard_normal((length, length)) + c[0] + 3 * c[1] * x + 3 * c[2] * y + 4 * c[3] * (x * x + y * y) + 2 * c[4] * x * y
    return out

