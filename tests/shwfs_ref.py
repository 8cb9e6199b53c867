"""numpy restatement of the Shack-Hartmann sensor (include/fastmpc.h: fmpc_sh_*), written from the formulas there: the spot as a
partial DFT (double or long double) and as OOMAO's literal sequence (val / nOut, half-pixel phasor, zero-padded FFT, crop about
centerIndex), the frame, the valid mask, the thresholds, the centre of gravity, the dark count, the interaction matrix D by
central differences and R = pinv(D).  Checker only.  Arrays are indexed [row, column]; a frame is (nL s, nL s) indexed
[row, column] (`colmajor` turns it into the array the device tensor is); lenslets are listed in the column-major order of the grid."""
import numpy as np

LD = np.longdouble
NONE, FLOOR, FRACTION = 0, 1, 2

# The rounding error of THIS restatement in double against itself in long double, on rough screens (tests/test_shwfs_ref.py
# measures and prints both and asserts them): a frame pixel within 5 ulp(1) of its lenslet's peak (1.0e-15 measured), a slope within
# 1.25 s ulp(1) pixels (a centroid is a number below s with a few roundings: 4.4e-16 at s = 2, 7.1e-15 at s = 32 measured).  The
# device sums in another order and has its own sincos, so its bars are 16 x these.
EPS = 2.0 ** -52
REF_FRAME_ERR = 5 * EPS


def ref_slope_err(s):
    return 1.25 * s * EPS


FRAME_BAR = 16 * REF_FRAME_ERR


def slope_bar(s):
    return 16 * ref_slope_err(s)


# the (npl, pad, s) at which the definition was checked against the literal sequence
SPOT_CASES = [(16, 2, 16), (16, 2, 32), (32, 1, 32), (16, 1, 8), (32, 2, 2), (16, 4, 6)]


def factors(npl, pad, s, dtype=np.float64):
    """F[x, a] = exp(-2 pi i x (a - (s - 1) / 2) / nOut) as (real, imaginary), the turn count reduced in integers."""
    nout = pad * npl
    n = np.outer(np.arange(npl), 2 * np.arange(s) - s + 1) % (2 * nout)              # x kappa_a = n / 2
    ang = -(np.arccos(dtype(-1)) * n.astype(dtype)) / dtype(nout)
    return np.cos(ang), np.sin(ang)


def field(amp, phi, dtype=np.float64):
    ph = np.where(amp != 0, phi, 0.0).astype(dtype)
    a = amp.astype(dtype)
    return a * np.cos(ph), a * np.sin(ph)


def spot(amp, phi, pad, s, scale, dtype=np.float64):
    """scale |F' E F|^2 / nOut^2 of one lenslet (amp, phi: npl x npl), indexed [row frequency, column frequency]."""
    npl = amp.shape[0]
    Fr, Fi = factors(npl, pad, s, dtype)
    Er, Ei = field(amp, phi, dtype)
    Tr, Ti = Er @ Fr - Ei @ Fi, Er @ Fi + Ei @ Fr
    Or, Oi = Fr.T @ Tr - Fi.T @ Ti, Fr.T @ Ti + Fi.T @ Tr
    return (Or * Or + Oi * Oi) * (dtype(scale) / dtype(pad * npl) ** 2)


def spot_fft(amp, phi, pad, s, scale):
    """lensletArray.propagateThrough, even branch: val ./ nOutWavePx, the phasor of setPhasor, fft to nOutWavePx, the crop
    (0 : nLensletImagePx - 1) + centerIndex - halfLength, then the intensity."""
    npl = amp.shape[0]
    nout = pad * npl
    Er, Ei = field(amp, phi)
    val = (Er + 1j * Ei) / nout
    u = np.arange(npl) * (1 - nout) / nout                                          # (~rem(npl, 2) - nOut) / nOut, npl even
    val = val * np.exp(-1j * np.pi * (u[:, None] + u[None, :]))
    W = np.fft.fft(np.fft.fft(val, nout, axis=0), nout, axis=1)
    if nout > s:
        k0 = (nout // 2 + 1) - s // 2 - 1                                           # centerIndex - halfLength, 0-based
        W = W[k0:k0 + s, k0:k0 + s]
    return scale * np.abs(W) ** 2


def lenslets(nL):
    """(i, j) of l = i + nL j, l = 0 .. nL^2 - 1."""
    return [(l % nL, l // nL) for l in range(nL * nL)]


def valid_mask(amp, npl, min_light=0.5):
    """(nL, nL) bool indexed [i, j]: mean(amplitude^2) over the lenslet >= min_light."""
    nL = amp.shape[0] // npl
    a2 = (amp.astype(LD) ** 2).reshape(nL, npl, nL, npl).sum(axis=(1, 3)) / LD(npl * npl)
    return a2.astype(np.float64) >= min_light


def valid_list(valid):
    """The lenslets l = i + nL j of the mask, in validLenslet(:)'s order."""
    return np.flatnonzero(valid.ravel(order="F"))


def frame(amp, phi, npl, pad, s, scale, dtype=np.float64):
    nL = amp.shape[0] // npl
    out = np.zeros((nL * s, nL * s), dtype=dtype)
    for i, j in lenslets(nL):
        a = amp[i * npl:(i + 1) * npl, j * npl:(j + 1) * npl]
        if (a > 0).any():
            out[i * s:(i + 1) * s, j * s:(j + 1) * s] = spot(a, phi[i * npl:(i + 1) * npl, j * npl:(j + 1) * npl], pad, s, scale, dtype)
    return out


def colmajor(fr):
    return np.ascontiguousarray(np.swapaxes(fr, -1, -2))


def centroids(fr, valid, s, threshold=(NONE, 0.0, 0.0), dtype=np.float64):
    """Raw centres of gravity of a frame [row, column]: (x (nvalid), y (nvalid), dark (nvalid) bool, mass fraction (nvalid): the
    light left after the threshold over the light before it)."""
    nL = valid.shape[0]
    mode, floor, frac = threshold
    xs, ys, dk, mf = [], [], [], []
    idx = np.arange(s).astype(dtype)
    for l in valid_list(valid):
        i, j = l % nL, l // nL
        b = fr[i * s:(i + 1) * s, j * s:(j + 1) * s].astype(dtype)
        tot = b.sum()
        if mode != NONE:
            t = dtype(floor) if mode == FLOOR else max(dtype(floor), dtype(frac) * b.max())
            b = np.maximum(b - t, 0)
        m = b.sum()
        if m > 0:
            xs.append((b.sum(axis=0) * idx).sum() / m); ys.append((b.sum(axis=1) * idx).sum() / m); dk.append(False)
        else:
            xs.append(dtype(0)); ys.append(dtype(0)); dk.append(True)
        mf.append(float(m / tot) if tot > 0 else 0.0)
    return np.array(xs, dtype=dtype), np.array(ys, dtype=dtype), np.array(dk), np.array(mf)


def slopes(fr, valid, s, threshold=(NONE, 0.0, 0.0), ref=None, units=1.0, dtype=np.float64):
    """([x; y] - ref) units with zeros for the dark lenslets, and the dark count."""
    x, y, dk, _ = centroids(fr, valid, s, threshold, dtype)
    v = np.concatenate([x, y])
    if ref is not None:
        v = v - np.asarray(ref).astype(dtype)
    v = v * dtype(units)
    v[np.concatenate([dk, dk])] = 0
    return v, int(dk.sum())


def measure(amp, phi, npl, pad, s, scale, valid, threshold=(NONE, 0.0, 0.0), ref=None, units=1.0, dtype=np.float64):
    fr = frame(amp, phi, npl, pad, s, scale, dtype)
    sl, dark = slopes(fr, valid, s, threshold, ref, units, dtype)
    return fr, sl, dark


def interaction(amp, Z, npl, pad, s, valid, h=0.05, threshold=(NONE, 0.0, 0.0)):
    """D (2 nvalid, nmode): central differences of the slopes over +- h Z_j."""
    cols = []
    for Zj in Z:
        p = slopes(frame(amp, h * Zj, npl, pad, s, 1.0), valid, s, threshold)[0]
        m = slopes(frame(amp, -h * Zj, npl, pad, s, 1.0), valid, s, threshold)[0]
        cols.append((p - m) / (2 * h))
    return np.stack(cols, axis=1)


def make_pupil(length, kind):
    """disk: the README's centred disk; offcentre: a smaller disk towards a corner (an asymmetric valid mask); annulus: the disk
    with a central obstruction and amplitude in [0.5, 1.5]; full: the whole square."""
    y, x = np.mgrid[0:length, 0:length] + 0.5 - length / 2
    if kind == "disk":
        return (np.hypot(x, y) <= length / 2 - 1).astype(np.float64)
    if kind == "offcentre":
        return (np.hypot(x + 0.11 * length, y - 0.07 * length) <= 0.33 * length).astype(np.float64)
    if kind == "annulus":
        r = np.hypot(x, y)
        return np.where((r <= length / 2 - 1) & (r > 0.14 * length), 0.5 + np.random.default_rng(11).random((length, length)), 0.0)
    if kind == "full":
        return np.ones((length, length))
    raise ValueError(kind)


def rough_screens(rng, Zm, batch, rough=1.0, amp=0.3):
    """amp randn(n) / sqrt(n) in the span of the modes Zm + `rough` rad of per-pixel roughness: every window carries light."""
    n0 = Zm.shape[0]
    al = amp * rng.standard_normal((batch, n0)) / np.sqrt(n0)
    return np.tensordot(al, Zm, axes=1) + rough * rng.standard_normal((batch,) + Zm.shape[1:])
