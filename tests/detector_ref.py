"""numpy restatement of the detector's photon and read-out noise from the text of include/fastmpc.h (fmpc_detector) and
csrc/fmpc_detector.h: the Poisson deviate K(seed, step, R, i; lam) -- inversion below lam = 10, Hoermann's PTRS from there on,
with its own exp and ln built from +, -, x, /, sqrt and bit operations in the header's order -- and the read-out model on top of
it.  The Philox generator and the normal draw are those of tests/noise_ref.py.  Everything is vectorised; every operation is an
IEEE double operation rounded once, so the result equals the library's bit for bit."""
import numpy as np

from tests import noise_ref as nr

SWITCH = 10.0
LAM_MAX = 2.0 ** 31
INV_CAP, PTRS_CAP = 128, 64
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
LNFACT = np.array([0.0, 0.0, 0.6931471805599453, 1.791759469228055, 3.1780538303479458, 4.787491742782046, 6.579251212010101,
                   8.525161361065415, 10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887,
                   19.987214495661885, 22.552163853123425, 25.19122118273868, 27.89927138384089])


def det_exp(x):
    """e^x on [-10.5, 0.5]: n = floor(x / ln 2 + 1/2), r = x - n ln2_hi - n ln2_lo, Taylor to degree 13 (Horner), times 2^n."""
    x = np.asarray(x, dtype=np.float64)
    n = np.floor(x * 1.4426950408889634 + 0.5)
    r = (x - n * LN2_HI) - n * LN2_LO
    q = 1.0 + r * (1.0 / 13.0)
    for k in (12.0, 11.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0):
        q = 1.0 + (r * (1.0 / k)) * q
    q = 1.0 + (r * 0.5) * q
    q = 1.0 + r * q
    two_n = ((np.int64(1023) + n.astype(np.int64)).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return q * two_n


def det_ln(x):
    """ln x for positive normal doubles: x = 2^e m, m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), 2 s (1 + s^2/3 + .. + s^22/23)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    bits = x.view(np.uint64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m >= 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    q = np.full_like(z, 1.0 / 23.0)
    for k in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = 1.0 / k + z * q
    s2 = 2.0 * s
    lm = s2 + s2 * (z * q)
    ed = e.astype(np.float64)
    return ed * LN2_HI + (ed * LN2_LO + lm)


def det_lnfact(k):
    """ln k!: the table below 16, Stirling's series to 1/k^7 from there on."""
    k = np.asarray(k, dtype=np.float64)
    small = k < 16.0
    kk = np.where(small, 16.0, k)
    r = 1.0 / kk
    r2 = r * r
    ser = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))))
    big = (((kk + 0.5) * det_ln(kk) - kk) + 0.9189385332046727) + ser
    return np.where(small, LNFACT[np.where(small, k, 0.0).astype(np.int64)], big)


def det_uniforms(seed, step, R, i, attempt):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    R, i = np.asarray(R, dtype=np.uint64), np.asarray(i, dtype=np.uint64)
    w0 = i | np.uint64((attempt + 1) << 24)
    return nr.uniforms(nr.philox4x32_10((w0, R, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32)))


def poisson(seed, step, R, i, lam):
    """K(seed, step, R, i; lam) for 0 <= lam <= 2^31; R, i, lam broadcast against each other."""
    R, i, lam = np.broadcast_arrays(np.asarray(R, dtype=np.uint64), np.asarray(i, dtype=np.uint64), np.asarray(lam, dtype=np.float64))
    shape = lam.shape
    R, i, lam = R.ravel(), i.ravel(), lam.ravel().copy()
    out = np.full(lam.shape, np.nan)
    with np.errstate(all="ignore"):
        # ---- inversion
        lo = np.flatnonzero(lam < SWITCH)
        if lo.size:
            l = lam[lo]
            u1, _ = det_uniforms(seed, step, R[lo], i[lo], 0)
            k = np.zeros(lo.size)
            t = det_exp(-l)
            s = t.copy()
            live = u1 > s
            for _ in range(INV_CAP):
                if not live.any():
                    break
                k = np.where(live, k + 1.0, k)
                t = np.where(live, t * l / np.where(live, k, 1.0), t)
                s = np.where(live, s + t, s)
                live = live & ~(t < 5.421010862427522e-20) & (u1 > s)
            out[lo] = k
        # ---- PTRS
        hi = np.flatnonzero(lam >= SWITCH)
        if hi.size:
            l = lam[hi]
            slam = np.sqrt(l)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            inva = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            lnlam, lninva = det_ln(l), det_ln(inva)
            res = np.floor(l + 0.5)                           # (the value at the cap)
            todo = np.ones(hi.size, dtype=bool)
            for at in range(PTRS_CAP):
                if not todo.any():
                    break
                u1, u2 = det_uniforms(seed, step, R[hi], i[hi], at)
                U = u1 - 0.5
                us = 0.5 - np.where(U < 0.0, -U, U)
                k = np.floor((2.0 * a / us + b) * U + l + 0.43)
                quick = (us >= 0.07) & (u2 <= vr)
                rejected = ~quick & ((k < 0.0) | ((us < 0.013) & (u2 > us)))
                ks = np.where(quick | rejected, 16.0, k)      # (the slow test only where it is taken)
                lhs = (det_ln(u2) + lninva) - det_ln(a / (us * us) + b)
                rhs = (ks * lnlam - l) - det_lnfact(ks)
                acc = todo & (quick | (~rejected & (lhs <= rhs)))
                res = np.where(acc, k, res)
                todo = todo & ~acc
            out[hi] = res
    return out.reshape(shape)


def read(Y0, gain=1.0, qe=1.0, background=0.0, read_noise=0.0, photon_noise=True, seed=0, step=0, first=0, normal=None):
    """The model on a (batch, p) array: gain a float or (batch,).  normal: (batch, p) values of g to use in place of
    noise_ref.normal (the library's own, where two libms must not be told apart)."""
    Y0 = np.asarray(Y0, dtype=np.float64)
    batch, p = Y0.shape
    gain = np.broadcast_to(np.asarray(gain, dtype=np.float64).reshape(-1, 1), (batch, 1))
    R, i = first + np.arange(batch)[:, None], np.arange(p)[None, :]
    with np.errstate(all="ignore"):
        lam = gain * Y0 + background
        ok = (lam >= 0.0) & (lam <= LAM_MAX)
        N = poisson(seed, step, R, i, np.where(ok, lam, 0.0)) if photon_noise else lam
        e = qe * (N - background)
        if read_noise != 0.0:
            g = nr.normal(seed, step, R, i) if normal is None else normal
            e = e + read_noise * g
        return np.where(ok, e / gain, np.nan)
