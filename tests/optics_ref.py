"""numpy restatement of the estimator's optics, written for the tests: zernfun.m's formula (power sums with the factorial
quotients, r**p) in zernmodfit.m:195-198's mode order, the README's geometry (README.md:366-396) and the analytic linearisation

    I_k = ft(pupil .* exp(1i*(phi0 + zd_k*W)))  (window only) ;  b_s = AU |I_k|^2 ;
    A_s(:, j) = 2 AU Re(conj(I_k) .* ft(1i*Z_j .* pupil .* exp(1i*(phi0 + zd_k*W))))

through np.fft.  tests/test_optics_ref_golden.py pins it to the reference's own model_approx.mat.  Checker only.
Arrays are indexed [row, column]."""
from math import factorial

import numpy as np


def zernike_modes(N):
    """zernmodfit.m:195-198: n = 0..N, m = -n:2:n."""
    n = [nn for nn in range(N + 1) for _ in range(nn + 1)]
    m = [mm for nn in range(N + 1) for mm in range(-nn, nn + 1, 2)]
    return np.array(n), np.array(m)


def radial_terms(n, ma):
    """zernfun.m:163-170: [(p_s, power n - 2 s)], s = 0 .. (n - |m|) / 2; exact integers."""
    out = []
    for s in range((n - ma) // 2 + 1):
        p = (1 - 2 * (s % 2)) * factorial(n - s) // factorial(s) // factorial((n - ma) // 2 - s) // factorial((n + ma) // 2 - s)
        out.append((float(p), n - 2 * s))
    return out


def zernfun(n, m, r, theta, normalized=False):
    """Returns (Z, S): Z[j] = zernfun(n_j, m_j, r, theta), S[j] = sum_s |p_s| r^pow_s (times the normalisation), the scale of
    the rounding error of any evaluation of the radial polynomial."""
    r = np.asarray(r, dtype=np.float64); theta = np.asarray(theta, dtype=np.float64)
    Z = np.zeros((len(n),) + r.shape); S = np.zeros_like(Z)
    for j, (nj, mj) in enumerate(zip(n, m)):
        nj, mj = int(nj), int(mj)
        ma = abs(mj)
        for p, pw in reversed(radial_terms(nj, ma)):            # zernfun.m:165: k = length(s):-1:1
            t = p * r ** pw
            Z[j] += t; S[j] += np.abs(t)
        if normalized:
            nf = np.sqrt((1 + (mj != 0)) * (nj + 1) / np.pi)
            Z[j] *= nf; S[j] *= nf
        if mj > 0:
            Z[j] *= np.cos(theta * ma)
        elif mj < 0:
            Z[j] *= np.sin(theta * ma)
    return Z, S


def grid_coords(length):
    """x = (-N:2:N)/N, N = length - 1; pixel [row y, column x] has X = x[x], Y = x[y]."""
    N = length - 1
    ax = np.arange(-N, N + 1, 2) / N
    X, Y = np.meshgrid(ax, ax)
    return np.hypot(X, Y), np.arctan2(Y, X)


def zernike_grid(N, length, normalized=False):
    """(nmode, length, length) indexed [j, row, column]; zero where r > 1."""
    n, m = zernike_modes(N)
    r, th = grid_coords(length)
    inside = r <= 1.0
    Z = np.zeros((len(n), length, length))
    Z[:, inside] = zernfun(n, m, r[inside], th[inside], normalized)[0]
    return Z


def readme_geometry(length=512, dx=6.5e-6, zd_dist=3.0, AU=1e12):
    """README.md:366-396: pupil, zd_list, the window as 0-based inclusive (rmin, rmax)."""
    df = 1.0 / (length * dx)
    fx = np.arange(-length // 2, length // 2) * df
    FX, FY = np.meshgrid(fx, -fx)
    pupil = (np.sqrt(FX ** 2 + FY ** 2) <= (length / 2 - 1) * df).astype(np.float64)
    xaxis = np.arange(-length // 2, length // 2) * dx
    rmin = int(np.nonzero(np.abs(xaxis + 1.0e-4) < 3e-6)[0][0]); rmax = int(np.nonzero(np.abs(xaxis - 1.0e-4) < 3e-6)[0][-1])
    return dict(len=length, dx=dx, AU=AU, pupil=pupil, zd_list=np.array([-zd_dist, 0.0, zd_dist]), rmin=rmin, rmax=rmax)


def model(pupil, W, zd_list, dx, rmin, rmax, Z, AU=1e12, phi0=None):
    """A_s (ndiv d^2, nmode), b_s (ndiv d^2): rows per diversity, the window column-major (README.md:471).  The window is
    rows / columns rmin..rmax (0-based, inclusive) of the centred transform."""
    d = rmax - rmin + 1
    nd, nm = len(zd_list), len(Z)
    ft = lambda P_: (np.fft.fftshift(np.fft.fft2(np.fft.fftshift(P_))) * dx ** 2)[rmin:rmax + 1, rmin:rmax + 1]
    b_s = np.zeros(nd * d * d); A_s = np.zeros((nd * d * d, nm))
    E = 1.0 if phi0 is None else np.exp(1j * np.asarray(phi0))
    for k, zd in enumerate(zd_list):
        P0 = pupil * np.exp(1j * zd * W) * E
        I0 = ft(P0)
        b_s[k * d * d:(k + 1) * d * d] = (np.abs(I0) ** 2 * AU).reshape(-1, order="F")
        for j in range(nm):
            A_s[k * d * d:(k + 1) * d * d, j] = (2.0 * AU * np.real(np.conj(I0) * ft(1j * Z[j] * P0))).reshape(-1, order="F")
    return A_s, b_s
