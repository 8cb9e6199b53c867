"""The atmosphere of include/fastmpc.h ("Atmosphere on the device") restated in numpy: covariance, extruders, start-up, the
displacement rule, extrusions and the output.  Windows are plain arrays [layer][r, y, x] that are shifted, not rings.

Operands come either from this file's own covariance (`extruders_own`: scipy's kv, a long double Cholesky) or from the library's
host builder (`extruders_lib`); the draws xi come from a callable, `xi_lib` wraps fmpc_noise_normal_host."""
import ctypes as C
import math

import numpy as np

LD = np.longdouble


def covariance(rho, r0, L0):
    """phaseStats.m:28-36 with a fraction of 1."""
    from scipy.special import gamma, kv
    rho = np.asarray(rho, dtype=np.float64)
    ratio = (L0 / r0) ** (5.0 / 3.0)
    lead = (24.0 * gamma(6.0 / 5.0) / 5.0) ** (5.0 / 6.0)
    cst = lead * (gamma(11.0 / 6.0) / (2.0 ** (5.0 / 6.0) * np.pi ** (8.0 / 3.0))) * ratio
    out = np.ones(rho.shape) * lead * (gamma(11.0 / 6.0) * gamma(5.0 / 6.0) / (2.0 * np.pi ** (8.0 / 3.0))) * ratio
    nz = rho != 0
    u = 2.0 * np.pi * rho[nz] / L0
    out[nz] = cst * u ** (5.0 / 6.0) * kv(5.0 / 6.0, u)
    return out


def variance(r0, L0):
    """phaseStats.m:13-15 with a fraction of 1."""
    from scipy.special import gamma
    return (24.0 * gamma(6.0 / 5.0) / 5.0) ** (5.0 / 6.0) * (gamma(11.0 / 6.0) * gamma(5.0 / 6.0) / (2.0 * np.pi ** (8.0 / 3.0))) * (L0 / r0) ** (5.0 / 3.0)


def structure_function(rho, r0, L0):
    """phaseStats.m:176-192: 2 (variance - covariance)."""
    return 2.0 * (variance(r0, L0) - covariance(rho, r0, L0))


def default_stencil(W):
    s = []
    while len(s) < 8 and (1 << len(s)) <= W - 1:
        s.append(1 << len(s))
    return s


def geometry_matrices(W, pitch, r0, L0, stencil, cov=covariance):
    """XX (W, W), ZX (q W, W), ZZ (q W, q W): the new line at (0, i p), the conditioning points (-s_j p, i p), j-major."""
    i = np.arange(W)
    di = i[:, None] - i[None, :]
    s = np.asarray(stencil, dtype=np.int64).reshape(-1)
    XX = cov(pitch * np.abs(di), r0, L0)
    q = s.size
    ZX = np.empty((q * W, W))
    ZZ = np.empty((q * W, q * W))
    for a in range(q):
        ZX[a * W:(a + 1) * W] = cov(pitch * np.hypot(s[a], di), r0, L0)
        for b in range(q):
            ZZ[a * W:(a + 1) * W, b * W:(b + 1) * W] = cov(pitch * np.hypot(s[a] - s[b], di), r0, L0)
    return XX, ZX, ZZ


def chol_lower_ld(M):
    """Lower Cholesky factor in long double (numpy's LAPACK has none); raises on a pivot that is not positive."""
    A = np.array(M, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for c in range(n):
        d = A[c, c] - np.dot(L[c, :c], L[c, :c])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[c, c] = np.sqrt(d)
        L[c + 1:, c] = (A[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return L


def extruder_own(W, pitch, r0, L0, stencil):
    """A = ZX' ZZ^-1 and B = chol_lower(XX - A ZX) in long double, rounded to double; an empty stencil gives (None, B_0)."""
    XX, ZX, ZZ = geometry_matrices(W, pitch, r0, L0, stencil)
    if len(stencil) == 0:
        return None, np.asarray(chol_lower_ld(XX), dtype=np.float64)
    L = chol_lower_ld(ZZ)
    n = L.shape[0]
    Y = np.zeros((n, W), dtype=LD)
    for r in range(n):                                     # L Y = ZX
        Y[r] = (ZX[r].astype(LD) - L[r, :r] @ Y[:r]) / L[r, r]
    At = np.zeros((n, W), dtype=LD)
    for r in range(n - 1, -1, -1):                         # L' A' = Y
        At[r] = (Y[r] - L[r + 1:, r] @ At[r + 1:]) / L[r, r]
    B = chol_lower_ld(XX.astype(LD) - Y.T @ Y)
    return np.asarray(At.T, dtype=np.float64), np.asarray(B, dtype=np.float64)


def extruders_own(W, pitch, r0, L0, stencil):
    """The extruders of every prefix of the stencil, j = 0 .. q."""
    return [extruder_own(W, pitch, r0, L0, list(stencil[:j])) for j in range(len(stencil) + 1)]


def extruder_lib(pkg, W, pitch, r0, L0, stencil):
    lib = pkg.load()
    q = len(stencil)
    A = np.empty((W, q * W)) if q else None
    B = np.empty((W, W))
    st = (C.c_int * max(q, 1))(*stencil)
    rc = lib.fmpc_atm_extruder_host(W, pitch, r0, L0, q, st, None if A is None else A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return A, B


def extruders_lib(pkg, W, pitch, r0, L0, stencil):
    return [extruder_lib(pkg, W, pitch, r0, L0, list(stencil[:j])) for j in range(len(stencil) + 1)]


def xi_lib(pkg, seed, batch, W, first=0):
    """xi(l, e) -> (batch, W): g(seed, (l << 48) | e, first + r, i) from the library's host draw."""
    lib = pkg.load()

    def xi(l, e):
        out = np.empty((batch, W))
        nz = pkg._lib.Noise(mode=0, value=1.0, sigma_dev=None, seed=seed, step=(l << 48) | e, step_dev=None, first=first)
        rc = lib.fmpc_noise_normal_host(out.ctypes.data_as(C.c_void_p), batch, W, W, C.byref(nz))
        assert rc == 0, rc
        return out
    return xi


def displacement(k, px_per_step):
    """(lines, fraction): floor(|k v|) and the rest, from k in double."""
    d = abs(float(k) * float(px_per_step))
    n = math.floor(d)
    return int(n), d - n


def pixels_per_step(speed, direction, dt, pitch):
    """speed cos(dir) dt / pitch and speed sin(dir) dt / pitch per layer, with the C library's cos and sin."""
    speed, direction = np.atleast_1d(np.asarray(speed, dtype=np.float64)), np.atleast_1d(np.asarray(direction, dtype=np.float64))
    vx = np.array([float(v) * math.cos(float(d)) * dt / pitch for v, d in zip(speed, direction)])
    vy = np.array([float(v) * math.sin(float(d)) * dt / pitch for v, d in zip(speed, direction)])
    return vx, vy


class AtmRef:
    """W, stencil, extruders [(A_j, B_j) for j = 0 .. q], frac, vpx, vpy (pixels per step, per layer), batch, xi(l, e).
    dtype: the arithmetic of the lines (float64 or longdouble); reverse: sum every product from the far end."""

    def __init__(self, W, stencil, extruders, frac, vpx, vpy, batch, xi, dtype=np.float64, reverse=False):
        self.W, self.s, self.ext = int(W), [int(v) for v in stencil], extruders
        self.sf = np.sqrt(np.asarray(frac, dtype=np.float64))
        self.vpx, self.vpy = np.asarray(vpx, dtype=np.float64).reshape(-1), np.asarray(vpy, dtype=np.float64).reshape(-1)
        self.layers, self.batch, self.xi, self.dtype, self.reverse = self.sf.size, int(batch), xi, dtype, reverse
        self.win = [np.zeros((self.batch, self.W, self.W), dtype=dtype) for _ in range(self.layers)]
        self.e = [0] * self.layers
        self.k = 0
        # the rounding bound of every sample that an extrusion since the latest clear_tol() made, 0 for the others:
        # (j + 1) W 2^-52 (sum |A||z| + sf sum |B||xi|); it moves with the window
        self.tol = [np.zeros((self.batch, self.W, self.W)) for _ in range(self.layers)]
        self._line_tol = None

    def _line(self, l, zs):
        """A_j z + sf B_j xi for the lines zs (each (batch, W)), newest side first; counts the extrusion."""
        j = len(zs)
        A, B = self.ext[j]
        xi = self.xi(l, self.e[l])
        self.e[l] += 1
        dt = self.dtype
        Bx, xx = np.asarray(B, dtype=dt), np.asarray(xi, dtype=dt)
        if self.reverse:
            Bx, xx = Bx[:, ::-1], xx[:, ::-1]
        line = dt(self.sf[l]) * (xx @ Bx.T)
        z = None
        if j:
            Az, z = np.asarray(A, dtype=dt), np.concatenate(zs, axis=1).astype(dt)
            line = (z[:, ::-1] @ Az[:, ::-1].T if self.reverse else z @ Az.T) + line
        t = self.sf[l] * (np.abs(np.asarray(xi, dtype=np.float64)) @ np.abs(B).T)
        if j:
            t = t + np.abs(np.asarray(z, dtype=np.float64)) @ np.abs(A).T
        self._line_tol = (j + 1) * self.W * 2.0 ** -52 * t
        return line

    def reset(self):
        W = self.W
        for l in range(self.layers):
            self.e[l] = 0
            w = np.zeros((self.batch, W, W), dtype=self.dtype)
            for t in range(W):
                w[:, :, t] = self._line(l, [w[:, :, t - s] for s in self.s if s <= t])
                self.tol[l][:, :, t] = self._line_tol
            self.win[l] = w
        self.k = 0
        return self

    def extrude(self, l, axis, side):
        """One line of layer l along axis 0 (x: a new column) or 1 (y: a new row); side +1: it enters at index 0, -1: at W - 1."""
        W = self.W
        w = self.win[l] if axis == 0 else self.win[l].transpose(0, 2, 1)          # [r, entry, line index]
        zs = [w[:, :, s - 1] if side > 0 else w[:, :, W - s] for s in self.s]
        line = self._line(l, zs)
        w = np.concatenate([line[:, :, None], w[:, :, :-1]] if side > 0 else [w[:, :, 1:], line[:, :, None]], axis=2)
        self.win[l] = np.ascontiguousarray(w if axis == 0 else w.transpose(0, 2, 1))
        t = self.tol[l] if axis == 0 else self.tol[l].transpose(0, 2, 1)
        lt = self._line_tol[:, :, None]
        t = np.concatenate([lt, t[:, :, :-1]] if side > 0 else [t[:, :, 1:], lt], axis=2)
        self.tol[l] = np.ascontiguousarray(t if axis == 0 else t.transpose(0, 2, 1))

    def clear_tol(self):
        for t in self.tol:
            t[...] = 0.0

    def advance(self, steps=1):
        for _ in range(steps):
            for l in range(self.layers):
                for axis, v in ((0, self.vpx[l]), (1, self.vpy[l])):
                    n = displacement(self.k + 1, v)[0] - displacement(self.k, v)[0]
                    for _ in range(n):
                        self.extrude(l, axis, 1 if v > 0 else -1)
            self.k += 1
        return self

    def coords(self, out_len, v):
        """Lattice index below and weight above of every output index of an axis, for a wind component v."""
        f = displacement(self.k, v)[1]
        s = 1.0 - f if v > 0 else f
        h = float(self.W - 2) / float(out_len - 1)
        c = np.arange(out_len, dtype=np.float64) * h + s                          # two roundings, as the kernel's
        i0 = np.minimum(np.floor(c), self.W - 2)
        return i0.astype(np.int64), c - i0

    def screen(self, out_len, mask=None, scale=1.0, want_abs=False):
        """(batch, out_len, out_len); with want_abs also sum_l of the |four samples| of every pixel and the sum before the mean."""
        dt = self.dtype
        S = np.zeros((self.batch, out_len, out_len), dtype=dt)
        absum = np.zeros((self.batch, out_len, out_len))
        for l in range(self.layers):
            y0, wy = self.coords(out_len, self.vpy[l])
            x0, wx = self.coords(out_len, self.vpx[l])
            w = self.win[l]
            a00, a01 = w[:, y0][:, :, x0], w[:, y0][:, :, x0 + 1]
            a10, a11 = w[:, y0 + 1][:, :, x0], w[:, y0 + 1][:, :, x0 + 1]
            wy_, wx_ = wy.astype(dt)[None, :, None], wx.astype(dt)[None, None, :]
            S = S + ((1 - wy_) * ((1 - wx_) * a00 + wx_ * a01) + wy_ * ((1 - wx_) * a10 + wx_ * a11))
            absum += np.abs(a00) + np.abs(a01) + np.abs(a10) + np.abs(a11)
        if mask is None:
            out = dt(scale) * S
        else:
            m = np.asarray(mask, dtype=dt)
            cnt = m.sum()
            mu = (S * m).sum(axis=(1, 2)) / cnt if cnt > 0 else np.zeros(self.batch, dtype=dt)
            out = dt(scale) * (m * (S - mu[:, None, None]))
        return (out, absum, S) if want_abs else out

    def state(self):
        return dict(windows=np.stack([np.asarray(w, dtype=np.float64) for w in self.win]), k=self.k, counts=list(self.e))

    def load_state(self, st):
        self.win = [np.array(w, dtype=self.dtype) for w in st["windows"]]
        self.k, self.e = int(st["k"]), [int(v) for v in st["counts"]]
        return self
