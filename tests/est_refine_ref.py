"""numpy restatement of the estimator's Gauss-Newton refinement (fmpc_est_refine_device), written for the tests, on top of
tests/optics_ref.model: per realisation, with phi = sum_j alpha_j Z_j and (J, y) = model(.., phi0 = phi),

    r = Y - y ;  H = J'J, H_ii <- H_ii (1 + damping) ;  g = J'r ;  delta = H \\ g (Cholesky) ;  alpha <- alpha + delta

and the same freeze rules: a cost ||r||^2 that is not finite (a pixel of phi with |phi| >= 1e6 or not finite, a NaN in Y) sets
BAD_INPUT, makes the row NaN and stops it; a pivot of the Cholesky factor that is not positive and finite sets FACTOR_FAILED,
leaves alpha at its last value and stops it; with tol > 0 a step with ||delta|| <= tol (1 + ||alpha||) (alpha after the step)
sets CONVERGED and stops it.  After the last step the cost is evaluated at the final alpha.  Checker only."""
import numpy as np

from tests import optics_ref as oref

CONVERGED, FACTOR_FAILED, BAD_INPUT = 1, 2, 4
COST0, COST, STEP, ITERS = range(4)
PHASE_LIMIT = 1.0e6


def cholesky(H):
    """Lower factor by columns with the device's pivot rule: None where a pivot is not positive and finite."""
    n = H.shape[0]
    L = np.zeros_like(H)
    A = H.copy()
    for k in range(n):
        piv = A[k, k]
        if not (np.isfinite(piv) and piv > 0.0):
            return None
        L[k, k] = np.sqrt(piv)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return L


def image_model(geom, Z, alpha):
    """(J, y) about phi = sum_j alpha_j Z_j; NaN where the phase rule refuses the screen."""
    p = len(geom["zd_list"]) * (geom["rmax"] - geom["rmin"] + 1) ** 2
    with np.errstate(invalid="ignore", over="ignore"):
        phi = np.tensordot(alpha, Z, axes=1)
    if not np.all(np.isfinite(phi)) or np.any(np.abs(phi) >= PHASE_LIMIT):
        return np.full((p, len(Z)), np.nan), np.full(p, np.nan)
    return oref.model(geom["pupil"], geom["W"], geom["zd_list"], geom["dx"], geom["rmin"], geom["rmax"], Z, geom["AU"], phi)


def refine(geom, Z, Y, alpha0, iters, damping=0.0, tol=0.0, want_cond=False):
    """geom: dict(pupil, W, zd_list, dx, rmin, rmax, AU) as optics_ref.model takes them; Z: (nmode, len, len) [j, row, column];
    Y: (batch, p); alpha0: (batch, nmode).  Returns dict(alphas (iters + 1, batch, nmode): the start and alpha after every
    iteration, info (batch, 4), status (batch,) [, cond: the largest cond(J'J) seen])."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64)); alpha0 = np.atleast_2d(np.asarray(alpha0, dtype=np.float64))
    batch, nmode = alpha0.shape
    alphas = np.zeros((iters + 1, batch, nmode)); info = np.zeros((batch, 4)); status = np.zeros(batch, dtype=np.int32)
    worst_cond = 0.0
    for b in range(batch):
        a = alpha0[b].copy()
        alphas[0, b] = a
        flag, steps, step, cost0 = 0, 0, 0.0, 0.0
        for it in range(iters):
            if not flag:
                J, y = image_model(geom, Z, a)
                r = Y[b] - y
                c = float(np.sum(r * r))
                if it == 0:
                    cost0 = c
                if not np.isfinite(c):
                    flag |= BAD_INPUT
                    a[:] = np.nan
                else:
                    H = J.T @ J
                    if want_cond and np.all(np.isfinite(H)):
                        worst_cond = max(worst_cond, float(np.linalg.cond(H)))
                    H[np.diag_indices(nmode)] *= 1.0 + damping
                    g = J.T @ r
                    L = cholesky(H)
                    if L is None:
                        flag |= FACTOR_FAILED
                    else:
                        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
                        a = a + delta
                        steps += 1
                        step = float(np.linalg.norm(delta))
                        if tol > 0.0 and step <= tol * (1.0 + float(np.linalg.norm(a))):
                            flag |= CONVERGED
            alphas[it + 1, b] = a
        _, y = image_model(geom, Z, a)
        r = Y[b] - y
        cost = float(np.sum(r * r))
        if iters == 0:
            cost0 = cost
        if (flag & BAD_INPUT) or not np.isfinite(cost):
            flag |= BAD_INPUT
            cost0 = cost = np.nan
            if iters > 0:
                alphas[iters, b] = np.nan
        info[b] = (cost0, cost, step, steps)
        status[b] = flag
    out = dict(alphas=alphas, info=info, status=status)
    if want_cond:
        out["cond"] = worst_cond
    return out


def images(geom, Z, alpha):
    """Y of a batch of coefficient rows: the exact noise-free images."""
    return np.stack([image_model(geom, Z, a)[1] for a in np.atleast_2d(alpha)])


def linear_start(geom, Z, Y):
    """The first-order estimate about zero aberration, ad_est = G (Y - b_s) with G = pinv(A_s): the loop's start."""
    A, b = image_model(geom, Z, np.zeros(len(Z)))
    return (np.linalg.pinv(A) @ (np.atleast_2d(Y) - b).T).T


def readme_geom(length, d, first, zd_list, Zdefocus):
    """The README's pupil and spacing at `length` with the window (d, first) and the defocus map W = Zdefocus [row, column]."""
    g = oref.readme_geometry(length)
    return dict(pupil=g["pupil"], W=np.asarray(Zdefocus), zd_list=np.asarray(zd_list, dtype=np.float64), dx=g["dx"], rmin=first,
                rmax=first + d - 1, AU=g["AU"])
