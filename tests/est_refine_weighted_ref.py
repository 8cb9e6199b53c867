"""numpy restatement of the estimator's refinement weighted by the detector's photon and read-out noise
(fmpc_est_refine_weighted_device), written for the tests, on top of tests/est_refine_ref.py (its image_model, cholesky and
constants).  Per realisation b with gain_b, det = dict(gain (a float or one per realisation), qe, background, read_noise,
photon_noise) and floor >= 0 in photo-electrons, in the header's order of rounding (every product, sum and quotient once):

    qe2 = qe qe ;  rn2 = read_noise read_noise ;  g2 = gain_b gain_b
    lam = gain_b max(y, 0) + background ;  v = photon_noise ? max(lam, floor) : 0 ;  var = (qe2 v + rn2) / g2 ;  w = 1 / var
    s = sqrt(w) ;  r = Y - qe y ;  A = s (qe J) (rows scaled) ;  c = s r
    H = A'A, H_ii <- H_ii (1 + damping) ;  g = A'c ;  delta = H \\ g (Cholesky) ;  alpha <- alpha + delta
    chi^2 = sum (w r) r ;  sigma = sqrt(diag(H^-1)) of the last step taken (NaN: none)

Iteration `it` is full when it % refresh == 0 ((J, y) about the current alpha) and held otherwise (y alone, the J of the last full
iteration); the weights come from the current y either way.  The freeze rules are rr.refine's, and BAD_INPUT is also set by a
gain, a weight or a chi^2 that is not positive and finite.  Checker only."""
import numpy as np

from tests import est_refine_ref as rr
from tests.est_refine_ref import BAD_INPUT, CONVERGED, COST, COST0, FACTOR_FAILED, ITERS, STEP, cholesky, image_model  # noqa: F401


def detector(gain=1.0, qe=1.0, background=0.0, read_noise=0.0, photon_noise=True):
    return dict(gain=gain, qe=float(qe), background=float(background), read_noise=float(read_noise), photon_noise=bool(photon_noise))


def weights(y, gain, det, floor):
    """w of the rows of a model image y for one gain, rounded as the device rounds it."""
    qe2, rn2, g2 = det["qe"] * det["qe"], det["read_noise"] * det["read_noise"], gain * gain
    with np.errstate(all="ignore"):
        lam = gain * np.where(y > 0.0, y, 0.0) + det["background"]
        v = np.where(lam > floor, lam, floor) if det["photon_noise"] else np.zeros_like(y)
        return 1.0 / ((qe2 * v + rn2) / g2)


def chi2(Y, y, gain, det, floor):
    """(chi^2, w, r); chi^2 is NaN when the gain, a weight or the sum itself is not positive and finite."""
    with np.errstate(all="ignore"):
        r = Y - det["qe"] * y
        w = weights(y, gain, det, floor)
        if not (np.isfinite(gain) and gain > 0.0) or not np.all(np.isfinite(w) & (w > 0.0)):
            return np.nan, w, r
        c = float(np.sum((w * r) * r))
        return (c if c > 0.0 else np.nan), w, r


def refine(geom, Z, Y, alpha0, iters, det, floor=1.0, refresh=1, damping=0.0, tol=0.0, want_cond=False):
    """As rr.refine (same geom, Z, Y, alpha0; alphas (iters + 1, batch, nmode), info (batch, 4) with chi^2 for the costs, status
    (batch,)) plus sigma (batch, nmode) [, cond: the largest cond(qe^2 J'WJ) seen]."""
    if refresh < 1:
        raise ValueError("refresh >= 1: the gain form has no weighted G")
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64)); alpha0 = np.atleast_2d(np.asarray(alpha0, dtype=np.float64))
    batch, nmode = alpha0.shape
    gains = np.broadcast_to(np.asarray(det["gain"], dtype=np.float64), (batch,))
    alphas = np.zeros((iters + 1, batch, nmode)); info = np.zeros((batch, 4)); status = np.zeros(batch, dtype=np.int32)
    sigma = np.full((batch, nmode), np.nan)
    worst_cond = 0.0
    for b in range(batch):
        gain = float(gains[b])
        a = alpha0[b].copy()
        alphas[0, b] = a
        flag, steps, step, cost0 = 0, 0, 0.0, 0.0
        J = None
        for it in range(iters):
            if not flag:
                if it % refresh == 0:
                    J, y = image_model(geom, Z, a)
                else:
                    y = image_model(geom, Z, a)[1]
                c, w, r = chi2(Y[b], y, gain, det, floor)
                if it == 0:
                    cost0 = c
                if not np.isfinite(c):
                    flag |= BAD_INPUT
                    a[:] = np.nan
                else:
                    s = np.sqrt(w)
                    A = s[:, None] * (det["qe"] * J)
                    H = A.T @ A
                    if want_cond and np.all(np.isfinite(H)):
                        worst_cond = max(worst_cond, float(np.linalg.cond(H)))
                    H[np.diag_indices(nmode)] *= 1.0 + damping
                    g = A.T @ (s * r)
                    L = cholesky(H)
                    if L is None:
                        flag |= FACTOR_FAILED
                    else:
                        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
                        Li = np.linalg.solve(L, np.eye(nmode))
                        sigma[b] = np.sqrt(np.sum(Li * Li, axis=0))
                        a = a + delta
                        steps += 1
                        step = float(np.linalg.norm(delta))
                        if tol > 0.0 and step <= tol * (1.0 + float(np.linalg.norm(a))):
                            flag |= CONVERGED
            alphas[it + 1, b] = a
        cost = chi2(Y[b], image_model(geom, Z, a)[1], gain, det, floor)[0]
        if iters == 0:
            cost0 = cost
        if (flag & BAD_INPUT) or not np.isfinite(cost):
            flag |= BAD_INPUT
            cost0 = cost = np.nan
            sigma[b] = np.nan
            if iters > 0:
                alphas[iters, b] = np.nan
        info[b] = (cost0, cost, step, steps)
        status[b] = flag
    out = dict(alphas=alphas, info=info, status=status, sigma=sigma)
    if want_cond:
        out["cond"] = worst_cond
    return out
