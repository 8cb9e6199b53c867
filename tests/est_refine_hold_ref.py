"""numpy restatement of the estimator's refinement with a held Jacobian and of its Jacobian-free gain form
(fmpc_est_refine_hold_device), written for the tests, on top of tests/est_refine_ref.py (its image_model, cholesky and constants).

refresh >= 1: iteration `it` is full when it % refresh == 0 -- (J, y) = model about the current alpha, as rr.refine does every
iteration -- and held otherwise: y alone about the current alpha, with the J of the last full iteration.  Then, either way,

    r = Y - y ;  H = J'J, H_ii <- H_ii (1 + damping) ;  g = J'r ;  delta = H \\ g (Cholesky) ;  alpha <- alpha + delta

refresh == 0 (the gain form): no J at all, alpha <- alpha + G (Y - y(alpha)) with G (nmode, p) the estimator's gain about zero
aberration, pinv(A_s) unless handed over.  The freeze rules, info and status are rr.refine's; FACTOR_FAILED cannot occur in the
gain form.  refresh = 1 is rr.refine operation by operation.  Checker only."""
import numpy as np

from tests import est_refine_ref as rr
from tests.est_refine_ref import BAD_INPUT, CONVERGED, COST, COST0, FACTOR_FAILED, ITERS, STEP, cholesky, image_model  # noqa: F401


def gain(geom, Z):
    """pinv of A_s about zero aberration: (nmode, p)."""
    return np.linalg.pinv(image_model(geom, Z, np.zeros(len(Z)))[0])


def refine(geom, Z, Y, alpha0, iters, refresh=1, G=None, damping=0.0, tol=0.0):
    """As rr.refine (same arguments, same dict: alphas (iters + 1, batch, nmode), info (batch, 4), status (batch,)) with the
    schedule `refresh` and, for refresh = 0, the gain G (None: gain(geom, Z))."""
    if refresh < 0 or (refresh == 0 and damping != 0.0):
        raise ValueError("refresh >= 0; the gain form takes no damping")
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64)); alpha0 = np.atleast_2d(np.asarray(alpha0, dtype=np.float64))
    batch, nmode = alpha0.shape
    if refresh == 0 and G is None:
        G = gain(geom, Z)
    alphas = np.zeros((iters + 1, batch, nmode)); info = np.zeros((batch, 4)); status = np.zeros(batch, dtype=np.int32)
    for b in range(batch):
        a = alpha0[b].copy()
        alphas[0, b] = a
        flag, steps, step, cost0 = 0, 0, 0.0, 0.0
        J = None
        for it in range(iters):
            if not flag:
                if refresh >= 1 and it % refresh == 0:
                    J, y = image_model(geom, Z, a)
                else:
                    y = image_model(geom, Z, a)[1]
                r = Y[b] - y
                c = float(np.sum(r * r))
                if it == 0:
                    cost0 = c
                if not np.isfinite(c):
                    flag |= BAD_INPUT
                    a[:] = np.nan
                else:
                    if refresh == 0:
                        delta = G @ r
                    else:
                        H = J.T @ J
                        H[np.diag_indices(nmode)] *= 1.0 + damping
                        g = J.T @ r
                        L = cholesky(H)
                        if L is None:
                            flag |= FACTOR_FAILED
                            delta = None
                        else:
                            delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
                    if delta is not None:
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
    return dict(alphas=alphas, info=info, status=status)


def contraction(alphas, truth, refresh, floor=1e-11):
    """The worst ratio err[it + 1] / err[it], err = ||alpha_it - truth||, over the realisations and the held (refresh >= 1,
    it % refresh != 0) or gain (refresh = 0) iterations: the condition under which a device and this restatement are compared
    (<= 0.5: rounding differences do not grow).  Iterations that start below floor max(1, ||truth||) are at rounding level and
    do not count."""
    err = np.linalg.norm(alphas - truth[None], axis=2)
    scale = np.maximum(1.0, np.linalg.norm(truth, axis=1))
    worst = 0.0
    for it in range(len(err) - 1):
        if refresh == 0 or (refresh >= 1 and it % refresh != 0):
            live = err[it] > floor * scale
            if np.any(live):
                worst = max(worst, float(np.max(err[it + 1][live] / err[it][live])))
    return worst
