"""numpy restatement of the reference's modal fit: zernmodfit.m:209 (c = z \\ data(:), one least-squares solve per frame, the
"modified" amplitude/angle half of that file being commented out) and README.md:271 (B = pinv(Zs'Zs) Zs' B_pupil).
Z: (n, npx) mode maps as rows, the layout the device entry reads."""
import numpy as np


def modal_fit(Z, screens):
    """screens: (batch, npx).  Returns (c (batch, n), cond_2(Z Z'))."""
    Z = np.asarray(Z, dtype=np.float64)
    c = np.linalg.lstsq(Z.T, np.asarray(screens, dtype=np.float64).T, rcond=None)[0].T
    return np.ascontiguousarray(c), float(np.linalg.cond(Z @ Z.T))


def influence_matrix(Z, I):
    """I: (m, npx) influence functions.  Returns (B (n, m), cond_2(Z Z')) as README.md:271 writes it."""
    Z = np.asarray(Z, dtype=np.float64)
    G = Z @ Z.T
    return np.linalg.pinv(G) @ Z @ np.asarray(I, dtype=np.float64).T, float(np.linalg.cond(G))
