"""numpy / scipy restatement of the mirror of spline actuators, written for this repository from the description of OOMAO's
influenceFunction.m (:96-118 the curve, :253-362 the maps): the Bezier control points and samples, MATLAB's spline() as
scipy.interpolate.CubicSpline(bc_type="not-a-knot") both ways, the maps as outer products of two profiles, the surface with its
error scale, the per-tile actuator sets straight from their definition, and a long-double evaluation of a pp form that also
returns the scales of its rounding error.
A pp form is (breaks (pieces + 1), coef (pieces, 4)) with f(d) = sum_k coef[i, k] (d - breaks[i])^k on piece i, the last piece
closed on the right and f = 0 outside.  Maps are (m, rows, cols) indexed [t, row, column]: the device's planes are their
transposes."""
import numpy as np
from scipy.interpolate import CubicSpline

LD = np.longdouble
MONOTONIC = (0.2, (0.4, 0.7), (0.6, 0.4), 1.0, 1.0)
OVERSHOOT = (0.2, (0.4, 0.7), (0.5, 0.4), 0.3, 1.0)          # OOMAO's 'overshoot': its ordinates are not monotone
TILE = 64


def control_points(p2x, p3, p4, ratio, p6x):
    P = np.zeros((7, 2))
    P[0] = (0.0, 1.0); P[1] = (p2x, 1.0); P[2] = p3; P[3] = p4
    P[4] = -P[2] / ratio + (1.0 + 1.0 / ratio) * P[3]
    P[5] = (p6x, 0.0); P[6] = (2.0, 0.0)
    return P


def bezier(points=MONOTONIC):
    """The 201 samples (bx, by) of the two cubic segments at t = linspace(0, 1, 101), the second without its t = 0."""
    P = control_points(*points)
    t = np.linspace(0.0, 1.0, 101)[:, None]
    seg = lambda a: (1 - t) ** 3 * P[a] + 3 * (1 - t) ** 2 * t * P[a + 1] + 3 * (1 - t) * t ** 2 * P[a + 2] + t ** 3 * P[a + 3]
    b = np.concatenate([seg(0), seg(3)[1:]])
    return b[:, 0].copy(), b[:, 1].copy()


def oomao_pp(mech, points=MONOTONIC):
    """(breaks, coef, R) of OOMAO's profile at mechanical coupling mech: 401 knots, 400 pieces, R = breaks[-1]."""
    bx, by = bezier(points)
    if not (np.all(np.diff(by) < 0) or np.all(np.diff(by) > 0)):
        raise ValueError("the ordinates are not strictly monotone: x is no function of y")
    order = np.argsort(by)
    scale = float(CubicSpline(by[order], bx[order], bc_type="not-a-knot")(mech))
    bx = bx / scale
    u = np.concatenate([-bx[::-1], bx[1:]])
    v = np.concatenate([by[::-1], by[1:]])
    u[200] = 0.0
    cs = CubicSpline(u, v, bc_type="not-a-knot")
    return u, np.ascontiguousarray(cs.c[::-1].T), float(bx[-1])


def asymmetric_pp():
    """A hand-made profile of 3 pieces on [-1.5, 2.25], not symmetric, not continuous at its ends (f(-1.5) = 0.25, f(2.25) != 0)."""
    breaks = np.array([-1.5, -0.25, 0.5, 2.25])
    coef = np.array([[0.25, 0.5, 0.125, -0.0625], [0.875, 0.25, -0.5, 0.1875], [0.75, -0.375, 0.0625, 0.03125]])
    return breaks, coef


def pp_eval(breaks, coef, d, dtype=LD):
    """(f, S, D) at d in dtype: f(d); S = sum_k |c_k| |t|^k, the scale of the Horner roundings; D = |d f'(d)|, what a relative
    error of d is worth.  All three are 0 outside [breaks[0], breaks[-1]]."""
    d = np.asarray(d, dtype=dtype)
    b = np.asarray(breaks, dtype=np.float64).astype(dtype)
    c = np.asarray(coef, dtype=np.float64).astype(dtype)
    inside = (d >= b[0]) & (d <= b[-1])
    i = np.clip(np.searchsorted(b, d, side="right") - 1, 0, len(b) - 2)
    t = d - b[i]
    ci = c[i]
    f = ci[..., 0] + t * (ci[..., 1] + t * (ci[..., 2] + t * ci[..., 3]))
    at = np.abs(t)
    S = np.abs(ci[..., 0]) + at * (np.abs(ci[..., 1]) + at * (np.abs(ci[..., 2]) + at * np.abs(ci[..., 3])))
    D = np.abs(d * (ci[..., 1] + t * (2 * ci[..., 2] + 3 * t * ci[..., 3])))
    z = dtype(0)
    return np.where(inside, f, z), np.where(inside, S, z), np.where(inside, D, z)


def offsets(axis, centres, pitch, dtype=np.float64):
    """d[t, p] = (axis[p] - centres[t]) / pitch in dtype from the double inputs: in double, what the device forms."""
    a = np.asarray(axis, dtype=np.float64).astype(dtype)
    c = np.asarray(centres, dtype=np.float64).astype(dtype)
    return (a[None, :] - c[:, None]) / dtype(pitch)


def factors(x, y, cx, cy, pitch, breaks, coef, dtype=LD):
    """((fx, Sx, Dx), (fy, Sy, Dy)): the column factors (m, cols) and the row factors (m, rows) with their error scales."""
    return pp_eval(breaks, coef, offsets(x, cx, pitch, dtype), dtype), pp_eval(breaks, coef, offsets(y, cy, pitch, dtype), dtype)


def influence(x, y, cx, cy, pitch, breaks, coef, dtype=np.float64):
    """The maps (m, rows, cols): fy_t[r] fx_t[c]."""
    (fx, _, _), (fy, _, _) = factors(x, y, cx, cy, pitch, breaks, coef, dtype)
    return fy[:, :, None] * fx[:, None, :]


def surface(x, y, cx, cy, pitch, breaks, coef, u, phase=None, dtype=LD):
    """(s, mag, elem) (batch, rows, cols): s = phase + sum_t u_t I_t; mag = |phase| + sum_t |u_t| |I_t|; elem = sum_t |u_t| E_t with
    E_t the bound of an element of map t whose factors carry an error of 16 * 2^-52 (S + D) each (tests/test_gpu_dm_spline.py)."""
    (fx, Sx, Dx), (fy, Sy, Dy) = factors(x, y, cx, cy, pitch, breaks, coef, dtype)
    k = dtype(16 * 2.0 ** -52)
    ex, ey = k * (Sx + Dx), k * (Sy + Dy)
    u = np.asarray(u, dtype=np.float64).astype(dtype)
    s, mag, elem = [], [], []
    for ub in u:
        au = np.abs(ub)[:, None]
        s.append((fy * ub[:, None]).T @ fx)
        mag.append((np.abs(fy) * au).T @ np.abs(fx))
        elem.append((ey * au).T @ np.abs(fx) + (np.abs(fy) * au).T @ ex + (ey * au).T @ ex)
    s, mag, elem = np.stack(s), np.stack(mag), np.stack(elem)
    if phase is not None:
        p = np.asarray(phase, dtype=np.float64).astype(dtype)
        s, mag = s + p, mag + np.abs(p)
    return s, mag, elem


def tile_sets(x, y, cx, cy, pitch, lo, hi, tile=TILE):
    """Per tile of tile x tile pixels (tile (tr, tc) at tr + ntr * tc) the ascending actuators for which some column of the tile and
    some row of the tile lie inside [lo, hi] -- the offsets in double, as the device forms them."""
    dx, dy = offsets(x, cx, pitch), offsets(y, cy, pitch)
    inx, iny = (dx >= lo) & (dx <= hi), (dy >= lo) & (dy <= hi)
    rows, cols = len(y), len(x)
    ntr, ntc = -(-rows // tile), -(-cols // tile)
    out = []
    for tc in range(ntc):
        for tr in range(ntr):
            hx = inx[:, tc * tile:(tc + 1) * tile].any(axis=1)
            hy = iny[:, tr * tile:(tr + 1) * tile].any(axis=1)
            out.append(np.flatnonzero(hx & hy))
    order = [tr + ntr * tc for tc in range(ntc) for tr in range(ntr)]
    assert order == list(range(ntr * ntc))
    return out


def oomao_geometry(n_act, resolution, ratio_tel_dm=1.0, offset=(0.0, 0.0), valid=None):
    """setInfluenceFunction's grid (influenceFunction.m:262-267, 301-311) in pitch units: actuator k column-major over the valid
    (i, j), its row profile centred on yIF[i], its column profile on xIF[j]."""
    xIF = np.linspace(-1, 1, n_act) * (n_act - 1) / 2 - offset[0]
    yIF = np.linspace(-1, 1, n_act) * (n_act - 1) / 2 - offset[1]
    u0 = ratio_tel_dm * np.linspace(-1, 1, resolution) * (n_act - 1) / 2
    cx, cy = [], []
    for j in range(n_act):
        for i in range(n_act):
            if valid is None or valid[i][j]:
                cy.append(yIF[i]); cx.append(xIF[j])
    return dict(x=u0.copy(), y=u0.copy(), cx=np.array(cx), cy=np.array(cy), pitch=1.0)
