"""numpy restatement of the reference's mirror of Gaussian actuators (README.md:184-272), written for this repository: the
geometry of README.md:194-263, the influence functions of README.md:226-232 in their direct double-sum form, and the surface
sum_t u_t I_t.  B of README.md:271 comes through tests/modal_fit_ref.influence_matrix.
Maps are (m, rows, cols) indexed [t, row, column]: the device's planes are their transposes."""
import numpy as np


def geometry(length=512, dx=6.5e-6, D=4.4e-3, m1=12, coupling=0.1, half_width=2.2e-3):
    """README.md:194-263 line by line; the index values are the reference's 1-based ones."""
    m = m1 * m1
    d = D / (m1 - 1)                                                      # :204
    len_dm = int(np.floor(half_width * 2 / dx + 0.5))                     # :206 round()
    xaxis_dm = np.array([-len_dm / 2 + k for k in range(len_dm)]) * dx    # :207 (-len_dm/2):(len_dm/2-1)
    yaxis_dm = -xaxis_dm                                                  # :208
    diff_dm_idx = int(np.floor(len_dm / (m1 - 1)))                        # :212
    x0_dm_idx = [1]
    for i in range(1, m1):
        x0_dm_idx.append(1 + i * diff_dm_idx)                             # :213-216
    x0_dm_idx[-1] = len_dm                                                # :217
    x0_dm_axis = [xaxis_dm[i - 1] for i in x0_dm_idx]                     # :219
    y0_dm_axis = [yaxis_dm[i - 1] for i in x0_dm_idx]                     # :220
    cx, cy = np.zeros(m), np.zeros(m)
    act_idx = 0
    for i in range(m1):                                                   # :224-234
        for j in range(m1):
            cx[act_idx], cy[act_idx] = x0_dm_axis[j], y0_dm_axis[i]
            act_idx += 1
    xaxis = np.array([-length / 2 + k for k in range(length)]) * dx       # :241
    first_min = lambda v: int(np.flatnonzero(v == v.min())[0]) + 1        # MATLAB's min: the first of equal minima
    max_idx = first_min(np.abs(xaxis_dm - xaxis[-1]))                     # :255
    min_idx = first_min(np.abs(xaxis_dm - xaxis[0]))                      # :256
    x = xaxis_dm[min_idx - 1:max_idx].copy()                              # :260 columns min_idx:max_idx of XX_dm
    y = yaxis_dm[min_idx - 1:max_idx].copy()                              #      rows of YY_dm
    return dict(x=x, y=y, cx=cx, cy=cy, pitch=d, coupling=coupling, len_dm=len_dm, x0_dm_idx=np.array(x0_dm_idx), min_idx=min_idx,
                max_idx=max_idx)


def alpha(coupling, pitch):
    """log(coupling) / d^2 in double: the one constant every device entry shares."""
    return float(np.log(np.float64(coupling)) / (np.float64(pitch) * np.float64(pitch)))


def arg(x, y, cx, cy, coupling, pitch, dtype=np.float64):
    """alpha ((x - cx)^2 + (y - cy)^2), (m, rows, cols), evaluated in dtype from the double alpha."""
    x, y, cx, cy = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (x, y, cx, cy))
    xd = x[None, None, :] - cx[:, None, None]
    yd = y[None, :, None] - cy[:, None, None]
    return dtype(alpha(coupling, pitch)) * (xd * xd + yd * yd)


def influence(x, y, cx, cy, coupling, pitch, dtype=np.float64):
    """README.md:230 in its direct form: exp(log(coupling) (x_diff^2 + y_diff^2) / d^2)."""
    return np.exp(arg(x, y, cx, cy, coupling, pitch, dtype))


def surface(x, y, cx, cy, coupling, pitch, u, phase=None, dtype=np.float64):
    """phase + sum_t u[b][t] I_t, (batch, rows, cols), and sum_t |u[b][t]| I_t (+ |phase|), the scale of its rounding error."""
    I = influence(x, y, cx, cy, coupling, pitch, dtype)
    u = np.asarray(u, dtype=np.float64).astype(dtype)
    s = np.tensordot(u, I, axes=1)
    mag = np.tensordot(np.abs(u), I, axes=1)
    if phase is not None:
        p = np.asarray(phase, dtype=np.float64).astype(dtype)
        s, mag = s + p, mag + np.abs(p)
    return s, mag
