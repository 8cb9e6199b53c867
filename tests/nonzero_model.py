"""A model of the AO configuration (n = 27) whose constants do not vanish, shared by tests/test_nonzero_model_ref.py (CPU) and
tests/test_gpu_nonzero_constants.py (GPU).  synthetic.make_model has q = r = qf = 0 and a box centred on zero, so umid, xmid, cu,
c2, u0c, zc, nuc, e, e0 and ep of the cold-start forms are all zero there; here linear costs and a box that is not centred on
zero make every one of them non-zero (|umid| ~ 42, |xmid| ~ 65), with the magnitudes of
tests/test_gpu_bank_first_move.py::nonvanishing and the same asymmetry on the x box.  Plain helper module: no fixtures."""
import numpy as np

K_BAR = 1e-2


def nonzero_model(pkg, T, var_order=2, xf=False, m=144, seed=7):
    md = pkg.synthetic.make_model(27, m, T, var_order=var_order)
    rng = np.random.default_rng(seed)
    n = md["n"]
    md["r"] = 0.05 * rng.standard_normal(m)
    md["q"] = 0.05 * rng.standard_normal(n); md["qf"] = 0.05 * rng.standard_normal(n)
    md["u_max"] = md["u_max"] * (1.0 + 0.5 * rng.random(m)); md["u_min"] = md["u_min"] * (1.0 + 0.1 * rng.random(m))
    md["x_max"] = md["x_max"] * (1.0 + 0.5 * rng.random(n)); md["x_min"] = md["x_min"] * (1.0 + 0.1 * rng.random(n))
    if xf:
        md["xf"] = 0.01 * rng.standard_normal(n)
    return md


def scale_box(md, s):
    """The u box scaled by s about zero: the asymmetry (umid / width) stays."""
    md = dict(md)
    md["u_min"] = s * md["u_min"]; md["u_max"] = s * md["u_max"]
    return md


def nonzero_data(pkg, md, batch, nu0=True, w=False, scale=None, seed=7):
    """make_replay_batch(md, r=5, steps=batch); nu0 ~ N(0, 1) over all block rows (the terminal one included), w = 0.05 randn
    on request, x0_pre = None for VAR(1); scale: per-problem factors on x0 and x0_pre."""
    T, n = md["T"], md["n"]
    rng = np.random.default_rng(seed + 100)
    data = pkg.synthetic.make_replay_batch(md, r=5, steps=batch, with_nu0=False)
    if scale is not None:
        data["x0"] = data["x0"] * np.asarray(scale)[:, None]; data["x0_pre"] = data["x0_pre"] * np.asarray(scale)[:, None]
    nb = T + (1 if md.get("xf") is not None else 0)
    data["nu0"] = rng.standard_normal((batch, nb * n)) if nu0 else None
    data["w"] = 0.05 * rng.standard_normal((batch, T * n)) if w else None
    if md.get("var_order", 2) == 1:
        data["x0_pre"] = None
    return data


def zero_data(data):
    """The same batch shape with d = 0 (one problem): what the forms' constant parts alone give."""
    return {k: (None if v is None else np.zeros_like(v[:1])) for k, v in data.items()}


def constants(md, k=K_BAR):
    """umid, xmid, the barrier curvature of the u rows at the mid-box start h = k (1/s+^2 + 1/s-^2), and
    cu = 2R umid + r + k (1/s+ - 1/s-)."""
    umid = 0.5 * (md["u_min"] + md["u_max"]); xmid = 0.5 * (md["x_min"] + md["x_max"])
    sp = md["u_max"] - umid; sm = umid - md["u_min"]
    h = k * (1.0 / sp ** 2 + 1.0 / sm ** 2)
    cu = 2.0 * np.diag(md["R"]) * umid + md["r"] + k * (1.0 / sp - 1.0 / sm)
    return umid, xmid, h, cu


def decision_margin(md, data, z, k=K_BAR):
    """Per problem ||e||^2 / (lower bound of rho^2) of the cold-start step that ends in z (w = None): e on the u rows is
    h (u+ - umid), and rho^2 >= ||r_p||^2 >= its stage 0, xmid - A1 x0 - A2 x0_pre - B umid.  The forms accept t = 1 without
    the exact path when ||e||^2 <= 0.5 rho^2."""
    T, n, m = md["T"], md["n"], md["m"]
    umid, xmid, h, _ = constants(md, k)
    Z = z.reshape(z.shape[0], T, m + n)
    e2 = ((h[None, None, :] * (Z[:, :, :m] - umid)) ** 2).sum(axis=(1, 2))
    rp0 = xmid - data["x0"] @ md["A1"].T - md["B"] @ umid
    if data.get("x0_pre") is not None:
        rp0 = rp0 - data["x0_pre"] @ md["A2"].T
    return e2 / (rp0 ** 2).sum(axis=1)


def oracle_decision_ratio(banded, data, k=K_BAR):
    """Per problem the oracle's own ||e||^2 / rho^2 of the first Newton step (the sums the step-length decision rests on).  The
    forms decide on an upper bound of the first and a lower bound of the second: a problem above 0.5 here must be handed over."""
    out = []
    for p in range(data["x0"].shape[0]):
        info = {}
        banded.solve(data["x0"][p], None if data.get("x0_pre") is None else data["x0_pre"][p], None if data.get("w") is None else data["w"][p],
                     1, k, nu0=None if data.get("nu0") is None else data["nu0"][p], info=info)
        out.append(info["eps2"][0] / info["rho2"][0])
    return np.array(out)
