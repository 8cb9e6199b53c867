"""GPU tests of the mirror of spline actuators (fmpc_kernel_dm_spline.hip; fmpc_dm_spline_*_device, pkg.SplineDM) against the
numpy / scipy restatement tests/dm_spline_ref.py.

Bars, all from the number formats (EPS = 2^-52; K = 16, or 32 where numpy.longdouble is no wider than double):
  factor   |f_dev - f_ref| <= K EPS (S + D) + 1e-300 against the long-double evaluation of the SAME pp arrays at the long-double
           offset: S = sum_k |c_k| |t|^k carries the three fused Horner steps and the rounding of t, D = |d f'(d)| the two roundings
           of d = (x - c) / pitch.  The device's factors are moreover bit for bit fmpc_dm_profile_eval_host at the double offset,
           and a map is bit for bit the product of its two factors.
  B        per column ||B_t - ref_t|| / ||ref_t|| <= max(1e-14 cond, 1e-12) with cond <= 1e3 asserted (tests/test_gpu_dm.py).
  surface  |out - ref| <= sum_t |u_t| E_t + m EPS mag + 1e-300, mag = |phase| + sum_t |u_t| |I_t|; E_t = |fy| ex + |fx| ey + ex ey is
           the bound of an element whose factors carry ex, ey = K EPS (S + D) (K leaves room for the two roundings of
           (fx u) fy); m EPS mag covers the accumulation and the phase.
  against the Gaussian mirror: the spline's interpolation error and the truncation at |d| = 4, computed in numpy, times
           sum_t |u_t|, plus the two rounding bars."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch
from scipy.interpolate import CubicSpline

from tests import dm_spline_ref as ref
from tests import optics_ref as oref
from tests.modal_fit_ref import influence_matrix

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52
K_ELEM = 16 if np.finfo(LD).eps < np.finfo(np.float64).eps else 32
TILE = 64


def _pkg():
    return importlib.import_module("mpc-sensorlessao_amd")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def profile(name):
    """(breaks, coef (pieces, 4)): 'oomao<mech>' from the host call (the pp arrays the device gets), 'asym' the 3-piece one,
    'gauss' the not-a-knot spline of exp(ln(0.1) d^2) on 201 knots over [-4, 4]."""
    if name.startswith("oomao"):
        p = _pkg().oomao_profile(float(name[5:]))
        return p.breaks, p.coef
    if name == "asym":
        return frozen(*ref.asymmetric_pp())
    k = np.linspace(-4.0, 4.0, 201)
    cs = CubicSpline(k, np.exp(np.log(0.1) * k * k), bc_type="not-a-knot")
    return frozen(k, np.ascontiguousarray(cs.c[::-1].T))


def make_dm(pkg, g, prof):
    b, c = profile(prof)
    return pkg.SplineDM(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], pkg.DMProfile(b, c))


def host(t):
    """Device planes [.., column, row] -> host [.., row, column]."""
    return np.swapaxes(t.cpu().numpy(), -1, -2)


def planes(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, -1, -2))).to(gpu)         # [b, row, column] -> [b, column, row]


# ------------------------------------------------------------------------------------------------------------ 1: tables and maps
@functools.lru_cache(maxsize=None)
def small_mirror():
    """rows = 70, cols = 133 (ragged tiles both ways), m = 19, pitch 9.3 px, y descending as the reference's, centres off the pixel
    grid; actuator 0 lies right of the grid and reaches nothing of it, actuator 1 above the first row and reaches it."""
    rows, cols, m = 70, 133, 19
    rng = np.random.default_rng(70133)
    x = np.arange(cols, dtype=np.float64)
    y = (rows - 1.0) - np.arange(rows, dtype=np.float64)
    cx, cy = rng.uniform(0.0, cols - 1.0, m), rng.uniform(0.0, rows - 1.0, m)
    cx[0] = cols + 40.3
    cy[1] = rows + 6.6
    frozen(x, y, cx, cy)
    return dict(x=x, y=y, cx=cx, cy=cy, pitch=9.3, rows=rows, cols=cols, m=m)


@pytest.mark.parametrize("prof", ["oomao0.1", "asym"])
def test_tables_and_maps(pkg, gpu, prof):
    g = small_mirror()
    rows, cols, m = g["rows"], g["cols"], g["m"]
    b, c = profile(prof)
    dm = make_dm(pkg, g, prof)
    assert (dm.m, dm.rows, dm.cols, dm.npx) == (m, rows, cols, rows * cols)
    I = dm.influence()
    torch.cuda.synchronize()
    assert tuple(I.shape) == (m, cols, rows) and I.is_contiguous()
    mpad, P = 32, 128 + 192
    tab = dm.ws[:8 * (rows + cols) * mpad].view(torch.float64).reshape(rows + cols, mpad).cpu().numpy()
    tabp = dm.ws[8 * (rows + cols) * mpad:8 * ((rows + cols) * mpad + m * P)].view(torch.float64).reshape(m, P).cpu().numpy()
    fx, fy = tab[:cols, :m].T, tab[cols:, :m].T
    assert np.all(tab[:, m:] == 0.0)
    # the pixel-minor copy: the same doubles, zeros in the padding
    assert np.array_equal(tabp[:, :cols], fx) and np.array_equal(tabp[:, 192:192 + rows], fy)
    assert np.all(tabp[:, cols:192] == 0.0) and np.all(tabp[:, 192 + rows:] == 0.0)
    prof_h = pkg.DMProfile(b, c)
    for f_dev, axis, centres, what in ((fx, g["x"], g["cx"], "fx"), (fy, g["y"], g["cy"], "fy")):
        d = ref.offsets(axis, centres, g["pitch"])                                        # in double, as the device forms it
        outside = (d < b[0]) | (d > b[-1])
        assert outside.any() and (~outside).any()
        assert np.all(f_dev[outside] == 0.0), what                                        # exactly zero beyond the support
        assert np.array_equal(f_dev, prof_h.eval(d)), what                                # the host's evaluation, bit for bit
        f, S, D = ref.pp_eval(b, c, ref.offsets(axis, centres, g["pitch"], LD))
        bar = K_ELEM * EPS * (S + D) + LD(1e-300)
        ratio = float(np.max(np.abs(f_dev.astype(LD) - f) / bar))
        print(f"{prof} {what}: worst |f - f_ref| / bar = {ratio:.3f}")
        assert ratio <= 1.0, (what, ratio)
    assert np.all(fx[0] == 0.0) and np.any(fy[1] != 0.0)                                  # the two actuators outside the grid
    # a map is the product of its factors, bit for bit; rows and columns are not swapped (another shape)
    Ih = host(I)
    assert np.array_equal(Ih, fy[:, :, None] * fx[:, None, :])
    assert torch.equal(dm.influence(3, 5), I[3:8]) and torch.equal(dm.influence(m - 1, 1), I[m - 1:]) and torch.equal(dm.influence(0, 1), I[:1])
    pad = torch.full((4, cols * rows + 7), -7.0, dtype=torch.float64, device=gpu)          # ldi padded: the guard stays
    view = pad[:, :cols * rows].view(4, cols, rows)
    got = dm.influence(11, 4, out=view)
    assert got.data_ptr() == pad.data_ptr()
    assert torch.equal(view, I[11:15]) and bool((pad[:, cols * rows:] == -7.0).all())
    # the lists of the two ragged-tile rows and three tile columns, against the definition
    lo, hi = (b[0], b[-1])
    sets = ref.tile_sets(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], lo, hi)
    lists = dm.tile_lists()
    assert len(lists) == 6 and all(np.array_equal(a, s) for a, s in zip(lists, sets)), (lists, sets)
    assert all(0 not in s for s in sets) and any(1 in s for s in sets)


# ------------------------------------------------------------------------------------------------------------ 2: B
from tests.test_gpu_dm import B_CASES, ORDER, mirror as gauss_mirror, z_dev, rel          # noqa: E402  (the sizes and geometries of the Gaussian test)

B_PROFILE = "oomao0.3"                      # support +-2.97 pitches: every actuator of those geometries reaches the grid


def b_geometry(rows, cols, m):
    g = gauss_mirror(rows, cols, m)
    return dict(x=g["x"], y=g["y"], cx=g["cx"], cy=g["cy"], pitch=g["pitch"])


@functools.lru_cache(maxsize=None)
def b_case(n, rows, cols, m):
    """Mode maps [j, row, column] as tests/test_gpu_dm.py makes them and the restatement's B (n, m) and cond on the numpy maps."""
    if m == 144:
        Z = oref.zernike_grid(ORDER[n], rows)
    else:
        Z = np.random.default_rng(7 * n + rows).standard_normal((n, cols, rows)).swapaxes(-1, -2)
    Z = np.ascontiguousarray(Z)
    g = b_geometry(rows, cols, m)
    I = ref.influence(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], *profile(B_PROFILE))
    out, cond = influence_matrix(Z.reshape(n, -1), I.reshape(m, -1))
    frozen(Z, out)
    return Z, out, cond


@pytest.mark.parametrize("n,rows,cols,m,skip", B_CASES)
def test_matrix_matches_numpy_restatement(pkg, gpu, n, rows, cols, m, skip):
    Z, want, cond = b_case(n, rows, cols, m)
    assert cond <= 1e3, cond
    bar = max(1e-14 * cond, 1e-12)
    dm = make_dm(pkg, b_geometry(rows, cols, m), B_PROFILE)
    mf = pkg.ModalFit(z_dev(Z, gpu))
    B = dm.influence_matrix(mf, skip=skip)
    torch.cuda.synchronize()
    assert int(mf.status) == 0
    assert tuple(B.shape) == (n - skip, m) and tuple(B.stride()) == (1, n - skip)
    Bh = B.cpu().numpy()
    assert all(np.linalg.norm(want[skip:, t]) > 0 for t in range(m))
    worst = max(rel(Bh[:, t], want[skip:, t]) for t in range(m))
    print(f"B ({n}, {rows}, {cols}, {m}): worst column {worst:.2e} (cond {cond:.2e}, bar {bar:.2e})")
    assert worst <= bar, worst
    # bits: a repeated call, the smallest workspace (one panel of 16 actuators at a time), a padded ldb
    assert torch.equal(dm.influence_matrix(mf, skip=skip), B)
    need = pkg.dm_spline_matrix_workspace_bytes(n, m, rows, cols, minimum=True)
    assert 0 < need <= pkg.dm_spline_matrix_workspace_bytes(n, m, rows, cols)
    small = torch.empty(need, dtype=torch.uint8, device=gpu)
    assert torch.equal(dm.influence_matrix(mf, skip=skip, workspace=small), B)
    with pytest.raises(pkg.FastMPCError) as e:
        dm.influence_matrix(mf, skip=skip, workspace=small[:need - 8])
    assert e.value.code == pkg.FMPC_E_DIM
    nc = n - skip
    pad = torch.full((m, nc + 5), -7.0, dtype=torch.float64, device=gpu)
    got = dm.influence_matrix(mf, skip=skip, out=pad[:, :nc].t())
    assert got.data_ptr() == pad.data_ptr()
    assert torch.equal(pad[:, :nc].t(), B) and bool((pad[:, nc:] == -7.0).all())


def test_matrix_of_a_failed_factor_is_nan(pkg, gpu):
    n, rows, cols, m, skip = B_CASES[1]
    Z = b_case(n, rows, cols, m)[0].copy()
    Z[5] = 0.0                                                                            # rank-deficient
    mf = pkg.ModalFit(z_dev(Z, gpu))
    B = make_dm(pkg, b_geometry(rows, cols, m), B_PROFILE).influence_matrix(mf, skip=skip)
    torch.cuda.synchronize()
    assert int(mf.status) == pkg.FMPC_E_NOT_PD_SCHUR
    assert tuple(B.shape) == (n - skip, m) and bool(torch.isnan(B).all())


# ------------------------------------------------------------------------------------------------------------ 3: surface
LIST_GRIDS = [(128, 192), (100, 150)]
BASE = {(0, 0): 1, (1, 0): 0, (0, 1): 16, (1, 1): 17, (0, 2): 48, (1, 2): 33}             # actuators on the lattice of tile (tr, tc)


@functools.lru_cache(maxsize=None)
def lists_mirror(rows, cols):
    """Pixel axes 0, 1, ..; pitch 2 px; OOMAO's profile at 0.1 reaches +-4.15 px.  Around the centre (31.7 + 64 tr, 31.7 + 64 tc) of
    each tile of the 128 x 192 grid sits a 6-px lattice within +-18 px holding BASE[tr, tc] actuators, which reach no other tile.
    One actuator sits on the corner the first four tiles share, one at column -3 (it reaches columns 0 and 1), one at column -50
    (it reaches nothing): m = 118.  The order of the actuators is shuffled, so a tile's list is no run of consecutive indices.
    On the 100 x 150 grid the same actuators meet ragged tiles, and some lie beyond the grid."""
    rng = np.random.default_rng(118)
    off = np.array([(a, b) for a in range(-18, 19, 6) for b in range(-18, 19, 6)], dtype=np.float64)
    pts = []
    for (tr, tc), count in BASE.items():
        pick = off[rng.permutation(len(off))[:count]]
        pts += [(31.7 + 64 * tc + dx, 31.7 + 64 * tr + dy) for dy, dx in pick]
    special = {"corner": (63.5, 63.5), "edge": (-3.0, 31.7), "far": (-50.0, 31.7)}
    pts += list(special.values())
    pts = np.array(pts)[rng.permutation(len(pts))]
    where = {k: int(np.flatnonzero((pts[:, 0] == v[0]) & (pts[:, 1] == v[1]))[0]) for k, v in special.items()}
    where["interior"] = int(np.flatnonzero((np.abs(pts[:, 0] - 159.7) <= 18) & (np.abs(pts[:, 1] - 31.7) <= 18))[0])
    x, y = np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64)
    cx, cy = pts[:, 0].copy(), pts[:, 1].copy()
    frozen(x, y, cx, cy)
    b, _ = profile("oomao0.1")
    sets = ref.tile_sets(x, y, cx, cy, 2.0, b[0], b[-1])
    return dict(x=x, y=y, cx=cx, cy=cy, pitch=2.0, rows=rows, cols=cols, m=len(pts), where=where, sets=sets)


@functools.lru_cache(maxsize=None)
def lists_case(rows, cols):
    """u (5, m), phase (5, rows, cols) and the long-double reference with and without the phase, mag and the element term."""
    g = lists_mirror(rows, cols)
    rng = np.random.default_rng(rows + cols)
    u = rng.uniform(-1.0, 1.0, (5, g["m"]))
    phase = rng.standard_normal((5, rows, cols))
    s, mag, elem = ref.surface(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], *profile("oomao0.1"), u)
    frozen(u, phase, s, mag, elem)
    return u, phase, s, mag, elem


def check_surface(out, want, mag, elem, m, what):
    bar = elem + m * EPS * mag + LD(1e-300)
    ratio = float(np.max(np.abs(out.astype(LD) - want) / bar))
    print(f"{what}: worst |out - ref| / bar = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


def test_list_sizes_by_construction():
    g = lists_mirror(128, 192)
    assert g["m"] == 118 and g["m"] % 16 != 0
    assert sorted(len(s) for s in g["sets"]) == [1, 3, 17, 18, 33, 48]
    w = g["where"]
    assert [i for i, s in enumerate(g["sets"]) if w["corner"] in s] == [0, 1, 2, 3]
    assert [i for i, s in enumerate(g["sets"]) if w["edge"] in s] == [0]
    assert not any(w["far"] in s for s in g["sets"]) and [i for i, s in enumerate(g["sets"]) if w["interior"] in s] == [4]
    assert any(np.any(np.diff(s) > 1) for s in g["sets"])


@pytest.mark.parametrize("rows,cols", LIST_GRIDS)
def test_surface(pkg, gpu, rows, cols):
    g = lists_mirror(rows, cols)
    m, npx = g["m"], rows * cols
    u, phase, s, mag, elem = lists_case(rows, cols)
    dm = make_dm(pkg, g, "oomao0.1")
    lists = dm.tile_lists()
    assert len(lists) == len(g["sets"]) and all(np.array_equal(a, b) for a, b in zip(lists, g["sets"]))
    pl = phase.astype(LD)
    for batch in (1, 2, 3, 5):                                                            # NB = 1, 2, 2 (ragged), 4 (ragged)
        ud, pd = torch.from_numpy(u[:batch].copy()).to(gpu), planes(phase[:batch], gpu)
        out = dm.surface(ud, phase=pd)
        alone = dm.surface(ud)                                                            # phase=None
        dense = dm.surface(ud, phase=pd, dense=True)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (batch, cols, rows) and out.is_contiguous()
        what = f"surface ({batch}, {rows}, {cols})"
        check_surface(host(out), s[:batch] + pl[:batch], mag[:batch] + np.abs(pl[:batch]), elem[:batch], m, what + " with phase")
        check_surface(host(alone), s[:batch], mag[:batch], elem[:batch], m, what + " alone")
        check_surface(host(dense), s[:batch] + pl[:batch], mag[:batch] + np.abs(pl[:batch]), elem[:batch], m, what + " dense")
        # dense against sparse within the same bar (not bitwise: the grouping into matrix instructions differs)
        gap = np.abs(host(dense).astype(LD) - host(out).astype(LD)) / (elem[:batch] + m * EPS * (mag[:batch] + np.abs(pl[:batch])) + LD(1e-300))
        assert float(gap.max()) <= 1.0
        # in place
        buf = pd.clone()
        got = dm.surface(ud, phase=buf, out=buf)
        assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, out)
        # ldu, ldp, ldo padded: the guards stay
        up = torch.full((batch, m + 3), 9.0, dtype=torch.float64, device=gpu); up[:, :m] = ud
        pp = torch.full((batch, npx + 5), 9.0, dtype=torch.float64, device=gpu); pp[:, :npx] = pd.reshape(batch, npx)
        op = torch.full((batch, npx + 11), -7.0, dtype=torch.float64, device=gpu)
        dm.surface(up[:, :m], phase=pp[:, :npx].view(batch, cols, rows), out=op[:, :npx].view(batch, cols, rows))
        assert torch.equal(op[:, :npx].reshape(batch, cols, rows), out) and bool((op[:, npx:] == -7.0).all())
        assert bool((pp[:, npx:] == 9.0).all()) and bool((up[:, m:] == 9.0).all())
        # the single-u form
        assert torch.equal(dm.surface(ud[0], phase=pd[0]), out[0])
    # u = 0 returns the phase bit for bit, the tile without actuators included
    assert torch.equal(dm.surface(torch.zeros_like(ud), phase=pd), pd)


def test_surface_of_a_unit_vector_is_the_map(pkg, gpu):
    g = lists_mirror(100, 150)
    m = g["m"]
    dm = make_dm(pkg, g, "oomao0.1")
    S = dm.surface(torch.eye(m, dtype=torch.float64, device=gpu))
    I = dm.influence()
    torch.cuda.synchronize()
    s, mag, elem = ref.surface(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], *profile("oomao0.1"), np.eye(m)[:8])
    check_surface(host(S[:8]), s, mag, elem, m, "surface(e_t)")
    gap = float((S - I).abs().max())
    print(f"surface(e_t) against influence(): {gap:.2e}")
    assert gap <= EPS                                                                     # (one product each, of factors <= 1 + 1e-8)
    assert float(I.abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------------------ 4: the lists are exact
@pytest.mark.parametrize("rows,cols", LIST_GRIDS)
def test_a_nan_u_marks_the_tiles_of_its_list(pkg, gpu, rows, cols):
    g = lists_mirror(rows, cols)
    dm = make_dm(pkg, g, "oomao0.1")
    u, phase, *_ = lists_case(rows, cols)
    pd = planes(phase[:1], gpu)
    ntr = -(-rows // TILE)
    for name, t in g["where"].items():
        ud = torch.from_numpy(u[:1].copy()).to(gpu)
        ud[0, t] = float("nan")
        got = torch.isnan(dm.surface(ud, phase=pd))[0].cpu().numpy().T                    # [row, column]
        want = np.zeros((rows, cols), dtype=bool)
        for tile, s in enumerate(g["sets"]):
            if t in s:
                tr, tc = tile % ntr, tile // ntr
                want[tr * TILE:(tr + 1) * TILE, tc * TILE:(tc + 1) * TILE] = True
        assert np.array_equal(got, want), name
        if (rows, cols) == LIST_GRIDS[0]:                                                 # (on the smaller grid others lie beyond it too)
            assert want.any() == (name != "far"), name
        else:
            assert want.any() == (name in ("corner", "edge")), name
        assert bool(torch.isnan(dm.surface(ud, phase=pd, dense=True)).all()), name


def test_lists_of_axes_that_are_not_monotone(pkg, gpu):
    g = dict(lists_mirror(100, 150))
    rng = np.random.default_rng(5)
    g["x"], g["y"] = g["x"][rng.permutation(150)], g["y"][rng.permutation(100)]
    b, _ = profile("oomao0.1")
    sets = ref.tile_sets(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], b[0], b[-1])
    assert [len(s) for s in sets] != [len(s) for s in lists_mirror(100, 150)["sets"]]
    lists = make_dm(pkg, g, "oomao0.1").tile_lists()
    assert all(np.array_equal(a, s) for a, s in zip(lists, sets))


# ------------------------------------------------------------------------------------------------------------ 5: bits
def test_bits(pkg, gpu):
    rows, cols = 100, 150
    g = lists_mirror(rows, cols)
    u, phase, *_ = lists_case(rows, cols)
    dm = make_dm(pkg, g, "oomao0.1")
    ud, pd = torch.from_numpy(u.copy()).to(gpu), planes(phase, gpu)
    for dense in (False, True):
        out = dm.surface(ud, phase=pd, dense=dense)
        assert torch.equal(dm.surface(ud, phase=pd, dense=dense), out)                    # two calls
        for b in range(5):                                                                # alone (NB = 1) and in a batch of 2 (NB = 2)
            assert torch.equal(dm.surface(ud[b:b + 1], phase=pd[b:b + 1], dense=dense), out[b:b + 1]), b
            lo = min(b, 3)
            assert torch.equal(dm.surface(ud[lo:lo + 2], phase=pd[lo:lo + 2], dense=dense)[b - lo], out[b]), b
    # two prepare calls leave the same bytes, whatever the workspace held
    n = dm.ws.numel()
    a = torch.full((n,), 0xAA, dtype=torch.uint8, device=gpu)
    b = torch.full((n,), 0x55, dtype=torch.uint8, device=gpu)
    first = dm.ws.clone()
    dm.prepare(ws=a)
    assert torch.equal(a, first)
    dm.prepare(ws=b)
    assert torch.equal(a, b) and dm.ws.data_ptr() == b.data_ptr()
    with pytest.raises(pkg.FastMPCError):
        dm.prepare(ws=a[:n - 8])
    # moved centres: prepare() again, and the surface follows
    dm.prepare(ws=a)
    before = dm.surface(ud, phase=pd)
    dm.cx.add_(1.0)
    dm.prepare()
    assert not torch.equal(dm.surface(ud, phase=pd), before)
    g2 = dict(g); g2["cx"] = g["cx"] + 1.0
    assert torch.equal(make_dm(pkg, g2, "oomao0.1").surface(ud, phase=pd), dm.surface(ud, phase=pd))


# ------------------------------------------------------------------------------------------------------------ 6: the Gaussian mirror
def test_against_the_gaussian_mirror(pkg, gpu):
    """Two independent kernels: the profile that interpolates exp(ln(0.1) d^2) on 201 knots over [-4, 4] against GaussianDM."""
    rows = cols = 64
    m, pitch, batch = 25, 11.3, 3
    rng = np.random.default_rng(64)
    x = np.arange(cols, dtype=np.float64); y = (rows - 1.0) - np.arange(rows, dtype=np.float64)
    cx, cy = np.meshgrid(4.1 + 13.9 * np.arange(5), 3.3 + 14.2 * np.arange(5))
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    g = dict(x=x, y=y, cx=cx, cy=cy, pitch=pitch)
    b, c = profile("gauss")
    # what the profile is off the Gaussian by: the interpolation error inside (64 points per piece, the knots' neighbourhoods
    # included; the error of a cubic interpolant between two samples 1/1600 apart moves by far less than the 2 % allowed for it)
    # and the Gaussian's own value beyond |d| = 4
    d = np.linspace(-4.0, 4.0, 200 * 64 + 1)
    e_in = 1.02 * float(np.max(np.abs(ref.pp_eval(b, c, d)[0] - np.exp(LD(np.log(0.1)) * d.astype(LD) ** 2))))
    e_out = 0.1 ** 16
    e = max(e_in, e_out)
    assert e_out < e < 1e-5, e
    u = rng.uniform(-1.0, 1.0, (batch, m))
    phase = rng.standard_normal((batch, rows, cols))
    sdm = make_dm(pkg, g, "gauss")
    gdm = pkg.GaussianDM(x, y, cx, cy, 0.1, pitch)
    ud, pd = torch.from_numpy(u).to(gpu), planes(phase, gpu)
    a, o = host(sdm.surface(ud, phase=pd)).astype(LD), host(gdm.surface(ud, phase=pd)).astype(LD)
    # |fy fx - gy gx| <= |fy - gy| |fx| + |gy| |fx - gx| <= e (1 + e) + e per actuator
    model = (2 * e + e * e) * np.abs(u).sum(axis=1)[:, None, None]
    _, mag_s, elem = ref.surface(x, y, cx, cy, pitch, b, c, u, phase)
    al = np.log(0.1) / pitch ** 2
    A = float(np.max(np.abs(al) * ((x[None, :] - cx[:, None]) ** 2).max(axis=1) + np.abs(al) * ((y[None, :] - cy[:, None]) ** 2).max(axis=1)))
    gy = np.exp(al * (y[None, :] - cy[:, None]) ** 2); gx = np.exp(al * (x[None, :] - cx[:, None]) ** 2)
    mag_g = np.stack([(gy * np.abs(ub)[:, None]).T @ gx for ub in u]) + np.abs(phase)
    bar = model + (elem + m * EPS * mag_s) + (K_ELEM * EPS * (1 + A) + m * EPS) * mag_g + 1e-300
    ratio = float(np.max(np.abs(a - o) / bar))
    print(f"spline against Gaussian: e = {e:.2e}, worst |a - o| / bar = {ratio:.3f}, largest gap {float(np.max(np.abs(a - o))):.2e}")
    assert ratio <= 1.0, ratio
    assert float(np.max(np.abs(a - o))) > 0.0                                             # (two kernels, not one)


# ------------------------------------------------------------------------------------------------------------ 7: graph
def test_prepare_and_surface_record_into_a_graph(pkg, gpu):
    rows, cols = 100, 150
    g = lists_mirror(rows, cols)
    u, phase, *_ = lists_case(rows, cols)
    dm = make_dm(pkg, g, "oomao0.1")
    ud, pd = torch.from_numpy(u[:3].copy()).to(gpu), planes(phase[:3], gpu)
    out = torch.zeros_like(pd)
    run = lambda: (dm.prepare(), dm.surface(ud, phase=pd, out=out))
    run()                                                     # eager, also the warm-up
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        run()
    for k in range(3):
        ud.copy_(torch.from_numpy(u[k:k + 3] * (1.0 + k)).to(gpu))
        want = dm.surface(ud, phase=pd)
        dm.ws.zero_(); out.zero_()                            # the replay prepares the mirror again
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), k


# ------------------------------------------------------------------------------------------------------------ 8: the loop
def test_loop_with_the_spline_mirror(pkg, gpu):
    """AOLoop(dm=SplineDM) against the same steps composed by hand from dm.surface, and the loop without dm against the hand
    composition with fmpc_phase_residual_device: u and ad_est bit for bit (as test_gpu_dm.test_loop_with_and_without_the_mirror)."""
    from tests.test_gpu_dm import hand_loop
    from tests.util import handle_from_model
    R, steps, L = 2, 3, 64
    opt = pkg.reference_optics(L)
    dm = pkg.oomao_dm(12, L, 0.3)
    assert (dm.rows, dm.cols, dm.m) == (L, L, 144)
    md = pkg.synthetic.make_model(27, 144, 10)
    rng = np.random.default_rng(4)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    Zc = opt.Z[1:].contiguous()
    phase = torch.tensordot(torch.from_numpy(a).to(gpu), Zc, dims=1) + 0.01 * torch.from_numpy(rng.standard_normal((steps, R, L, L))).to(gpu)
    npx = L * L
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def modal_residual(h):
        def f(s, ph, u1):
            scrn = torch.empty_like(ph)
            rc = h._lib.fmpc_phase_residual_device(h._h, R, npx, vp(ph), vp(u1) if s >= 1 else None, vp(Zc), vp(scrn),
                                                   C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
            assert rc == 0
            return scrn
        return f

    zonal_residual = lambda s, ph, u1: dm.surface(u1, phase=ph) if s >= 1 else ph.clone()
    runs = {}
    for which in ("loop-dm", "hand-dm", "loop", "hand"):
        h = handle_from_model(pkg, md)
        est = opt.estimator(opt.Z, skip=1)
        if which.startswith("loop"):
            kw = dict(dm=dm) if which == "loop-dm" else {}
            if kw:
                with pytest.raises(ValueError):                                           # a mirror on another grid
                    pkg.AOLoop(h, est, Zc, R, dm=pkg.oomao_dm(12, 128, 0.3), z_colmajor=True)
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True, **kw)
            seen = []
            for s in range(steps):
                uu, x0 = loop.step(phase[s], colmajor=True)
                seen.append((uu.clone(), x0.clone()))
        else:
            seen = hand_loop(pkg, gpu, h, est, R, [phase[s] for s in range(steps)], zonal_residual if which == "hand-dm" else modal_residual(h))
        torch.cuda.synchronize()
        runs[which] = seen
        est.close(); h.close()
    for a_, b_ in (("loop-dm", "hand-dm"), ("loop", "hand")):
        for s, ((u0, x0), (u1, x1)) in enumerate(zip(runs[a_], runs[b_])):
            assert torch.equal(u0, u1) and torch.equal(x0, x1), (a_, s)
    assert not torch.equal(runs["loop-dm"][1][1], runs["loop"][1][1])
    assert torch.equal(runs["loop-dm"][0][0], runs["loop"][0][0])                         # (no correction before the first move)
    opt.close()
