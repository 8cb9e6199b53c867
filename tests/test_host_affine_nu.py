"""The u rows of the affine cold-start step through nu+ (csrc/fmpc_kernel_affine_nu.hip), host side, through the debug exports of
csrc/fmpc_host.cpp; no GPU needed.

The tile plan (fmpc_host_plan_nu): every 16-row tile of z is a u tile of one stage j >= 1 (wholly inside that stage's u rows) or a
direct tile; stage item j owns the tiles whose first row lies in stage j and splits into parts.  Checked against a restatement of
the rule in this file.

The factorisation (fmpc_host_build_affine): the u-tile images [diag(wc) B' | umid - wc o cu] times the padded [J_j | nuc_j] images are
the same map as the u rows of [Kz | zc].  Both are built in long double from the same inputs and every image entry is rounded to
double once (J and nuc ARE doubles), so per entry |G nu - Kz| <= 3 eps (sum_r |G_r| |nu_rc| + |a|): half an eps per rounded entry of
G, half an eps for the rounding of Kz itself, the rest is margin.  The test prints the worst ratio to that bound."""
import ctypes as C
import importlib

import numpy as np
import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")

SHAPES = [(144, 27, 30), (144, 27, 3), (144, 27, 1), (5, 27, 4), (16, 27, 17), (17, 27, 33)]
KS, NU_KS, KC = 14, 7, 56


def plan_nu(m, n, T, W=64):
    lib = pkg._lib.load()
    fn = lib.fmpc_debug_plan_nu
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    out = (C.c_int * (4 * T))()
    parts, swap = C.c_int(-1), C.c_int(-1)
    assert fn(m, n, T, W, out, C.byref(parts), C.byref(swap)) == 0
    return [tuple(out[4 * j:4 * j + 4]) for j in range(T)], parts.value, swap.value


def cut(cnt, p, parts):
    """The share [b, e) of cnt tiles that part p of `parts` takes: the library's own cut, as the kernel applies it."""
    lib = pkg._lib.load()
    fn = lib.fmpc_debug_nu_cut
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    b, e = C.c_int(-1), C.c_int(-1)
    assert fn(cnt, p, parts, C.byref(b), C.byref(e)) == 0
    return b.value, e.value


def kind_of_tile(t, m, n, T):
    """The rule as the design states it: ('u', j) or ('d', stage of the first row)."""
    s, rows = n + m, T * (n + m)
    first, last = 16 * t, min(16 * t + 15, rows - 1)
    j = first // s
    if j >= 1 and 16 * t + 16 <= rows and first >= j * s and 16 * t + 15 < j * s + m:
        return ("u", j)
    assert last >= first
    return ("d", j)


@pytest.mark.parametrize("m,n,T", SHAPES)
def test_tile_plan(m, n, T):
    s, rows = n + m, T * (n + m)
    tiles = (rows + 15) // 16
    plan, _, _ = plan_nu(m, n, T)
    seen, nut = {}, 0
    for j, (tb, nu, nd, ub) in enumerate(plan):
        assert ub == nut                                           # u-tile images in row order
        nut += nu
        for t in range(tb, tb + nu):
            assert t not in seen
            seen[t] = ("u", j)
            assert j >= 1 and j * s <= 16 * t and 16 * t + 16 <= j * s + m     # wholly inside the u rows of stage j >= 1
        for t in range(tb + nu, tb + nu + nd):
            assert t not in seen
            seen[t] = ("d", j)
            assert j * s <= 16 * t < (j + 1) * s                               # its first row lies in stage j
    assert sorted(seen) == list(range(tiles))                      # every tile, hence every row of z, exactly once
    assert plan[0][1] == 0                                         # stage 0 has no u tile
    for t in range(tiles):
        assert seen[t] == kind_of_tile(t, m, n, T), t              # (and no tile that could be a u tile is left direct)
    # items and parts, through the library's own cut: consecutive, disjoint shares that cover the item's u tiles and its direct tiles
    for P in (1, 2, 3):
        got = []
        for tb, nu, nd, ub in plan:
            for cnt, first in ((nu, tb), (nd, tb + nu)):
                edges = [cut(cnt, p, P) for p in range(P)]
                assert edges[0][0] == 0 and edges[-1][1] == cnt and all(edges[p][1] == edges[p + 1][0] for p in range(P - 1))
                for b_, e_ in edges:
                    assert b_ <= e_
                    got += list(range(first + b_, first + e_))
        assert sorted(got) == list(range(tiles)), P


def test_tile_plan_at_the_headline_size():
    plan, _, _ = plan_nu(144, 27, 30)
    assert sum(p[1] for p in plan) == 233 and sum(p[2] for p in plan) == 88
    assert sorted((171 * j) % 16 for j in range(16)) == list(range(16))        # the stages' offsets: all sixteen residues
    assert {(171 * j) % 16 for j in range(30)} == set(range(16))
    assert plan[0] == (0, 0, 11, 0) and plan[16][:3] == (171, 9, 2)            # stage 16 starts on a tile: 9 u tiles
    # parts per item: a single call at 2000 problems has 64 wavefronts per group, the bench's four lanes 16; stage 0 then changes
    # places with stage 15, the item of the last wavefront, which has one item where the first fourteen have two
    assert plan_nu(144, 27, 30, 64)[1:] == (2, 0)
    assert plan_nu(144, 27, 30, 16)[1:] == (1, 15)
    for W in (1, 4, 7, 16, 30, 31, 64, 324):
        _, parts, swap = plan_nu(144, 27, 30, W)
        assert 1 <= parts <= 8 and 0 <= swap < 30 and (swap == 0 or parts == 1)


def _build(T, nb, has_xf, seed):
    n, m = 27, 144
    rng = np.random.default_rng(seed)
    umid = 0.1 * rng.standard_normal(m)
    a = dict(bt=rng.standard_normal((m, n)), umax=umid + rng.uniform(0.3, 2.0, m), umin=umid - rng.uniform(0.3, 2.0, m), umid=umid,
             xmid=0.1 * rng.standard_normal(n), R2=rng.uniform(0.5, 3.0, m), rl=rng.standard_normal(m), Q2=rng.uniform(0.5, 3.0, n),
             Qf2=rng.uniform(0.5, 3.0, n), ql=rng.standard_normal(n), qfl=rng.standard_normal(n), a1=0.3 * rng.standard_normal((n, n)),
             a2=0.2 * rng.standard_normal((n, n)), J=rng.standard_normal((nb * n, 2 * n)), nuc=rng.standard_normal(nb * n))
    order = ["bt", "umax", "umin", "umid", "xmid", "R2", "rl", "Q2", "Qf2", "ql", "qfl", "a1", "a2", "J", "nuc"]
    keep = [np.ascontiguousarray(a[k], dtype=np.float64) for k in order]
    ptrs = (C.POINTER(C.c_double) * len(keep))(*[x.ctypes.data_as(C.POINTER(C.c_double)) for x in keep])
    rows = T * (n + m)
    plan, _, _ = plan_nu(m, n, T)
    nut = sum(p[1] for p in plan)
    Kz = np.zeros((rows, KC)); imgJ = np.zeros((2 * (T - 1), KS, 64)); imgG = np.zeros((nut, NU_KS, 64))
    lib = pkg._lib.load()
    fn = lib.fmpc_debug_build_affine_nu
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    k = 1e-2
    assert fn(n, m, T, nb, has_xf, k, C.cast(ptrs, C.c_void_p), Kz.ctypes.data, imgJ.ctypes.data, imgG.ctypes.data) == nut
    return a, plan, Kz, imgJ, imgG, k


@pytest.mark.parametrize("T,has_xf", [(3, 0), (4, 1), (30, 0)])
def test_u_tile_images_times_the_stage_images_are_the_u_rows_of_kz(T, has_xf):
    n, m = 27, 144
    a, plan, Kz, imgJ, imgG, k = _build(T, T + has_xf, has_xf, seed=11 + T)
    eps = 2.0 ** -52
    worst = 0.0
    for j, (tb, nu, nd, ub) in enumerate(plan):
        if nu == 0:
            continue
        # the 32 padded rows of stage j from its two images: lane 16 g + r of k-step q holds [16 t' + r][4 q + g]
        Jp = imgJ[2 * (j - 1):2 * j].reshape(2, KS, 4, 16).transpose(0, 3, 1, 2).reshape(32, KC)
        assert np.array_equal(Jp[:n, :2 * n], a["J"][j * n:(j + 1) * n]) and np.array_equal(Jp[:n, 2 * n], a["nuc"][j * n:(j + 1) * n])
        unit = np.zeros(KC); unit[2 * n] = 1.0
        assert np.array_equal(Jp[n], unit) and not Jp[n + 1:].any() and not Jp[:, 2 * n + 1].any()
        nuv = Jp[:n + 1].astype(np.longdouble)                     # [nu+_j ; 1] as a map of [d ; 1]
        for u in range(nu):
            G = imgG[ub + u].reshape(NU_KS, 4, 16).transpose(2, 0, 1).reshape(16, 4 * NU_KS).astype(np.longdouble)
            got = G @ nuv
            bound = 3.0 * eps * (np.abs(G) @ np.abs(nuv))          # (the term of the constant, |a| x 1, is part of the sum)
            want = Kz[16 * (tb + u):16 * (tb + u) + 16].astype(np.longdouble)
            assert not want[:, 2 * n + 1].any()
            ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
            ratio[(got == want)] = 0.0
            worst = max(worst, float(ratio.max()))
    print("worst |G nu - Kz| / bound = %.3f" % worst)
    assert worst <= 1.0
    # the constant column of a u-tile image is umid - wc o cu in long double, rounded once
    tb, nu, nd, ub = plan[1]
    rows = np.arange(16 * tb, 16 * tb + 16) - (n + m)
    ld = np.longdouble
    dp = 1 / (ld(1) * a["umax"][rows] - a["umid"][rows]); dm = 1 / (ld(1) * a["umid"][rows] - a["umin"][rows])
    cu = ld(1) * a["R2"][rows] * a["umid"][rows] + a["rl"][rows] + ld(k) * (dp - dm)
    wc = 1 / (ld(1) * a["R2"][rows] + ld(k) * (dp * dp + dm * dm))
    G = imgG[ub].reshape(NU_KS, 4, 16).transpose(2, 0, 1).reshape(16, 4 * NU_KS)
    assert np.array_equal(G[:, n], (a["umid"][rows] - wc * cu).astype(np.float64))
