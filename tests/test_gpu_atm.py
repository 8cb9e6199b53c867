"""The atmosphere on the device (include/fastmpc.h: fmpc_atm, atmosphere.py) against its numpy restatement tests/atm_ref.py, which
takes the device's own operands (fmpc_atm_extruder_host) and the library's host draw.  Lattice pitch 1 and dt 1, so that a wind
speed is a pixel step."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import atm_ref as ar

pytestmark = pytest.mark.gpu

R0, L0 = 3.0, 600.0
EPS = 2.0 ** -52
_EXT = {}


def _ext(pkg, W, stencil):
    key = (W, tuple(stencil))
    if key not in _EXT:
        _EXT[key] = ar.extruders_lib(pkg, W, 1.0, R0, L0, list(stencil))
    return _EXT[key]


def _pair(pkg, W, stencil, winds, frac, batch, seed=11, first=0, dtype=np.longdouble, reverse=False, ref=True):
    """An `Atmosphere` with pitch 1, dt 1 and the winds (vx, vy) in pixels per step, and its restatement."""
    st = ar.default_stencil(W) if stencil is None else list(stencil)
    speed = [math.hypot(vx, vy) for vx, vy in winds]
    direc = [math.atan2(vy, vx) for vx, vy in winds]
    atm = pkg.Atmosphere(R0, L0, frac, speed, direc, W - 1, float(W - 2), 1.0, batch, seed, first=first, stencil=stencil)
    assert atm.pitch == 1.0 and atm.stencil == st
    if not ref:
        return atm, None
    vpx, vpy = ar.pixels_per_step(speed, direc, 1.0, 1.0)
    return atm, ar.AtmRef(W, st, _ext(pkg, W, st), frac, vpx, vpy, batch, ar.xi_lib(pkg, seed, batch, W, first), dtype=dtype, reverse=reverse)


def _dev_state(atm):
    import torch
    st = atm.state()
    torch.cuda.synchronize()
    return dict(windows=st["windows"].cpu().numpy(), k=st["k"], counts=st["counts"])


# winds of every quadrant, along one axis only and a still layer; pixel steps 0.3, 1.0 and 2.6
CASES = [
    (18, [1, 2], [(1.0, 0.0)], [1.0], 1, 0),
    (18, [1, 2, 17], [(-1.0, 0.0), (0.0, 1.0), (0.0, 0.0)], [0.5, 0.3, 0.2], 17, 0),
    (33, None, [(1.2, 1.2), (-1.2, 1.2), (1.2, -1.2)], [0.028, 0.004, 0.008], 40, 0),
    (33, [1, 2], [(-0.3, -0.3)], [1.0], 17, 3),            # the lines enter at the fourth step of 0.3 pixels
]


def one_extrusion(atm, ref, st):
    """Both sides load the state `st`, take one step and are compared; `ref` is the long double restatement of `atm`."""
    k0 = st["k"]
    ref.load_state(st)
    atm.load_state(st)
    got0 = _dev_state(atm)
    assert np.array_equal(got0["windows"], st["windows"]) and got0["k"] == k0 and got0["counts"] == list(st["counts"])
    ref.clear_tol()
    ref.advance(1)
    atm.advance(1)
    got = _dev_state(atm)
    assert got["k"] == k0 + 1 and got["counts"] == ref.e
    new, worst = 0, 0.0
    for l in range(ref.layers):
        want, tol = ref.win[l], ref.tol[l]
        old = tol == 0
        assert np.array_equal(got["windows"][l][old], np.asarray(want, dtype=np.float64)[old])
        err = np.abs(got["windows"][l].astype(np.longdouble) - want)
        assert np.all(err <= tol), float((err - tol).max())
        if (~old).any():
            worst = max(worst, float((err[~old] / tol[~old].clip(1e-300)).max()))
        new += int((~old).sum())
        nx, ny = (ar.displacement(k0 + 1, v)[0] - ar.displacement(k0, v)[0] for v in (ref.vpx[l], ref.vpy[l]))
        assert nx <= 1 and ny <= 1 and int((~old[0]).sum()) == (nx + ny) * ref.W - nx * ny
    assert new > 0
    print(f"atm W={ref.W} layers={ref.layers} one extrusion: worst error / bound {worst:.3f}")
    return got


@pytest.mark.parametrize("W,stencil,winds,frac,batch,k0", CASES)
def test_one_extrusion_per_axis_against_long_double(pkg, gpu, W, stencil, winds, frac, batch, k0):
    """set_state from the restatement's start-up, one step, get_state: a new line entry lies within (q + 1) W 2^-52 (sum |A||z| +
    sqrt(f) sum |B||xi|) of the long double restatement, every other sample is the one it was, moved by one, bit for bit, and the
    dropped line is gone (the whole window is compared)."""
    atm, ref = _pair(pkg, W, stencil, winds, frac, batch)
    ref.reset()
    st = ref.state()
    st["k"] = k0
    one_extrusion(atm, ref, st)
    atm.close()


RUNS = [
    (18, [1, 2, 17], [(0.3, -2.6), (-1.0, 0.3), (0.0, 0.0)], [0.5, 0.3, 0.2], 17),
    (33, None, [(2.6, 1.0), (-0.3, -1.0), (-2.6, 0.3)], [0.028, 0.004, 0.008], 40),
    (129, None, [(1.0, -2.6)], [0.04], 1),
    # more than twelve row tiles, so that a wavefront takes a second pass over the operands: 14 tiles with W % 4 = 1 and a far
    # line whose gather wraps the ring, 16 full tiles
    (209, [1, 2, 208], [(2.6, -1.0), (-1.0, 2.6)], [0.6, 0.4], 3),
    (256, [1, 2, 255], [(-1.0, -2.6), (2.6, -1.0)], [0.6, 0.4], 3),
]


@pytest.mark.parametrize("W,stencil,winds,frac,batch", RUNS)
def test_start_up_and_forty_steps_against_the_restatement(pkg, gpu, W, stencil, winds, frac, batch):
    """The windows after the start-up and after 40 steps.  The error of the recursion is not derived line by line; the yardstick is
    measured: the restatement in float64 with every sum taken from the far end, against the restatement in long double, gives
    a spread (its maximum over the samples of all windows).  The matrix cores sum in a third order, and the device's draw differs
    from the host's in the last bit of a few xi, so the device must stay within 8 x that spread of the long double windows.
    Measured on one MI355X (spread, device), after the start-up / after the run:
        W = 18, 3 layers, 17 realisations:   8.1e-14, 1.3e-13 / 1.8e-13, 8.8e-13   (window rms 14 rad)
        W = 33, 3 layers, 40 realisations:   5.2e-14, 1.2e-13 / 7.1e-14, 2.4e-13   (rms 2.9)
        W = 129, 1 layer, 1 realisation:     6.4e-14, 2.8e-13 / 1.0e-13, 3.2e-13   (rms 4.6; 8 steps)
        W = 209, 2 layers, 3 realisations:   5.9e-13, 1.1e-12 / 5.3e-13, 1.1e-12   (rms 13.8; 8 steps; lines 1, 2, 208)
        W = 256, 2 layers, 3 realisations:   9.7e-13, 1.5e-12 / 1.0e-12, 1.5e-12   (rms 13.4; 8 steps; lines 1, 2, 255)
    i.e. the device at 1.5 to 4.8 times the spread."""
    steps = 40 if W < 129 else 8                           # (W >= 129 is there for the tiles of a line, not for the length)
    atm, ld = _pair(pkg, W, stencil, winds, frac, batch)
    rv = ar.AtmRef(W, ld.s, ld.ext, frac, ld.vpx, ld.vpy, batch, ld.xi, dtype=np.float64, reverse=True)
    atm.reset()
    ld.reset(); rv.reset()
    for stage in ("start-up", "run"):
        if stage == "run":
            atm.advance(steps); ld.advance(steps); rv.advance(steps)
        got = _dev_state(atm)
        assert got["k"] == ld.k and got["counts"] == ld.e
        want = np.stack(ld.win)
        spread = float(np.abs(np.stack(rv.win).astype(np.longdouble) - want).max())
        err = float(np.abs(got["windows"].astype(np.longdouble) - want).max())
        print(f"atm W={W} {stage}: spread {spread:.3e} device {err:.3e} rms {float(np.sqrt((want.astype(np.float64) ** 2).mean())):.3e}")
        assert spread > 0 and err <= 8 * spread, (stage, err, spread)
    atm.close()


def _disk(n):
    x = (np.arange(n) - (n - 1) / 2.0) / ((n - 1) / 2.0)
    return (x[:, None] ** 2 + x[None, :] ** 2 <= 1.0).astype(np.float64)


def screens_against_the_restatement(atm, ref, sizes, masks=(None, "disk")):
    """The screens of `atm` at every out_len of `sizes` and every mask (None, "disk" or an array) against `ref`, the long double
    restatement that holds the device's own windows; the bound of test_output_against_the_restatement.  Returns the worst error
    over bound."""
    import torch
    layers, worst = ref.layers, 0.0
    for n in sizes:
        for mask in masks:
            mask = _disk(n) if isinstance(mask, str) else mask
            got = atm.screen(n, mask=mask)
            got4 = atm.screen(n, mask=mask, scale=4.0)
            torch.cuda.synchronize()
            got, got4 = got.cpu().numpy(), got4.cpu().numpy()
            want, ab, S = ref.screen(n, mask=mask, want_abs=True)
            tol = (8 + layers) * EPS * ab
            if mask is not None:
                cnt = mask.sum()
                tol = tol + cnt * EPS * (np.abs(np.asarray(S, dtype=np.float64)) * mask).sum(axis=(1, 2))[:, None, None] / max(cnt, 1.0)
                assert np.all(got[:, mask == 0] == 0.0)
            err = np.abs(got.astype(np.longdouble) - want)
            assert np.all(err <= tol), (n, mask is not None, float((err / tol.clip(1e-300)).max()))
            assert np.array_equal(got4, 4.0 * got)
            if mask is None or mask.sum() > 1:               # (a mask of no pixel or of one gives zeros everywhere)
                assert np.abs(got).max() > 0
            worst = max(worst, float((err / tol.clip(1e-300)).max()))
    return worst


@pytest.mark.parametrize("W,stencil,winds,frac,batch,steps", [
    (18, [1, 2], [(0.3, -2.6), (-1.0, 0.3), (0.0, 0.0)], [0.5, 0.3, 0.2], 17, 3),
    (33, None, [(2.6, 1.0)], [1.0], 40, 2),
    (33, None, [(-0.3, -1.0), (1.0, 0.0), (0.3, 2.6)], [0.028, 0.004, 0.008], 1, 5),
])
def test_output_against_the_restatement(pkg, gpu, W, stencil, winds, frac, batch, steps):
    """Screens at out_len = W - 1, 20 and 64, with and without a mask, from the device's own windows.  Per pixel within (8 + layers)
    2^-52 sum_l |four samples| -- three products and sums per layer with weights in [0, 1], the layer sum, the mean's
    subtraction and the scale -- plus, with a mask, npix_mask 2^-52 mean|phi| for the mean's sum; masked pixels are exactly
    zero; a power-of-two scale is exact."""
    atm, ref = _pair(pkg, W, stencil, winds, frac, batch, dtype=np.longdouble)
    atm.reset().advance(steps)
    ref.load_state(_dev_state(atm))
    screens_against_the_restatement(atm, ref, (W - 1, 20, 64))
    atm.close()


def test_a_realisation_does_not_depend_on_the_batch_or_on_first(pkg, gpu):
    """Screens of the realisations with the global indices 5 .. 44: in a batch of 40, alone, and in a batch whose `first` differs
    (so that they sit in other columns of other groups), and in batches of exactly one and two groups of 16 -- the same bits;
    another seed gives other screens."""
    import torch
    W, winds, frac = 33, [(2.6, 1.0), (-0.3, -1.0), (-2.6, 0.3)], [0.028, 0.004, 0.008]
    mask = _disk(20)

    def run(batch, first, seed=11):
        atm, _ = _pair(pkg, W, None, winds, frac, batch, seed=seed, first=first, ref=False)
        atm.reset()
        out = [atm.step(20, mask=mask).clone() for _ in range(4)]
        torch.cuda.synchronize()
        atm.close()
        return torch.stack(out).cpu().numpy()                 # (4, batch, 20, 20)

    a = run(40, 5)
    assert np.array_equal(run(40, 5), a)                     # two objects with the same seed
    assert np.array_equal(run(1, 5 + 23)[:, 0], a[:, 23])
    b = run(17, 2)                                           # global 5 is column 3 there
    assert np.array_equal(b[:, 3:], a[:, :14])
    for full in (16, 32):                                    # whole groups of 16: no column of the last group is idle
        assert np.array_equal(run(full, 5), a[:, :full])
    c = run(40, 5, seed=12)
    assert not np.array_equal(c, a) and np.abs(c - a).max() > 1e-3


def test_advance_three_is_three_times_one_and_a_state_round_trip_continues(pkg, gpu):
    import torch
    W, winds, frac = 18, [(0.3, -2.6), (-1.0, 0.3), (0.7, 0.0)], [0.5, 0.3, 0.2]
    a, _ = _pair(pkg, W, [1, 2, 17], winds, frac, 17, ref=False)
    b, _ = _pair(pkg, W, [1, 2, 17], winds, frac, 17, ref=False)
    c, _ = _pair(pkg, W, [1, 2, 17], winds, frac, 17, seed=11, ref=False)
    a.reset().advance(3)
    b.reset().advance(1).advance(1).advance(1)
    sa, sb = _dev_state(a), _dev_state(b)
    assert sa["k"] == sb["k"] == 3 and sa["counts"] == sb["counts"] and np.array_equal(sa["windows"], sb["windows"])
    c.load_state(a.state())                                  # c was never started: everything comes from the state
    sc = _dev_state(c)
    assert sc["k"] == 3 and sc["counts"] == sa["counts"] and np.array_equal(sc["windows"], sa["windows"])
    xa = [a.step(20).clone() for _ in range(5)]
    xc = [c.step(20).clone() for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(xa, xc))
    assert not torch.equal(xa[0], xa[1])
    for o in (a, b, c):
        o.close()


def test_reference_chain_into_the_var_fit_and_the_loop(pkg, gpu):
    """reference_atmosphere at npix 32 -> series(60, ModalFit) -> identify_var_device gives finite A1, A2; AOLoop.step takes
    what step(out_len=64) returns."""
    import torch
    from tests.util import handle_from_model
    op = pkg.synthetic.estimator_optics(64)
    atm = pkg.reference_atmosphere(4, 3, npix=32)
    assert atm.W == 33 and atm.layers == 3 and atm.stencil == [1, 2, 4, 8, 16, 32]
    atm.reset()
    Z = torch.from_numpy(np.ascontiguousarray(op["Z"][:10])).to(gpu)
    mf = pkg.ModalFit(Z)
    pupil = op["pupil"]
    ser = atm.series(60, mf, skip=1, mask=pupil)
    assert tuple(ser.shape) == (4, 60, 9) and ser.is_contiguous()
    A1, A2, st = pkg.identify_var_device(ser, order=2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(A1).all()) and bool(torch.isfinite(A2).all()) and bool(torch.isfinite(ser).all())
    assert float(ser.abs().max()) > 0 and atm.k == 60
    md = pkg.synthetic.make_model(27, 144, 10)
    h = handle_from_model(pkg, md)
    est = pkg.PhaseDiversityEstimator(op["pupil"], op["W"], op["zd_list"], op["dx"], op["range_min"] + 1, op["range_max"] + 1, op["A_s"], op["b_s"])
    loop = pkg.AOLoop(h, est, op["Z"][1:], 4, n_newton=1, k=1e-2)
    u, x0 = loop.step(atm.step(out_len=64, mask=pupil, scale=0.05))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(x0).all())
    est.close(); h.close(); atm.close()


def test_refused_calls_leave_the_state_and_the_output_untouched(pkg, gpu):
    import torch
    lib = pkg.load()
    atm, _ = _pair(pkg, 18, [1, 2], [(1e6, 0.0)], [1.0], 3, ref=False)       # 1e6 pixels per step: the limit is 2^20
    atm.reset().advance(2)
    before = _dev_state(atm)
    out = torch.full((3, 20, 20), 7.0, dtype=torch.float64, device=gpu)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(pkg.FastMPCError) as e:
        atm.advance(2 ** 40)                                  # 2^40 x 1e6 pixels: beyond 2^52
    assert e.value.code == pkg.FMPC_E_UNSUPPORTED
    assert lib.fmpc_atm_screen_device(atm._h, 70000, None, 1.0, C.c_void_p(out.data_ptr()), s) == pkg.FMPC_E_UNSUPPORTED
    assert lib.fmpc_atm_screen_device(atm._h, 1, None, 1.0, C.c_void_p(out.data_ptr()), s) == pkg.FMPC_E_DIM
    assert lib.fmpc_atm_set_state(atm._h, None, 2 ** 50, None, s) == pkg.FMPC_E_UNSUPPORTED
    assert lib.fmpc_atm_advance_device(atm._h, -1, s) == pkg.FMPC_E_DIM
    after = _dev_state(atm)
    assert after["k"] == before["k"] == 2 and after["counts"] == before["counts"] and np.array_equal(after["windows"], before["windows"])
    assert bool((out == 7.0).all())
    # limits of create: found on the host, no handle comes back
    h = C.c_void_p(1)
    one = (C.c_double * 1)(1.0)
    big = (C.c_double * 1)(2.0 ** 21)
    zero = (C.c_double * 1)(0.0)
    nine = (C.c_int * 9)(*range(1, 10))
    assert lib.fmpc_atm_create(C.byref(h), 18, 1.0, R0, L0, 1, one, one, zero, 1.0, 9, nine, 1, 0, 0, 0) == pkg.FMPC_E_UNSUPPORTED and not h.value
    assert lib.fmpc_atm_create(C.byref(h), 1025, 1.0, R0, L0, 1, one, one, zero, 1.0, 5, nine, 1, 0, 0, 0) == pkg.FMPC_E_UNSUPPORTED
    assert lib.fmpc_atm_create(C.byref(h), 18, 1.0, R0, L0, 1, one, big, zero, 1.0, 2, nine, 1, 0, 0, 0) == pkg.FMPC_E_UNSUPPORTED
    atm.close()
