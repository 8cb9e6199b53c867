"""GPU tests of the refinement with a held Jacobian and of its gain form (fmpc_est_refine_hold_device; fer_gain_step in
fmpc_kernel_est_refine.hip; EstimatorOptics.refine(refresh=, G=), EstimatorOptics.gain, AOLoop(refine=dict(refresh=, G=))) against
the numpy restatement tests/est_refine_hold_ref.py, which tests/test_est_refine_hold_ref.py pins.  Setup, helpers and tolerances
are those of tests/test_gpu_est_refine.py: len 64, the device's own maps, Y made by the restatement from a true alpha, the start
the linear estimate; alpha and ||delta|| 1e-8 max(1, ||alpha_ref||), costs 1e-8 relative plus 1e-20 ||Y||^2, iterations and
status equal.

A condition, not a measurement: device and restatement are compared only where the restatement itself contracts -- the worst
ratio of the errors of consecutive held or gain iterations (hr.contraction) is <= 0.5, so that rounding differences do not grow.
Every parity case asserts it.  Measured on the CPU (5 iterations, per realisation of norm 0.3 / 1.0 or 0.3 / 0.1):
    window (31, 17), 3 div, 27 modes: gain 0.047 / 0.430, held 0.007 / 0.088 (0.017 / 0.080 with damping 1e-3)
    window (32, 16), 3 div, 27 modes at 0.3: gain 0.050, held 0.006      (9, 28), 3 div, 5 modes: gain 0.027 / 0.296, held 0.001 / 0.054
    (9, 28), 1 div, 1 mode: gain 0.054 / 0.365, held 0.001 / 0.055       (31, 17), 1 div, 17 modes at 0.3 / 0.1: gain 0.114 / 0.024, held 0.007
    (31, 17), 3 div, 64 modes at 0.3: gain 0.035, held 0.004             (32, 16), 1 div, 5 modes at 0.3 / 0.1: gain 0.071 / 0.025, held 0.001
||alpha|| = 2 is left out: its ratio is 0.59 with refresh 2 and 0.72 with refresh 3 (0.94 in the gain form, which diverges)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import est_refine_hold_ref as hr
from tests import est_refine_ref as rr
from tests import test_gpu_est_refine as base
from tests.test_gpu_est_refine import check_against, dev, geometry, optics, problem, same_bits, select

pytestmark = pytest.mark.gpu
L = base.L
ONCE = 1000                                                      # refresh >= iters: J once


@functools.lru_cache(maxsize=None)
def gain_ref(d, first, ndiv, nmode):
    G = hr.gain(geometry(d, first, ndiv), select(nmode)[1])
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def reference(d, first, ndiv, nmode, norms, iters, refresh, damping=0.0, tol=0.0):
    _, Y, start = problem(d, first, ndiv, nmode, norms)
    G = gain_ref(d, first, ndiv, nmode) if refresh == 0 else None
    return hr.refine(geometry(d, first, ndiv), select(nmode)[1], Y, start, iters, refresh, G, damping, tol)


def run(pkg, gpu, opt, Z, Y, start, iters, refresh, G=None, damping=0.0, tol=0.0, workspace=None):
    """One call of fmpc_est_refine_hold_device on fresh outputs (refresh = 1 included: straight through the C ABI):
    (alpha, info, status) as host arrays."""
    batch, nmode = Y.shape[0], int(Z.shape[0])
    info = torch.full((batch, pkg.FMPC_REFINE_FIELDS), -7.0, dtype=torch.float64, device=gpu)
    status = torch.full((batch,), -7, dtype=torch.int32, device=gpu)
    Yd, alpha = dev(Y, gpu), dev(start, gpu)
    if workspace is None:
        workspace = torch.empty(opt.refine_workspace_bytes(nmode, batch, refresh=refresh), dtype=torch.uint8, device=gpu)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = pkg.load().fmpc_est_refine_hold_device(opt._h, nmode, vp(Z), batch, vp(Yd), opt.p, vp(alpha), iters, refresh, vp(G), opt.p, damping, tol,
                                                vp(info), vp(status), vp(workspace), workspace.numel(),
                                                C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == pkg.FMPC_OK, rc
    torch.cuda.synchronize()
    return alpha.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy()


def all_same(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y))


PARITY = [  # d, first, ndiv, nmode, norms (one realisation each), damping, the schedules
    (31, 17, 3, 27, (0.3, 1.0), 0.0, (0, 2, 3, ONCE)),
    (31, 17, 3, 27, (0.3, 1.0), 1e-3, (2,)),
    (32, 16, 3, 27, (0.3,), 0.0, (0, 2, 3, ONCE)),
    (9, 28, 3, 5, (0.3, 1.0), 0.0, (0, 2, 3, ONCE)),
    (9, 28, 1, 1, (0.3, 1.0), 0.0, (0, 2, 3, ONCE)),             # p = 81: one row past a multiple of 4
    (9, 28, 1, 1, (0.3, 1.0), 1e-3, (2,)),
    (31, 17, 1, 17, (0.3, 0.1), 0.0, (0, 2, 3, ONCE)),           # p = 961, a second mode tile with one column
    (31, 17, 3, 64, (0.3,), 0.0, (0, 2, 3, ONCE)),               # p = 2883: three rows past; four full mode tiles
    (32, 16, 1, 5, (0.3, 0.1), 0.0, (0, 2, 3, ONCE)),            # p = 1024
]


@pytest.mark.parametrize("d,first,ndiv,nmode,norms,damping,schedules", PARITY)
def test_parity_with_the_restatement(pkg, gpu, d, first, ndiv, nmode, norms, damping, schedules):
    opt = optics(pkg, d, first, ndiv)
    Z = select(nmode)[0]
    a, Y, start = problem(d, first, ndiv, nmode, norms)
    G = dev(gain_ref(d, first, ndiv, nmode), gpu) if 0 in schedules else None
    for refresh in schedules:
        ratio = hr.contraction(reference(d, first, ndiv, nmode, norms, 5, refresh, damping)["alphas"], a, refresh)
        print(f"refresh {refresh}: the restatement contracts by {ratio:.3f}")
        assert ratio <= 0.5, (refresh, ratio)                                             # the condition of the comparison
        for iters in (1, 2, 3, 4, 5):
            alpha, info, status = run(pkg, gpu, opt, Z, Y, start, iters, refresh, G if refresh == 0 else None, damping)
            check_against(reference(d, first, ndiv, nmode, norms, iters, refresh, damping), alpha, info, status, Y, f"refresh {refresh} iters {iters}")
    opt.close()


@pytest.mark.parametrize("d,first,ndiv,nmode,norms,damping", base.CASES)
def test_refresh_one_is_the_existing_call_bit_for_bit(pkg, gpu, d, first, ndiv, nmode, norms, damping):
    opt = optics(pkg, d, first, ndiv)
    Z = select(nmode)[0]
    _, Y, start = problem(d, first, ndiv, nmode, norms)
    for iters, tol in ((1, 0.0), (3, 0.0), (3, 1e-6)):
        want = base.run(pkg, gpu, opt, Z, Y, start, iters, damping, tol)
        assert all_same(want, run(pkg, gpu, opt, Z, Y, start, iters, 1, None, damping, tol)), (iters, tol)
    least = opt.refine_workspace_bytes(nmode, minimum=True)                               # .. and through the field panels
    ws = torch.empty(least + 8, dtype=torch.uint8, device=gpu)
    assert all_same(base.run(pkg, gpu, opt, Z, Y, start, 2, damping), run(pkg, gpu, opt, Z, Y, start, 2, 1, None, damping, workspace=ws))
    opt.close()


MANY = tuple([0.3, 1.0, 0.1] * 11)                               # 33 realisations


@pytest.mark.parametrize("refresh", [0, 2])
def test_a_row_has_the_same_bits_wherever_it_runs(pkg, gpu, refresh):
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, s = problem(*case, MANY)
    G = dev(gain_ref(*case), gpu) if refresh == 0 else None
    go = lambda rows, ws=None: run(pkg, gpu, opt, Z, Y[rows], s[rows], 3, refresh, G, workspace=ws)
    every = np.arange(33)
    full = go(every)
    assert all_same(full, go(every))                                                      # two calls
    for batch in (1, 15, 16, 17):
        assert all_same([x[:batch] for x in full], go(every[:batch])), batch
    for row in (15, 16, 32):                                                              # alone
        assert all_same([x[row:row + 1] for x in full], go(every[row:row + 1])), row
    turned = go(every[::-1])                                                              # every place of the batch, and of a tile
    assert all_same([x[::-1] for x in full], turned)
    shifted = go(np.roll(every, 5))
    assert all_same([np.roll(x, 5, axis=0) for x in full], shifted)
    least, rec = opt.refine_workspace_bytes(27, minimum=True, refresh=refresh), opt.refine_workspace_bytes(27, 33, refresh=refresh)
    one = opt.refine_workspace_bytes(27, 1, refresh=refresh)
    assert 0 < least <= one < rec
    sizes = [least, one, 3 * one + 64, 17 * one + 8, rec] + ([least + 4 * ((one - least) // 27) + 8] if refresh else [])
    for nbytes in sizes:                                                                  # 1, 3, 17 (two tiles, the second with one row) .. at a time
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
        assert all_same(full, go(every, ws)), nbytes
    opt.close()


@pytest.mark.parametrize("refresh", [0, ONCE])
def test_tol_freezes_a_row_inside_a_tile_of_live_ones(pkg, gpu, refresh):
    """Norms 1 / 0.003 / 1 with tol 1e-4: the small one's first step is about 1e-6 and freezes it, the others' third steps are
    6.9e-4 (held) and 1.2e-2 (gain) against the 2e-4 that would stop them."""
    case, norms, tol = (31, 17, 3, 27), (1.0, 0.003, 1.0), 1e-4
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start = problem(*case, norms)
    G = dev(gain_ref(*case), gpu) if refresh == 0 else None
    ref = reference(*case, norms, 3, refresh, 0.0, tol)
    assert ref["info"][:, rr.ITERS].tolist() == [3, 1, 3] and ref["status"].tolist() == [0, rr.CONVERGED, 0]
    alpha, info, status = run(pkg, gpu, opt, Z, Y, start, 3, refresh, G, tol=tol)
    check_against(ref, alpha, info, status, Y, f"tol, refresh {refresh}")
    live = run(pkg, gpu, opt, Z, Y[[0, 2]], start[[0, 2]], 3, refresh, G, tol=tol)        # the live ones without it
    assert all_same([x[[0, 2]] for x in (alpha, info, status)], live)
    once = run(pkg, gpu, opt, Z, Y, start, 1, refresh, G)                                 # the frozen one took one step
    assert same_bits(alpha[1], once[0][1]) and same_bits(info[1, [rr.COST0, rr.COST, rr.STEP]], once[1][1, [rr.COST0, rr.COST, rr.STEP]])
    opt.close()


@pytest.mark.parametrize("refresh", [0, 3])
def test_bad_input_stays_in_its_row_and_nothing_faults(pkg, gpu, refresh):
    """A NaN in Y and a start of 1e7 rad are found in iteration 0; images 1e12 too bright make a first step of more than 1e6 rad,
    which the next iteration -- a held one, or a gain step -- finds.  The neighbours in the tile do not notice."""
    case, norms = (31, 17, 3, 27), (0.3, 1.0, 0.3, 1.0, 0.3, 1.0)
    opt = optics(pkg, *case[:3])
    Z, Zh = select(27)
    a, Y, start = problem(*case, norms)
    G = dev(gain_ref(*case), gpu) if refresh == 0 else None
    good = run(pkg, gpu, opt, Z, Y, start, 3, refresh, G)
    Yb = Y.copy(); Yb[3, 7] = np.nan; Yb[4] *= 1e12
    sb = start.copy(); sb[1] = 1e7 * a[1]
    ref = hr.refine(geometry(*case[:3]), Zh, Yb, sb, 3, refresh, gain_ref(*case) if refresh == 0 else None)
    assert ref["status"].tolist() == [0, rr.BAD_INPUT, 0, rr.BAD_INPUT, rr.BAD_INPUT, 0] and ref["info"][:, rr.ITERS].tolist() == [3, 0, 3, 0, 1, 3]
    for iters in (3, 0):
        alpha, info, status = run(pkg, gpu, opt, Z, Yb, sb, iters, refresh, G)
        bad = [1, 3, 4] if iters else [1, 3]
        assert status.tolist() == [pkg.FMPC_REFINE_BAD_INPUT if b in bad else 0 for b in range(6)], status
        assert np.all(np.isnan(info[bad, :2]))
        if iters:
            assert np.all(np.isnan(alpha[bad])) and info[:, rr.ITERS].tolist() == [3, 0, 3, 0, 1, 3]
            for b in (0, 2, 5):
                assert same_bits(alpha[b], good[0][b]) and same_bits(info[b], good[1][b]), b
        else:
            # (the gain step sums ||r||^2 in its lanes' order, the final pass in fer_cost's: the same cost to rounding)
            assert same_bits(alpha, sb) and same_bits(info[:, rr.COST0], info[:, rr.COST])
            assert np.allclose(info[[0, 2, 5], rr.COST0], good[1][[0, 2, 5], rr.COST0], rtol=1e-12, atol=0.0)
    assert all_same(good, run(pkg, gpu, opt, Z, Y, start, 3, refresh, G))                 # the handle is fine afterwards
    opt.close()


def test_a_map_that_vanishes_fails_the_factorisation_but_not_the_gain_form(pkg, gpu):
    opt = optics(pkg, 31, 17, 3)
    Z, Zh = select(5)
    Z = Z.clone(); Z[2].zero_()
    Zh = Zh.copy(); Zh[2] = 0.0
    a = np.random.default_rng(3).standard_normal((2, 5)); a *= 0.3 / np.linalg.norm(a, axis=1, keepdims=True)
    Y = rr.images(geometry(31, 17, 3), Zh, a)
    start = 0.9 * a
    alpha, info, status = run(pkg, gpu, opt, Z, Y, start, 3, 2)
    assert np.all(status == pkg.FMPC_REFINE_FACTOR_FAILED) and np.all(info[:, rr.ITERS] == 0) and same_bits(alpha, start)
    G = opt.gain(Z)                                                                       # (its row of the vanishing map is zero)
    assert tuple(G.shape) == (5, opt.p) and G.is_contiguous() and float(G[2].abs().max()) <= 1e-12 * float(G.abs().max())
    alpha, info, status = run(pkg, gpu, opt, Z, Y, start, 3, 0, G)
    assert not status.any() and np.all(info[:, rr.ITERS] == 3) and np.all(np.isfinite(alpha)) and np.all(info[:, rr.COST] < info[:, rr.COST0])
    check_against(hr.refine(geometry(31, 17, 3), Zh, Y, start, 3, 0, G.cpu().numpy()), alpha, info, status, Y, "gain form, a vanishing map")
    opt.close()


@pytest.mark.parametrize("refresh", [0, 2])
def test_the_call_records_into_a_graph(pkg, gpu, refresh):
    """No allocation, no synchronisation, no read-back: the call is captured and replayed to the same bits."""
    case, norms = (31, 17, 3, 27), (1.0, 0.3, 0.1)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start = problem(*case, norms)
    G = dev(gain_ref(*case), gpu) if refresh == 0 else None
    eager = run(pkg, gpu, opt, Z, Y, start, 3, refresh, G, tol=1e-6)
    Yd, a0 = dev(Y, gpu), dev(start, gpu)
    out = torch.zeros_like(a0); info = torch.zeros((3, pkg.FMPC_REFINE_FIELDS), dtype=torch.float64, device=gpu)
    status = torch.zeros(3, dtype=torch.int32, device=gpu)
    ws = torch.empty(opt.refine_workspace_bytes(27, 3, refresh=refresh), dtype=torch.uint8, device=gpu)
    call = lambda: opt.refine(Z, Yd, alpha0=a0, out=out, iters=3, tol=1e-6, info=info, status=status, workspace=ws, refresh=refresh, G=G)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    out.zero_(); info.zero_(); status.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), eager[0]) and same_bits(info.cpu().numpy(), eager[1]) and same_bits(status.cpu().numpy(), eager[2])
    opt.close()


def test_python_takes_the_schedule_and_makes_the_gain_itself(pkg, gpu):
    case, norms = (31, 17, 3, 27), (0.3, 1.0)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start = problem(*case, norms)
    G = opt.gain(Z)
    assert tuple(G.shape) == (27, opt.p) and G.is_contiguous() and G.is_cuda and G.dtype == torch.float64
    want = gain_ref(*case)
    assert np.linalg.norm(G.cpu().numpy() - want) <= 1e-8 * np.linalg.norm(want)
    for refresh in (0, 3):
        info = torch.zeros((2, pkg.FMPC_REFINE_FIELDS), dtype=torch.float64, device=gpu); status = torch.zeros(2, dtype=torch.int32, device=gpu)
        alpha = opt.refine(Z, dev(Y, gpu), alpha0=dev(start, gpu), iters=4, refresh=refresh, info=info, status=status)    # G=None: gain(Z)
        torch.cuda.synchronize()
        check_against(reference(*case, norms, 4, refresh), alpha.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy(), Y, f"python, refresh {refresh}")
    assert same_bits(opt.refine(Z, dev(Y, gpu), alpha0=dev(start, gpu), iters=2, refresh=1).cpu().numpy(), base.run(pkg, gpu, opt, Z, Y, start, 2)[0])
    with pytest.raises(pkg.FastMPCError) as e:
        opt.refine(Z, dev(Y, gpu), refresh=0, damping=1e-3, G=G)
    assert e.value.code == pkg.FMPC_E_DIM
    with pytest.raises(pkg.FastMPCError):
        opt.refine(Z, dev(Y, gpu), refresh=0, G=G[:, :-1])
    with pytest.raises(pkg.FastMPCError):
        opt.refine(Z, dev(Y, gpu), refresh=-1)
    opt.close()


@pytest.mark.parametrize("refresh,iters,norm", [(0, 2, 0.3), (3, 3, 1.0)])
def test_loop_refines_its_estimate_with_either_form(pkg, gpu, refresh, iters, norm):
    """AOLoop(refine=dict(refresh=)): x0 of step 0 is closer to the true coefficients than the linear estimate, by what the
    restatement gains on the same inputs: within a factor 4 of its error, plus this file's tolerance for alpha."""
    from tests.util import handle_from_model
    R = 2
    opt = pkg.reference_optics(L)
    Zh = np.ascontiguousarray(np.swapaxes(opt.Z.cpu().numpy(), -1, -2))
    geom = dict(pupil=opt.pupil, W=Zh[4], zd_list=opt.zd_list, dx=opt.dx, rmin=opt.range_min - 1, rmax=opt.range_max - 1, AU=opt.AU)
    md = pkg.synthetic.make_model(27, 144, 10)
    a = np.random.default_rng(8).standard_normal((R, 27))
    a *= norm / np.linalg.norm(a, axis=1, keepdims=True)
    phase = torch.from_numpy(np.tensordot(a, Zh[1:], axes=1)).to(gpu)
    Y = rr.images(geom, Zh[1:], a)
    start = rr.linear_start(geom, Zh[1:], Y)
    ref = hr.refine(geom, Zh[1:], Y, start, iters, refresh)
    e_lin, e_want = np.linalg.norm(start - a, axis=1), np.linalg.norm(ref["alphas"][-1] - a, axis=1)
    h = handle_from_model(pkg, md)
    est = opt.estimator(opt.Z, skip=1)
    loop = pkg.AOLoop(h, est, opt.Z[1:], R, n_newton=1, k=1e-2, z_colmajor=True, refine=dict(optics=opt, iters=iters, refresh=refresh))
    _, x0 = loop.step(phase)
    torch.cuda.synchronize()
    e_got = np.linalg.norm(x0.cpu().numpy() - a, axis=1)
    print(f"refresh {refresh}: linear {e_lin}, the restatement {e_want}, the loop {e_got}")
    assert np.all(e_want < e_lin / 4)                                                     # (there is something to gain)
    assert np.all(e_got <= 4 * e_want + 1e-8 * max(1.0, norm)) and np.all(e_got < e_lin), (e_got, e_want, e_lin)
    assert not bool(loop.refine_status.any()) and bool((loop.refine_info[:, pkg.FMPC_REFINE_ITERS] == iters).all())
    with pytest.raises(ValueError):
        pkg.AOLoop(h, est, opt.Z[1:], R, z_colmajor=True, refine=dict(optics=opt, refresh=2, hold=True))
    with pytest.raises(ValueError):
        pkg.AOLoop(h, est, opt.Z[1:], R, z_colmajor=True, refine=dict(optics=opt, refresh=-1))
    if refresh == 0:                                                                      # a gain handed over is used as it is
        G = opt.gain(opt.Z[1:].contiguous())
        again = pkg.AOLoop(h, est, opt.Z[1:], R, n_newton=1, k=1e-2, z_colmajor=True, refine=dict(optics=opt, iters=iters, refresh=0, G=G))
        _, x1 = again.step(phase)
        torch.cuda.synchronize()
        assert torch.equal(x0, x1)
    est.close(); h.close(); opt.close()


def test_refusals_that_need_a_handle_the_sizes_and_the_empty_calls(pkg, gpu):
    opt = optics(pkg, 31, 17, 3)
    lib, Z = pkg.load(), select(27)[0]
    norms = (1.0, 0.3, 0.1)
    _, Y, start = problem(31, 17, 3, 27, norms)
    Yd, ad, G = dev(Y, gpu), dev(start, gpu), dev(gain_ref(31, 17, 3, 27), gpu)
    size = lambda batch, refresh, nmode=27: int(lib.fmpc_est_refine_hold_workspace_bytes(opt._h, nmode, batch, refresh))
    # the sizes: refresh >= 1 is the existing call's; refresh = 0 is monotone in the batch, a whole number of blocks, below it
    for batch in (0, 1, 2, 15, 16, 17, 100, 128, 129, 5000):
        assert size(batch, 1) == size(batch, 2) == size(batch, ONCE) == int(lib.fmpc_est_refine_workspace_bytes(opt._h, 27, batch))
        for nmode in (1, 27, 64):
            assert 0 < size(batch, 0, nmode) < size(batch, 1, nmode) and size(batch, 0, nmode) % size(1, 0, nmode) == 0
            assert size(batch, 0, nmode) <= size(batch + 1, 0, nmode) and size(batch, 1, nmode) <= size(batch + 1, 1, nmode)
    assert size(0, 0) == size(1, 0) and size(17, 0) == 17 * size(1, 0) and size(5000, 0) == size(128, 0) == 128 * size(1, 0)
    assert size(1, 0) == size(1, 0, 64) and size(1, 0) * 8 < size(1, 1)                   # no J, one slot: an eighth of the block at most
    assert size(1, -1) == 0 and size(1, 0, 65) == 0 and size(-1, 0) == 0
    assert opt.refine_workspace_bytes(27, 40, refresh=0) == size(40, 0) and opt.refine_workspace_bytes(27, 40, minimum=True, refresh=0) == size(1, 0)
    assert opt.refine_workspace_bytes(27, 40, refresh=3) == opt.refine_workspace_bytes(27, 40)
    assert opt.refine_workspace_bytes(27, 40, minimum=True, refresh=3) == opt.refine_workspace_bytes(27, minimum=True)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for refresh in (0, 2):
        least = opt.refine_workspace_bytes(27, minimum=True, refresh=refresh)
        ws = torch.empty(least, dtype=torch.uint8, device=gpu)
        call = lambda batch=3, ldY=opt.p, iters=2, nbytes=least, g=G, ldG=opt.p, damping=0.0: lib.fmpc_est_refine_hold_device(
            opt._h, 27, vp(Z), batch, vp(Yd), ldY, vp(ad), iters, refresh, vp(g), ldG, damping, 0.0, None, None, vp(ws), nbytes, None)
        assert call(ldY=opt.p - 1) == pkg.FMPC_E_DIM and call(nbytes=least - 8) == pkg.FMPC_E_DIM and call(nbytes=0) == pkg.FMPC_E_DIM
        assert call(ldG=opt.p - 1) == (pkg.FMPC_E_DIM if refresh == 0 else pkg.FMPC_OK)   # ldG, G and the damping rule: the gain form's alone
        assert call(g=None) == (pkg.FMPC_E_NULL if refresh == 0 else pkg.FMPC_OK)
        assert call(damping=1e-3) == (pkg.FMPC_E_DIM if refresh == 0 else pkg.FMPC_OK)
        assert call(batch=0) == pkg.FMPC_OK and call(batch=0, ldY=opt.p - 1) == pkg.FMPC_E_DIM
    torch.cuda.synchronize()
    for refresh in (0, 2):
        assert tuple(opt.refine(Z, Yd[:0], refresh=refresh, G=G).shape) == (0, 27)
        alpha, info, status = run(pkg, gpu, opt, Z, Y, start, 0, refresh, G if refresh == 0 else None)      # iters = 0: the costs, alpha left alone
        assert same_bits(alpha, start) and same_bits(info[:, rr.COST0], info[:, rr.COST]) and not status.any()
        assert np.all(info[:, rr.ITERS] == 0) and np.all(info[:, rr.STEP] == 0)
        check_against(reference(31, 17, 3, 27, norms, 0, refresh), alpha, info, status, Y, f"iters 0, refresh {refresh}")
        assert all_same((alpha, info, status), base.run(pkg, gpu, opt, Z, Y, start, 0))
    opt.close()
