"""GPU tests of the refinement weighted by the detector's noise (fmpc_est_refine_weighted_device; fer_step<true>, fer_final<true>
and the sigma pass in fmpc_kernel_est_refine.hip; EstimatorOptics.refine(detector=, floor=, sigma=), AOLoop(refine=dict(weighted=)))
against the numpy restatement tests/est_refine_weighted_ref.py, which tests/test_est_refine_weighted_ref.py pins.  Setup: len 64, the
device's own maps, the cases, detectors (1e5 photo-electrons per call) and noisy images of that file (`detector_read_host`, seeded),
5 realisations of norm 0.3 / 1.0 / 0.1 / 0.3 / 1.0 per case, the start the linear estimate of the noisy images, 3 iterations.

Tolerance on alpha and ||delta||: the unweighted tests' agreement, 2.1e-14 max(1, ||alpha_ref||) at cond(J'J) <= 3.2e2, scaled by
cond(qe^2 J'WJ) / 3.2e2 with the largest condition number of these cases, which the CPU file records (COND = 2.3e2): 1.5e-14.
chi^2 and sigma, scalars made from a model good to 1e-10: 1e-8 relative, the existing tests' rule for the costs.  Measured on one
MI355X over every case: alpha and ||delta|| 6.9e-15, chi^2 1.3e-13, sigma 6.0e-15."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import est_refine_weighted_ref as wr
from tests import test_est_refine_weighted_ref as cpu
from tests import test_gpu_est_refine as base
from tests.test_gpu_est_refine import dev, geometry, optics, same_bits

pytestmark = pytest.mark.gpu
L = base.L
ONCE, NORMS = cpu.ONCE, cpu.NORMS
TOL = 2.1e-14 * cpu.COND / 3.2e2                                 # alpha, ||delta||: see above
WORST = dict(alpha=0.0, chi2=0.0, sigma=0.0)


def select(nmode):
    """(device maps, host maps) of a mode count, chosen as the CPU file chooses them."""
    Z6, Zh6 = base.maps(6)
    Z10, Zh10 = base.maps(10) if nmode in (48, 64) else (None, None)
    return cpu.select(nmode, Z6, Z10).contiguous(), cpu.select(nmode, Zh6, Zh10)


@functools.lru_cache(maxsize=None)
def problem(d, first, ndiv, nmode, kind, norms=NORMS):
    """(true alpha, noisy Y, linear start, detector dict, floor): computed once, shared, read-only."""
    out = cpu.noisy_problem(geometry(d, first, ndiv), select(nmode)[1], norms, kind)
    for v in out[:3]:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(d, first, ndiv, nmode, refresh, kind, iters=3, damping=0.0, tol=0.0):
    _, Y, start, det, floor = problem(d, first, ndiv, nmode, kind)
    return wr.refine(geometry(d, first, ndiv), select(nmode)[1], Y, start, iters, det, floor, refresh, damping, tol)


def noise_of(pkg, det, gpu, gains=None):
    """The DetectorNoise of a detector dict; gains: one per realisation, handed over on the device."""
    gain = det["gain"] if gains is None else torch.from_numpy(np.array(gains, dtype=np.float64)).to(gpu)
    return pkg.DetectorNoise(gain, photon_noise=det["photon_noise"], read_noise=det["read_noise"], qe=det["qe"], background=det["background"])


def run(pkg, gpu, opt, Z, Y, start, iters, refresh, det, floor, damping=0.0, tol=0.0, workspace=None, want_sigma=True, gains=None):
    """One call on fresh outputs: (alpha, info, status, sigma) as host arrays (sigma None when not asked for)."""
    batch, nmode = Y.shape[0], int(Z.shape[0])
    info = torch.full((batch, pkg.FMPC_REFINE_FIELDS), -7.0, dtype=torch.float64, device=gpu)
    status = torch.full((batch,), -7, dtype=torch.int32, device=gpu)
    sigma = torch.full((batch, nmode), -7.0, dtype=torch.float64, device=gpu) if want_sigma else None
    alpha = opt.refine(Z, dev(Y, gpu), alpha0=dev(start, gpu), iters=iters, damping=damping, tol=tol, info=info, status=status, workspace=workspace,
                       refresh=refresh, detector=noise_of(pkg, det, gpu, gains), floor=floor, sigma=sigma)
    torch.cuda.synchronize()
    return alpha.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy(), None if sigma is None else sigma.cpu().numpy()


def all_same(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y) if a is not None and b is not None)


def rows(out, idx):
    return [None if x is None else x[idx] for x in out]


def check_against(ref, alpha, info, status, sigma, what):
    a_ref = ref["alphas"][-1]
    for b in range(len(a_ref)):
        scale = max(1.0, float(np.linalg.norm(a_ref[b])))
        ea = float(np.linalg.norm(alpha[b] - a_ref[b])) / scale
        es = abs(info[b, wr.STEP] - ref["info"][b, wr.STEP]) / scale
        ec = max(abs(info[b, f] - ref["info"][b, f]) / ref["info"][b, f] for f in (wr.COST0, wr.COST))
        eg = float(np.max(np.abs(sigma[b] - ref["sigma"][b]) / ref["sigma"][b]))
        WORST["alpha"] = max(WORST["alpha"], ea, es); WORST["chi2"] = max(WORST["chi2"], ec); WORST["sigma"] = max(WORST["sigma"], eg)
        print(f"{what} row {b}: alpha {ea:.2e}, step {es:.2e}, chi^2 {ec:.2e} ({info[b, 0]:.4e} -> {info[b, 1]:.4e}), sigma {eg:.2e}")
    for b in range(len(a_ref)):
        scale = max(1.0, float(np.linalg.norm(a_ref[b])))
        assert float(np.linalg.norm(alpha[b] - a_ref[b])) / scale <= TOL, (what, b)       # 2.1e-14 x COND / 3.2e2
        assert abs(info[b, wr.STEP] - ref["info"][b, wr.STEP]) / scale <= TOL, (what, b)
        assert all(abs(info[b, f] - ref["info"][b, f]) <= 1e-8 * ref["info"][b, f] for f in (wr.COST0, wr.COST)), (what, b)
        assert np.all(np.abs(sigma[b] - ref["sigma"][b]) <= 1e-8 * ref["sigma"][b]), (what, b)
        assert info[b, wr.ITERS] == ref["info"][b, wr.ITERS] and status[b] == ref["status"][b], (what, b)


@pytest.mark.parametrize("d,first,ndiv,nmode,refresh,kind", cpu.CASES)
def test_parity_with_the_restatement(pkg, gpu, d, first, ndiv, nmode, refresh, kind):
    opt = optics(pkg, d, first, ndiv)
    Z = select(nmode)[0]
    _, Y, start, det, floor = problem(d, first, ndiv, nmode, kind)
    ref = reference(d, first, ndiv, nmode, refresh, kind)
    assert not ref["status"].any() and np.all(ref["info"][:, wr.ITERS] == 3)
    got = run(pkg, gpu, opt, Z, Y, start, 3, refresh, det, floor)
    try:
        check_against(ref, *got, f"{kind}, refresh {refresh}")
    finally:
        print(f"worst so far: alpha {WORST['alpha']:.2e} (tolerance {TOL:.2e}), chi^2 {WORST['chi2']:.2e}, sigma {WORST['sigma']:.2e}")
    opt.close()


def test_damping_and_tol_are_the_unweighted_calls_rules(pkg, gpu):
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start, det, floor = problem(*case, "both")
    ref = reference(*case, 2, "both", 8, 1e-3, 1e-4)             # (the rows stop after 4, 6, 4, 6 and 6 steps)
    assert np.all(ref["status"] == wr.CONVERGED) and len(set(ref["info"][:, wr.ITERS])) > 1 and np.all(ref["info"][:, wr.ITERS] < 8)
    check_against(ref, *run(pkg, gpu, opt, Z, Y, start, 8, 2, det, floor, 1e-3, 1e-4), "damping 1e-3, tol 1e-4")
    opt.close()


def test_a_gain_per_realisation_is_the_scalar_call_of_each_row(pkg, gpu):
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z, Zh = select(27)
    _, Y, start, det, floor = problem(*case, "both")
    gains = det["gain"] * np.array([1.0, 0.5, 2.0, 1.5, 0.25])
    got = run(pkg, gpu, opt, Z, Y, start, 3, 2, det, floor, gains=gains)
    for b in range(5):
        alone = run(pkg, gpu, opt, Z, Y[b:b + 1], start[b:b + 1], 3, 2, dict(det, gain=float(gains[b])), floor)
        assert all_same(rows(got, slice(b, b + 1)), alone), b
    check_against(wr.refine(geometry(*case[:3]), Zh, Y, start, 3, dict(det, gain=gains), floor, 2), *got, "gain_dev")
    opt.close()


MANY = tuple([0.3, 1.0, 0.1] * 5 + [0.3, 1.0])                   # 17 realisations


@pytest.mark.parametrize("refresh", [1, 2])
def test_a_row_has_the_same_bits_wherever_it_runs(pkg, gpu, refresh):
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, s, det, floor = problem(*case, "both", MANY)
    go = lambda idx, ws=None, want_sigma=True: run(pkg, gpu, opt, Z, Y[idx], s[idx], 3, refresh, det, floor, workspace=ws, want_sigma=want_sigma)
    every = np.arange(17)
    full = go(every)
    assert not full[2].any() and np.all(np.isfinite(full[3]))
    assert all_same(full, go(every))                                                      # a second call
    for row in (3, 16):                                                                   # alone, against two places of the batch
        assert all_same(rows(full, slice(row, row + 1)), go(every[row:row + 1])), row
    plain = go(every, want_sigma=False)                                                   # sigma not asked for: alpha, info, status
    assert plain[3] is None and all_same(full[:3], plain[:3])
    rec, least = opt.refine_workspace_bytes(27, 17, refresh=refresh, detector=True), opt.refine_workspace_bytes(27, 17, minimum=True, refresh=refresh, detector=True)
    one = opt.refine_workspace_bytes(27, 1, refresh=refresh, detector=True)
    assert 0 < least < one < rec == 16 * one
    for nbytes in (rec, least, 3 * one + 64):                                             # 16, one field, 3 blocks (refresh 2: the 4-slot form) at a time
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
        assert all_same(full, go(every, ws)), nbytes
    opt.close()


def test_the_call_records_into_a_graph(pkg, gpu):
    """No allocation, no synchronisation, no read-back: the call is captured and replayed twice to the same bits."""
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start, det, floor = problem(*case, "both")
    eager = run(pkg, gpu, opt, Z, Y, start, 3, 2, det, floor, tol=1e-6)
    Yd, a0 = dev(Y, gpu), dev(start, gpu)
    out = torch.zeros_like(a0); info = torch.zeros((5, pkg.FMPC_REFINE_FIELDS), dtype=torch.float64, device=gpu)
    status = torch.zeros(5, dtype=torch.int32, device=gpu); sigma = torch.zeros_like(a0)
    ws = torch.empty(opt.refine_workspace_bytes(27, 5, refresh=2, detector=True), dtype=torch.uint8, device=gpu)
    noise = noise_of(pkg, det, gpu)
    call = lambda: opt.refine(Z, Yd, alpha0=a0, out=out, iters=3, tol=1e-6, info=info, status=status, workspace=ws, refresh=2, detector=noise,
                              floor=floor, sigma=sigma)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        out.zero_(); info.zero_(); status.zero_(); sigma.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all_same(eager, (out.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy(), sigma.cpu().numpy()))
    opt.close()


def test_bad_input_stays_in_its_row_and_nothing_faults(pkg, gpu):
    """A NaN in Y, a gain of -1 and a gain of 0 each stop their row alone; the others are the batch without them."""
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    Z = select(27)[0]
    _, Y, start, det, floor = problem(*case, "both")
    gains = np.full(5, det["gain"])
    keep = [0, 4]
    good = run(pkg, gpu, opt, Z, Y[keep], start[keep], 3, 2, det, floor, gains=gains[keep])
    Yb = Y.copy(); Yb[1, 7] = np.nan
    gb = gains.copy(); gb[2] = -1.0; gb[3] = 0.0
    for iters in (3, 0):
        alpha, info, status, sigma = run(pkg, gpu, opt, Z, Yb, start, iters, 2, det, floor, gains=gb)
        assert status.tolist() == [0, pkg.FMPC_REFINE_BAD_INPUT, pkg.FMPC_REFINE_BAD_INPUT, pkg.FMPC_REFINE_BAD_INPUT, 0], status
        assert np.all(np.isnan(info[1:4, :2])) and np.all(np.isnan(sigma[1:4]))
        if iters:
            assert np.all(np.isnan(alpha[1:4])) and info[:, wr.ITERS].tolist() == [3, 0, 0, 0, 3]
            assert all_same(rows((alpha, info, status, sigma), keep), good)
        else:
            assert same_bits(alpha, start) and same_bits(info[:, wr.COST0], info[:, wr.COST]) and np.all(np.isnan(sigma))
            assert same_bits(info[keep, wr.COST0], good[1][:, wr.COST0])
    assert all_same(good, run(pkg, gpu, opt, Z, Y[keep], start[keep], 3, 2, det, floor, gains=gains[keep]))     # the handle is fine afterwards
    opt.close()


def test_a_map_that_vanishes_fails_the_factorisation_only(pkg, gpu):
    opt = optics(pkg, 31, 17, 3)
    Z, Zh = select(5)
    Z = Z.clone(); Z[2].zero_()
    _, Y, start, det, floor = problem(31, 17, 3, 5, "photon")
    alpha, info, status, sigma = run(pkg, gpu, opt, Z, Y, start, 3, 1, det, floor)
    assert np.all(status == pkg.FMPC_REFINE_FACTOR_FAILED) and np.all(info[:, wr.ITERS] == 0)
    assert same_bits(alpha, start) and np.all(np.isnan(sigma)) and np.all(np.isfinite(info)) and same_bits(info[:, wr.COST0], info[:, wr.COST])
    opt.close()


def test_loop_refines_with_the_detector_of_the_step(pkg, gpu):
    """AOLoop(refine=dict(weighted=True)) with a DetectorNoise: x0, refine_info and refine_sigma of two steps are the calls made
    by hand on the loop's screen; a loop without the key makes the unweighted call, as before."""
    from tests.util import handle_from_model
    R = 2
    opt = pkg.reference_optics(L)
    Zh = np.ascontiguousarray(np.swapaxes(opt.Z.cpu().numpy(), -1, -2))
    md = pkg.synthetic.make_model(27, 144, 10)
    a = np.random.default_rng(8).standard_normal((2, R, 27))
    a *= 0.3 / np.linalg.norm(a, axis=2, keepdims=True)
    phase = torch.from_numpy(np.tensordot(a, Zh[1:], axes=1)).to(gpu)
    h = handle_from_model(pkg, md)
    est = opt.estimator(opt.Z, skip=1)
    noise = pkg.DetectorNoise(est.photon_gain(3e4), read_noise=2.0, seed=3)
    Zl = opt.Z[1:].contiguous()
    for weighted in (True, False):
        kw = dict(weighted=True, floor=2.0) if weighted else {}
        loop = pkg.AOLoop(h, est, opt.Z[1:], R, n_newton=1, k=1e-2, z_colmajor=True, refine=dict(optics=opt, iters=2, refresh=2, **kw))
        assert hasattr(loop, "refine_sigma") == weighted
        for s_ in range(2):
            _, x0 = loop.step(phase[s_], noise)
            lin, Y = est.apply_device(loop.scrn, noise, want_Y=True, colmajor=True, step=s_)
            info = torch.zeros((R, pkg.FMPC_REFINE_FIELDS), dtype=torch.float64, device=gpu)
            sigma = torch.zeros((R, 27), dtype=torch.float64, device=gpu) if weighted else None
            hand = opt.refine(Zl, Y, alpha0=lin, iters=2, refresh=2, info=info, sigma=sigma, **(dict(detector=noise, floor=2.0) if weighted else {}))
            torch.cuda.synchronize()
            assert torch.equal(x0, hand) and torch.equal(loop.refine_info, info) and not bool(loop.refine_status.any()), (weighted, s_)
            if weighted:
                assert torch.equal(loop.refine_sigma, sigma) and bool((sigma > 0).all())
                chi = info[:, pkg.FMPC_REFINE_COST].cpu().numpy() / (opt.p - 27)
                print(f"step {s_}: reduced chi^2 {chi}, sigma {sigma.min().item():.2e} .. {sigma.max().item():.2e}")
        if weighted:
            with pytest.raises(TypeError):                                                # another kind of noise: nothing to weight by
                loop.step(phase[0], None)
            with pytest.raises(TypeError):
                loop.step(phase[0], pkg.EstimatorNoise(sigma=1e-6))
    with pytest.raises(ValueError):
        pkg.AOLoop(h, est, opt.Z[1:], R, z_colmajor=True, refine=dict(optics=opt, weighted=True, refresh=0))
    with pytest.raises(ValueError):
        pkg.AOLoop(h, est, opt.Z[1:], R, z_colmajor=True, refine=dict(optics=opt, floor=1.0))
    est.close(); h.close(); opt.close()


def test_refusals_that_need_a_handle_the_sizes_and_the_empty_calls(pkg, gpu):
    case = (31, 17, 3, 27)
    opt = optics(pkg, *case[:3])
    lib, Z = pkg.load(), select(27)[0]
    _, Y, start, det, floor = problem(*case, "both")
    Yd, ad = dev(Y, gpu), dev(start, gpu)
    size = lambda batch, refresh, nmode=27: int(lib.fmpc_est_refine_weighted_workspace_bytes(opt._h, nmode, batch, refresh))
    for batch in (0, 1, 2, 15, 16, 17, 5000):                                             # the hold call's sizes for refresh >= 1
        for refresh in (1, 2, ONCE):
            for nmode in (1, 27, 64):
                assert size(batch, refresh, nmode) == int(lib.fmpc_est_refine_hold_workspace_bytes(opt._h, nmode, batch, refresh)) > 0
    assert size(1, 0) == 0 and size(1, -1) == 0 and size(1, 1, 65) == 0 and size(-1, 1) == 0
    assert opt.refine_workspace_bytes(27, 40, refresh=3, detector=True) == opt.refine_workspace_bytes(27, 40, refresh=3)
    assert opt.refine_workspace_bytes(27, 40, minimum=True, detector=True) == opt.refine_workspace_bytes(27, minimum=True)
    assert opt.refine_workspace_bytes(27, 40, refresh=0, detector=True) == 0
    least = opt.refine_workspace_bytes(27, minimum=True)
    ws = torch.empty(least, dtype=torch.uint8, device=gpu)
    blk = noise_of(pkg, det, gpu)._block(0, 5)
    vp = lambda t: C.c_void_p(t.data_ptr())
    call = lambda batch=5, ldY=opt.p, iters=2, nbytes=least: lib.fmpc_est_refine_weighted_device(
        opt._h, 27, vp(Z), batch, vp(Yd), ldY, vp(ad), iters, 2, C.byref(blk), floor, 0.0, 0.0, None, None, None, vp(ws), nbytes, None)
    assert call(ldY=opt.p - 1) == pkg.FMPC_E_DIM and call(nbytes=least - 8) == pkg.FMPC_E_DIM and call(nbytes=0) == pkg.FMPC_E_DIM
    assert call(batch=0) == pkg.FMPC_OK and call(batch=0, ldY=opt.p - 1) == pkg.FMPC_E_DIM
    torch.cuda.synchronize()
    assert same_bits(ad.cpu().numpy(), start)                                             # nothing was touched so far
    noise = noise_of(pkg, det, gpu)
    assert tuple(opt.refine(Z, Yd[:0], detector=noise).shape) == (0, 27)
    with pytest.raises(pkg.FastMPCError) as e:
        opt.refine(Z, Yd, detector=noise, refresh=0)
    assert e.value.code == pkg.FMPC_E_DIM
    with pytest.raises(pkg.FastMPCError):
        opt.refine(Z, Yd, sigma=torch.zeros((5, 27), dtype=torch.float64, device=gpu))    # sigma is the weighted call's
    with pytest.raises(pkg.FastMPCError):
        opt.refine(Z, Yd, detector=noise, floor=0.0 if det["read_noise"] == 0.0 else -1.0)
    alpha, info, status, sigma = run(pkg, gpu, opt, Z, Y, start, 0, 2, det, floor)        # iters = 0: chi^2, alpha left alone, no sigma
    ref = reference(*case, 2, "both", 0)
    assert same_bits(alpha, start) and same_bits(info[:, wr.COST0], info[:, wr.COST]) and not status.any() and np.all(np.isnan(sigma))
    assert np.all(info[:, wr.ITERS] == 0) and np.all(info[:, wr.STEP] == 0)
    assert np.allclose(info[:, wr.COST], ref["info"][:, wr.COST], rtol=1e-8, atol=0.0)
    opt.close()
