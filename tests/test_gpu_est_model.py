"""GPU tests of the estimator's linearised image model on the device (fmpc_kernel_est_model.hip; fmpc_est_optics_*,
fmpc_est_model_device, fmpc_est_create_from_model) against the numpy restatement tests/optics_ref.py -- which
tests/test_optics_ref_golden.py pins to the reference's model_approx.mat -- and against that fixture itself at len = 512.

Tolerances: b_s per diversity block 1e-10 relative (the project's tolerance for a 512-point sum against an FFT,
tests/test_gpu_estimator.py); every column of A_s within 1e-10 of the largest column norm; ad_est 1e-8; the loop 1e-7."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import optics_ref as oref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "model_approx_As_bs.npz")
L = 64
ZD = np.array([-3.0, 0.0, 3.0])
DX, AU = 6.5e-6, 1e12
WINDOWS = [(31, 17), (5, 30), (32, 0)]                        # (d, first): the README's width, a small window, the spectrum's edge


@functools.lru_cache(maxsize=None)
def maps(length=L):
    """The device's own unnormalised maps of N = 6: the tensor [j, column, row] and a host copy [j, row, column]."""
    import importlib
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    Z = pkg.zernike_grid(6, length)
    torch.cuda.synchronize()
    Zh = np.ascontiguousarray(np.swapaxes(Z.cpu().numpy(), -1, -2))
    Zh.setflags(write=False)
    return Z, Zh


@functools.lru_cache(maxsize=None)
def phi0_host():
    p = 0.25 * np.random.default_rng(31).standard_normal((L, L))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref_model(d, first, ndiv, nmode, with_phi0):
    """The restatement's (A_s, b_s) of a case: computed once, shared, read-only."""
    _, Zh = maps()
    g = oref.readme_geometry(L)
    Zsel = Zh if nmode == 28 else Zh[7:7 + nmode]
    A, b = oref.model(g["pupil"], Zh[4], ZD[:ndiv], DX, first, first + d - 1, Zsel, AU, phi0_host() if with_phi0 else None)
    A.setflags(write=False); b.setflags(write=False)
    return A, b


def optics(pkg, d, first, ndiv):
    _, Zh = maps()
    return pkg.EstimatorOptics(oref.readme_geometry(L)["pupil"], Zh[4], ZD[:ndiv], DX, first + 1, first + d, AU=AU)


def zsel(nmode):
    Z, _ = maps()
    return Z if nmode == 28 else Z[7:7 + nmode]


def check(A, b, Ar, br, d, ndiv, tol=1e-10):
    A = A.cpu().numpy(); b = b.cpu().numpy()
    assert A.shape == Ar.shape and b.shape == br.shape
    worst_b = 0.0
    for k in range(ndiv):
        s = slice(k * d * d, (k + 1) * d * d)
        e = np.linalg.norm(b[s] - br[s]) / np.linalg.norm(br[s])
        worst_b = max(worst_b, e)
    big = np.linalg.norm(Ar, axis=0).max()
    errs = np.linalg.norm(A - Ar, axis=0) / big
    print(f"b_s worst block {worst_b:.2e}; A_s worst column {errs.max():.2e} of the largest column norm {big:.3e}")
    assert worst_b <= tol, worst_b
    assert np.all(errs <= tol), errs.max()


@pytest.mark.parametrize("d,first", WINDOWS)
@pytest.mark.parametrize("ndiv", [1, 3])
@pytest.mark.parametrize("nmode", [1, 28])
def test_model_at_zero_aberration(pkg, gpu, d, first, ndiv, nmode):
    opt = optics(pkg, d, first, ndiv)
    A, b = opt.model(zsel(nmode))
    torch.cuda.synchronize()
    assert tuple(A.shape) == (ndiv * d * d, nmode) and A.t().is_contiguous()
    check(A, b, *ref_model(d, first, ndiv, nmode, False), d, ndiv)
    opt.close()


@pytest.mark.parametrize("d,first", WINDOWS)
def test_model_about_an_operating_point(pkg, gpu, d, first):
    opt = optics(pkg, d, first, 3)
    phi = torch.from_numpy(np.ascontiguousarray(phi0_host().T)).to(gpu)                 # [column, row]
    A, b = opt.model(zsel(28), phi0=phi)
    torch.cuda.synchronize()
    check(A, b, *ref_model(d, first, 3, 28, True), d, 3)
    A0, b0 = opt.model(zsel(28))
    assert not torch.equal(b, b0)                                                        # phi0 was used
    opt.close()


def test_a_pixel_beyond_the_phase_range_gives_nan_and_no_fault(pkg, gpu):
    opt = optics(pkg, 31, 17, 3)
    phi = torch.from_numpy(np.ascontiguousarray(phi0_host().T)).to(gpu)
    phi[L // 2, L // 2 + 3] = 2.0e6                                                      # inside the pupil
    A, b = opt.model(zsel(28), phi0=phi)
    torch.cuda.synchronize()
    assert bool(torch.isnan(b).all()) and bool(torch.isnan(A).all())                     # E is shared by the diversities: all of them
    A1, b1 = opt.model(zsel(28))                                                         # the handle is fine afterwards
    torch.cuda.synchronize()
    check(A1, b1, *ref_model(31, 17, 3, 28, False), 31, 3)
    opt.close()


@pytest.mark.parametrize("with_phi0", [False, True])
def test_panels_and_repeatability_are_bitwise(pkg, gpu, with_phi0):
    opt = optics(pkg, 31, 17, 3)
    phi = torch.from_numpy(np.ascontiguousarray(phi0_host().T)).to(gpu) if with_phi0 else None
    least, full = opt.workspace_bytes(1), opt.workspace_bytes(28)
    assert 0 < least < full and opt.workspace_bytes(0) == 0 and opt.workspace_bytes(129) == 0
    A, b = opt.model(zsel(28), phi0=phi)
    A, b = A.clone(), b.clone()
    A2, b2 = opt.model(zsel(28), phi0=phi)
    assert torch.equal(A, A2) and torch.equal(b, b2)                                     # two calls
    slot = (full - least) // 27
    for nbytes in (least, least + 3 * slot + 8, full - 8, full + 4096):                  # 2, 5, 28 and 29 fields at a time
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
        Ap, bp = opt.model(zsel(28), phi0=phi, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(A, Ap) and torch.equal(b, bp), nbytes
    # the rules that read the handle
    from tests.test_host_optics_api import check_handle_rules
    check_handle_rules(pkg.load(), opt._h)
    with pytest.raises(pkg.FastMPCError) as e:
        opt.model(zsel(28), workspace=torch.empty(least - 8, dtype=torch.uint8, device=gpu))
    assert e.value.code == pkg.FMPC_E_DIM
    opt.close()


def test_model_records_into_a_graph(pkg, gpu):
    """No allocation, no synchronisation, no read-back: the call is captured and replayed."""
    opt = optics(pkg, 31, 17, 3)
    Z = zsel(28)
    A, b = opt.model(Z)
    A, b = A.clone(), b.clone()
    ws = torch.empty(opt.workspace_bytes(28), dtype=torch.uint8, device=gpu)
    out = (torch.zeros_like(A.t()).t(), torch.zeros_like(b))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.model(Z, workspace=ws, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.model(Z, workspace=ws, out=out)
    out[0].zero_(); out[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], A) and torch.equal(out[1], b)
    opt.close()


def test_the_references_own_model_at_512(pkg, gpu):
    """fmpc_zernike_grid_device (N = 6, unnormalised) -> D_k from its defocus map and the README pupil -> fmpc_est_model_device
    against model_approx.mat, all 28 columns and b_s; then fmpc_est_create_from_model(skip = 1) against the estimator built
    from the fixture."""
    v = np.load(FIX)
    A_fix, b_fix = v["A_s"], v["b_s"].reshape(-1)
    opt = pkg.reference_optics(512)
    assert (opt.range_min, opt.range_max, opt.d, opt.p) == (242, 272, 31, 2883) and tuple(opt.Z.shape) == (28, 512, 512)
    A, b = opt.model(opt.Z)
    torch.cuda.synchronize()
    check(A, b, A_fix, b_fix, 31, 3)
    est = opt.estimator(opt.Z, skip=1)
    W = opt.Z[4].t().cpu().numpy()
    est_fix = pkg.PhaseDiversityEstimator(opt.pupil, W, opt.zd_list, opt.dx, opt.range_min, opt.range_max, A_fix[:, 1:], b_fix, AU=opt.AU)
    assert (est.nx, est.p, est.d, est.rank) == (27, 2883, 31, 27) and est_fix.rank == 27
    rng = np.random.default_rng(21)
    scr = 0.25 * rng.standard_normal((3, 512, 512))
    noise = 1e-2 * rng.standard_normal((3, 2883))
    ad = est.apply(scr, noise=noise); adf = est_fix.apply(scr, noise=noise)
    for s_ in range(3):
        e = np.linalg.norm(ad[s_] - adf[s_]) / np.linalg.norm(adf[s_])
        print(f"screen {s_}: ad_est {e:.2e}")
        assert e <= 1e-8, (s_, e)
    est.close(); est_fix.close(); opt.close()


def test_python_layer_through_the_loop(pkg, gpu):
    """reference_optics(64) -> EstimatorOptics.estimator -> AOLoop for three steps, against an estimator built from
    optics_ref's arrays and host maps: estimates and first moves within 1e-7 (the loop tolerance of tests/test_gpu_estimator.py)."""
    from tests.util import handle_from_model
    R, steps = 2, 3
    opt = pkg.reference_optics(L)
    assert (opt.range_min, opt.range_max, opt.d) == (18, 48, 31)
    _, Zh = maps()
    g = oref.readme_geometry(L)
    A_ref, b_ref = oref.model(g["pupil"], Zh[4], ZD, DX, g["rmin"], g["rmax"], Zh, AU)
    md = pkg.synthetic.make_model(27, 144, 10)
    rng = np.random.default_rng(4)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    phase = np.tensordot(a, Zh[1:], axes=1) + 0.01 * rng.standard_normal((steps, R, L, L))
    outs = []
    for which in ("device", "reference"):
        h = handle_from_model(pkg, md)
        if which == "device":
            est = opt.estimator(opt.Z, skip=1)
            loop = pkg.AOLoop(h, est, opt.Z[1:], R, n_newton=1, k=1e-2, z_colmajor=True)
        else:
            est = pkg.PhaseDiversityEstimator(g["pupil"], Zh[4], ZD, DX, g["rmin"] + 1, g["rmax"] + 1, A_ref[:, 1:], b_ref, AU=AU)
            loop = pkg.AOLoop(h, est, Zh[1:], R, n_newton=1, k=1e-2)
        assert est.rank == 27 and est.nx == 27
        seen = []
        for s_ in range(steps):
            u, x0 = loop.step(torch.from_numpy(phase[s_]).to(gpu))
            seen.append((u.clone(), x0.clone()))
        torch.cuda.synchronize()
        outs.append(seen)
        est.close(); h.close()
    for (u0, x0), (u1, x1) in zip(*outs):
        eu = float(torch.linalg.norm(u0 - u1) / torch.linalg.norm(u1)); ex = float(torch.linalg.norm(x0 - x1) / torch.linalg.norm(x1))
        print(f"loop: u {eu:.2e}, ad_est {ex:.2e}")
        assert eu <= 1e-7 and ex <= 1e-7, (eu, ex)
    opt.close()
