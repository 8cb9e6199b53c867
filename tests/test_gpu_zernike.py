"""GPU tests of the Zernike kernel (fmpc_kernel_zernike.hip; fmpc_zernike_device, fmpc_zernike_grid_device) against the numpy
restatement of zernfun.m in tests/optics_ref.py.

THE BOUND.  Per element |Z - Z_ref| <= 64 eps S norm, S = sum_s |p_s| r^pow_s the sum of the absolute terms of the radial
polynomial (optics_ref returns it with the normalisation in).  64 is the sum of: <= 8 terms of a recursive sum, each with <= 14
roundings of a repeated product (the coefficients are exact integers); 2 ulp of the trigonometric factor; |m| pi eps <= 44 eps
of argument rounding in m theta.  It bounds any sound evaluation order of either side; a wrong coefficient is off by O(S)."""
import functools

import numpy as np
import pytest
import torch

from tests import optics_ref as oref

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NPX = 1009                                                     # odd: the two-pixel threads have a tail


@functools.lru_cache(maxsize=None)
def points():
    rng = np.random.default_rng(5)
    r = rng.random(NPX); th = rng.uniform(-np.pi, np.pi, NPX)
    r[:4] = [0.0, 1.0, 1.0, 0.0]; th[:4] = [0.3, np.pi, -np.pi, -np.pi]
    r[4], th[4] = 1.0, 0.0
    r.setflags(write=False); th.setflags(write=False)
    return r, th


@functools.lru_cache(maxsize=None)
def ref(N, normalized):
    n, m = oref.zernike_modes(N)
    r, th = points()
    Z, S = oref.zernfun(n, m, r, th, bool(normalized))
    Z.setflags(write=False); S.setflags(write=False)
    return Z, S


@pytest.mark.parametrize("N", [6, 14])
@pytest.mark.parametrize("normalized", [0, 1])
@pytest.mark.parametrize("pad", [0, 7])
def test_point_form(pkg, gpu, N, normalized, pad):
    n, m = pkg.zernike_modes(N)
    r, th = points()
    Zr, S = ref(N, normalized)
    nmode = len(n)
    assert nmode == (28 if N == 6 else 120)
    buf = torch.full((nmode, NPX + pad), -7.25, dtype=torch.float64, device=gpu)
    out = pkg.zernike_basis(n, m, torch.from_numpy(np.array(r)).to(gpu), torch.from_numpy(np.array(th)).to(gpu), normalized=bool(normalized), out=buf)
    torch.cuda.synchronize()
    assert out is buf and buf.stride(0) == NPX + pad
    got = buf.cpu().numpy()
    assert np.all(got[:, NPX:] == -7.25)                       # the padding of every row is untouched
    err = np.abs(got[:, :NPX] - Zr)
    ratio = float((err / (EPS * S + 1e-300)).max())
    print(f"point form N = {N} normalized = {normalized} ldz = {NPX + pad}: max |err| / (eps S) = {ratio:.2f}")
    assert np.all(err <= 64 * EPS * S), ratio
    assert abs(got[0, 0] - (np.sqrt(1 / np.pi) if normalized else 1.0)) <= 2 * EPS


@functools.lru_cache(maxsize=None)
def grid_ref(L):
    r, th = oref.grid_coords(L)                                # [row, column]
    return r, th


@pytest.mark.parametrize("L", [64, 128])
def test_grid_form(pkg, gpu, L):
    n, m = pkg.zernike_modes(6)
    r, th = grid_ref(L)
    Zg = pkg.zernike_grid(6, L)                                # [j, column, row]
    assert tuple(Zg.shape) == (28, L, L) and Zg.is_contiguous()
    # the point form on the grid's own (r, theta), in the same pixel order
    rc = torch.from_numpy(np.ascontiguousarray(r.T).reshape(-1)).to(gpu); tc = torch.from_numpy(np.ascontiguousarray(th.T).reshape(-1)).to(gpu)
    Zp = pkg.zernike_basis(n, m, rc, tc).view(28, L, L)
    torch.cuda.synchronize()
    g = Zg.cpu().numpy(); p = Zp.cpu().numpy()
    inside = (r <= 1.0).T                                      # [column, row]
    _, S = oref.zernfun(*oref.zernike_modes(6), r.T, th.T)
    err = np.abs(g - p)[:, inside]
    ratio = float((err / (EPS * S[:, inside])).max())
    print(f"grid form L = {L}: max |err| / (eps S) = {ratio:.2f}")
    assert np.all(err <= 64 * EPS * S[:, inside]), ratio
    assert np.all(g[:, ~inside] == 0.0)                        # exactly 0 where r > 1
    assert int(np.count_nonzero(g[0])) == int(np.count_nonzero(r <= 1.0))          # the piston is 1 on the support
    assert np.all(g[0][inside] == 1.0)
    # against the restatement itself (its r ** p power sums), same bound
    Zr = oref.zernike_grid(6, L)                               # [j, row, column]
    errr = np.abs(g - np.swapaxes(Zr, -1, -2))[:, inside]
    assert np.all(errr <= 64 * EPS * S[:, inside]), float((errr / (EPS * S[:, inside])).max())
    # storage order on a mode that is not symmetric under transposition: (1, -1) = r sin(theta) = Y, which grows with the ROW
    assert (int(n[1]), int(m[1])) == (1, -1)
    N = L - 1
    c, y0, y1 = L // 2, L // 2 - 3, L // 2 + 5
    assert abs(g[1, c, y1] - (2 * y1 - N) / N) <= 4 * EPS and abs(g[1, c, y0] - (2 * y0 - N) / N) <= 4 * EPS      # [column, row]
    assert abs(g[1, y1, c] - (2 * c - N) / N) <= 4 * EPS
    Zrow = pkg.zernike_grid(6, L, rowmajor=True)
    assert torch.equal(Zrow, Zg.transpose(-1, -2))
    # pairs instead of an order, normalised
    Zn = pkg.zernike_grid((n[3:6], m[3:6]), L, normalized=True).cpu().numpy()
    nf = np.sqrt((1 + (m[3:6] != 0)) * (n[3:6] + 1) / np.pi)
    assert np.all(np.abs(Zn - nf[:, None, None] * g[3:6]) <= 4 * EPS * np.abs(nf[:, None, None] * g[3:6]))


def test_modal_fit_takes_the_grid_maps(pkg, gpu):
    """ModalFit(zernike_grid(6, 64)) recovers the coefficients of a synthesised screen, as tests/test_gpu_modal_fit.py does
    for host-built maps: no host round trip in between."""
    from tests.modal_fit_ref import modal_fit
    L = 64
    Z = pkg.zernike_grid(6, L)
    mf = pkg.ModalFit(Z)
    rng = np.random.default_rng(9)
    c_true = rng.standard_normal((3, 28))
    Zh = Z.cpu().numpy().reshape(28, -1)
    screens = c_true @ Zh + 0.3 * rng.standard_normal((3, L * L)) * (Zh[0] != 0)
    refc, cond = modal_fit(Zh, screens)
    c = mf.fit(torch.from_numpy(screens).to(gpu).view(3, L, L), skip=1)
    torch.cuda.synchronize()
    assert int(mf.status) == 0
    bar = max(1e-14 * cond, 1e-12)                             # the bar of tests/test_gpu_modal_fit.py
    for b in range(3):
        e = float(np.linalg.norm(c[b].cpu().numpy() - refc[b, 1:]) / np.linalg.norm(refc[b, 1:]))
        assert e <= bar, (b, e)
    assert np.linalg.norm(refc - c_true) <= 0.05 * np.linalg.norm(c_true)
