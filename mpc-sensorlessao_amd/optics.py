"""The estimator's optics on the device: the Zernike mode maps (the reference's zernfun.m in zernmodfit.m's mode order; its
Zs.mat is not shipped) and the first-order image model y = b_s + A_s alpha (its model_approx.mat, loaded at README.md:294),
above `fmpc_zernike_*`, `fmpc_est_optics_*`, `fmpc_est_model_device` and `fmpc_est_create_from_model` (include/fastmpc.h).

    Z = zernike_grid(6, 512)                                   # (28, 512, 512) HIP tensor indexed [j, column, row]
    opt = reference_optics(512)                                # the README's geometry (README.md:366-396)
    A_s, b_s = opt.model(opt.Z)                                # (p, 28), (p,): model_approx.mat
    est = opt.estimator(opt.Z, skip=1)                         # a PhaseDiversityEstimator (piston removed, README.md:289)

PIXEL ORDER.  The maps come out in MATLAB's order: pixel (row y, column x) at y + len x, i.e. a tensor indexed
[j, column, row] -- what `fmpc_est_create` takes for D, what `PhaseDiversityEstimator.apply_device(colmajor=True)`,
`AOLoop(z_colmajor=True)` and `AOLoop.step(colmajor=True)` take without a copy.  rowmajor=True gives [j, row, column]
(a transposed copy on the device)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError
from .estimator import PhaseDiversityEstimator


def zernike_modes(N):
    """(n, m) of zernmodfit.m:195-198: for n = 0..N, m = -n, -n + 2, .., n; two int32 arrays of (N + 1)(N + 2) / 2."""
    lib = _lib.load()
    cnt = lib.fmpc_zernike_modes(int(N), None, None)
    n = np.zeros(cnt, dtype=np.int32); m = np.zeros(cnt, dtype=np.int32)
    lib.fmpc_zernike_modes(int(N), n.ctypes.data_as(_lib._ip), m.ctypes.data_as(_lib._ip))
    return n, m


def _pairs(N_or_pairs):
    if np.ndim(N_or_pairs) == 0:
        return zernike_modes(int(N_or_pairs))
    n, m = N_or_pairs
    return np.ascontiguousarray(n, dtype=np.int32).reshape(-1), np.ascontiguousarray(m, dtype=np.int32).reshape(-1)


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def zernike_basis(n, m, r, theta, normalized=False, out=None):
    """zernfun(n, m, r, theta[, 'norm']) on the device.  r, theta: contiguous float64 HIP tensors of npx points; returns
    (nmode, npx), or fills out: (nmode, >= npx) with unit column stride (its row stride is passed as ldz).  r outside [0, 1] is
    evaluated as the polynomial."""
    import torch
    n, m = _pairs((n, m))
    for t in (r, theta):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise FastMPCError(_lib.FMPC_E_DIM, "r, theta: need contiguous float64 HIP tensors")
    npx = int(r.numel())
    if int(theta.numel()) != npx or len(n) != len(m):
        raise FastMPCError(_lib.FMPC_E_DIM, "r and theta, n and m: equal lengths")
    Z = torch.empty((len(n), npx), dtype=torch.float64, device=r.device) if out is None else out
    if not Z.is_cuda or Z.dtype != torch.float64 or Z.dim() != 2 or Z.shape[0] != len(n) or Z.shape[1] < npx or (Z.shape[1] > 1 and Z.stride(1) != 1):
        raise FastMPCError(_lib.FMPC_E_DIM, "out: need a float64 HIP tensor (nmode, >= npx) with unit column stride")
    ldz = int(Z.stride(0)) if len(n) > 1 else npx
    rc = _lib.load().fmpc_zernike_device(len(n), n.ctypes.data_as(_lib._ip), m.ctypes.data_as(_lib._ip), npx, C.c_void_p(r.data_ptr()),
                                         C.c_void_p(theta.data_ptr()), int(bool(normalized)), C.c_void_p(Z.data_ptr()), ldz, _stream(r.device))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_zernike_device")
    return Z


def zernike_grid(N_or_pairs, length, normalized=False, rowmajor=False, device=0):
    """The modes on the length x length grid x = (-N:2:N)/N, N = length - 1, zero where r > 1: a HIP tensor
    (nmode, length, length) indexed [j, column, row] (MATLAB's order in memory); rowmajor=True: [j, row, column]."""
    import torch
    n, m = _pairs(N_or_pairs)
    dev = torch.device("cuda", int(device))
    Z = torch.empty((len(n), int(length), int(length)), dtype=torch.float64, device=dev)
    rc = _lib.load().fmpc_zernike_grid_device(len(n), n.ctypes.data_as(_lib._ip), m.ctypes.data_as(_lib._ip), int(length),
                                              int(bool(normalized)), C.c_void_p(Z.data_ptr()), _stream(dev))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_zernike_grid_device")
    return Z.transpose(-1, -2).contiguous() if rowmajor else Z


class EstimatorOptics:
    """pupil, W: (len, len) indexed [row, column], host arrays or tensors; zd_list: the diversities; range_min, range_max: the
    reference's 1-based window bounds (README.md:378-379).  D_k = pupil .* exp(1i*zd_list(k)*W) is formed here once."""

    def __init__(self, pupil, W, zd_list, dx, range_min, range_max, AU=1e12, device=0):
        self._lib = _lib.load()
        to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        pupil = np.asarray(to_np(pupil), dtype=np.float64); W = np.asarray(to_np(W), dtype=np.float64)
        zd = np.asarray(zd_list, dtype=np.float64).reshape(-1)
        D = pupil[None] * np.exp(1j * zd[:, None, None] * W[None])           # README.md:464-465 without the screen
        Dre = np.ascontiguousarray(np.swapaxes(D.real, -1, -2)); Dim = np.ascontiguousarray(np.swapaxes(D.imag, -1, -2))
        self.len, self.d, self.first, self.ndiv = int(pupil.shape[0]), int(range_max) - int(range_min) + 1, int(range_min) - 1, len(zd)
        self.p, self.device = self.ndiv * self.d * self.d, int(device)
        h = C.c_void_p()
        rc = self._lib.fmpc_est_optics_create(C.byref(h), self.len, self.first, self.d, self.ndiv, Dre.ctypes.data_as(C.c_void_p),
                                              Dim.ctypes.data_as(C.c_void_p), float(dx) ** 4 * float(AU), self.device)
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_est_optics_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fmpc_est_optics_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, nmode=1):
        """Recommended workspace of `model` in bytes (nmode = 1: the minimum)."""
        return int(self._lib.fmpc_est_model_workspace_bytes(self._h, int(nmode)))

    def _maps(self, Z, phi0):
        import torch
        if not Z.is_cuda or Z.dtype != torch.float64 or not Z.is_contiguous() or tuple(Z.shape[1:]) != (self.len, self.len):
            raise FastMPCError(_lib.FMPC_E_DIM, "Z: need a contiguous float64 HIP tensor (nmode, len, len) indexed [j, column, row]")
        if phi0 is not None and (not phi0.is_cuda or phi0.dtype != torch.float64 or not phi0.is_contiguous() or tuple(phi0.shape) != (self.len, self.len)):
            raise FastMPCError(_lib.FMPC_E_DIM, "phi0: need a contiguous float64 HIP tensor (len, len) indexed [column, row]")
        return int(Z.shape[0])

    def model(self, Z, phi0=None, workspace=None, out=None):
        """Z: (nmode, len, len) HIP tensor indexed [j, column, row] (`zernike_grid`); phi0: (len, len) indexed [column, row] or
        None (zero aberration).  Returns (A_s (p, nmode), b_s (p,)) on torch's current stream; A_s is a view over column-major
        storage.  workspace: a torch.uint8 HIP tensor of at least `workspace_bytes(1)`; out: (A_s, b_s) of an earlier call."""
        import torch
        nmode = self._maps(Z, phi0)
        if workspace is None:
            workspace = torch.empty(self.workspace_bytes(nmode), dtype=torch.uint8, device=Z.device)
        if out is None:
            At = torch.empty((nmode, self.p), dtype=torch.float64, device=Z.device); b = torch.empty(self.p, dtype=torch.float64, device=Z.device)
        else:
            At, b = out[0].t(), out[1]
            assert At.is_contiguous() and tuple(At.shape) == (nmode, self.p) and b.is_contiguous() and tuple(b.shape) == (self.p,)
        rc = self._lib.fmpc_est_model_device(self._h, nmode, C.c_void_p(Z.data_ptr()), None if phi0 is None else C.c_void_p(phi0.data_ptr()),
                                             C.c_void_p(At.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                             workspace.numel(), _stream(Z.device))
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_est_model_device")
        return At.t(), b

    def refine_workspace_bytes(self, nmode, batch=1, minimum=False, refresh=1, detector=None):
        """Recommended workspace of `refine` in bytes (refresh >= 1: every field of up to 16 realisations at a time; refresh = 0,
        the gain form: one field of up to 128); minimum=True: the smallest it takes (one realisation, one field at a time),
        whatever the batch.  detector=: the size of the weighted call (that of the same refresh >= 1; 0 for refresh = 0, which
        it refuses)."""
        if detector is not None:
            full = int(self._lib.fmpc_est_refine_weighted_workspace_bytes(self._h, int(nmode), int(batch), int(refresh)))
            if not minimum or full == 0:
                return full
            return self.refine_workspace_bytes(nmode, batch, minimum=True)
        if int(refresh) == 0:
            return int(self._lib.fmpc_est_refine_hold_workspace_bytes(self._h, int(nmode), 1 if minimum else int(batch), 0))
        if int(refresh) == 1:
            full = int(self._lib.fmpc_est_refine_workspace_bytes(self._h, int(nmode), int(batch)))
        else:
            full = int(self._lib.fmpc_est_refine_hold_workspace_bytes(self._h, int(nmode), int(batch), int(refresh)))
        if not minimum or full == 0:
            return full
        one = int(self._lib.fmpc_est_refine_workspace_bytes(self._h, int(nmode), 1))
        return one - int(nmode) * self.ndiv * (self.len // 16) * 16384

    def gain(self, Z):
        """The estimator's gain about zero aberration for the gain form of `refine`: pinv of `model(Z)`'s A_s as an (nmode, p)
        contiguous HIP tensor (hand over the maps without the piston).  Runs the model, reads A_s back, takes the
        pseudo-inverse on the host and uploads it: it synchronises and is not for the hot loop -- call it once and keep G."""
        import torch
        A, _ = self.model(Z)
        torch.cuda.current_stream(Z.device).synchronize()
        G = np.linalg.pinv(A.cpu().numpy())
        return torch.from_numpy(np.ascontiguousarray(G)).to(Z.device)

    def refine(self, Z, Y, alpha0=None, iters=3, damping=0.0, tol=0.0, workspace=None, out=None, info=None, status=None, refresh=1,
               G=None, detector=None, floor=1.0, sigma=None):
        """Gauss-Newton on ||Y_b - y(alpha_b)||^2 with the exact image model (`fmpc_est_refine_device`).  Z: (nmode <= 64, len, len)
        HIP tensor indexed [j, column, row], every map an unknown (no piston); Y: (batch, p) measured images, unit column stride;
        alpha0: (batch, nmode) start, None: zero.  Returns alpha (batch, nmode) on torch's current stream: `out` if given
        (out may be alpha0 itself: refined in place), else a new tensor.  info: (batch, FMPC_REFINE_FIELDS) float64 and
        status: (batch,) int32 tensors to fill, or None.  workspace: a torch.uint8 HIP tensor of at least
        `refine_workspace_bytes(nmode, minimum=True, refresh=refresh)`.
        refresh (`fmpc_est_refine_hold_device`): 1, the default, rebuilds J every iteration (the call above); r > 1 rebuilds it
        every r-th iteration and holds it in between (one field instead of nmode + 1); 0 is the gain form
        alpha += G (Y - y(alpha)) without a Jacobian, G: (nmode, p) float64 HIP tensor with unit column stride, None:
        `gain(Z)` (which synchronises: hand G over in a loop); damping must then be 0.  See include/fastmpc.h for when each
        converges.
        detector (`fmpc_est_refine_weighted_device`): a `DetectorNoise`; the fit is then weighted by the variance that detector
        gives the model image -- its gain (a float or a tensor of batch doubles), qe, background, read_noise and photon_noise;
        seed, first and counter are not used -- with `floor` photo-electrons the least photon variance of a row.  info then
        holds chi^2 for the costs, and `sigma`, a contiguous (batch, nmode) float64 HIP tensor or None, takes
        sqrt(diag(H^-1)) of every realisation's last step (NaN where it took none).  refresh >= 1; G is not used."""
        import torch
        nmode = self._maps(Z, None)
        refresh = int(refresh)
        if detector is None and sigma is not None:
            raise FastMPCError(_lib.FMPC_E_DIM, "sigma: only with detector=")
        if refresh == 0 and detector is None:
            if G is None:
                G = self.gain(Z)
            if not G.is_cuda or G.dtype != torch.float64 or G.dim() != 2 or tuple(G.shape) != (nmode, self.p) or (self.p > 1 and G.stride(1) != 1):
                raise FastMPCError(_lib.FMPC_E_DIM, "G: need a float64 HIP tensor (nmode, p) with unit column stride")
        if not Y.is_cuda or Y.dtype != torch.float64 or Y.dim() != 2 or Y.shape[1] != self.p or (self.p > 1 and Y.stride(1) != 1):
            raise FastMPCError(_lib.FMPC_E_DIM, "Y: need a float64 HIP tensor (batch, p) with unit column stride")
        batch = int(Y.shape[0])
        ldY = int(Y.stride(0)) if batch > 1 else self.p
        alpha = out if out is not None else torch.empty((batch, nmode), dtype=torch.float64, device=Z.device)
        if not alpha.is_cuda or alpha.dtype != torch.float64 or not alpha.is_contiguous() or tuple(alpha.shape) != (batch, nmode):
            raise FastMPCError(_lib.FMPC_E_DIM, "out: need a contiguous float64 HIP tensor (batch, nmode)")
        if alpha0 is None:
            alpha.zero_()
        elif alpha0 is not alpha:
            alpha.copy_(alpha0)
        if info is not None and (not info.is_cuda or info.dtype != torch.float64 or not info.is_contiguous() or
                                 tuple(info.shape) != (batch, _lib.FMPC_REFINE_FIELDS)):
            raise FastMPCError(_lib.FMPC_E_DIM, "info: need a contiguous float64 HIP tensor (batch, FMPC_REFINE_FIELDS)")
        if status is not None and (not status.is_cuda or status.dtype != torch.int32 or not status.is_contiguous() or tuple(status.shape) != (batch,)):
            raise FastMPCError(_lib.FMPC_E_DIM, "status: need a contiguous int32 HIP tensor (batch,)")
        if sigma is not None and (not sigma.is_cuda or sigma.dtype != torch.float64 or not sigma.is_contiguous() or tuple(sigma.shape) != (batch, nmode)):
            raise FastMPCError(_lib.FMPC_E_DIM, "sigma: need a contiguous float64 HIP tensor (batch, nmode)")
        if batch == 0:                       # (an empty tensor has no pointer to hand over; the library takes batch = 0 and does nothing)
            return alpha
        if workspace is None:
            workspace = torch.empty(self.refine_workspace_bytes(nmode, batch, refresh=max(refresh, 0 if detector is None else 1)), dtype=torch.uint8,
                                    device=Z.device)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        if detector is not None:
            name = "fmpc_est_refine_weighted_device"
            blk = detector._block(0, batch)
            rc = self._lib.fmpc_est_refine_weighted_device(self._h, nmode, vp(Z), batch, vp(Y), ldY, vp(alpha), int(iters), refresh, C.byref(blk),
                                                           float(floor), float(damping), float(tol), vp(info), vp(status), vp(sigma),
                                                           vp(workspace), workspace.numel(), _stream(Z.device))
        elif refresh == 1:
            name = "fmpc_est_refine_device"
            rc = self._lib.fmpc_est_refine_device(self._h, nmode, vp(Z), batch, vp(Y), ldY, vp(alpha), int(iters), float(damping), float(tol),
                                                  vp(info), vp(status), vp(workspace), workspace.numel(), _stream(Z.device))
        else:
            name = "fmpc_est_refine_hold_device"
            ldG = (int(G.stride(0)) if nmode > 1 else self.p) if refresh == 0 else 0
            rc = self._lib.fmpc_est_refine_hold_device(self._h, nmode, vp(Z), batch, vp(Y), ldY, vp(alpha), int(iters), refresh,
                                                       vp(G) if refresh == 0 else None, ldG, float(damping), float(tol), vp(info), vp(status),
                                                       vp(workspace), workspace.numel(), _stream(Z.device))
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, name)
        return alpha

    def estimator(self, Z, skip=1, phi0=None):
        """The estimator of this model without its first `skip` columns (README.md:289 removes the piston).  Synchronises."""
        import torch
        nmode = self._maps(Z, phi0)
        torch.cuda.current_stream(Z.device).synchronize()                  # (the library runs the model on the null stream)
        h = C.c_void_p()
        rc = self._lib.fmpc_est_create_from_model(C.byref(h), self._h, nmode, int(skip), C.c_void_p(Z.data_ptr()),
                                                  None if phi0 is None else C.c_void_p(phi0.data_ptr()))
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_est_create_from_model")
        return PhaseDiversityEstimator._from_handle(h, self.device)


def reference_pupil(length=512, dx=6.5e-6):
    """The README's pin-hole pupil (README.md:383-391): 1 where the spatial frequency is within (length / 2 - 1) df of the centre,
    a host array (length, length) indexed [row, column]."""
    length = int(length)
    df = 1.0 / (length * dx)
    fx = np.arange(-length // 2, length // 2) * df
    FX, FY = np.meshgrid(fx, -fx)
    return (np.sqrt(FX ** 2 + FY ** 2) <= (length / 2 - 1) * df).astype(np.float64)


def reference_science_camera(d=32, sampling=1.0, length=512, device=0):
    """A `ScienceCamera` behind the README's pin-hole pupil with its dx = 6.5e-6 and AU = 1e12: at sampling 1 and d = 32 the
    image of a zero screen is the zero-diversity block of the reference's b_s (its first row and column apart)."""
    from .science import ScienceCamera
    return ScienceCamera(reference_pupil(length, 6.5e-6), d=d, sampling=sampling, dx=6.5e-6, AU=1e12, device=device)


def reference_optics(length=512, dx=6.5e-6, N=6, zd_dist=3.0, AU=1e12, device=0):
    """The README's geometry (README.md:366-396): the pin-hole pupil, defocus (mode index 4 of zernmodfit's order, unnormalised)
    as the diversity, zd_list = [-3 0 3], the window |x| <= 1e-4 m (31 samples on the 512 grid).  Returns an `EstimatorOptics`
    with `.Z` (the (N + 1)(N + 2) / 2 mode maps on the device, [j, column, row]), `.zd_list`, `.range_min`, `.range_max`
    (1-based), `.dx`, `.AU` and `.pupil` (host)."""
    length = int(length)
    Z = zernike_grid(N, length, device=device)
    pupil = reference_pupil(length, dx)
    xaxis = np.arange(-length // 2, length // 2) * dx
    rmin = int(np.nonzero(np.abs(xaxis + 1.0e-4) < 3e-6)[0][0]) + 1                       # README.md:378-379 (1-based)
    rmax = int(np.nonzero(np.abs(xaxis - 1.0e-4) < 3e-6)[0][-1]) + 1
    zd_list = np.array([-zd_dist, 0.0, zd_dist])
    W = Z[4].t()                                                                          # [row, column]
    opt = EstimatorOptics(pupil, W, zd_list, dx, rmin, rmax, AU=AU, device=device)
    opt.Z, opt.zd_list, opt.range_min, opt.range_max, opt.dx, opt.AU, opt.pupil = Z, zd_list, rmin, rmax, dx, AU, pupil
    return opt
