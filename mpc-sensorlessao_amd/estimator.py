"""Phase-diversity estimator on the device (include/fastmpc.h: fmpc_est_*): the "% Estimator" block of the reference's
simulation loop, README.md:456-480, for a batch of residual phase screens at once.

    est = PhaseDiversityEstimator(pupil, W, zd_list, dx, range_min, range_max, A_s, b_s)   # MATLAB's 1-based range_min/max
    ad_est = est.apply_device(scrn)            # scrn: (batch, len, len) HIP tensor, scrn[b, i, j] = MATLAB's scrn(i, j)

Arrays are handed over as MATLAB has them (column-major); numpy / torch arrays indexed [row, column] are transposed here.

Measurement noise (README.md:473-475, "SNR = 10 [dB]") is drawn on the device from a counter (`EstimatorNoise`, include/fastmpc.h:
fmpc_noise): `est.apply_device(scrn, noise=EstimatorNoise(snr_db=10, seed=1), step=k)`.  A detector's photon and read-out noise
(OOMAO detector.m:315-321) likewise: `noise=DetectorNoise(est.photon_gain(1e4), read_noise=2.0, seed=1)`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError


def _colmajor(a):
    """(len, len) or (k, len, len) indexed [.., row, column] -> contiguous column-major planes."""
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


class EstimatorNoise:
    """Noise drawn inside the estimator's finish pass: Y_M[r][i] += sigma_r g(seed, step, first + r, i), g a standard normal that is
    a pure function of its four arguments (Philox4x32-10 + Box-Muller, include/fastmpc.h), so a realisation gets the same noise
    wherever it sits in a batch.  Exactly one of
        snr_db   sigma_r = sqrt(mean(Y0[r]^2) 10^(-snr_db / 10)) from this call's noise-free Y_M -- MATLAB's awgn(x, snr, 'measured');
                 the reference's own convention is unknown (SNR_10.mat is not shipped);
        sigma    a float, or a HIP tensor of batch doubles (`PhaseDiversityEstimator.snr_sigma` gives the fixed sigma of an SNR
                 against the unaberrated image).
    first: the global index of realisation 0 of the batches this is used with.  counter: a HIP tensor of one uint64 / int64 whose
    value is added to the step when the kernel runs (a captured graph: `counter.add_(1)` in the same capture)."""

    def __init__(self, snr_db=None, sigma=None, seed=0, first=0, counter=None):
        if (snr_db is None) == (sigma is None):
            raise ValueError("EstimatorNoise: exactly one of snr_db and sigma")
        self.snr_db = None if snr_db is None else float(snr_db)
        self.sigma = sigma if hasattr(sigma, "data_ptr") or sigma is None else float(sigma)
        self.seed, self.first, self.counter = int(seed), int(first), counter
        if hasattr(self.sigma, "data_ptr"):
            import torch
            assert self.sigma.is_cuda and self.sigma.dtype == torch.float64 and self.sigma.is_contiguous()
        if counter is not None:
            import torch
            assert counter.is_cuda and counter.numel() == 1 and counter.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))

    def _block(self, step=0, batch=None):
        """The fmpc_noise block of a call at `step` (the tensors it points to stay owned by this object)."""
        nz = _lib.Noise()
        if self.snr_db is not None:
            nz.mode, nz.value, nz.sigma_dev = _lib.FMPC_NOISE_SNR_MEASURED, self.snr_db, None
        elif hasattr(self.sigma, "data_ptr"):
            if batch is not None and self.sigma.numel() != batch:
                raise ValueError("EstimatorNoise: sigma tensor needs one entry per realisation of the batch")
            nz.mode, nz.value, nz.sigma_dev = _lib.FMPC_NOISE_SIGMA, 0.0, self.sigma.data_ptr()
        else:
            nz.mode, nz.value, nz.sigma_dev = _lib.FMPC_NOISE_SIGMA, self.sigma, None
        nz.seed, nz.step = self.seed & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        nz.step_dev = None if self.counter is None else self.counter.data_ptr()
        nz.first = self.first
        return nz


def normal_noise(batch, p, noise, step=0, out=None, device=None):
    """The array sigma_r g(seed, step, first + r, i) that `apply_device(noise=<EstimatorNoise>)` adds, as a (batch, p) HIP tensor on
    torch's current stream (fmpc_noise_normal_device; `noise` with sigma, not snr_db).  out: a float64 HIP tensor (batch, >= p) with
    contiguous rows to fill (columns from p on are left alone)."""
    import torch
    lib = _lib.load()
    if out is None:
        out = torch.empty((batch, p), dtype=torch.float64, device=torch.device("cuda", 0) if device is None else device)
    assert out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[0] == batch and out.shape[1] >= p
    assert out.stride(1) == 1 or out.shape[1] == 1
    ld = out.stride(0) if batch > 1 else max(out.shape[1], p)
    nz = noise._block(step, batch)
    rc = lib.fmpc_noise_normal_device(C.c_void_p(out.data_ptr()), batch, p, ld, C.byref(nz), C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream))
    if rc != 0:
        raise FastMPCError(rc, "fmpc_noise_normal_device")
    return out


def normal_noise_host(batch, p, noise, step=0, out=None):
    """The same array from the host restatement of the draw (fmpc_noise_normal_host; no device): a (batch, p) numpy array."""
    lib = _lib.load()
    if out is None:
        out = np.empty((batch, p))
    assert out.dtype == np.float64 and out.ndim == 2 and out.shape[0] == batch and out.shape[1] >= p and out.strides[1] == 8
    ld = out.strides[0] // 8 if batch > 1 else max(out.shape[1], p)
    nz = noise._block(step, batch)
    rc = lib.fmpc_noise_normal_host(out.ctypes.data_as(C.c_void_p), batch, p, ld, C.byref(nz))
    if rc != 0:
        raise FastMPCError(rc, "fmpc_noise_normal_host")
    return out


class DetectorNoise:
    """Photon and read-out noise of a detector, drawn inside the estimator's finish pass (include/fastmpc.h: fmpc_detector; OOMAO
    detector.m:315-321): with lam = gain Y0 + background photo-electrons expected in a measurement,
        Y_M = (qe (N - background) + read_noise g) / gain,   N ~ Poisson(lam) (photon_noise) or N = lam,
    N and the standard normal g pure functions of (seed, step, first + r, i), exact in law for lam up to 2^31 and the same bits on
    host and device.  gain: photo-electrons per unit of Y_M, a float or a HIP tensor of batch doubles
    (`PhaseDiversityEstimator.photon_gain` gives the gain of a flux).  read_noise: electrons rms.  qe scales the image as OOMAO's
    does: fold it into the gain for an unbiased estimate.  first, counter: as in `EstimatorNoise`."""

    def __init__(self, gain, photon_noise=True, read_noise=0.0, qe=1.0, background=0.0, seed=0, first=0, counter=None):
        self.gain = gain if hasattr(gain, "data_ptr") else float(gain)
        self.photon_noise, self.read_noise, self.qe, self.background = bool(photon_noise), float(read_noise), float(qe), float(background)
        self.seed, self.first, self.counter = int(seed), int(first), counter
        if hasattr(self.gain, "data_ptr"):
            import torch
            assert self.gain.is_cuda and self.gain.dtype == torch.float64 and self.gain.is_contiguous()
        if counter is not None:
            import torch
            assert counter.is_cuda and counter.numel() == 1 and counter.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))

    def _block(self, step=0, batch=None):
        """The fmpc_detector block of a call at `step` (the tensors it points to stay owned by this object)."""
        det = _lib.Detector()
        if hasattr(self.gain, "data_ptr"):
            if batch is not None and self.gain.numel() != batch:
                raise ValueError("DetectorNoise: gain tensor needs one entry per realisation of the batch")
            det.gain, det.gain_dev = 0.0, self.gain.data_ptr()
        else:
            det.gain, det.gain_dev = self.gain, None
        det.qe, det.background, det.read_noise, det.photon_noise = self.qe, self.background, self.read_noise, int(self.photon_noise)
        det.seed, det.step = self.seed & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        det.step_dev = None if self.counter is None else self.counter.data_ptr()
        det.first = self.first
        return det


def detector_read(Y0, det, step=0, out=None):
    """The detector's read-out of a (batch, p) float64 HIP tensor Y0 with contiguous rows (fmpc_detector_read_device), on torch's
    current stream: what `apply_device(noise=<DetectorNoise>)` makes of its noise-free Y_M.  out: a tensor of Y0's shape and strides
    (Y0 itself: in place); columns are the measurements i < p of realisation first + r."""
    import torch
    lib = _lib.load()
    assert Y0.is_cuda and Y0.dtype == torch.float64 and Y0.dim() == 2 and (Y0.stride(1) == 1 or Y0.shape[1] == 1)
    if out is None:
        out = torch.empty_strided(tuple(Y0.shape), Y0.stride(), dtype=torch.float64, device=Y0.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == Y0.shape and out.stride() == Y0.stride()
    batch, p = Y0.shape
    ld = Y0.stride(0) if batch > 1 else p
    blk = det._block(step, batch)
    rc = lib.fmpc_detector_read_device(C.c_void_p(out.data_ptr()), C.c_void_p(Y0.data_ptr()), batch, p, ld, C.byref(blk),
                                       C.c_void_p(torch.cuda.current_stream(Y0.device).cuda_stream))
    if rc != 0:
        raise FastMPCError(rc, "fmpc_detector_read_device")
    return out


def detector_read_host(Y0, det, step=0, out=None):
    """The same read-out on the host (fmpc_detector_read_host; no device): Y0 a (batch, p) float64 numpy array with contiguous
    rows; returns an array of its shape (out: one of Y0's shape and strides, Y0 itself for in place)."""
    lib = _lib.load()
    Y0 = np.asarray(Y0)
    if out is None:
        Y0 = np.ascontiguousarray(Y0, dtype=np.float64)
        out = np.empty_like(Y0)
    assert Y0.dtype == np.float64 and Y0.ndim == 2 and Y0.strides[1] == 8
    assert out.dtype == np.float64 and out.shape == Y0.shape and out.strides == Y0.strides
    batch, p = Y0.shape
    ld = Y0.strides[0] // 8 if batch > 1 else p
    blk = det._block(step, batch)
    rc = lib.fmpc_detector_read_host(out.ctypes.data_as(C.c_void_p), Y0.ctypes.data_as(C.c_void_p), batch, p, ld, C.byref(blk))
    if rc != 0:
        raise FastMPCError(rc, "fmpc_detector_read_host")
    return out


class PhaseDiversityEstimator:
    def __init__(self, pupil, W, zd_list, dx, range_min, range_max, A_s, b_s, AU=1e12, device=0):
        """range_min, range_max: the reference's 1-based window bounds (README.md:378-379); A_s (p, nx), b_s (p)."""
        self._lib = _lib.load()
        pupil = np.asarray(pupil, dtype=np.float64)
        W = np.asarray(W, dtype=np.float64)
        zd = np.asarray(zd_list, dtype=np.float64).reshape(-1)
        length = pupil.shape[0]
        D = pupil[None] * np.exp(1j * zd[:, None, None] * W[None])       # README.md:464-465 without the screen
        Dre, Dim = _colmajor(D.real), _colmajor(D.imag)
        A_s = np.asfortranarray(np.asarray(A_s, dtype=np.float64))
        b_s = np.ascontiguousarray(np.asarray(b_s, dtype=np.float64))
        p, nx = A_s.shape
        d = int(range_max) - int(range_min) + 1
        h = C.c_void_p()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self._lib.fmpc_est_create(C.byref(h), length, int(range_min) - 1, d, len(zd), ptr(Dre), ptr(Dim), float(dx) ** 4 * float(AU),
                                       ptr(A_s), ptr(b_s), p, nx, int(device))
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_create")
        self._h, self.len, self.d, self.ndiv, self.nx, self.p, self.device = h, length, d, len(zd), nx, p, int(device)
        rk = C.c_int()
        self._lib.fmpc_est_dims(self._h, None, None, None, None, None, C.byref(rk))
        self.rank = rk.value

    @classmethod
    def _from_handle(cls, h, device):
        """An estimator around a handle the library made (fmpc_est_create_from_model); it owns the handle."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        v = [C.c_int() for _ in range(6)]
        rc = self._lib.fmpc_est_dims(h, *[C.byref(x) for x in v])
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_dims")
        self._h, self.device = h, int(device)
        self.len, self.d, self.ndiv, self.nx, self.p, self.rank = (x.value for x in v)
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fmpc_est_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def snr_sigma(self, snr_db):
        """sqrt(mean(b_s^2) 10^(-snr_db / 10)): the fixed sigma of an SNR against the unaberrated image (fmpc_est_snr_sigma)."""
        s = C.c_double()
        rc = self._lib.fmpc_est_snr_sigma(self._h, float(snr_db), C.byref(s))
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_snr_sigma")
        return s.value

    def photon_gain(self, n_photons):
        """n_photons ndiv / sum(b_s): the gain [photo-electrons per unit of Y_M] at which the unaberrated system puts n_photons
        photo-electrons, on average, into one diversity's window (fmpc_est_photon_gain)."""
        g = C.c_double()
        rc = self._lib.fmpc_est_photon_gain(self._h, float(n_photons), C.byref(g))
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_photon_gain")
        return g.value

    def apply_device(self, scrn, noise=None, want_Y=False, colmajor=False, out=None, step=0, want_sigma=False):
        """scrn: (batch, len, len) float64 HIP tensor indexed [b, row, column] (colmajor=True: already [b, column, row], no copy).
        noise: None, a (batch, p) HIP tensor that is added to Y_M, an `EstimatorNoise` or a `DetectorNoise` drawn on the device
        at `step`.
        Returns ad_est (batch, nx) [, Y_M (batch, p)] [, sigma (batch): want_sigma, with an EstimatorNoise] on torch's current
        stream; out: a (batch, nx) tensor to write ad_est into."""
        import torch
        if not colmajor:
            scrn = scrn.transpose(-1, -2).contiguous()
        assert scrn.is_cuda and scrn.dtype == torch.float64 and scrn.is_contiguous() and tuple(scrn.shape[1:]) == (self.len, self.len)
        batch = scrn.shape[0]
        if out is not None:
            assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (batch, self.nx)
        ad = out if out is not None else torch.empty((batch, self.nx), dtype=torch.float64, device=scrn.device)
        Y = torch.empty((batch, self.p), dtype=torch.float64, device=scrn.device) if want_Y else None
        if isinstance(noise, EstimatorNoise):
            sig = torch.empty(batch, dtype=torch.float64, device=scrn.device) if want_sigma else None
            nz = noise._block(step, batch)
            rc = self._lib.fmpc_est_apply_noisy_device(self._h, batch, C.c_void_p(scrn.data_ptr()), C.byref(nz), C.c_void_p(ad.data_ptr()),
                                                       None if Y is None else C.c_void_p(Y.data_ptr()), None if sig is None else C.c_void_p(sig.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream(scrn.device).cuda_stream))
            if rc != 0:
                raise FastMPCError(rc, "fmpc_est_apply_noisy_device")
            res = (ad,) + ((Y,) if want_Y else ()) + ((sig,) if want_sigma else ())
            return res if len(res) > 1 else ad
        if want_sigma:
            raise ValueError("want_sigma: only with an EstimatorNoise")
        if isinstance(noise, DetectorNoise):
            det = noise._block(step, batch)
            rc = self._lib.fmpc_est_apply_detector_device(self._h, batch, C.c_void_p(scrn.data_ptr()), C.byref(det), C.c_void_p(ad.data_ptr()),
                                                          None if Y is None else C.c_void_p(Y.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream(scrn.device).cuda_stream))
            if rc != 0:
                raise FastMPCError(rc, "fmpc_est_apply_detector_device")
            return (ad, Y) if want_Y else ad
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.float64 and noise.is_contiguous() and tuple(noise.shape) == (batch, self.p)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = self._lib.fmpc_est_apply_device(self._h, batch, vp(scrn), vp(noise), vp(ad), vp(Y),
                                             C.c_void_p(torch.cuda.current_stream(scrn.device).cuda_stream))
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_apply_device")
        return (ad, Y) if want_Y else ad

    def apply(self, scrn, noise=None, want_Y=False):
        """Host arrays: scrn (batch, len, len) indexed [b, row, column]."""
        scrn = _colmajor(scrn)
        batch = scrn.shape[0]
        ad = np.empty((batch, self.nx)); Y = np.empty((batch, self.p)) if want_Y else None
        nz = None if noise is None else np.ascontiguousarray(np.asarray(noise, dtype=np.float64))
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = self._lib.fmpc_est_apply(self._h, batch, ptr(scrn), ptr(nz), ptr(ad), ptr(Y))
        if rc != 0:
            raise FastMPCError(rc, "fmpc_est_apply")
        return (ad, Y) if want_Y else ad
