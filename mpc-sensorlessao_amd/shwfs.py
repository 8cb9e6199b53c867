"""Shack-Hartmann sensor on the device: the spots of a lenslet array behind a batch of screens, their centres of gravity and a
modal estimate, above `fmpc_sh_*` (include/fastmpc.h, where the definitions are).  OOMAO's lensletArray.m and shackHartmann.m
(centroiding branch) for a batch: what a wavefront sensor would have measured on the residual screen the sensorless estimator sees.

    sh = ShackHartmann(pupil, npl=16)                           # pad = 2 (Nyquist), spot window = npl, valid at half the light
    sh.set_reference()                                          # the centroids of a flat wavefront
    D, sv, rank = sh.calibrate(Z)                               # Z: (nmode, len, len) mode maps; R = pinv(D) goes to the device
    slopes = sh.measure(scrn)                                   # (batch, 2 nvalid): all x, then all y
    coef = sh.coefficients(scrn)                                # (batch, nmode)
    frame, slopes, dark = sh.measure(scrn, want_frame=True, want_dark=True)
    noisy = detector_read(frame.view(batch, -1), det)           # photon and read-out noise on the frame ...
    slopes = sh.slopes_from_frame(noisy)                        # ... and the slopes of what the detector read

PIXEL ORDER.  Screens are indexed [b, row, column] (colmajor=True: [b, column, row] already, MATLAB's order, no copy).  A frame is
stored column-major (nL s) x (nL s) per screen: the tensor (batch, nL s, nL s) is indexed [b, column, row].  `valid` is (nL, nL)
indexed [i, j]; slopes follow the column-major order of the grid (validLenslet(:))."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError

FMPC_SH_THRESHOLD_NONE, FMPC_SH_THRESHOLD_FLOOR, FMPC_SH_THRESHOLD_FRACTION = 0, 1, 2


def _to_np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def sh_valid_host(pupil, npl, min_light=0.5):
    """The valid mask of `fmpc_sh_valid_host` without a device: (nL, nL) bool indexed [i, j].  pupil: (len, len) [row, column]."""
    pupil = np.asarray(_to_np(pupil), dtype=np.float64)
    if pupil.ndim != 2 or pupil.shape[0] != pupil.shape[1]:
        raise FastMPCError(_lib.FMPC_E_DIM, "pupil: need a square (len, len) array")
    length = int(pupil.shape[0])
    pc = np.ascontiguousarray(pupil.T)
    nL = length // int(npl) if int(npl) > 0 else 0
    mask = np.zeros(max(nL * nL, 1), dtype=np.uint8)
    nv = C.c_int(0)
    rc = _lib.load().fmpc_sh_valid_host(length, int(npl), pc.ctypes.data_as(C.c_void_p), float(min_light), mask.ctypes.data_as(C.c_void_p), C.byref(nv))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_sh_valid_host")
    return mask[:nL * nL].reshape(nL, nL).T.astype(bool)                   # (column-major l = i + nL j)


class ShackHartmann:
    """pupil: (len, len) real amplitude >= 0 indexed [row, column], a host array or a tensor; npl in {16, 32}: pixels per lenslet;
    pad in {1, 2, 3, 4}: nOut = pad npl; spot: the even window s <= min(32, nOut) (None: min(npl, 32, nOut)); min_light: the valid
    rule mean(amplitude^2) >= min_light, or valid: the caller's own (nL, nL) mask [i, j]; threshold: None, a floor, or
    (floor, frac) for t = max(floor, frac max(b)); spot = scale |F' E F|^2 / nOut^2.
    Attributes: .len, .npl, .pad, .s, .nL, .nvalid, .valid, .nmode (0 until a reconstructor is set)."""

    def __init__(self, pupil, npl, pad=2, spot=None, min_light=0.5, valid=None, threshold=None, scale=1.0, device=0):
        self._lib = _lib.load()
        pupil = np.asarray(_to_np(pupil), dtype=np.float64)
        if pupil.ndim != 2 or pupil.shape[0] != pupil.shape[1]:
            raise FastMPCError(_lib.FMPC_E_DIM, "pupil: need a square (len, len) array")
        pc = np.ascontiguousarray(pupil.T)                                    # column-major
        self.len, self.npl, self.pad, self.device = int(pupil.shape[0]), int(npl), int(pad), int(device)
        self.s = int(spot) if spot is not None else min(self.npl, 32, self.pad * self.npl)
        self.scale = float(scale)
        vm = None
        if valid is not None:
            v = np.asarray(_to_np(valid)).astype(bool)
            nL = self.len // self.npl if self.npl > 0 else 0
            if v.shape != (nL, nL):
                raise FastMPCError(_lib.FMPC_E_DIM, "valid: need an (nL, nL) mask")
            vm = np.ascontiguousarray(v.T).astype(np.uint8).reshape(-1)
        h = C.c_void_p()
        rc = self._lib.fmpc_sh_create(C.byref(h), self.len, self.npl, self.pad, self.s, pc.ctypes.data_as(C.c_void_p),
                                      None if vm is None else vm.ctypes.data_as(C.c_void_p), float(min_light), self.scale, self.device)
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_create")
        self._h = h
        nL, nv = C.c_int(), C.c_int()
        self._lib.fmpc_sh_dims(h, None, C.byref(nL), None, None, None, C.byref(nv), None)
        self.nL, self.nvalid, self.nmode = nL.value, nv.value, 0
        self.valid = v if valid is not None else sh_valid_host(pupil, self.npl, min_light)
        self.slopes_units = 1.0
        self.set_threshold(threshold)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fmpc_sh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self._dev()).cuda_stream)

    @property
    def frame_len(self):
        """nL s: the side of a frame."""
        return self.nL * self.s

    def set_threshold(self, threshold=None):
        """None: no threshold; a float: b <- max(b - floor, 0); (floor, frac): t = max(floor, frac max(b)) per lenslet."""
        if threshold is None:
            mode, floor, frac = FMPC_SH_THRESHOLD_NONE, 0.0, 0.0
        elif np.ndim(threshold) == 0:
            mode, floor, frac = FMPC_SH_THRESHOLD_FLOOR, float(threshold), 0.0
        else:
            mode, floor, frac = FMPC_SH_THRESHOLD_FRACTION, float(threshold[0]), float(threshold[1])
        rc = self._lib.fmpc_sh_set_threshold(self._h, mode, floor, frac)
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_set_threshold")
        self.threshold = (mode, floor, frac)

    def _screens(self, scrn, colmajor):
        import torch
        s = scrn.unsqueeze(0) if scrn.dim() == 2 else scrn
        if not s.is_cuda or s.dtype != torch.float64 or s.dim() != 3 or tuple(s.shape[1:]) != (self.len, self.len):
            raise FastMPCError(_lib.FMPC_E_DIM, "scrn: need a float64 HIP tensor (batch, len, len)")
        return (s if colmajor else s.transpose(-1, -2)).contiguous()

    def _out(self, t, shape, dtype, name):
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
            raise FastMPCError(_lib.FMPC_E_DIM, "%s: need a contiguous HIP tensor %s" % (name, shape))
        return t

    def measure(self, scrn, want_frame=False, want_coef=None, colmajor=False, out=None, want_dark=False, want_slopes=True):
        """scrn: (batch, len, len) float64 HIP tensor, or one screen (len, len).  On torch's current stream.  Returns the slopes
        (batch, 2 nvalid), or the tuple (frame, slopes, coef, dark) without the entries that are not asked for when more than
        the slopes are: frame (batch, nL s, nL s) indexed [b, column, row], coef (batch, nmode) (want_coef None: when a
        reconstructor is set and more than the slopes are asked for), dark (batch,) int32.
        out: a dict of tensors to fill, by the names 'frame', 'slopes', 'coef', 'dark' (an entry given is asked for): with every
        output given nothing is allocated, the form to record into a graph."""
        import torch
        s = self._screens(scrn, colmajor)
        batch = int(s.shape[0])
        out = dict(out or {})
        want_frame = want_frame or "frame" in out
        want_dark = want_dark or "dark" in out
        if want_coef is None:
            want_coef = "coef" in out or (self.nmode > 0 and (want_frame or want_dark))
        want_coef = want_coef or "coef" in out
        want_slopes = want_slopes or "slopes" in out
        f64 = dict(dtype=torch.float64, device=s.device)
        fl = self.frame_len
        fr = sl = cf = dk = None
        if want_frame:
            fr = self._out(out["frame"], (batch, fl, fl), torch.float64, "frame") if "frame" in out else torch.empty((batch, fl, fl), **f64)
        if want_slopes:
            sl = self._out(out["slopes"], (batch, 2 * self.nvalid), torch.float64, "slopes") if "slopes" in out else torch.empty((batch, 2 * self.nvalid), **f64)
        if want_coef:
            if self.nmode == 0:
                raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "measure: coefficients without a reconstructor (calibrate or set_reconstructor first)")
            cf = self._out(out["coef"], (batch, self.nmode), torch.float64, "coef") if "coef" in out else torch.empty((batch, self.nmode), **f64)
        if want_dark:
            dk = self._out(out["dark"], (batch,), torch.int32, "dark") if "dark" in out else torch.empty((batch,), dtype=torch.int32, device=s.device)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = self._lib.fmpc_sh_measure_device(self._h, batch, vp(s), vp(fr), vp(sl), vp(cf), vp(dk), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_measure_device")
        got = [t for t in (fr, sl, cf, dk) if t is not None]
        return got[0] if len(got) == 1 else tuple(got)

    def slopes_from_frame(self, frame, want_coef=False, want_dark=False, out=None):
        """frame: (batch, nL s, nL s) or (batch, (nL s)^2) float64 HIP tensor with contiguous screens (its batch stride is passed
        on), as `measure(want_frame=True)` stores it.  Returns the slopes, or (slopes, coef, dark) without what is not asked for."""
        import torch
        fl = self.frame_len
        f = frame.unsqueeze(0) if frame.dim() == 2 and tuple(frame.shape) == (fl, fl) else frame
        f = f.reshape(f.shape[0], -1) if f.dim() == 3 and f[0].is_contiguous() else f
        if not f.is_cuda or f.dtype != torch.float64 or f.dim() != 2 or f.shape[1] != fl * fl or f.stride(1) != 1:
            raise FastMPCError(_lib.FMPC_E_DIM, "frame: need a float64 HIP tensor (batch, nL s, nL s) with contiguous screens")
        batch = int(f.shape[0])
        ld = int(f.stride(0)) if batch > 1 else fl * fl
        out = dict(out or {})
        f64 = dict(dtype=torch.float64, device=f.device)
        sl = self._out(out["slopes"], (batch, 2 * self.nvalid), torch.float64, "slopes") if "slopes" in out else torch.empty((batch, 2 * self.nvalid), **f64)
        cf = dk = None
        if want_coef or "coef" in out:
            if self.nmode == 0:
                raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "slopes_from_frame: coefficients without a reconstructor")
            cf = self._out(out["coef"], (batch, self.nmode), torch.float64, "coef") if "coef" in out else torch.empty((batch, self.nmode), **f64)
        if want_dark or "dark" in out:
            dk = self._out(out["dark"], (batch,), torch.int32, "dark") if "dark" in out else torch.empty((batch,), dtype=torch.int32, device=f.device)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = self._lib.fmpc_sh_slopes_device(self._h, batch, vp(f), ld, vp(sl), vp(cf), vp(dk), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_slopes_device")
        got = [t for t in (sl, cf, dk) if t is not None]
        return got[0] if len(got) == 1 else tuple(got)

    def set_reference(self, scrn=None, slopes_units=None, colmajor=False):
        """Measures a flat wavefront (scrn None) or the given screen (len, len) with a zero reference and unit slopes_units, and
        stores the raw centroids as the reference.  Returns them (2 nvalid)."""
        import torch
        units = self.slopes_units if slopes_units is None else float(slopes_units)
        rc = self._lib.fmpc_sh_set_reference_device(self._h, None, 1.0, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_set_reference_device")
        if scrn is None:
            scrn = torch.zeros((self.len, self.len), dtype=torch.float64, device=self._dev())
        ref = self.measure(scrn, colmajor=colmajor)[0].clone()
        rc = self._lib.fmpc_sh_set_reference_device(self._h, C.c_void_p(ref.data_ptr()), units, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_set_reference_device")
        torch.cuda.current_stream(self._dev()).synchronize()                  # (the copy has read `ref` before it may be freed)
        self.slopes_units = units
        return ref

    def set_reconstructor(self, R):
        """R: (nmode, 2 nvalid) host array or tensor, or None for none: coef = R slopes."""
        import torch
        if R is None:
            rc = self._lib.fmpc_sh_set_reconstructor_device(self._h, 0, None, self._stream())
            self.nmode = 0
        else:
            Rt = (R if torch.is_tensor(R) else torch.from_numpy(np.array(R, dtype=np.float64))).to(device=self._dev(), dtype=torch.float64)
            if Rt.dim() != 2 or Rt.shape[1] != 2 * self.nvalid:
                raise FastMPCError(_lib.FMPC_E_DIM, "R: need (nmode, 2 nvalid)")
            Rc = Rt.t().contiguous()                                          # column-major nmode x 2 nvalid
            rc = self._lib.fmpc_sh_set_reconstructor_device(self._h, int(Rt.shape[0]), C.c_void_p(Rc.data_ptr()), self._stream())
            torch.cuda.current_stream(self._dev()).synchronize()
            if rc == _lib.FMPC_OK:
                self.nmode = int(Rt.shape[0])
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sh_set_reconstructor_device")

    def calibrate(self, Z, h=0.05, rcond=None, colmajor=False):
        """Z: (nmode, len, len) mode maps indexed [j, row, column] (colmajor=True: [j, column, row]), a host array or a tensor.
        Measures +h Z_j and -h Z_j in two batches on the device, takes central differences for D (2 nvalid, nmode) in the
        sensor's slopes_units, computes R = pinv(D, rcond) on the host and uploads it.  Returns (D, singular values, rank)."""
        import torch
        Zt = (Z if torch.is_tensor(Z) else torch.from_numpy(np.array(Z, dtype=np.float64))).to(device=self._dev(), dtype=torch.float64)
        if Zt.dim() != 3 or tuple(Zt.shape[1:]) != (self.len, self.len):
            raise FastMPCError(_lib.FMPC_E_DIM, "Z: need (nmode, len, len)")
        if Zt.shape[0] > 128:
            raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "calibrate: at most 128 modes")
        h = float(h)
        plus = self.measure(Zt * h, colmajor=colmajor)
        minus = self.measure(Zt * (-h), colmajor=colmajor)
        D = ((plus - minus) / (2.0 * h)).t().cpu().numpy()
        sv = np.linalg.svd(D, compute_uv=False)
        cut = (np.finfo(np.float64).eps * max(D.shape) if rcond is None else float(rcond)) * sv[0]
        rank = int((sv > cut).sum())
        self.set_reconstructor(np.linalg.pinv(D, rcond=cut / sv[0]))
        return D, sv, rank

    def coefficients(self, scrn, out=None, colmajor=False):
        """coef = R slopes of the screens, (batch, nmode); out: the tensor to fill."""
        return self.measure(scrn, want_coef=True, want_slopes=False, colmajor=colmajor, out=None if out is None else dict(coef=out))
