"""Frozen-flow von Karman atmosphere on the device (the reference's README.md:24-75: OOMAO's layered atmosphere seen by one on-axis
source) above the `fmpc_atm_*` calls of include/fastmpc.h, which states the process.  Altitudes do not enter; OOMAO's random
stream, and so its samples, cannot be reproduced -- its covariance and its extrusion are."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError


def atm_covariance(rho, r0, L0):
    """C(rho) of phaseStats.covariance (fraction 1) on the host; rho >= 0, any shape."""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    out = np.empty_like(rho)
    rc = _lib.load().fmpc_atm_covariance_host(rho.size, rho.ctypes.data_as(C.c_void_p), float(r0), float(L0), out.ctypes.data_as(C.c_void_p))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_atm_covariance_host")
    return out


def atm_default_stencil(W):
    """1, 2, 4, ..: the powers of two <= W - 1, at most 8."""
    s = []
    while len(s) < 8 and (1 << len(s)) <= int(W) - 1:
        s.append(1 << len(s))
    return s


def atm_extruder(W, pitch, r0, L0, stencil=None):
    """A (W, q W) and B (W, W) lower of one stencil (None: the default), built on the host in long double."""
    W = int(W)
    st = atm_default_stencil(W) if stencil is None else [int(s) for s in stencil]
    q = len(st)
    if q < 1 or q > 64 or W < 1:
        raise FastMPCError(_lib.FMPC_E_DIM, "atm_extruder: need W >= 3 and a stencil of 1 .. 8 lines")
    A = np.empty((W, q * W))
    B = np.empty((W, W))
    rc = _lib.load().fmpc_atm_extruder_host(W, float(pitch), float(r0), float(L0), q, (C.c_int * q)(*st), A.ctypes.data_as(C.c_void_p),
                                            B.ctypes.data_as(C.c_void_p))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_atm_extruder_host")
    return A, B


def atm_displacement(k, px_per_step):
    """(lines, fraction) of the displacement k * px_per_step: floor(|d|) and the rest in [0, 1)."""
    n, f = C.c_longlong(), C.c_double()
    rc = _lib.load().fmpc_atm_displacement_host(int(k), float(px_per_step), C.byref(n), C.byref(f))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_atm_displacement_host")
    return n.value, f.value


class Atmosphere:
    """`batch` realisations (global indices first .. first + batch - 1) of a layered atmosphere.  fractional_r0, wind_speed [m/s],
    wind_direction [rad]: one entry per layer.  The window of a layer is W = npix + 1 samples across at pitch p = D / (npix - 1), so
    that a screen spans (W - 2) p = D; screens come out as (batch, out_len, out_len) float64 HIP tensors indexed [r, y, x].  The
    operands are built on the host on construction (seconds at npix 128); `reset()` fills the windows."""

    def __init__(self, r0, L0, fractional_r0, wind_speed, wind_direction, npix, D, dt, batch, seed, first=0, stencil=None, device=None):
        import torch
        self._lib = _lib.load()
        self._h = C.c_void_p()
        dev = 0 if device is None else device
        self.device = dev if isinstance(dev, torch.device) else torch.device("cuda", int(dev))
        frac, speed, direc = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (fractional_r0, wind_speed, wind_direction))
        if not (frac.ndim == 1 and frac.shape == speed.shape == direc.shape and frac.size >= 1):
            raise FastMPCError(_lib.FMPC_E_DIM, "Atmosphere: need as many fractions as wind speeds and directions")
        self.npix, self.W, self.D = int(npix), int(npix) + 1, float(D)
        if self.npix < 2:
            raise FastMPCError(_lib.FMPC_E_DIM, "Atmosphere: npix >= 2")
        self.pitch = self.D / (self.npix - 1)
        self.r0, self.L0, self.dt = float(r0), float(L0), float(dt)
        self.layers, self.batch, self.seed, self.first = int(frac.size), int(batch), int(seed), int(first)
        self.stencil = atm_default_stencil(self.W) if stencil is None else [int(s) for s in stencil]
        self.fractional_r0, self.wind_speed, self.wind_direction = frac, speed, direc
        q = len(self.stencil)
        st = (C.c_int * max(q, 1))(*self.stencil)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self._lib.fmpc_atm_create(C.byref(self._h), self.W, self.pitch, self.r0, self.L0, self.layers, p(frac), p(speed), p(direc), self.dt,
                                       q, st, self.batch, self.seed & 0xFFFFFFFFFFFFFFFF, self.first, self.device.index or 0)
        if rc != _lib.FMPC_OK:
            self._h = C.c_void_p()
            raise FastMPCError(rc, "fmpc_atm_create")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fmpc_atm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def k(self):
        k = C.c_longlong()
        self._lib.fmpc_atm_dims(self._h, None, None, None, None, C.byref(k))
        return k.value

    def reset(self):
        """Start-up: fills every window; k = 0."""
        rc = self._lib.fmpc_atm_reset_device(self._h, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_atm_reset_device")
        return self

    def advance(self, steps=1):
        rc = self._lib.fmpc_atm_advance_device(self._h, int(steps), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_atm_advance_device")
        return self

    def screen(self, out_len=None, mask=None, scale=1.0, out=None):
        """The screens of the current step: scale * mask * (sum of the layers - mean over the mask), (batch, out_len, out_len); out_len
        None: npix.  mask: (out_len, out_len) of 0 / 1 (any dtype, host or device) or None (then no mean is removed); out: a
        contiguous float64 HIP tensor of that shape to fill (nothing is allocated then)."""
        import torch
        n = self.npix if out_len is None else int(out_len)
        if n < 2:
            raise FastMPCError(_lib.FMPC_E_DIM, "screen: out_len >= 2")
        if out is None:
            out = torch.empty((self.batch, n, n), dtype=torch.float64, device=self.device)
        elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (self.batch, n, n)
              or not out.is_contiguous()):
            raise FastMPCError(_lib.FMPC_E_DIM, "out: need a contiguous float64 HIP tensor (batch, out_len, out_len)")
        m = None
        if mask is not None:
            m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64))
            m = m.to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(m.shape) != (n, n):
                raise FastMPCError(_lib.FMPC_E_DIM, "mask: need (out_len, out_len)")
        rc = self._lib.fmpc_atm_screen_device(self._h, n, None if m is None else C.c_void_p(m.data_ptr()), float(scale),
                                              C.c_void_p(out.data_ptr()) if out.numel() else C.c_void_p(8), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_atm_screen_device")
        return out

    def step(self, out_len=None, mask=None, scale=1.0, out=None, steps=1):
        """advance(steps), then screen(...)."""
        self.advance(steps)
        return self.screen(out_len, mask, scale, out)

    def series(self, steps, modal, skip=1, mask=None, scale=1.0):
        """The Zernike coefficient series of README.md:86-93 for `identify_var_device`: `steps` times step() and `modal.fit`, screen
        by screen -- one (batch, len, len) buffer, never a steps x batch x len^2 array.  modal: a `ModalFit` over maps of shape
        (len, len).  Returns (batch, steps, n - skip), contiguous."""
        import torch
        shape = tuple(modal.pixel_shape)
        if len(shape) != 2 or shape[0] != shape[1] or modal.Z.device != self.device:
            raise FastMPCError(_lib.FMPC_E_DIM, "modal: need a ModalFit over square maps on the atmosphere's device")
        steps, nc = int(steps), modal.n - int(skip)
        c = torch.empty((self.batch, steps, nc), dtype=torch.float64, device=self.device)
        buf = torch.empty((self.batch, shape[0], shape[0]), dtype=torch.float64, device=self.device)
        ws = modal._workspace(None, self.batch)
        for s in range(steps):
            self.step(shape[0], mask, scale, out=buf)
            modal.fit(buf, skip=skip, workspace=ws, out=c[:, s, :])
        return c

    def extruder(self):
        """A (W, q W) and B (W, W) of the full stencil as numpy arrays."""
        return atm_extruder(self.W, self.pitch, self.r0, self.L0, self.stencil)

    def state(self):
        """dict of windows (layers, batch, W, W) float64 HIP tensor indexed [layer, r, y, x], k and counts (the extrusions of each
        layer so far)."""
        import torch
        w = torch.empty((self.layers, self.batch, self.W, self.W), dtype=torch.float64, device=self.device)
        k = C.c_longlong()
        cnt = (C.c_ulonglong * self.layers)()
        rc = self._lib.fmpc_atm_get_state(self._h, C.c_void_p(w.data_ptr()) if w.numel() else None, C.byref(k), cnt, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_atm_get_state")
        return dict(windows=w, k=k.value, counts=[int(v) for v in cnt])

    def load_state(self, state):
        import torch
        w = state["windows"]
        w = w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
        w = w.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(w.shape) != (self.layers, self.batch, self.W, self.W) or len(state["counts"]) != self.layers:
            raise FastMPCError(_lib.FMPC_E_DIM, "load_state: need windows (layers, batch, W, W) and one count per layer")
        cnt = (C.c_ulonglong * self.layers)(*[int(v) for v in state["counts"]])
        rc = self._lib.fmpc_atm_set_state(self._h, C.c_void_p(w.data_ptr()) if w.numel() else None, int(state["k"]), cnt, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_atm_set_state")
        self._held = w                                     # (the copy kernel may still be reading it)
        return self


def reference_atmosphere(batch, seed, npix=128, first=0, stencil=None, device=None):
    """The atmosphere of README.md:24-75: r0 0.2 m, L0 42 m, three layers of fractions [0.7, 0.1, 0.2] / 25 with winds 5 / 7.5 /
    10 m/s towards 0 / pi/3 / 5 pi/3, a 1 m telescope sampled at 200 Hz with npix = 128 across (the altitudes do not enter)."""
    return Atmosphere(0.2, 42.0, np.array([0.7, 0.1, 0.2]) / 25.0, [5.0, 7.5, 10.0], [0.0, np.pi / 3, 5 * np.pi / 3], npix, 1.0, 1.0 / 200.0,
                      batch, seed, first=first, stencil=stencil, device=device)
