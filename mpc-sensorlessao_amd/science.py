"""Science camera on the device: the in-focus PSF window of a batch of residual screens at any sampling, accumulated over an
exposure, and the wavefront statistics of every screen (mean, rms, Strehl, Marechal, min, max), above `fmpc_sci_*`
(include/fastmpc.h, where the definitions are).  The reference sends the residual wavefront "onto a scientific camera ... to
measure the PSF"; OOMAO's imager.m:92-133 is that camera.

    cam = reference_science_camera(d=32, sampling=2.0)          # the README's pin-hole pupil, dx, AU
    image, quality = cam.expose(scrn)                           # (batch, d, d), (batch, FMPC_SCI_FIELDS)
    cam.expose(scrn2, image=image, accumulate=True, want_quality=False)
    out = cam.summary(image, frames=2)                          # (batch, 2 + nrad): Strehl, window energy, encircled energy

PIXEL ORDER.  Screens are indexed [b, row, column] (colmajor=True: [b, column, row] already, MATLAB's order, no copy).  An image
is stored column-major d x d per screen, the order of the estimator's Y_M blocks: the tensor (batch, d, d) is indexed [b, v, u]."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError

FMPC_SCI_FIELDS = 6
FMPC_SCI_MEAN, FMPC_SCI_RMS, FMPC_SCI_STREHL, FMPC_SCI_MARECHAL, FMPC_SCI_MIN, FMPC_SCI_MAX = range(6)
FMPC_SCI_FIELD_NAMES = ("mean", "rms", "strehl", "marechal", "min", "max")
FMPC_SCI_FORM_STANDARD = 1
FMPC_SCI_FORM_FEW = 2


class ScienceCamera:
    """pupil: (len, len) real amplitude >= 0 indexed [row, column], a host array or a tensor; d in {16, 32, 48, 64}: the window;
    sampling >= 1: samples per 1 / len cycles per pixel (1: the reference's fft2 grid, 2: Nyquist for a pupil that fills the
    grid); psf = dx^4 AU |I|^2.  Attributes: .len, .d, .sampling, .I0 (the unaberrated central value), .sum_a, .sum_a2."""

    def __init__(self, pupil, d=32, sampling=1.0, dx=1.0, AU=1.0, device=0):
        self._lib = _lib.load()
        to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        pupil = np.asarray(to_np(pupil), dtype=np.float64)
        if pupil.ndim != 2 or pupil.shape[0] != pupil.shape[1]:
            raise FastMPCError(_lib.FMPC_E_DIM, "pupil: need a square (len, len) array")
        pc = np.ascontiguousarray(pupil.T)                                    # column-major
        self.len, self.d, self.sampling, self.device = int(pupil.shape[0]), int(d), float(sampling), int(device)
        self.scale = float(dx) ** 4 * float(AU)
        h = C.c_void_p()
        rc = self._lib.fmpc_sci_create(C.byref(h), self.len, self.d, self.sampling, pc.ctypes.data_as(C.c_void_p), self.scale, self.device)
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sci_create")
        self._h = h
        sa, sa2, i0 = C.c_double(), C.c_double(), C.c_double()
        self._lib.fmpc_sci_dims(h, None, None, None, C.byref(sa), C.byref(sa2), C.byref(i0))
        self.sum_a, self.sum_a2, self.I0 = sa.value, sa2.value, i0.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fmpc_sci_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, batch=1):
        """Recommended workspace of `expose` in bytes (batch = 1: the minimum, one screen's slot)."""
        return int(self._lib.fmpc_sci_workspace_bytes(self._h, int(batch)))

    @property
    def last_form(self):
        """FMPC_SCI_FORM_STANDARD or FMPC_SCI_FORM_FEW: the kernel form of the last chunk of the last `expose` (0: none yet)."""
        return int(self._lib.fmpc_sci_last_form(self._h))

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self._dev()).cuda_stream)

    def expose(self, scrn, image=None, accumulate=False, quality=None, want_image=True, want_quality=True, colmajor=False, workspace=None):
        """scrn: (batch, len, len) float64 HIP tensor, or one screen (len, len).  Returns (image, quality) on torch's current
        stream: image (batch, d, d) indexed [b, v, u] or None, quality (batch, FMPC_SCI_FIELDS) or None.
        image: the tensor of an earlier call to fill again or, with accumulate=True, to add this exposure to (contiguous);
        quality: a (batch, >= FMPC_SCI_FIELDS) tensor with unit column stride (its row stride is passed as ldq; further columns
        are left alone); workspace: a torch.uint8 HIP tensor of at least `workspace_bytes(1)` (allocated at the recommended size
        when None).  With image, quality and workspace given nothing is allocated: the form to record into a graph."""
        import torch
        single = scrn.dim() == 2
        s = scrn.unsqueeze(0) if single else scrn
        if not s.is_cuda or s.dtype != torch.float64 or s.dim() != 3 or tuple(s.shape[1:]) != (self.len, self.len):
            raise FastMPCError(_lib.FMPC_E_DIM, "scrn: need a float64 HIP tensor (batch, len, len)")
        s = s if colmajor else s.transpose(-1, -2)
        s = s.contiguous()
        batch = int(s.shape[0])
        if accumulate and image is None:
            raise FastMPCError(_lib.FMPC_E_NULL, "accumulate: needs the image to add to")
        img = None
        if image is not None or want_image:
            if image is None:
                img = torch.empty((batch, self.d, self.d), dtype=torch.float64, device=s.device)
            else:
                img = image
                if not img.is_cuda or img.dtype != torch.float64 or not img.is_contiguous() or img.numel() != batch * self.d * self.d:
                    raise FastMPCError(_lib.FMPC_E_DIM, "image: need a contiguous float64 HIP tensor (batch, d, d)")
        q, ldq = None, 0
        if quality is not None or want_quality:
            if quality is None:
                q = torch.empty((batch, FMPC_SCI_FIELDS), dtype=torch.float64, device=s.device)
            else:
                q = quality
                if (not q.is_cuda or q.dtype != torch.float64 or q.dim() != 2 or q.shape[0] != batch or q.shape[1] < FMPC_SCI_FIELDS
                        or q.stride(1) != 1 or (batch > 1 and q.stride(0) < FMPC_SCI_FIELDS)):
                    raise FastMPCError(_lib.FMPC_E_DIM, "quality: need a float64 HIP tensor (batch, >= FMPC_SCI_FIELDS) with unit column stride")
            ldq = int(q.stride(0)) if batch > 1 else max(int(q.shape[1]), FMPC_SCI_FIELDS)
        if img is None and q is None:
            raise FastMPCError(_lib.FMPC_E_NULL, "expose: neither an image nor the quality is asked for")
        if batch == 0:
            return img, q
        if workspace is None:
            workspace = torch.empty(self.workspace_bytes(batch), dtype=torch.uint8, device=s.device)
        elif not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise FastMPCError(_lib.FMPC_E_DIM, "workspace: need a contiguous torch.uint8 HIP tensor")
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = self._lib.fmpc_sci_expose_device(self._h, batch, vp(s), vp(img), int(bool(accumulate)), vp(q), ldq, vp(workspace),
                                              workspace.numel(), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sci_expose_device")
        return img, q

    def quality(self, scrn, colmajor=False, workspace=None):
        """The (batch, FMPC_SCI_FIELDS) quality rows alone: no matrix instruction is issued."""
        return self.expose(scrn, want_image=False, colmajor=colmajor, workspace=workspace)[1]

    def summary(self, image, frames=1, nrad=None):
        """image: (batch, d, d) accumulated over `frames` exposures.  Returns (batch, 2 + nrad): the long-exposure Strehl ratio,
        the share of the energy inside the window, and the encircled energy within rho = 0 .. nrad - 1 samples of the centre
        (nrad None: d / 2)."""
        import torch
        nrad = self.d // 2 if nrad is None else int(nrad)
        if not image.is_cuda or image.dtype != torch.float64 or not image.is_contiguous() or image.numel() % (self.d * self.d) != 0:
            raise FastMPCError(_lib.FMPC_E_DIM, "image: need a contiguous float64 HIP tensor (batch, d, d)")
        batch = image.numel() // (self.d * self.d)
        out = torch.empty((batch, 2 + max(nrad, 0)), dtype=torch.float64, device=image.device)
        rc = self._lib.fmpc_sci_summary_device(self._h, batch, C.c_void_p(image.data_ptr()), int(frames), nrad, C.c_void_p(out.data_ptr()),
                                               self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_sci_summary_device")
        return out


def sci_tables_host(pupil, d=32, sampling=1.0, scale=1.0):
    """The host tables of a camera without a device (`fmpc_sci_tables_host`): F (len, d) complex, qrange (len / 16, 2) int32,
    (sum A, sum A^2, I0).  pupil: (len, len) indexed [row, column]."""
    pupil = np.asarray(pupil, dtype=np.float64)
    length = int(pupil.shape[0])
    pc = np.ascontiguousarray(pupil.T)
    d = int(d)
    Fre = np.zeros((length, max(d, 1))); Fim = np.zeros((length, max(d, 1)))
    qr = np.zeros((max(length // 16, 1), 2), dtype=np.int32); sums = np.zeros(3)
    rc = _lib.load().fmpc_sci_tables_host(length, d, float(sampling), pc.ctypes.data_as(C.c_void_p), float(scale), Fre.ctypes.data_as(C.c_void_p),
                                          Fim.ctypes.data_as(C.c_void_p), qr.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_sci_tables_host")
    return Fre + 1j * Fim, qr, tuple(sums)
