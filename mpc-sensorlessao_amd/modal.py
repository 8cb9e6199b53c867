"""Modal fit on the device: the least-squares projection of phase maps onto mode maps (the reference's zernmodfit.m:201-213,
c = z \\ data(:), which run over all frames gives the series ad_acc of README.md:86-93, and README.md:268-271, the same
projection of the influence functions, B), above `fmpc_modal_factor_device` and `fmpc_modal_fit_device` (include/fastmpc.h)."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import FastMPCError


def modal_workspace_bytes(n, npx, batch=1):
    """Recommended workspace of `ModalFit.fit` in bytes (batch = 1: the minimum, one panel of 16 screens; 0: refused sizes)."""
    return int(_lib.load().fmpc_modal_workspace_bytes(int(n), int(npx), int(batch)))


class ModalFit:
    """Z: contiguous float64 HIP tensor (n, ...) -- n mode maps over any pixel shape: compressed vectors z(is_in) or full grids
    that vanish outside the support.  Factors Z Z' on construction, without synchronising: `.R` (n, n) holds the upper Cholesky
    factor as R[j, i] = R(i, j) (column-major storage), `.status` 0 or FMPC_E_NOT_PD_SCHUR, both on the device; after a failed
    factorisation R and every later fit are NaN."""

    def __init__(self, Z, workspace=None):
        import torch
        if not Z.is_cuda or Z.dtype != torch.float64 or not Z.is_contiguous() or Z.dim() < 2:
            raise FastMPCError(_lib.FMPC_E_DIM, "Z: need a contiguous float64 HIP tensor (n, ...)")
        self._lib = _lib.load()
        self.Z = Z
        self.n = int(Z.shape[0])
        self.pixel_shape = tuple(Z.shape[1:])
        self.npx = int(Z[0].numel())
        self.R = torch.empty((self.n, self.n), dtype=torch.float64, device=Z.device)
        self.status = torch.zeros((), dtype=torch.int32, device=Z.device)
        ws = self._workspace(workspace, self.n)
        rc = self._lib.fmpc_modal_factor_device(self.n, self.npx, self._p(Z), self._p(self.R), self._p(self.status), self._p(ws), ws.numel(),
                                                self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_modal_factor_device")

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.Z.device).cuda_stream)

    def _workspace(self, workspace, batch):
        import torch
        if workspace is None:
            return torch.empty(modal_workspace_bytes(self.n, self.npx, batch), dtype=torch.uint8, device=self.Z.device)
        if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise FastMPCError(_lib.FMPC_E_DIM, "workspace: need a contiguous torch.uint8 HIP tensor")
        return workspace

    def fit(self, screens, skip=0, workspace=None, out=None):
        """screens: float64 HIP tensor (batch, ...) or one screen (...), each screen contiguous; rows further apart than a screen
        are passed through as lds (no copy).  Returns the coefficients skip .. n-1, (batch, n - skip) or (n - skip,).
        workspace: a torch.uint8 HIP tensor of at least `modal_workspace_bytes(n, npx, 1)` bytes (allocated at the recommended
        size when None); out: the tensor of an earlier call -- or any (batch, n - skip) tensor with unit column stride -- to fill
        again (nothing is allocated then: the form to record into a graph)."""
        import torch
        single = screens.dim() == len(self.pixel_shape)
        s = screens.unsqueeze(0) if single else screens
        if not s.is_cuda or s.dtype != torch.float64 or tuple(s.shape[1:]) != self.pixel_shape:
            raise FastMPCError(_lib.FMPC_E_DIM, "screens: need a float64 HIP tensor (batch, ...) over the pixel shape of Z")
        batch = int(s.shape[0])
        skip = int(skip)
        nc = self.n - skip
        lds = int(s.stride(0)) if batch > 1 else self.npx
        if batch and (not s[0].is_contiguous() or lds < self.npx):
            raise FastMPCError(_lib.FMPC_E_DIM, "screens: every screen must be contiguous and the screens must not overlap")
        if out is None:
            c = torch.empty((batch, max(nc, 0)), dtype=torch.float64, device=s.device)
        else:
            c = out.unsqueeze(0) if out.dim() == 1 else out
            if (not c.is_cuda or c.dtype != torch.float64 or tuple(c.shape) != (batch, nc) or (nc > 1 and c.stride(1) != 1)
                    or (batch > 1 and c.stride(0) < nc)):
                raise FastMPCError(_lib.FMPC_E_DIM, "out: need a float64 HIP tensor (batch, n - skip) with unit column stride")
        if batch == 0:
            return c
        ldc = int(c.stride(0)) if batch > 1 else nc
        ws = self._workspace(workspace, batch)
        rc = self._lib.fmpc_modal_fit_device(self.n, self.npx, batch, self._p(self.Z), self._p(self.R), self._p(s), lds, skip, self._p(c), ldc,
                                             self._p(ws), ws.numel(), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_modal_fit_device")
        return c[0] if single else c

    def series(self, screens, skip=1, workspace=None):
        """screens: contiguous (R, S, ...) -- S frames of R realisations.  Returns (R, S, n - skip), contiguous: with skip = 1 the
        reference's ad_acc without its piston column, which goes straight into `identify_var_device`."""
        if screens.dim() != 2 + len(self.pixel_shape) or not screens.is_contiguous():
            raise FastMPCError(_lib.FMPC_E_DIM, "screens: need a contiguous (R, S, ...) tensor")
        R, S = int(screens.shape[0]), int(screens.shape[1])
        c = self.fit(screens.reshape((R * S,) + self.pixel_shape), skip=skip, workspace=workspace)
        return c.view(R, S, self.n - int(skip))

    def influence_matrix(self, I, skip=1, workspace=None):
        """I: (m, ...) influence functions.  Returns B = pinv(Z Z') Z I' without its first `skip` rows (README.md:268-271), an
        (n - skip, m) view over column-major storage: the layout `fmpc_create` takes (README.md:290)."""
        return self.fit(I, skip=skip, workspace=workspace).t()
