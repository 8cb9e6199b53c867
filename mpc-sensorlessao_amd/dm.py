"""Deformable mirror of Gaussian actuators on the device (the reference's README.md:184-272): influence maps, the influence matrix
B = pinv(Zs'Zs) Zs' B_pupil without the maps in memory, and the surface sum_t u_t I_t the mirror makes, above
`fmpc_dm_influence_device`, `fmpc_dm_matrix_device` and `fmpc_dm_surface_device` (include/fastmpc.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError


def dm_matrix_workspace_bytes(n, m, rows, cols, minimum=False):
    """Workspace of `GaussianDM.influence_matrix` in bytes: the recommended size, or with minimum=True the smallest the call
    takes (the ex / ey tables and the partial sums of one panel of 16 actuators, include/fastmpc.h); 0 for refused sizes."""
    lib = _lib.load()
    rec = int(lib.fmpc_dm_matrix_workspace_bytes(int(n), int(m), int(rows), int(cols)))
    if not minimum or rec == 0:
        return rec
    tiles = (int(n) + 15) // 16
    chunk = 64 * (4 if tiles <= 2 else 2 if tiles == 3 else 1)            # pixels per chunk of the modal fit
    supers = -(-int(rows) * int(cols) // (4 * chunk))                     # one partial per four chunks
    return 8 * ((int(rows) + int(cols)) * 16 * ((int(m) + 15) // 16) + supers * 16 * 16 * tiles)


def reference_dm_geometry(length=512, dx=6.5e-6, D=4.4e-3, m1=12, coupling=0.1, half_width=2.2e-3):
    """The mirror of README.md:194-263 in numpy: the 12 x 12 actuators on the len_dm^2 mirror grid and the crop to the length^2
    pupil grid.  Returns a dict of x (length), y = -x, cx, cy (m1^2; actuator (i-1) m1 + j at (x0[j], y0[i])), pitch, coupling and
    the reference's 1-based len_dm, x0_dm_idx, min_idx, max_idx.  Ties of the two argmins go to the first index, as MATLAB's min."""
    length, m1 = int(length), int(m1)
    len_dm = int(np.floor(half_width * 2 / dx + 0.5))                     # round(): halves away from zero
    xaxis_dm = (-len_dm / 2 + np.arange(len_dm)) * dx                     # README.md:207
    diff = len_dm // (m1 - 1)
    x0_dm_idx = 1 + diff * np.arange(m1)
    x0_dm_idx[-1] = len_dm                                                # README.md:217
    x0 = xaxis_dm[x0_dm_idx - 1]
    y0 = -x0                                                              # yaxis_dm = -xaxis_dm
    xaxis = (-length / 2 + np.arange(length)) * dx                        # README.md:241
    max_idx = int(np.argmin(np.abs(xaxis_dm - xaxis[-1]))) + 1            # README.md:255-256 (argmin: the first of a tie)
    min_idx = int(np.argmin(np.abs(xaxis_dm - xaxis[0]))) + 1
    if max_idx - min_idx + 1 != length:
        raise ValueError(f"reference_dm_geometry: the crop {min_idx}:{max_idx} of the {len_dm}-pixel mirror grid is not {length} wide")
    x = np.ascontiguousarray(xaxis_dm[min_idx - 1:max_idx])
    return dict(x=x, y=-x, cx=np.tile(x0, m1), cy=np.repeat(y0, m1), pitch=D / (m1 - 1), coupling=float(coupling), len_dm=len_dm,
                x0_dm_idx=x0_dm_idx, min_idx=min_idx, max_idx=max_idx)


class GaussianDM:
    """x (cols), y (rows): abscissae of the columns and ordinates of the rows; cx, cy (m): the actuator centres; host arrays or
    tensors, kept on the device as float64.  Maps and screens are (cols, rows) planes indexed [column, row] -- pixel (r, c) at
    r + rows c, the order of `zernike_grid` and of `AOLoop.step(colmajor=True)`."""

    def __init__(self, x, y, cx, cy, coupling, pitch, device=0):
        import torch
        self._lib = _lib.load()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        conv = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1))).to(
            device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        self.x, self.y, self.cx, self.cy = conv(x), conv(y), conv(cx), conv(cy)
        self.coupling, self.pitch = float(coupling), float(pitch)
        self.m, self.rows, self.cols = int(self.cx.numel()), int(self.y.numel()), int(self.x.numel())
        if self.m < 1 or int(self.cy.numel()) != self.m or self.rows < 1 or self.cols < 1:
            raise FastMPCError(_lib.FMPC_E_DIM, "GaussianDM: need x, y and as many cx as cy")
        if not (0.0 < self.coupling < 1.0) or not (self.pitch > 0.0 and np.isfinite(self.pitch)):
            raise FastMPCError(_lib.FMPC_E_DIM, "GaussianDM: coupling in (0, 1) and a positive pitch")
        self.npx = self.rows * self.cols

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _planes(self, t, count, what):
        """A (count, cols, rows) float64 HIP tensor of contiguous planes that do not overlap; returns the distance between two."""
        import torch
        if (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != (count, self.cols, self.rows)
                or not t[0].is_contiguous() or (count > 1 and t.stride(0) < self.npx)):
            raise FastMPCError(_lib.FMPC_E_DIM, f"{what}: need a float64 HIP tensor ({count}, cols, rows) of contiguous planes")
        return int(t.stride(0)) if count > 1 else self.npx

    def influence(self, first=0, count=None, out=None):
        """The maps of actuators first .. first + count - 1 (count None: to the last): (count, cols, rows) indexed [t, column, row]."""
        import torch
        first = int(first)
        count = self.m - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.m:
            raise FastMPCError(_lib.FMPC_E_DIM, "influence: first, count outside the actuators")
        I = torch.empty((count, self.cols, self.rows), dtype=torch.float64, device=self.device) if out is None else out
        ldi = self._planes(I, count, "out")
        rc = self._lib.fmpc_dm_influence_device(self.m, self.rows, self.cols, self._p(self.x), self._p(self.y), self._p(self.cx), self._p(self.cy),
                                                self.coupling, self.pitch, first, count, self._p(I), ldi, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_influence_device")
        return I

    def influence_matrix(self, modal, skip=1, workspace=None, out=None):
        """B = pinv(Z Z') Z I' without its first `skip` rows (README.md:268-271, 290) for the mode maps of `modal`, a `ModalFit` over
        maps of shape (cols, rows); the maps I are never in memory.  Returns what `ModalFit.influence_matrix` returns: an
        (n - skip, m) view with strides (1, n - skip), the layout `fmpc_create` takes.  workspace: a torch.uint8 HIP tensor of at
        least `dm_matrix_workspace_bytes(n, m, rows, cols, minimum=True)` bytes; out: an (n - skip, m) view with strides (1, ldb),
        ldb >= n - skip, to fill (nothing is allocated with both: the form to record into a graph)."""
        import torch
        if tuple(modal.pixel_shape) != (self.cols, self.rows) or modal.Z.device != self.device:
            raise FastMPCError(_lib.FMPC_E_DIM, "modal: need a ModalFit over maps of shape (cols, rows) on the mirror's device")
        n, skip = modal.n, int(skip)
        nc = n - skip
        if skip < 0 or nc < 1:
            raise FastMPCError(_lib.FMPC_E_DIM, "skip: outside [0, n)")
        if out is None:
            B = torch.empty((self.m, nc), dtype=torch.float64, device=self.device).t()
        else:
            B = out
            if (not B.is_cuda or B.dtype != torch.float64 or tuple(B.shape) != (nc, self.m) or (nc > 1 and B.stride(0) != 1)
                    or (self.m > 1 and B.stride(1) < nc)):
                raise FastMPCError(_lib.FMPC_E_DIM, "out: need a float64 HIP view (n - skip, m) with strides (1, ldb >= n - skip)")
        ldb = int(B.stride(1)) if self.m > 1 else nc
        if workspace is None:
            ws = torch.empty(dm_matrix_workspace_bytes(n, self.m, self.rows, self.cols), dtype=torch.uint8, device=self.device)
        else:
            ws = workspace
            if not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
                raise FastMPCError(_lib.FMPC_E_DIM, "workspace: need a contiguous torch.uint8 HIP tensor")
        rc = self._lib.fmpc_dm_matrix_device(n, self.m, self.rows, self.cols, self._p(modal.Z), self._p(modal.R), self._p(self.x), self._p(self.y),
                                             self._p(self.cx), self._p(self.cy), self.coupling, self.pitch, skip, self._p(B), ldb,
                                             self._p(ws), ws.numel(), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_matrix_device")
        return B

    def surface(self, u, phase=None, out=None):
        """phase + sum_t u[b][t] I_t (phase None: the surface alone).  u: float64 HIP tensor (batch, m) with unit column stride, or
        (m,); phase, out: (batch, cols, rows) of contiguous planes (or one plane for a single u); out may be phase."""
        import torch
        single = u.dim() == 1
        uu = u.unsqueeze(0) if single else u
        if (not uu.is_cuda or uu.dtype != torch.float64 or uu.dim() != 2 or uu.shape[0] < 1 or uu.shape[1] != self.m
                or (self.m > 1 and uu.stride(1) != 1) or (uu.shape[0] > 1 and uu.stride(0) < self.m)):
            raise FastMPCError(_lib.FMPC_E_DIM, "u: need a float64 HIP tensor (batch, m) with unit column stride")
        batch = int(uu.shape[0])
        ldu = int(uu.stride(0)) if batch > 1 else self.m
        ph = phase.unsqueeze(0) if (phase is not None and single and phase.dim() == 2) else phase
        ldp = self._planes(ph, batch, "phase") if ph is not None else self.npx
        if out is None:
            o = torch.empty((batch, self.cols, self.rows), dtype=torch.float64, device=self.device)
        else:
            o = out.unsqueeze(0) if (single and out.dim() == 2) else out
        ldo = self._planes(o, batch, "out")
        rc = self._lib.fmpc_dm_surface_device(batch, self.m, self.rows, self.cols, self._p(self.x), self._p(self.y), self._p(self.cx),
                                              self._p(self.cy), self.coupling, self.pitch, self._p(uu), ldu, self._p(ph), ldp, self._p(o), ldo,
                                              self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_surface_device")
        return o[0] if single else o


def reference_dm(length=512, dx=6.5e-6, D=4.4e-3, m1=12, coupling=0.1, half_width=2.2e-3, device=0):
    """The `GaussianDM` of `reference_dm_geometry`, with the entries of that dict as attributes (x, y, cx, cy on the device; the
    host arrays are in `.geometry`)."""
    g = reference_dm_geometry(length, dx, D, m1, coupling, half_width)
    dm = GaussianDM(g["x"], g["y"], g["cx"], g["cy"], g["coupling"], g["pitch"], device=device)
    dm.geometry = g
    for k in ("len_dm", "x0_dm_idx", "min_idx", "max_idx"):
        setattr(dm, k, g[k])
    return dm
