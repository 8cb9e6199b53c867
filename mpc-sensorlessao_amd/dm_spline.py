"""Deformable mirror of spline actuators on the device: OOMAO's influence function (influenceFunction.m:96-118 the curve, :253-362 the
maps) -- a separable piecewise-cubic profile with compact support -- above `fmpc_dm_profile_oomao_host`, `fmpc_dm_profile_eval_host`
and the `fmpc_dm_spline_*_device` calls (include/fastmpc.h).  `SplineDM` takes the argument conventions of `GaussianDM` and can
stand in for it in `AOLoop(dm=...)`; its surface multiplies a 64 x 64 tile of pixels through the actuators whose support meets
the tile, not through all m."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FastMPCError

FMPC_DM_TILE = 64
FMPC_DM_DENSE = 1
# influenceFunction.m's two named curves; 'overshoot' has no y -> x spline and is refused by the host call
OOMAO_POINTS = {"monotonic": (0.2, (0.4, 0.7), (0.6, 0.4), 1.0, 1.0), "overshoot": (0.2, (0.4, 0.7), (0.5, 0.4), 0.3, 1.0)}


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class DMProfile:
    """A piecewise cubic in pitch units: strictly ascending breaks (pieces + 1) and coef (pieces, 4) with
    f(d) = sum_k coef[i, k] (d - breaks[i])^k on breaks[i] <= d < breaks[i + 1], the last piece closed on the right, and f = 0
    exactly outside [breaks[0], breaks[-1]].  It need not be symmetric."""

    def __init__(self, breaks, coef):
        self.breaks = np.ascontiguousarray(np.asarray(breaks, dtype=np.float64).reshape(-1))
        self.coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1, 4))
        self.pieces = int(self.coef.shape[0])
        if self.pieces < 1 or self.pieces > 4096 or self.breaks.size != self.pieces + 1:
            raise FastMPCError(_lib.FMPC_E_DIM, "DMProfile: need 1 .. 4096 pieces, pieces + 1 breaks and 4 coefficients per piece")
        if not (np.all(np.diff(self.breaks) > 0.0) and np.all(np.isfinite(self.coef))):
            raise FastMPCError(_lib.FMPC_E_DIM, "DMProfile: need strictly ascending breaks and finite coefficients")
        self.breaks.setflags(write=False); self.coef.setflags(write=False)

    @property
    def support(self):
        """(breaks[0], breaks[-1]): the profile is exactly zero outside."""
        return float(self.breaks[0]), float(self.breaks[-1])

    def eval(self, d):
        """f(d) by `fmpc_dm_profile_eval_host`: the evaluation the device does, the same bits."""
        dd = np.ascontiguousarray(np.asarray(d, dtype=np.float64))
        out = np.empty_like(dd)
        rc = _lib.load().fmpc_dm_profile_eval_host(self.pieces, _hp(self.breaks), _hp(self.coef), dd.size, _hp(dd), _hp(out))
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_profile_eval_host")
        return out


def oomao_profile(mech, kind="monotonic", points=None):
    """OOMAO's influence curve at mechanical coupling `mech` (f(1) = mech up to the interpolation of the scale) as a `DMProfile`
    of 400 pieces.  points = (p2x, (p3x, p3y), (p4x, p4y), ratio, p6x) overrides `kind`; a curve whose ordinates are not strictly
    monotone ('overshoot') is refused: pass pp arrays of your own to `DMProfile`."""
    if points is None:
        if kind not in OOMAO_POINTS:
            raise FastMPCError(_lib.FMPC_E_DIM, f"oomao_profile: unknown kind {kind!r}")
        points = OOMAO_POINTS[kind]
    p2x, p3, p4, ratio, p6x = points
    p3 = np.array(p3, dtype=np.float64).reshape(2); p4 = np.array(p4, dtype=np.float64).reshape(2)
    cap = 400
    breaks, coef = np.empty(cap + 1), np.empty(4 * cap)
    pieces = C.c_int(0)
    rc = _lib.load().fmpc_dm_profile_oomao_host(float(p2x), _hp(p3), _hp(p4), float(ratio), float(p6x), float(mech), cap, _hp(breaks), _hp(coef),
                                                C.byref(pieces))
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_dm_profile_oomao_host")
    return DMProfile(breaks[:pieces.value + 1], coef[:4 * pieces.value])


def dm_spline_matrix_workspace_bytes(n, m, rows, cols, minimum=False):
    """Second workspace of `SplineDM.influence_matrix` in bytes: the recommended size, or with minimum=True the smallest the call
    takes (the partial sums of one panel of 16 actuators); 0 for refused sizes."""
    rec = int(_lib.load().fmpc_dm_spline_matrix_workspace_bytes(int(n), int(m), int(rows), int(cols)))
    if not minimum or rec == 0:
        return rec
    tiles = (int(n) + 15) // 16
    chunk = 64 * (4 if tiles <= 2 else 2 if tiles == 3 else 1)
    supers = -(-int(rows) * int(cols) // (4 * chunk))
    return 8 * supers * 16 * 16 * tiles


class SplineDM:
    """x (cols), y (rows), cx, cy (m) as for `GaussianDM`; pitch in their unit; profile: a `DMProfile`.  The mirror is prepared
    once here (tables and per-tile actuator lists in `.ws`); after changing `.cx` / `.cy` in place call `.prepare()`.  Maps and
    screens are (cols, rows) planes indexed [column, row] -- pixel (r, c) at r + rows c."""

    def __init__(self, x, y, cx, cy, pitch, profile, device=0):
        import torch
        self._lib = _lib.load()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        conv = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1))).to(
            device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        self.x, self.y, self.cx, self.cy = conv(x), conv(y), conv(cx), conv(cy)
        self.pitch, self.profile = float(pitch), profile
        self.m, self.rows, self.cols = int(self.cx.numel()), int(self.y.numel()), int(self.x.numel())
        if self.m < 1 or int(self.cy.numel()) != self.m or self.rows < 1 or self.cols < 1:
            raise FastMPCError(_lib.FMPC_E_DIM, "SplineDM: need x, y and as many cx as cy")
        if not (self.pitch > 0.0 and np.isfinite(self.pitch)) or not isinstance(profile, DMProfile):
            raise FastMPCError(_lib.FMPC_E_DIM, "SplineDM: need a positive pitch and a DMProfile")
        self.npx = self.rows * self.cols
        self.breaks, self.coef = conv(profile.breaks), conv(profile.coef)
        need = int(self._lib.fmpc_dm_spline_workspace_bytes(self.m, self.rows, self.cols))
        if need == 0:
            raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "fmpc_dm_spline_workspace_bytes")
        self.ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self.prepare()

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def prepare(self, ws=None):
        """Writes the prepared mirror (tables, lists) from the current x, y, cx, cy into `.ws`, or into `ws`, a torch.uint8 HIP
        tensor of at least `.ws.numel()` bytes, which then becomes `.ws`.  Nothing is allocated: the call can be recorded."""
        if ws is not None:
            import torch
            if not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
                raise FastMPCError(_lib.FMPC_E_DIM, "ws: need a contiguous torch.uint8 HIP tensor")
        else:
            ws = self.ws
        rc = self._lib.fmpc_dm_spline_prepare_device(self.m, self.rows, self.cols, self._p(self.x), self._p(self.y), self._p(self.cx), self._p(self.cy),
                                                     self.pitch, self.profile.pieces, self._p(self.breaks), self._p(self.coef), self._p(ws),
                                                     ws.numel(), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_spline_prepare_device")
        self.ws = ws
        return self

    def tile_lists(self):
        """The prepared lists on the host: a list over tiles (tile (tr, tc) at tr + ntr * tc) of ascending actuator arrays."""
        ntr, ntc = -(-self.rows // FMPC_DM_TILE), -(-self.cols // FMPC_DM_TILE)
        mpad = 16 * ((self.m + 15) // 16)
        off = 8 * ((self.rows + self.cols) * mpad + self.m * FMPC_DM_TILE * (ntr + ntc))
        ints = self.ws[off:off + 4 * ntr * ntc * (1 + mpad)].cpu().numpy().view(np.int32)
        cnt, lists = ints[:ntr * ntc], ints[ntr * ntc:].reshape(ntr * ntc, mpad)
        return [lists[i, :cnt[i]].copy() for i in range(ntr * ntc)]

    def _planes(self, t, count, what):
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
        rc = self._lib.fmpc_dm_spline_influence_device(self.m, self.rows, self.cols, self._p(self.ws), first, count, self._p(I), ldi, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_spline_influence_device")
        return I

    def influence_matrix(self, modal, skip=1, workspace=None, out=None):
        """B = pinv(Z Z') Z I' without its first `skip` rows for the mode maps of `modal`, a `ModalFit` over maps of shape (cols,
        rows): arguments and result as `GaussianDM.influence_matrix`; workspace: a torch.uint8 HIP tensor of at least
        `dm_spline_matrix_workspace_bytes(n, m, rows, cols, minimum=True)` bytes."""
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
            ws2 = torch.empty(dm_spline_matrix_workspace_bytes(n, self.m, self.rows, self.cols), dtype=torch.uint8, device=self.device)
        else:
            ws2 = workspace
            if not ws2.is_cuda or ws2.dtype != torch.uint8 or not ws2.is_contiguous():
                raise FastMPCError(_lib.FMPC_E_DIM, "workspace: need a contiguous torch.uint8 HIP tensor")
        rc = self._lib.fmpc_dm_spline_matrix_device(n, self.m, self.rows, self.cols, self._p(modal.Z), self._p(modal.R), self._p(self.ws), skip,
                                                    self._p(B), ldb, self._p(ws2), ws2.numel(), self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_spline_matrix_device")
        return B

    def surface(self, u, phase=None, out=None, dense=False):
        """phase + sum_t u[b][t] I_t (phase None: the surface alone); arguments as `GaussianDM.surface`.  dense=True walks all m
        actuators in every tile instead of the tile's list (for timing and tests)."""
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
        rc = self._lib.fmpc_dm_spline_surface_device(batch, self.m, self.rows, self.cols, self._p(self.ws), self._p(uu), ldu, self._p(ph), ldp,
                                                     self._p(o), ldo, FMPC_DM_DENSE if dense else 0, self._stream())
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_dm_spline_surface_device")
        return o[0] if single else o


def oomao_dm_geometry(n_act, resolution, ratio_tel_dm=1.0, offset=(0.0, 0.0), valid=None):
    """The grid of OOMAO's setInfluenceFunction (influenceFunction.m:253-314) in pitch units (pitch = 1):
    xIF = linspace(-1, 1, n_act) (n_act - 1) / 2 - offset[0], yIF alike with offset[1]; the pixel axis
    u0 = ratio_tel_dm linspace(-1, 1, resolution) (n_act - 1) / 2 for rows and columns alike; actuator k runs column-major over the
    valid (i, j) of `valid` ((n_act, n_act) bool, None: all).  The maps OOMAO forms are wv(:, i) * wu(:, j)': k's ROW profile is
    centred on yIF[i] and its COLUMN profile on xIF[j], so cy = yIF[i], cx = xIF[j].  With a non-zero offset OOMAO's own
    actuatorCoord (xIF[i] + 1i yIF[j]) says the opposite; this follows the maps.  Returns a dict of x, y, cx, cy, pitch."""
    n_act, resolution = int(n_act), int(resolution)
    if n_act < 2 or resolution < 1:
        raise ValueError("oomao_dm_geometry: need n_act >= 2 and resolution >= 1")
    half = (n_act - 1) / 2
    xIF = np.linspace(-1.0, 1.0, n_act) * half - float(offset[0])
    yIF = np.linspace(-1.0, 1.0, n_act) * half - float(offset[1])
    u0 = float(ratio_tel_dm) * np.linspace(-1.0, 1.0, resolution) * half
    v = np.ones((n_act, n_act), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(n_act, n_act)
    i, j = np.nonzero(v.T)[::-1]                                          # column-major over (i, j): j outer, i inner
    return dict(x=u0.copy(), y=u0.copy(), cx=xIF[j], cy=yIF[i], pitch=1.0)


def oomao_dm(n_act, resolution, mech, kind="monotonic", points=None, ratio_tel_dm=1.0, offset=(0.0, 0.0), valid=None, device=0):
    """The `SplineDM` of `oomao_dm_geometry` with `oomao_profile(mech, kind, points)`; the host geometry is in `.geometry`."""
    g = oomao_dm_geometry(n_act, resolution, ratio_tel_dm, offset, valid)
    dm = SplineDM(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], oomao_profile(mech, kind, points), device=device)
    dm.geometry = g
    return dm
