"""VAR identification on the device: the step of the reference notebook that produces A1, A2 from an open-loop
series of Zernike coefficients (README.md:108-130) and scores the model on the validation stretch (README.md:132-153),
above `fmpc_var_identify_device`, `fmpc_var_fit_device` and `fmpc_var_validate_device` (include/fastmpc.h)."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import FastMPCError


def identify_var2_device(series, num_train=None):
    """series: torch float64 HIP tensor (batch, num_samples, n) or (num_samples, n) -- ad_acc with the piston column
    removed, one row per time step.  Returns (A1, A2, status): (batch, n, n) tensors with A[b, i, j] = A_b(i, j)."""
    import torch
    lib = _lib.load()
    single = series.dim() == 2
    s = series.unsqueeze(0) if single else series
    if not s.is_cuda or s.dtype != torch.float64 or not s.is_contiguous():
        raise FastMPCError(_lib.FMPC_E_DIM, "series: need a contiguous float64 HIP tensor")
    batch, ns, n = s.shape
    nt = ns if num_train is None else int(num_train)
    A1 = torch.empty((batch, n, n), dtype=torch.float64, device=s.device)       # filled column-major: transposed below
    A2 = torch.empty_like(A1)
    st = torch.zeros(batch, dtype=torch.int32, device=s.device)
    stream = C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.fmpc_var_identify_device(n, nt, ns, batch, p(s), p(A1), p(A2), p(st), stream)
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_var_identify_device")
    A1, A2 = A1.transpose(1, 2), A2.transpose(1, 2)                              # column-major n x n -> [i, j]
    return (A1[0], A2[0], st[0]) if single else (A1, A2, st)


def _series3(series):
    import torch
    single = series.dim() == 2
    s = series.unsqueeze(0) if single else series
    if not s.is_cuda or s.dtype != torch.float64 or not s.is_contiguous():
        raise FastMPCError(_lib.FMPC_E_DIM, "series: need a contiguous float64 HIP tensor")
    return s, single


def var_fit_workspace_bytes(n, order=2, batch=1):
    """Recommended workspace of `identify_var_device` in bytes (batch = 1: the minimum, one slot; 0: none needed)."""
    return int(_lib.load().fmpc_var_fit_workspace_bytes(int(n), int(order), int(batch)))


def identify_var_device(series, order=2, num_train=None, workspace=None, out=None):
    """VAR(order) identification, order 1 or 2, p = order * n <= 224.  series as for `identify_var2_device`.  Returns
    (A1, A2, status), (A, None, status) at order 1, with the strides of `identify_var2_device` (A[b, i, j] = A_b(i, j) over
    column-major storage, so they go into `set_model_bank` by pointer).  workspace: a torch.uint8 HIP tensor of at least
    `var_fit_workspace_bytes(n, order, 1)` bytes (allocated at the recommended size when None); out: (A1, A2, status) tensors
    of an earlier call to fill again (nothing is allocated then: the form to record into a graph)."""
    import torch
    lib = _lib.load()
    s, single = _series3(series)
    batch, ns, n = s.shape
    order = int(order)
    nt = ns if num_train is None else int(num_train)
    if workspace is None:
        workspace = torch.empty(var_fit_workspace_bytes(n, order, batch), dtype=torch.uint8, device=s.device)
    if out is None:
        A1 = torch.empty((batch, n, n), dtype=torch.float64, device=s.device)   # filled column-major: transposed below
        A2 = torch.empty_like(A1) if order == 2 else None
        st = torch.zeros(batch, dtype=torch.int32, device=s.device)
    else:
        A1, A2, st = (t if t is None or not single else t.unsqueeze(0) for t in out)
        A1 = A1.transpose(1, 2)
        A2 = None if A2 is None else A2.transpose(1, 2)
        if not A1.is_contiguous() or (A2 is not None and not A2.is_contiguous()) or tuple(A1.shape) != (batch, n, n):
            raise FastMPCError(_lib.FMPC_E_DIM, "out: need the tensors an earlier call returned")
    stream = C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)
    p = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    rc = lib.fmpc_var_fit_device(n, order, nt, ns, batch, p(s), p(A1), p(A2), p(st), p(workspace), workspace.numel(), stream)
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_var_fit_device")
    A1 = A1.transpose(1, 2)                                                      # column-major n x n -> [i, j]
    A2 = None if A2 is None else A2.transpose(1, 2)
    return (A1[0], None if A2 is None else A2[0], st[0]) if single else (A1, A2, st)


def validate_var_device(series, A1, A2=None, first=None, count=None, want_rrmse=True, out=None):
    """One-step prediction errors of the model (A1, A2) -- per series, as `identify_var_device` returns them, or any strided
    view -- on samples first .. first + count - 1 (0-based) of each series: returns (rmse, rrmse), (batch, n) tensors, rrmse
    None with want_rrmse=False.  first defaults to num_samples // 2, count to the rest of the series.  out: (rmse, rrmse) to
    fill again."""
    import torch
    lib = _lib.load()
    s, single = _series3(series)
    batch, ns, n = s.shape
    order = 1 if A2 is None else 2
    first = ns // 2 if first is None else int(first)
    count = ns - first if count is None else int(count)

    def colmajor(A):                                                            # [b, i, j] -> contiguous column-major storage
        A = A.unsqueeze(0) if single else A
        if tuple(A.shape) != (batch, n, n) or A.dtype != torch.float64 or not A.is_cuda:
            raise FastMPCError(_lib.FMPC_E_DIM, "A1, A2: need (batch, n, n) float64 HIP tensors")
        At = A.transpose(1, 2)
        return At if At.is_contiguous() else At.contiguous()
    M1 = colmajor(A1)
    M2 = None if A2 is None else colmajor(A2)
    if out is None:
        rmse = torch.empty((batch, n), dtype=torch.float64, device=s.device)
        rrmse = torch.empty_like(rmse) if want_rrmse else None
    else:
        rmse, rrmse = (t if t is None or not single else t.unsqueeze(0) for t in out)
    stream = C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.fmpc_var_validate_device(n, order, first, count, ns, batch, p(s), p(M1), p(M2), p(rmse), p(rrmse), stream)
    if rc != _lib.FMPC_OK:
        raise FastMPCError(rc, "fmpc_var_validate_device")
    return (rmse[0], None if rrmse is None else rrmse[0]) if single else (rmse, rrmse)
