"""Closed-loop records on the device: what the reference's timestep computes after the solve (README.md:576-622) --
X_predicted (:592), x_prev (:594), the per-stage error norms X_err (:603-607), the cost J (:588), du_prev (:611-615) and the
rad -> V conversion U_v (:576-585) -- for all realisations at once, from the loop's own device buffers
(`fmpc_loop_records_device`, `fmpc_loop_records_run_device` in include/fastmpc.h; with one VAR model per realisation their
`..._bank_device` forms).
"""
from __future__ import annotations


class LoopRecords:
    """Owns the output tensors of the records of `batch` realisations.  volts = (coeff_a, coeff_b, unit_change) of the rad -> V
    conversion (README.md:350, 577-583); None: no `uv`.

    `.step(...)` fills and returns views of  Xp (batch, stages, n), x_prev (batch, n) = Xp[:, 0], xerr (batch, stages),
    J (batch,) (full horizon only), du (batch, m), uv (batch, m).  `.stretch(...)` returns Xp0 (steps, batch, n),
    xerr0 (steps, batch), dU, Uv (steps, batch, m) in tensors of its own size (kept and reused while `steps` stays the same).

    With a model bank (`handle.set_model_bank`): `.step_bank(..., model_of=...)` and `.stretch(..., bank=True, model_of=...)` predict
    with model model_of[p] of the handle's bank per realisation (int32 HIP tensor of (batch,); None: model p)."""

    def __init__(self, handle, batch, volts=None, device=None):
        import torch
        self.h, self.batch = handle, int(batch)
        self.volts = None if volts is None else tuple(float(v) for v in volts)
        if self.volts is not None and len(self.volts) != 3:
            raise ValueError("volts: (coeff_a, coeff_b, unit_change)")
        dev = torch.device("cuda", handle.device) if device is None else device
        f64 = dict(dtype=torch.float64, device=dev)
        n, m, T = handle.n, handle.m, handle.T
        self._f64 = f64
        self.Xp = torch.zeros((self.batch, T, n), **f64)
        self.xerr = torch.zeros((self.batch, T), **f64)
        self.J = torch.zeros((self.batch,), **f64)
        self.du = torch.zeros((self.batch, m), **f64)
        self.uv = torch.zeros((self.batch, m), **f64) if self.volts is not None else None
        self._stretch = None

    def step(self, x0, x0_pre, w, u1, z=None, u0=None):
        """The records of one timestep.  z (batch, nz), rows possibly padded: all T stages and J; else u0 (batch, m): stage 0 only."""
        return self._step(x0, x0_pre, w, u1, z, u0, False, None)

    def step_bank(self, x0, x0_pre, w, u1, z=None, u0=None, model_of=None):
        """`step` where realisation p predicts with model model_of[p] of the handle's bank (None: model p)."""
        return self._step(x0, x0_pre, w, u1, z, u0, True, model_of)

    def _step(self, x0, x0_pre, w, u1, z, u0, bank, model_of):
        if (z is None) == (u0 is None):
            raise ValueError("LoopRecords.step: exactly one of z and u0")
        h, b = self.h, self.batch
        if bank:
            call = lambda *a, **kw: h.loop_records_bank_device(*a, model_of=model_of, **kw)
        else:
            call = h.loop_records_device
        if z is not None:
            call(x0, x0_pre, w, z, u1, stages=h.T, ldu=z.stride(0), stage_stride=h.n + h.m, volts=self.volts,
                 Xp=self.Xp, xerr=self.xerr, J=self.J, du=self.du, uv=self.uv)
            out = {"Xp": self.Xp, "x_prev": self.Xp[:, 0], "xerr": self.xerr, "J": self.J, "du": self.du}
        else:
            Xp = self.Xp.view(-1)[: b * h.n].view(b, 1, h.n)
            xerr = self.xerr.view(-1)[:b].view(b, 1)
            call(x0, x0_pre, w, u0, u1, stages=1, ldu=h.m, volts=self.volts, Xp=Xp, xerr=xerr, du=self.du, uv=self.uv)
            out = {"Xp": Xp, "x_prev": Xp[:, 0], "xerr": xerr, "du": self.du}
        if self.uv is not None:
            out["uv"] = self.uv
        return out

    def stretch(self, X0, U0, x0_before=None, u_before1=None, u_before2=None, model_of=None, bank=False):
        """The stage-0 records of every step of a recorded stretch (X0, U0 of `ClosedLoop.run_recorded`) in one launch.
        bank=True: with A1, A2 of the bank's model model_of[p] (None: model p)."""
        import torch
        steps = X0.shape[0]
        h, b = self.h, self.batch
        if self._stretch is None or self._stretch["Xp0"].shape[0] != steps:
            self._stretch = {"Xp0": torch.zeros((steps, b, h.n), **self._f64), "xerr0": torch.zeros((steps, b), **self._f64),
                             "dU": torch.zeros((steps, b, h.m), **self._f64)}
            if self.volts is not None:
                self._stretch["Uv"] = torch.zeros((steps, b, h.m), **self._f64)
        S = self._stretch
        if model_of is not None and not bank:
            raise ValueError("model_of needs bank=True")
        out = dict(volts=self.volts, Xp0=S["Xp0"], xerr0=S["xerr0"], dU=S["dU"], Uv=S.get("Uv"))
        if bank:
            h.loop_records_run_bank_device(X0, U0, x0_before, u_before1, u_before2, model_of=model_of, **out)
        else:
            h.loop_records_run_device(X0, U0, x0_before, u_before1, u_before2, **out)
        return dict(S)
