"""Device-resident coefficient-space closed loop around the fastMPC solve.

Mirrors the steps either side of the solver in the reference's simulation loop (README.md:444-622) for R
independent realisations at once, with the phase-screen estimator (README.md:456-480, out of scope) replaced by
the caller's residual-free turbulence coefficients a[k]:

    x0 = a[k] + B u[k-1]                      residual after the mirror's correction (README.md:482-483, 589-590)
    x0_pre = previous x0                      README.md:484-488
    w = b_ref = -M1 B u[k-1] - M2 B u[k-2]    README.md:490-497
    z = Fast_MPC2(..., w, [], []).mpc_fixed_log_newton(n_fix, k_fix)      README.md:547-555
    u[k] = U(1:nu)                            README.md:589

Everything stays in HBM between the steps: one call per step on torch's current stream (`fmpc_loop_step_device` =
`fmpc_loop_inputs_device` + `fmpc_solve_u0_device`; the two separate calls with `fused=False` or ramp rows), no host
round trip.
"""
from __future__ import annotations


class ClosedLoop:
    """ramp=True (after `handle.set_ramp`): every solve carries the VAR_1 variant's ramp-rate rows against the
    previous first move, u_prev = U(1:nu) (README.md:589; VAR_1/fast_mpc_ineq_const.m:58-76), zeros at the first step."""

    def __init__(self, handle, batch, n_newton=1, k=1e-2, device=None, ramp=False, fused=True, keep_z=True, bank=False, model_of=None):
        import torch
        # bank=True (after `handle.set_model_bank`): realisation p runs with model model_of[p] of the handle's bank (int32 HIP tensor;
        # None: model p), as in the reference, where every realisation identifies its own A1, A2 (README.md:108-130) -- `step` and
        # `run_recorded` go through fmpc_loop_step_bank_device / fmpc_loop_run_bank_device; with `handle.prefactor_model_bank(k)`
        # every step sweeps through its model's stored cold-start factor.
        self.bank = bool(bank)
        if self.bank and ramp:
            raise ValueError("ClosedLoop: the model bank has no form with ramp-rate rows")
        if model_of is not None and not (self.bank and model_of.is_cuda and model_of.dtype == torch.int32 and model_of.is_contiguous()
                                         and model_of.numel() == int(batch)):
            raise ValueError("model_of: needs bank=True and a contiguous int32 HIP tensor of (batch,)")
        self.model_of = model_of
        self.h, self.batch, self.n_newton, self.k = handle, int(batch), int(n_newton), float(k)
        dev = torch.device("cuda", handle.device) if device is None else device
        f64 = dict(dtype=torch.float64, device=dev)
        n, m, T = handle.n, handle.m, handle.T
        # x0 alternates between two buffers (the fused step reads x0[k-1] while it writes x0[k]: with the update in place the
        # library cannot do loop inputs, first moves and decision in ONE launch -- fmpc_loop_step_device in include/fastmpc.h)
        self._xb = [torch.zeros((batch, n), **f64) for _ in range(2)]
        self._cur = 0
        self.x0_pre = torch.zeros((batch, n), **f64)
        self.w = torch.zeros((batch, T * n), **f64)
        self.u = [torch.zeros((batch, m), **f64) for _ in range(3)]     # ring: u[k], u[k-1], u[k-2]
        # keep_z=False: only the first moves leave the solve (z_out = NULL at the C ABI; README.md:589 applies U(1:nu) only)
        self.z = torch.empty((batch, handle.nz), **f64) if keep_z else None
        self.status = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.steps_done = 0
        self.ramp = bool(ramp)
        self.fused = bool(fused)        # one C call per step (fmpc_loop_step_device) instead of two
        # The fused step is one C call whose arguments, apart from a[k] and nu0, are this object's own buffers: their
        # pointers are built once (a sequential loop of one realisation is bound by the HOST time per step otherwise:
        # tensor checks and ctypes conversions cost more than the two launches of the first-move form).
        import ctypes as C
        self._C, self._torch, self._dev = C, torch, dev
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._p = dict(xb=[vp(b) for b in self._xb], x0_pre=vp(self.x0_pre), w=vp(self.w), u=[vp(u) for u in self.u], z=vp(self.z),
                       status=vp(self.status), iters=vp(self.iters))
        self._fn = handle._lib.fmpc_loop_step_device
        self._p["model_of"] = vp(model_of)
        self._n_newton_c, self._k_c = int(self.n_newton), float(self.k)

    @property
    def x0(self):
        """x0 of the last step (batch, n)."""
        return self._xb[self._cur]

    def _step_fused(self, a_k, nu0, s):
        torch, C = self._torch, self._C
        if a_k.dtype != torch.float64 or not a_k.is_cuda or not a_k.is_contiguous() or a_k.shape[0] != self.batch or a_k.shape[-1] != self.h.n:
            raise ValueError("a_k: need a contiguous float64 HIP tensor of shape (batch, n)")
        if nu0 is not None and (nu0.dtype != torch.float64 or not nu0.is_contiguous() or nu0.numel() != self.batch * self.h.nu_len):
            raise ValueError("nu0: need a contiguous float64 HIP tensor of shape (batch, nu_len)")
        P = self._p
        u = P["u"]
        cur = self._cur
        rc = self._fn(self.h._h, self.batch, C.c_void_p(a_k.data_ptr()), P["xb"][cur] if s >= 1 else None, u[(s - 1) % 3] if s >= 1 else None,
                      u[(s - 2) % 3] if s >= 2 else None, P["xb"][1 - cur], P["x0_pre"], P["w"], None if nu0 is None else C.c_void_p(nu0.data_ptr()),
                      self._n_newton_c, self._k_c, P["z"], None, P["status"], P["iters"], None, u[s % 3],
                      C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream))
        if rc != 0:
            from ._lib import FastMPCError
            raise FastMPCError(rc, "fmpc_loop_step_device")
        self._cur = 1 - cur

    def step(self, a_k, nu0=None):
        """One closed-loop step for all realisations.  a_k: (batch, n) device tensor.  Returns u[k] (batch, m),
        a view into the loop's ring buffer (valid until two further steps)."""
        s = self.steps_done
        u_new, u1, u2 = self.u[s % 3], self.u[(s - 1) % 3], self.u[(s - 2) % 3]
        if self.bank:
            # (x0 in place: fmpc_loop_inputs_bank_device reads x0_last before it writes x0)
            self.h.loop_step_bank(a_k, self.x0 if s >= 1 else None, u1 if s >= 1 else None, u2 if s >= 2 else None, self.x0, self.x0_pre,
                                  self.w, nu0, self.n_newton, self.k, model_of=self.model_of, z_out=self.z, status=self.status,
                                  iters=self.iters, u0_out=u_new)
        elif self.ramp or not self.fused:
            self.h.loop_inputs_device(a_k, self.x0 if s >= 1 else None, u1 if s >= 1 else None, u2 if s >= 2 else None,
                                      self.x0, self.x0_pre, self.w)
            self.h.solve_device(self.x0, self.x0_pre, self.w, None, nu0, self.n_newton, self.k, z_out=self.z,
                                status=self.status, iters=self.iters, u_prev=u1 if self.ramp else None, u0_out=u_new,
                                want_z=self.z is not None)
        else:
            self._step_fused(a_k, nu0, s)
        self.steps_done = s + 1
        return u_new

    def records(self, rec):
        """The records of the step just done (README.md:576-622) through `rec` (a `LoopRecords`): the full horizon and J from z with
        keep_z, stage 0 from the newest first move without; on the bank, with this loop's model_of.  Returns rec.step's dict of views."""
        if self.steps_done < 1:
            raise ValueError("records: no step has been done")
        s = self.steps_done - 1
        u1 = self.u[(s - 1) % 3] if s >= 1 else None
        # (a bank loop predicts with its own model_of: fmpc_loop_records_bank_device)
        step = (lambda *a, **kw: rec.step_bank(*a, model_of=self.model_of, **kw)) if self.bank else rec.step
        if self.z is not None:
            return step(self.x0, self.x0_pre, self.w, u1, z=self.z)
        return step(self.x0, self.x0_pre, self.w, u1, u0=self.u[s % 3])

    def run_recorded(self, a, nu0=None, want_x0=True, records=None):
        """The whole stretch a (steps, batch, n) in ONE C call (fmpc_loop_run_device): first moves only, fed back on the device.
        Continues from this object's state.  Returns (U0 (steps, batch, m), X0 (steps, batch, n) or None).
        records (a `LoopRecords`): the stage-0 records of every step of the stretch as well, in one more launch
        (`LoopRecords.stretch` on U0, X0 and the ring state from before the stretch, with the loop's model_of when it runs on
        the bank); returns (U0, X0, dict of records)."""
        if records is not None:
            if not want_x0:
                raise ValueError("run_recorded: records need X0")
            s0 = self.steps_done
            before = (self.x0.clone() if s0 >= 1 else None, self.u[(s0 - 1) % 3].clone() if s0 >= 1 else None,
                      self.u[(s0 - 2) % 3].clone() if s0 >= 2 else None)
            U0, X0 = self.run_recorded(a, nu0, True)
            return U0, X0, records.stretch(X0, U0, *before, model_of=self.model_of, bank=self.bank)
        torch, C = self._torch, self._C
        if not self.bank and (self.ramp or not self.fused):
            raise ValueError("run_recorded: the fused step without ramp rows only")
        steps = a.shape[0]
        assert a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and tuple(a.shape[1:]) == (self.batch, self.h.n)
        assert nu0 is None or (nu0.is_contiguous() and nu0.dtype == torch.float64 and nu0.numel() == steps * self.batch * self.h.nu_len)
        U0 = torch.empty((steps, self.batch, self.h.m), dtype=torch.float64, device=a.device)
        X0 = torch.empty((steps, self.batch, self.h.n), dtype=torch.float64, device=a.device) if want_x0 else None
        s = self.steps_done
        P = self._p
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        if self.bank:
            self.h.loop_run_bank(a, self.x0, self.x0_pre, self.w, U0, X0, None if nu0 is None else nu0.view(steps, self.batch, self.h.nu_len),
                                 self.u[(s - 1) % 3] if s >= 1 else None, self.u[(s - 2) % 3] if s >= 2 else None, s >= 1,
                                 self.n_newton, self.k, model_of=self.model_of, status=self.status, iters=self.iters)
            for j in range(min(steps, 2)):
                self.u[(s + steps - 1 - j) % 3].copy_(U0[steps - 1 - j])
            self.steps_done = s + steps
            return U0, X0
        rc = self.h._lib.fmpc_loop_run_device(self.h._h, self.batch, steps, vp(a), vp(nu0), P["u"][(s - 1) % 3] if s >= 1 else None,
                                              P["u"][(s - 2) % 3] if s >= 2 else None, 1 if s >= 1 else 0, self._n_newton_c, self._k_c,
                                              P["xb"][self._cur], P["x0_pre"], P["w"], vp(U0), vp(X0), P["status"], P["iters"],
                                              C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream))
        if rc != 0:
            from ._lib import FastMPCError
            raise FastMPCError(rc, "fmpc_loop_run_device")
        # keep the ring consistent for a following step(): u[k-1], u[k-2] of the next step
        for j in range(min(steps, 2)):
            self.u[(s + steps - 1 - j) % 3].copy_(U0[steps - 1 - j])
        self.steps_done = s + steps
        return U0, X0

    def run(self, a, nu0=None):
        """a: (steps, batch, n) device tensor.  Returns (U0 (steps, batch, m), X0 (steps, batch, n))."""
        import torch
        steps = a.shape[0]
        U0 = torch.empty((steps, self.batch, self.h.m), dtype=torch.float64, device=a.device)
        X0 = torch.empty((steps, self.batch, self.h.n), dtype=torch.float64, device=a.device)
        for s in range(steps):
            u = self.step(a[s], None if nu0 is None else nu0[s])
            U0[s].copy_(u); X0[s].copy_(self.x0)
        return U0, X0


class AOLoop:
    """The reference's simulation loop WITH its estimator on the device (README.md:444-626) for `batch` realisations at once:
    residual screen = phase_valid[k] + sum_j (B u[k-1])_j Z_j (`fmpc_phase_residual_device`), the phase-diversity estimator
    (`PhaseDiversityEstimator`: three PSF windows, ad_est = G (Y_M - b_s)), x0 = ad_est, x0_pre = the previous ad_est,
    b_ref from the last two first moves (`fmpc_loop_inputs_device`), the fastMPC solve, u[k] = U(1:nu).
    Z: (n, len, len) mode maps indexed [j, row, column] (piston removed), a host array or a tensor (a HIP tensor is not taken
    through the host; z_colmajor=True: it is indexed [j, column, row] already, the order of `optics.zernike_grid`).  Screens are handed over indexed [b, row, column].
    modal (optional): a `ModalFit` over the n + 1 mode maps WITH the piston, indexed as the screens are handed over; it gives
    `true_coefficients`, the reference's ad_acc_valid, and changes nothing else.
    dm (optional): a `GaussianDM` on the estimator's grid (rows = cols = len); the residual screen of a step is then
    phase_valid[k] + sum_t u[k-1]_t I_t, the surface the mirror of Gaussian actuators makes (`fmpc_dm_surface_device`), instead of
    the modal one; nothing else changes.  A `SplineDM` (dm_spline.py) has the same rows, cols, m and surface() and goes in alike.
    science (optional): a `ScienceCamera` on the estimator's grid; every step exposes the residual screen it has just formed
    (`scrn`, column-major, no copy): `science_quality` (batch, FMPC_SCI_FIELDS) holds this step's rows, `science_image` (batch, d, d)
    the exposure accumulated over `science_frames` steps since the last `science_reset()`; nothing else changes.
    sensor (optional): a calibrated `ShackHartmann` on the estimator's grid with the handle's n modes; x0 of a step is then
    `sensor.coefficients(scrn)` instead of the estimator's ad_est, and `noise` of `step` may be None or a `DetectorNoise`, which is
    applied to the sensor's frame (measure the frame, `detector_read` on it, slopes and coefficients from what was read) with
    `steps_done` as its step; nothing else changes.
    refine (optional): dict(optics=an `EstimatorOptics` of the estimator's geometry, iters=3, damping=0.0, tol=0.0); a step then
    takes Y_M of `apply_device` (noise of any kind included) and refines x0 in place from it with the exact image model
    (`EstimatorOptics.refine` over the loop's own Z, the start the linear estimate) before the solve; `refine_info`
    (batch, FMPC_REFINE_FIELDS) and `refine_status` (batch,) hold the last call's rows; nothing else changes.  Not with sensor=.
    Two further keys are optional: refresh (1: J every iteration; r > 1: every r-th, held in between; 0: the gain form without a
    Jacobian, damping 0) and G, the gain form's (n, p) matrix (None: `optics.gain(Z)`, computed once here).
    weighted=True (with floor=1.0, refresh >= 1): a step whose `noise` is a `DetectorNoise` refines with that detector's
    parameters (`EstimatorOptics.refine(detector=noise, floor=)`: the fit weighted by the photon and read-out variance);
    `refine_info` then holds chi^2 and `refine_sigma` (batch, n) the predicted standard deviation of x0; a step with another
    kind of noise, or none, raises.  Without the key every path is as above."""

    def __init__(self, handle, estimator, Z, batch, n_newton=1, k=1e-2, one_call=True, modal=None, z_colmajor=False, science=None, sensor=None,
                 refine=None, dm=None):
        import ctypes as C
        import numpy as np
        import torch
        self.h, self.est, self.batch, self.n_newton, self.k = handle, estimator, int(batch), int(n_newton), float(k)
        self.one_call = bool(one_call)      # b_ref + fastMPC step as ONE C call (fmpc_ao_step_device); False: loop inputs and solve as two
        dev = torch.device("cuda", handle.device)
        f64 = dict(dtype=torch.float64, device=dev)
        n, m, T = handle.n, handle.m, handle.T
        assert Z.shape[0] == n and Z.shape[1] == estimator.len
        if torch.is_tensor(Z):               # a device tensor (optics.zernike_grid) stays on the device
            Zt = Z.to(device=dev, dtype=torch.float64)
            self.Z = Zt.contiguous() if z_colmajor else Zt.transpose(-1, -2).contiguous()
        else:
            if z_colmajor:
                raise ValueError("z_colmajor: only for a tensor Z")
            self.Z = torch.from_numpy(np.ascontiguousarray(np.swapaxes(np.asarray(Z, dtype=np.float64), -1, -2))).to(dev)   # column-major planes
        self.npx = estimator.len ** 2
        self.scrn = torch.empty((batch, estimator.len, estimator.len), **f64)
        self._xb = [torch.zeros((batch, n), **f64) for _ in range(2)]          # ad_est of this and of the previous step, in turn
        self.x0, self.x0_pre = self._xb[0], self._xb[1]
        self.w = torch.zeros((batch, T * n), **f64)
        self._scr_x = torch.zeros((batch, n), **f64); self._scr_xp = torch.zeros((batch, n), **f64); self._zero_a = torch.zeros((batch, n), **f64)
        self.u = [torch.zeros((batch, m), **f64) for _ in range(3)]
        self.status = torch.zeros(batch, dtype=torch.int32, device=dev); self.iters = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.steps_done = 0
        self._C, self._torch, self._dev = C, torch, dev
        if modal is not None and modal.n != n + 1:
            raise ValueError("modal: need the fit over the n + 1 modes with the piston")
        self.modal = modal
        if dm is not None and (dm.rows != estimator.len or dm.cols != estimator.len or dm.m != m):
            raise ValueError("dm: need a GaussianDM of the handle's m actuators on the estimator's len x len grid")
        self.dm = dm
        if science is not None and science.len != estimator.len:
            raise ValueError("science: need a ScienceCamera on the estimator's len x len grid")
        self.science = science
        if science is not None:
            from .science import FMPC_SCI_FIELDS
            self.science_image = torch.zeros((batch, science.d, science.d), **f64)
            self.science_quality = torch.zeros((batch, FMPC_SCI_FIELDS), **f64)
            self.science_frames = 0
            self._science_ws = torch.empty(science.workspace_bytes(batch), dtype=torch.uint8, device=dev)
        if sensor is not None and (sensor.len != estimator.len or sensor.nmode != n):
            raise ValueError("sensor: need a ShackHartmann on the estimator's len x len grid, calibrated for the handle's n modes")
        self.sensor = sensor
        if sensor is not None:
            self._sensor_frame = torch.empty((batch, sensor.frame_len, sensor.frame_len), **f64)
            self._sensor_slopes = torch.empty((batch, 2 * sensor.nvalid), **f64)
        self.refine = None
        if refine is not None:
            if sensor is not None:
                raise ValueError("refine: the refinement works on the estimator's images; not together with sensor=")
            unknown = set(refine) - {"optics", "iters", "damping", "tol", "refresh", "G", "weighted", "floor"}
            if unknown or "optics" not in refine:
                raise ValueError("refine: need dict(optics=, iters=, damping=, tol=[, refresh=, G=, weighted=, floor=])")
            opt = refine["optics"]
            if (opt.len, opt.p) != (estimator.len, estimator.p):
                raise ValueError("refine: need an EstimatorOptics of the estimator's grid, window and diversities")
            from ._lib import FMPC_REFINE_FIELDS
            refresh = int(refine.get("refresh", 1))
            if refresh < 0:
                raise ValueError("refine: refresh >= 0")
            weighted = bool(refine.get("weighted", False))
            if weighted and refresh < 1:
                raise ValueError("refine: the weighted fit needs refresh >= 1 (the gain form has no weighted G)")
            if "floor" in refine and not weighted:
                raise ValueError("refine: floor= is the weighted fit's")
            G = refine.get("G")
            if refresh == 0 and G is None:   # the gain about zero aberration, once (it synchronises)
                G = opt.gain(self.Z)
            self.refine = dict(optics=opt, iters=int(refine.get("iters", 3)), damping=float(refine.get("damping", 0.0)), tol=float(refine.get("tol", 0.0)),
                               refresh=refresh, G=G if refresh == 0 else None, weighted=weighted, floor=float(refine.get("floor", 1.0)))
            if weighted:
                from .estimator import DetectorNoise
                self._DetectorNoise = DetectorNoise
                self.refine_sigma = torch.full((batch, n), float("nan"), **f64)
            self.refine_info = torch.zeros((batch, FMPC_REFINE_FIELDS), **f64)
            self.refine_status = torch.zeros(batch, dtype=torch.int32, device=dev)
            self._refine_ws = torch.empty(opt.refine_workspace_bytes(n, batch, refresh=refresh), dtype=torch.uint8, device=dev)

    def science_reset(self):
        """Start a new exposure: the accumulated image and the frame count go back to zero (after the uncorrected first step, say)."""
        if self.science is None:
            raise ValueError("science_reset: this loop was built without science=")
        self.science_image.zero_()
        self.science_frames = 0

    def science_summary(self, nrad=None):
        """`ScienceCamera.summary` of the current exposure: long-exposure Strehl, window energy, encircled energy."""
        if self.science is None:
            raise ValueError("science_summary: this loop was built without science=")
        if self.science_frames < 1:
            raise ValueError("science_summary: no frame since the last science_reset")
        return self.science.summary(self.science_image, self.science_frames, nrad)

    def true_coefficients(self, phase_k, workspace=None, out=None):
        """The modal fit of the incoming screens with the piston dropped (zernmodfit of phase_valid(:,:,k): a row of ad_acc_valid,
        what X_est_err of README.md:479 is judged against).  phase_k: (batch, ...) over the pixel shape of the `ModalFit`."""
        if self.modal is None:
            raise ValueError("true_coefficients: this loop was built without modal=")
        return self.modal.fit(phase_k, skip=1, workspace=workspace, out=out)

    def step(self, phase_k, noise=None, colmajor=False):
        """phase_k: (batch, len, len) float64 HIP tensor indexed [b, row, column] (phase_valid(:,:,k) of every realisation);
        colmajor=True: indexed [b, column, row] already -- the order MATLAB keeps phase_valid(:,:,k) in -- and no copy is made.
        noise: None, the (batch, p) tensor Y_M_noise of this step, or an `EstimatorNoise` / a `DetectorNoise` that is drawn on the
        device with `steps_done` as its step (README.md:473-475).
        Returns (u[k] (batch, m), ad_est (batch, n)); both views valid until two further steps / the next step."""
        torch, C = self._torch, self._C
        s = self.steps_done
        u_new, u1, u2 = self.u[s % 3], self.u[(s - 1) % 3], self.u[(s - 2) % 3]
        ph = phase_k if colmajor else phase_k.transpose(-1, -2).contiguous()          # column-major planes, as the mode maps
        assert ph.is_contiguous() and ph.dtype == torch.float64
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)
        if self.dm is not None:              # the zonal surface of the mirror (no correction before the first move: README.md:447)
            if s >= 1:
                self.dm.surface(u1, phase=ph, out=self.scrn)
            else:
                self.scrn.copy_(ph)
        else:
            rc = self.h._lib.fmpc_phase_residual_device(self.h._h, self.batch, self.npx, vp(ph), vp(u1) if s >= 1 else None, vp(self.Z), vp(self.scrn), stream)
            if rc != 0:
                from ._lib import FastMPCError
                raise FastMPCError(rc, "fmpc_phase_residual_device")
        if self.science is not None:         # the camera sees the residual wavefront the estimator sees
            self.science.expose(self.scrn, image=self.science_image, accumulate=True, quality=self.science_quality, colmajor=True,
                                workspace=self._science_ws)
            self.science_frames += 1
        # x0 = ad_est, x0_pre = the previous ad_est (README.md:482-488): two buffers in turn, the estimator writes into this step's
        self.x0, self.x0_pre = self._xb[s % 2], self._xb[(s + 1) % 2]
        if s == 0:
            self.x0_pre.zero_()
        if self.refine is not None:          # the linear estimate, then Gauss-Newton on the images it was made from
            Y = self.est.apply_device(self.scrn, noise, want_Y=True, colmajor=True, out=self.x0, step=s)[1]
            rf = self.refine
            if rf["weighted"]:
                if not isinstance(noise, self._DetectorNoise):
                    raise TypeError("step: refine=dict(weighted=True) takes its weights from the step's DetectorNoise")
                rf["optics"].refine(self.Z, Y, alpha0=self.x0, out=self.x0, iters=rf["iters"], damping=rf["damping"], tol=rf["tol"],
                                    info=self.refine_info, status=self.refine_status, workspace=self._refine_ws, refresh=rf["refresh"],
                                    detector=noise, floor=rf["floor"], sigma=self.refine_sigma)
            else:
                rf["optics"].refine(self.Z, Y, alpha0=self.x0, out=self.x0, iters=rf["iters"], damping=rf["damping"], tol=rf["tol"],
                                    info=self.refine_info, status=self.refine_status, workspace=self._refine_ws, refresh=rf["refresh"], G=rf["G"])
        elif self.sensor is None:
            self.est.apply_device(self.scrn, noise, colmajor=True, out=self.x0, step=s)
        elif noise is None:                  # what a wavefront sensor measures on the same residual screen
            self.sensor.coefficients(self.scrn, out=self.x0, colmajor=True)
        else:
            from .estimator import DetectorNoise, detector_read
            if not isinstance(noise, DetectorNoise):
                raise TypeError("step: with sensor= the noise is None or a DetectorNoise")
            self.sensor.measure(self.scrn, want_coef=False, want_slopes=False, colmajor=True, out=dict(frame=self._sensor_frame))
            fr = self._sensor_frame.view(self.batch, -1)
            detector_read(fr, noise, step=s, out=fr)
            self.sensor.slopes_from_frame(fr, out=dict(slopes=self._sensor_slopes, coef=self.x0))
        # b_ref = -M1 B u[k-1] - M2 B u[k-2] (README.md:490-497) and the fastMPC step on (x0, x0_pre, b_ref) in one call
        if self.one_call:
            rc = self.h._lib.fmpc_ao_step_device(self.h._h, self.batch, vp(self.x0), vp(self.x0_pre), vp(u1) if s >= 1 else None, vp(u2) if s >= 2 else None,
                                                 vp(self.w), None, self.n_newton, self.k, None, None, vp(self.status), vp(self.iters), None, vp(u_new), stream)
            if rc != 0:
                from ._lib import FastMPCError
                raise FastMPCError(rc, "fmpc_ao_step_device")
        else:
            self.h.loop_inputs_device(self._zero_a, None, u1 if s >= 1 else None, u2 if s >= 2 else None, self._scr_x, self._scr_xp, self.w)
            self.h.solve_device(self.x0, self.x0_pre, self.w, None, None, self.n_newton, self.k, z_out=None, status=self.status, iters=self.iters,
                                u0_out=u_new, want_z=False)
        self.steps_done = s + 1
        return u_new, self.x0

    def records(self, rec):
        """The stage-0 records of the step just done (README.md:576-622) through `rec` (a `LoopRecords`): this loop keeps first
        moves only, so X_predicted(1:nx), its norm, du_prev and U_v.  Returns rec.step's dict of views."""
        if self.steps_done < 1:
            raise ValueError("records: no step has been done")
        s = self.steps_done - 1
        return rec.step(self.x0, self.x0_pre, self.w, self.u[(s - 1) % 3] if s >= 1 else None, u0=self.u[s % 3])
