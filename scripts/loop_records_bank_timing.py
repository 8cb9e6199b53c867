"""Timing of the closed-loop records with the model bank on one MI355X: nothing is asserted.

    python scripts/loop_records_bank_timing.py [--reps 20] [--calls 20] [--batches 256,2048] [--steps 64]

At (n, m, T) = (27, 144, 30), one model per realisation, per batch size:
  bank      fmpc_loop_records_bank_device, stages = T, all five outputs, u = z of the bank loop step
  shared    (a) fmpc_loop_records_device on the same inputs (one model for all: the floor; its kernels are those of the commit before
            the bank form, instruction for instruction)
  torch     (b) the same records composed in torch: unpack_device for U, torch.bmm with a stack of per-model M1, M2
            (T n x 2 n doubles per model) and elementwise kernels; its results are compared with `bank`
  step      (c) the bank loop step that produced z (fmpc_loop_step_bank_device, cold start, one Newton step, full z)
and for a stretch of --steps steps
  bank_run    fmpc_loop_records_run_bank_device
  shared_run  (a) fmpc_loop_records_run_device
  torch_run   (b) [A1 | A2] D per model through torch.bmm on the corrected states
  run         (c) fmpc_loop_run_bank_device over the same number of steps (few windows: it is milliseconds long)
Times are medians over --reps windows of --calls back-to-back calls between two device events, after 3 warm-up windows, in one
process, the two sides of a comparison alternating; boxes differ by up to 10 %.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, M, T = 27, 144, 30
VOLTS = (0.047275, 2.709264, 1.0)


def timed(fn, reps, calls, warm=3):
    """Median time of one call in microseconds."""
    import torch
    for _ in range(warm):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", default="256,2048")
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    import torch
    from oracle.closed_loop_ref import design_matrices
    from tests.util import handle_from_model
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    dev = torch.device("cuda:0")
    md = pkg.synthetic.make_model(N, M, T)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    tBt = t(md["B"].T)
    qst = np.tile(np.diag(md["Q"]), (T, 1)); qst[T - 1] = np.diag(md["Qf"])
    tQ, tR = t(qst), t(np.diag(md["R"]))
    ca, cb, uc = VOLTS
    rel = lambda a, b: float((a.reshape(b.shape) - b).norm() / b.norm())
    out = {"device": torch.cuda.get_device_name(0), "shape": [N, M, T], "reps": args.reps, "calls_per_window": args.calls, "steps": args.steps}
    for batch in (int(b) for b in args.batches.split(",")):
        rng = np.random.default_rng(batch)
        mods = [pkg.synthetic.make_model(N, M, T, seed=1000 + p) for p in range(batch)]
        A1, A2 = np.stack([q["A1"] for q in mods]), np.stack([q["A2"] for q in mods])
        MM = [design_matrices(q["A1"], q["A2"], T) for q in mods]
        tM12 = t(np.stack([np.concatenate([a, b], axis=1) for a, b in MM]))                  # (batch, T n, 2 n)
        tA12 = t(np.concatenate([A1, A2], axis=2))                                           # (batch, n, 2 n)
        h = handle_from_model(pkg, md)
        h.set_model_bank(t(A1), t(A2))
        a_k = np.stack([pkg.synthetic.make_realisation(mods[p], r=p, steps=2)[1:3] for p in range(batch)], axis=1)       # (2, batch, n)
        loop = pkg.ClosedLoop(h, batch, n_newton=1, k=1e-2, keep_z=True, bank=True)
        ta = t(a_k)
        loop.step(ta[0]); loop.step(ta[1]); torch.cuda.synchronize()
        x0, x0p, w, z, u1 = loop.x0, loop.x0_pre, loop.w, loop.z, loop.u[0]
        rec, recs = pkg.LoopRecords(h, batch, volts=VOLTS), pkg.LoopRecords(h, batch, volts=VOLTS)
        bank = lambda: rec.step_bank(x0, x0p, w, u1, z=z)
        shared = lambda: recs.step(x0, x0p, w, u1, z=z)
        U = torch.empty((batch, T, M), dtype=torch.float64, device=dev)
        u0 = torch.empty((batch, M), dtype=torch.float64, device=dev)
        xx = torch.empty((batch, 2 * N, 1), dtype=torch.float64, device=dev)

        def composed():
            h.unpack_device(z, U=U, u0=u0)
            xx[:, :N, 0] = x0; xx[:, N:, 0] = x0p
            F = torch.baddbmm(w.view(batch, T * N, 1), tM12, xx)
            Xp = F.view(batch, T, N) + torch.matmul(U, tBt)
            xerr = torch.linalg.vector_norm(Xp, dim=2)
            J = (Xp * Xp * tQ).sum(dim=(1, 2)) + (U * U * tR).sum(dim=(1, 2))
            du = u0 - u1
            uv = torch.sign(u0) * (-cb + torch.sqrt(cb * cb + 4.0 * ca * uc * u0.abs())) / (2.0 * ca)
            return Xp, xerr, J, du, uv

        sx0, sxp, sw, sz = (torch.empty_like(v) for v in (x0, x0p, w, z))                    # (the step's own outputs: the records' inputs stay)
        sx0.copy_(x0)
        nu_step = lambda: h.loop_step_bank(ta[1], sx0, loop.u[1], loop.u[0], sx0, sxp, sw, None, 1, 1e-2, z_out=sz, status=loop.status,
                                           iters=loop.iters, u0_out=u0)
        r = {}
        ref = composed(); got = bank(); torch.cuda.synchronize()
        r["bank_vs_torch_rel"] = {k: rel(got[k], v) for k, v in zip(("Xp", "xerr", "J", "du", "uv"), ref)}
        a1 = timed(bank, args.reps, args.calls); b1 = timed(composed, args.reps, args.calls); c1 = timed(shared, args.reps, args.calls)
        a2 = timed(bank, args.reps, args.calls); b2 = timed(composed, args.reps, args.calls); c2 = timed(shared, args.reps, args.calls)
        r["bank_us"], r["torch_us"], r["shared_us"] = [a1, a2], [b1, b2], [c1, c2]
        r["step_us"] = timed(nu_step, max(3, args.reps // 4), max(1, args.calls // 4))
        r["bank_over_shared"] = min(a1, a2) / min(c1, c2)
        r["bank_over_torch"] = min(a1, a2) / min(b1, b2)
        r["bank_share_of_step"] = min(a1, a2) / r["step_us"]
        r["torch_stack_MB"] = tM12.numel() * 8 / 1e6
        # ---- a stretch
        S = args.steps
        X0 = t(rng.standard_normal((S, batch, N))); U0 = t(rng.standard_normal((S, batch, M)))
        bank_run = lambda: rec.stretch(X0, U0, bank=True)
        shared_run = lambda: recs.stretch(X0, U0)
        zu, zx = torch.zeros((1, batch, M), dtype=torch.float64, device=dev), torch.zeros((1, batch, N), dtype=torch.float64, device=dev)

        def composed_run():
            BU = torch.matmul(U0, tBt)                                                       # (S, batch, n)
            U1 = torch.cat([zu, U0[:-1]]); BU1 = torch.cat([zx, BU[:-1]]); BU2 = torch.cat([zx, zx, BU[:-2]])
            D = torch.cat([X0 - BU1, torch.cat([zx, X0[:-1]]) - BU2], dim=2)                 # (S, batch, 2 n)
            Xp0 = torch.bmm(tA12, D.permute(1, 2, 0)).permute(2, 0, 1) + BU
            xerr0 = torch.linalg.vector_norm(Xp0, dim=2)
            dU = U0 - U1
            Uv = torch.sign(U0) * (-cb + torch.sqrt(cb * cb + 4.0 * ca * uc * U0.abs())) / (2.0 * ca)
            return Xp0, xerr0, dU, Uv

        ref = composed_run(); got = bank_run(); torch.cuda.synchronize()
        r["bank_run_vs_torch_rel"] = {k: rel(got[k], v) for k, v in zip(("Xp0", "xerr0", "dU", "Uv"), ref)}
        cr = max(1, args.calls // 4)
        a1 = timed(bank_run, args.reps, cr); b1 = timed(composed_run, args.reps, cr); c1 = timed(shared_run, args.reps, cr)
        a2 = timed(bank_run, args.reps, cr); b2 = timed(composed_run, args.reps, cr); c2 = timed(shared_run, args.reps, cr)
        r["bank_run_us"], r["torch_run_us"], r["shared_run_us"] = [a1, a2], [b1, b2], [c1, c2]
        arun = t(np.tile(a_k[:1], (S, 1, 1)))
        lr = pkg.ClosedLoop(h, batch, n_newton=1, k=1e-2, keep_z=False, bank=True)
        r["run_us"] = timed(lambda: lr.run_recorded(arun), 3, 1, warm=1)
        r["bank_run_over_shared"] = min(a1, a2) / min(c1, c2)
        r["bank_run_over_torch"] = min(a1, a2) / min(b1, b2)
        r["bank_run_share_of_run"] = min(a1, a2) / r["run_us"]
        out["batch_%d" % batch] = r
        h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
