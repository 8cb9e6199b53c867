"""Timing of the closed-loop records on one MI355X: nothing is asserted.

    python scripts/loop_records_timing.py [--reps 20] [--calls 20] [--batches 256,2000]

At (n, m, T) = (27, 144, 30), per batch size:
  full      fmpc_loop_records_device, stages = T, all five outputs, u = z of a solve
  first     the same call with stages = 1 on the first moves (no J)
  stretch   fmpc_loop_records_run_device over 100 recorded steps
  torch     the records of `full` composed from what the library offered before: unpack_device for U, then torch.matmul and
            elementwise kernels on preloaded M1, M2, B, Q, R on the device -- the baseline; its results are compared with `full`
  solve     solve_device of the same batch with the full z (cold start, one Newton step), for scale
and the bytes `full` has to move, 8 (T m + T n + 2 n + m) in and 8 (T n + T + 1 + 2 m) out per problem, as a fraction of the
HBM roofline (8 TB/s peak).  Times are medians over --reps windows of --calls back-to-back calls between two device events, after
3 warm-up windows, in one process; boxes differ by up to 10 %.
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
HBM_PEAK = 8.0e12


def timed(fn, reps, calls):
    """Median time of one call in microseconds."""
    import torch
    for _ in range(3):
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
    ap.add_argument("--batches", default="256,2000")
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    import torch
    from oracle.closed_loop_ref import design_matrices
    from tests.util import handle_from_model
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    dev = torch.device("cuda:0")
    md = pkg.synthetic.make_model(N, M, T)
    h = handle_from_model(pkg, md)
    M1, M2 = design_matrices(md["A1"], md["A2"], T)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    tM1t, tM2t, tBt = t(M1.T), t(M2.T), t(md["B"].T)
    qst = np.tile(np.diag(md["Q"]), (T, 1)); qst[T - 1] = np.diag(md["Qf"])
    tQ, tR = t(qst), t(np.diag(md["R"]))
    ca, cb, uc = VOLTS
    out = {"device": torch.cuda.get_device_name(0), "shape": [N, M, T], "reps": args.reps, "calls_per_window": args.calls}
    for batch in (int(b) for b in args.batches.split(",")):
        rng = np.random.default_rng(batch)
        d = pkg.synthetic.make_replay_batch(md, r=0, steps=min(batch, 64))
        idx = np.arange(batch) % d["x0"].shape[0]
        x0, x0p = t(d["x0"][idx]), t(d["x0_pre"][idx])
        w, u1 = t(0.01 * rng.standard_normal((batch, T * N))), t(rng.standard_normal((batch, M)))
        z = torch.empty((batch, T * (N + M)), dtype=torch.float64, device=dev)
        u0 = torch.empty((batch, M), dtype=torch.float64, device=dev)
        st = torch.zeros(batch, dtype=torch.int32, device=dev); it = torch.zeros(batch, dtype=torch.int32, device=dev)
        solve = lambda: h.solve_device(x0, x0p, w, None, None, 1, 1e-2, z_out=z, status=st, iters=it, u0_out=u0)
        solve(); torch.cuda.synchronize()
        rec = pkg.LoopRecords(h, batch, volts=VOLTS)
        full = lambda: rec.step(x0, x0p, w, u1, z=z)
        first = lambda: rec.step(x0, x0p, w, u1, u0=u0)
        X0 = t(rng.standard_normal((args.steps, batch, N))); U0 = t(rng.standard_normal((args.steps, batch, M)))
        stretch = lambda: rec.stretch(X0, U0)
        U = torch.empty((batch, T, M), dtype=torch.float64, device=dev)

        def composed():
            h.unpack_device(z, U=U, u0=u0)
            F = torch.addmm(w, x0, tM1t)
            F.addmm_(x0p, tM2t)
            Xp = F.view(batch, T, N) + torch.matmul(U, tBt)
            xerr = torch.linalg.vector_norm(Xp, dim=2)
            J = (Xp * Xp * tQ).sum(dim=(1, 2)) + (U * U * tR).sum(dim=(1, 2))
            du = u0 - u1
            uv = torch.sign(u0) * (-cb + torch.sqrt(cb * cb + 4.0 * ca * uc * u0.abs())) / (2.0 * ca)
            return Xp, xerr, J, du, uv

        r = {}
        ref = composed(); got = full(); torch.cuda.synchronize()
        r["full_vs_torch_rel"] = {k: float((got[k].reshape(v.shape) - v).norm() / v.norm())
                                  for k, v in zip(("Xp", "xerr", "J", "du", "uv"), ref)}
        # the two sides of the one bar alternate
        a1 = timed(full, args.reps, args.calls); b1 = timed(composed, args.reps, args.calls)
        a2 = timed(full, args.reps, args.calls); b2 = timed(composed, args.reps, args.calls)
        r["full_us"], r["torch_us"] = [a1, a2], [b1, b2]
        r["first_us"] = timed(first, args.reps, args.calls)
        r["stretch_%d_steps_us" % args.steps] = timed(stretch, args.reps, max(1, args.calls // 4))
        r["solve_full_z_us"] = timed(solve, args.reps, args.calls)
        by = 8 * (T * M + T * N + 2 * N + M) + 8 * (T * N + T + 1 + 2 * M)
        r["bytes_per_problem"] = by
        r["full_GBps"] = by * batch / (min(a1, a2) * 1e-6) / 1e9
        r["full_fraction_of_hbm_peak"] = by * batch / (min(a1, a2) * 1e-6) / HBM_PEAK
        r["full_over_solve"] = min(a1, a2) / r["solve_full_z_us"]
        r["full_over_torch"] = min(a1, a2) / min(b1, b2)
        out["batch_%d" % batch] = r
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
