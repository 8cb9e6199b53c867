"""Timing of the estimator's Gauss-Newton refinement on one MI355X: fmpc_est_refine_device on a batch
against what a user could write before it existed, and against the linear estimate it refines.

    python scripts/est_refine_timing.py [--rounds 3] [--reps 3] [--len 512] [--batches 1,16,256,2000] [--iters 1,3] [--out FILE]

Setting: the README's geometry at --len (d = 31 at 512, 3 diversities), the 27 modes of N = 6 without the piston, images of
||alpha|| = 1 made on the device, the start the linear estimate.
  refine    EstimatorOptics.refine with out=, info=, status= and workspace= at the recommended size (nothing allocated per call)
  composed  per realisation EstimatorOptics.model(Z, phi_b) with out= and workspace=, H = A'A, g = A'(Y_b - b_s) and
            torch.linalg.cholesky / cholesky_solve, phi_b from one torch product for the batch; the final cost is left out (in its
            favour).  Its result is compared with `refine` before anything is timed.
  apply     fmpc_est_apply_device on the same batch of screens: the linear estimate
Times are medians over --reps windows of back-to-back calls between two device events (calls per window sized from a pilot so
that a window lasts about 20 ms, one call where a call is longer), after a warm-up window, in one process, the sides alternating
for --rounds rounds; every round's median is listed and the best of each side is compared.  A side whose call takes more than
half a second is timed once per round.  The matrix-core roofline is the nominal work -- per iteration and realisation the
model's (nmode + 1) ndiv (6 len^2 32 + 8 x 32 x 32 len) and 2 p (nmode + 1)(nmode + 2) / 2 for the normal equations, plus one
base field for the final cost -- over the fp64 matrix peak of 78.6 TFLOP/s."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_MATRIX_PEAK = 78.6e12


def window(fn, calls):
    import torch
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def timed(fn, reps, calls):
    """Median time of one call in microseconds."""
    window(fn, calls)
    return float(np.median([window(fn, calls) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--len", type=int, default=512)
    ap.add_argument("--batches", default="1,16,256,2000")
    ap.add_argument("--iters", default="1,3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    L = args.len
    opt = pkg.reference_optics(L)
    Z = opt.Z[1:].contiguous()
    nmode, nd, p = int(Z.shape[0]), opt.ndiv, opt.p
    est = opt.estimator(opt.Z, skip=1)
    Zflat = Z.view(nmode, -1)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "len": L, "nmode": nmode, "ndiv": nd, "d": opt.d,
           "cases": []}
    ws_model = torch.empty(opt.workspace_bytes(nmode), dtype=torch.uint8, device=dev)
    res = (torch.empty((nmode, p), **f64).t(), torch.empty(p, **f64))
    for batch in (int(s) for s in args.batches.split(",")):
        gen = torch.Generator(device=dev); gen.manual_seed(77 + batch)
        a = torch.randn((batch, nmode), generator=gen, **f64)
        a /= a.norm(dim=1, keepdim=True)
        scr = (a @ Zflat).view(batch, L, L)                                              # [b, column, row]
        start, Y = est.apply_device(scr, want_Y=True, colmajor=True)
        start = start.clone()
        alpha = torch.empty_like(start); info = torch.empty((batch, pkg.FMPC_REFINE_FIELDS), **f64)
        status = torch.empty(batch, dtype=torch.int32, device=dev)
        ws = torch.empty(opt.refine_workspace_bytes(nmode, batch), dtype=torch.uint8, device=dev)
        ad = torch.empty_like(start)
        apply_ = lambda: est.apply_device(scr, colmajor=True, out=ad)
        for iters in (int(s) for s in args.iters.split(",")):
            refine = lambda: opt.refine(Z, Y, alpha0=start, out=alpha, iters=iters, info=info, status=status, workspace=ws)
            acomp = torch.empty_like(start)

            def composed():
                acomp.copy_(start)
                for _ in range(iters):
                    phi = (acomp @ Zflat).view(batch, L, L)
                    for b in range(batch):
                        A, b_s = opt.model(Z, phi0=phi[b], workspace=ws_model, out=res)
                        H = A.t() @ A
                        g = A.t() @ (Y[b] - b_s)
                        acomp[b] += torch.cholesky_solve(g[:, None], torch.linalg.cholesky(H))[:, 0]
                return acomp

            refine(); composed(); torch.cuda.synchronize()
            gap = float((alpha - acomp).norm(dim=1).max())
            err = float((alpha - a).norm(dim=1).max())
            assert not bool(status.any()), status
            sides = {"refine": refine, "composed": composed, "apply": apply_}
            pilot = {k: window(fn, 1) for k, fn in sides.items()}
            calls = {k: int(min(200, max(1, 2.0e4 / pilot[k]))) for k in sides}
            t = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    t[k].append(window(fn, 1) if pilot[k] > 5e5 else timed(fn, args.reps, calls[k]))
            best = {k: min(v) for k, v in t.items()}
            model_flops = (nmode + 1) * nd * (6.0 * L * L * 32 + 8.0 * 32 * 32 * L)
            flops = batch * (iters * (model_flops + 2.0 * p * (nmode + 1) * (nmode + 2) / 2) + model_flops / (nmode + 1))
            r = {"batch": batch, "iters": iters, "calls_per_window": calls, "us": t, "best_us": best,
                 "spread": {k: max(v) / min(v) for k, v in t.items()}, "refine_vs_composed_alpha": gap, "refined_error": err,
                 "composed_over_refine": best["composed"] / best["refine"], "refine_over_apply": best["refine"] / best["apply"],
                 "us_per_realisation_iteration": best["refine"] / (batch * iters), "nominal_flops": flops,
                 "matrix_roofline_fraction": flops / FP64_MATRIX_PEAK * 1e6 / best["refine"], "workspace_bytes": ws.numel()}
            out["cases"].append(r)
            print(json.dumps(r), flush=True)
        del ws, scr, Y
        torch.cuda.empty_cache()
    est.close(); opt.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
