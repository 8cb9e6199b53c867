"""Timing of the refinement with a held Jacobian and of its gain form on one MI355X:
fmpc_est_refine_hold_device under the schedules below against fmpc_est_refine_device (refresh = 1: the same launches, the same
bits) and against the linear estimate, with the error each schedule reaches.

    python scripts/est_refine_hold_timing.py [--rounds 3] [--reps 3] [--len 512] [--batches 1,16,256,2000] [--norms 0.3,1] [--out FILE]

Setting: the README's geometry at --len (d = 31 at 512, 3 diversities), the 27 modes of N = 6 without the piston, images of
||alpha|| = norm made on the device, the start the linear estimate, G = EstimatorOptics.gain(Z) computed once outside the timing.
  gn-K      refresh 1, K = 1, 2, 3 iterations: EstimatorOptics.refine as before (the yardstick)
  once+K    J built in iteration 0, then K = 1 .. 4 held iterations (refresh >= iters)
  r3-K      refresh 3, K = 4 and 6 iterations
  gain-K    the gain form, K = 1 .. 4 steps
  apply     fmpc_est_apply_device on the same screens: the linear estimate
Every side runs with out=, info=, status= and workspace= at the recommended size (nothing allocated per call).  Times are medians
over --reps windows of back-to-back calls between two device events (calls per window sized from a pilot so that a window lasts
about 20 ms, one call where a call is longer), after a warm-up window, in one process, the sides alternating for --rounds rounds;
the best round of each side is reported with the spread of the rounds.  A side whose call takes more than half a second is timed
once per round.  error: the worst ||alpha_hat - alpha|| / ||alpha|| of the batch after the call."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ONCE = 1 << 20
SCHEDULES = ([(f"gn-{k}", 1, k) for k in (1, 2, 3)] + [(f"once+{k}", ONCE, k + 1) for k in (1, 2, 3, 4)] + [(f"r3-{k}", 3, k) for k in (4, 6)] +
             [(f"gain-{k}", 0, k) for k in (1, 2, 3, 4)])


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
    ap.add_argument("--norms", default="0.3,1")
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
    nmode = int(Z.shape[0])
    est = opt.estimator(opt.Z, skip=1)
    G = opt.gain(Z)
    Zflat = Z.view(nmode, -1)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "len": L, "nmode": nmode, "ndiv": opt.ndiv, "d": opt.d,
           "cases": []}
    for batch in (int(s) for s in args.batches.split(",")):
        ws = {0: torch.empty(opt.refine_workspace_bytes(nmode, batch, refresh=0), dtype=torch.uint8, device=dev),
              1: torch.empty(opt.refine_workspace_bytes(nmode, batch), dtype=torch.uint8, device=dev)}
        for norm in (float(s) for s in args.norms.split(",")):
            gen = torch.Generator(device=dev); gen.manual_seed(77 + batch)
            a = torch.randn((batch, nmode), generator=gen, **f64)
            a *= norm / a.norm(dim=1, keepdim=True)
            scr = (a @ Zflat).view(batch, L, L)                                          # [b, column, row]
            start, Y = est.apply_device(scr, want_Y=True, colmajor=True)
            start = start.clone()
            alpha = torch.empty_like(start); info = torch.empty((batch, pkg.FMPC_REFINE_FIELDS), **f64)
            status = torch.empty(batch, dtype=torch.int32, device=dev)
            ad = torch.empty_like(start)

            def side(refresh, iters):
                return lambda: opt.refine(Z, Y, alpha0=start, out=alpha, iters=iters, info=info, status=status, workspace=ws[min(refresh, 1)],
                                          refresh=refresh, G=G if refresh == 0 else None)

            sides = {name: side(refresh, iters) for name, refresh, iters in SCHEDULES}
            sides["apply"] = lambda: est.apply_device(scr, colmajor=True, out=ad)
            error, pilot = {"apply": float(((start - a).norm(dim=1) / norm).max())}, {}
            for name, fn in sides.items():
                pilot[name] = window(fn, 1)
                if name != "apply":
                    assert not bool(status.any()), (name, status)
                    error[name] = float(((alpha - a).norm(dim=1) / norm).max())
            if batch > 1:                                                                 # refresh = 1 of the new call: the same bits
                opt.refine(Z, Y, alpha0=start, out=alpha, iters=2, workspace=ws[1])
                first = alpha.clone()
                opt._lib.fmpc_est_refine_hold_device(opt._h, nmode, Z.data_ptr(), batch, Y.data_ptr(), int(Y.stride(0)), alpha.copy_(start).data_ptr(), 2, 1,
                                                     None, 0, 0.0, 0.0, None, None, ws[1].data_ptr(), ws[1].numel(),
                                                     torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize()
                assert torch.equal(first, alpha)
            calls = {k: int(min(200, max(1, 2.0e4 / pilot[k]))) for k in sides}
            t = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    t[k].append(window(fn, 1) if pilot[k] > 5e5 else timed(fn, args.reps, calls[k]))
            best = {k: min(v) for k, v in t.items()}
            r = {"batch": batch, "norm": norm, "calls_per_window": calls, "best_us": best, "spread": {k: max(v) / min(v) for k, v in t.items()},
                 "error": error, "us_per_realisation": {k: v / batch for k, v in best.items()},
                 "workspace_bytes": {"gain": ws[0].numel(), "jacobian": ws[1].numel()}}
            out["cases"].append(r)
            print(json.dumps(r), flush=True)
            del scr, Y
        del ws
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
