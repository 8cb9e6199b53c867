"""Timing and error of the refinement weighted by the detector's noise on one MI355X:
fmpc_est_refine_weighted_device against fmpc_est_refine_hold_device(refresh = 1) on the same build and the same noisy images.

    python scripts/est_refine_weighted_timing.py [--runs 5] [--reps 3] [--len 512] [--batches 1,16,256,2000] [--out FILE]

Setting: the README's geometry at --len (d = 31 at 512, 3 diversities), the 27 modes of N = 6 without the piston, images of
||alpha|| = 0.3 made on the device and read out by fmpc_detector_read_device at 1e6 photo-electrons per call with 2 e- of read
noise, the start the linear estimate of the noisy images.
  hold-K       fmpc_est_refine_hold_device, refresh 1, K = 1 and 3 iterations (the yardstick: the unweighted call)
  weighted-K   fmpc_est_refine_weighted_device, refresh 1, floor 1, sigma = NULL
  sigma-K      the same with sigma asked for
Every side is a copy of the start into alpha and one call straight through the C ABI, with info, status and a workspace of the
recommended size (nothing allocated per call): the sides differ in the entry point alone.  A run is the median
over --reps windows of back-to-back calls between two device events (calls per window sized from a pilot so that a window lasts
about 20 ms, one call where a call is longer) after a warm-up window; the sides alternate, --runs runs each, in one process, and
the range of the runs is reported: a difference inside the ranges is no difference.

The error table (tests/test_est_refine_weighted_ref.py has it at len 64 on the CPU): rms of ||alpha_hat - alpha|| / ||alpha|| over
6 draws x 4 noise trials after 5 iterations, weighted against unweighted on the same Y, the noise that of
fmpc_detector_read_device with gain = e- per call / sum(b_s)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = [(0.3, 1e4, 0.0), (0.3, 1e6, 0.0), (0.3, 1e6, 2.0), (0.3, 1e8, 0.0), (1.0, 1e4, 0.0), (1.0, 1e4, 2.0), (1.0, 1e6, 2.0), (1.0, 1e8, 2.0)]
DRAWS, TRIALS = 6, 4


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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--len", type=int, default=512)
    ap.add_argument("--batches", default="1,16,256,2000")
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
    b_s = opt.model(Z)[1]
    torch.cuda.synchronize()
    per_unit = float(b_s.sum())
    Zflat = Z.view(nmode, -1)
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "reps": args.reps, "len": L, "nmode": nmode, "ndiv": opt.ndiv, "d": opt.d,
           "timing": [], "error": []}

    def problem(batch, norm, electrons, read_noise, seed, repeat=1):
        """alpha (batch, n), the noisy images of `repeat` noise trials of every alpha (repeat batch, p) and their linear estimates."""
        gen = torch.Generator(device=dev); gen.manual_seed(seed)
        a = torch.randn((batch, nmode), generator=gen, **f64)
        a *= norm / a.norm(dim=1, keepdim=True)
        a = a.repeat(repeat, 1)
        Y0 = est.apply_device((a @ Zflat).view(-1, L, L), want_Y=True, colmajor=True)[1]
        noise = pkg.DetectorNoise(electrons / per_unit, photon_noise=True, read_noise=read_noise, seed=seed)
        Y = pkg.detector_read(Y0.clone(), noise)                                          # (row r draws as realisation r: every trial afresh)
        return a, Y, ((Y - b_s) @ G.t()).contiguous(), noise

    # ---- the error table
    for norm, electrons, read_noise in ROWS:
        a, Y, start, noise = problem(DRAWS, norm, electrons, read_noise, 5 + int(10 * norm), TRIALS)
        status = torch.empty(len(a), dtype=torch.int32, device=dev)
        unweighted = opt.refine(Z, Y, alpha0=start, iters=5, status=status)
        assert not bool(status.any()), status
        weighted = opt.refine(Z, Y, alpha0=start, iters=5, status=status, detector=noise, floor=1.0)
        assert not bool(status.any()), status
        rms = lambda x: float((((x - a).norm(dim=1) / norm) ** 2).mean().sqrt())
        r = {"norm": norm, "electrons": electrons, "read_noise": read_noise, "unweighted": rms(unweighted), "weighted": rms(weighted)}
        r["ratio"] = r["unweighted"] / r["weighted"]
        out["error"].append(r)
        print(json.dumps(r), flush=True)

    # ---- the timing
    for batch in (int(s) for s in args.batches.split(",")):
        ws = torch.empty(opt.refine_workspace_bytes(nmode, batch), dtype=torch.uint8, device=dev)
        assert ws.numel() == opt.refine_workspace_bytes(nmode, batch, detector=True)
        a, Y, start, noise = problem(batch, 0.3, 1e6, 2.0, 77 + batch)
        alpha = torch.empty_like(start); info = torch.empty((batch, pkg.FMPC_REFINE_FIELDS), **f64)
        status = torch.empty(batch, dtype=torch.int32, device=dev); sigma = torch.empty_like(start)
        vp = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream

        blk = noise._block(0, batch)
        ldY = int(Y.stride(0)) if batch > 1 else opt.p

        def hold(iters):                                                                  # both sides straight through the C ABI, called alike
            def fn():
                alpha.copy_(start)
                rc = opt._lib.fmpc_est_refine_hold_device(opt._h, nmode, vp(Z), batch, vp(Y), ldY, vp(alpha), iters, 1, None, 0, 0.0, 0.0,
                                                          vp(info), vp(status), vp(ws), ws.numel(), stream)
                assert rc == 0, rc
            return fn

        def weighted(iters, sg):
            def fn():
                alpha.copy_(start)
                rc = opt._lib.fmpc_est_refine_weighted_device(opt._h, nmode, vp(Z), batch, vp(Y), ldY, vp(alpha), iters, 1, C.byref(blk), 1.0, 0.0, 0.0,
                                                              vp(info), vp(status), vp(sg), vp(ws), ws.numel(), stream)
                assert rc == 0, rc
            return fn

        sides = {}
        for k in (1, 3):
            sides[f"hold-{k}"] = hold(k); sides[f"weighted-{k}"] = weighted(k, None); sides[f"sigma-{k}"] = weighted(k, sigma)
        pilot, error = {}, {}
        for name, fn in sides.items():
            pilot[name] = window(fn, 1)
            assert not bool(status.any()), (name, status)
            error[name] = float((((alpha - a).norm(dim=1) / 0.3) ** 2).mean().sqrt())
        calls = {k: int(min(200, max(1, 2.0e4 / pilot[k]))) for k in sides}
        t = {k: [] for k in sides}
        for _ in range(args.runs):
            for k, fn in sides.items():
                t[k].append(window(fn, 1) if pilot[k] > 5e5 else timed(fn, args.reps, calls[k]))
        r = {"batch": batch, "calls_per_window": calls, "us": {k: [min(v), max(v)] for k, v in t.items()}, "rms_error": error,
             "weighted_over_hold": {str(k): [min(t[f"weighted-{k}"]) / max(t[f"hold-{k}"]), max(t[f"weighted-{k}"]) / min(t[f"hold-{k}"])] for k in (1, 3)},
             "sigma_over_weighted": {str(k): [min(t[f"sigma-{k}"]) / max(t[f"weighted-{k}"]), max(t[f"sigma-{k}"]) / min(t[f"weighted-{k}"])] for k in (1, 3)},
             "workspace_bytes": ws.numel()}
        out["timing"].append(r)
        print(json.dumps(r), flush=True)
        del ws, Y
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
