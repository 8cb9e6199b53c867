"""Timing of the modal fit on one MI355X: fmpc_modal_fit_device against the same result composed in torch.

    python scripts/modal_fit_timing.py [--rounds 5] [--reps 5] [--shapes 512:1,512:144,512:256,512:2000,128c:32000] [--out FILE]

Shapes are L:batch over synthetic.zernike_modes(L, 28) on the full L x L grid, or Lc:batch compressed to the support (128c: 12 644
pixels, the reference's own fit size).  Screens are seeded normal deviates generated on the device; skip = 1.  Per shape:
  modal    ModalFit.fit with out= and workspace= at the recommended size (nothing allocated per call)
  torch    the yardstick: S = screens @ Z.T (one matmul), then torch.cholesky_solve with the precomputed upper factor of Z Z'; the
           largest relative gap to `modal` per screen is reported before anything is timed
Times are medians over --reps windows of back-to-back calls between two device events (the calls per window sized from a pilot so
that a window lasts about 20 ms), after a warm-up window, in one process, the two sides alternating for --rounds rounds; every
round's median is listed, the best of each side is compared, and the spread is the worst round over the best.  The HBM roofline
is the compulsory bytes 8 (batch npx + n npx + batch n) over the 6.3 TB/s measured copy rate of the part (8.0 TB/s peak).
workspace_share: the partial sums written and read back, as a share of the screen bytes.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, SKIP = 28, 1
HBM_COPY_RATE = 6.3e12


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="512:1,512:144,512:256,512:2000,128c:32000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "n": N, "skip": SKIP, "rounds": args.rounds, "reps": args.reps, "shapes": {}}
    fits = {}
    for shape in args.shapes.split(","):
        grid, batch = shape.split(":")
        batch = int(batch)
        if grid not in fits:
            L = int(grid.rstrip("c"))
            Zh = pkg.synthetic.zernike_modes(L, N).reshape(N, -1)
            if grid.endswith("c"):
                Zh = Zh[:, Zh[0] != 0]
            Z = torch.from_numpy(np.ascontiguousarray(Zh)).to(dev)
            fits[grid] = (pkg.ModalFit(Z), Z, Z.t().contiguous(), torch.linalg.cholesky(Z @ Z.t(), upper=True))
        mf, Z, Zt, U = fits[grid]
        npx = mf.npx
        gen = torch.Generator(device=dev); gen.manual_seed(1234 + batch)
        screens = torch.randn((batch, npx), dtype=torch.float64, device=dev, generator=gen)
        ws = torch.empty(pkg.modal_workspace_bytes(N, npx, batch), dtype=torch.uint8, device=dev)
        c = torch.empty((batch, N - SKIP), dtype=torch.float64, device=dev)
        modal = lambda: mf.fit(screens, skip=SKIP, workspace=ws, out=c)
        composed = lambda: torch.cholesky_solve((screens @ Zt).t(), U, upper=True)[SKIP:].t()
        modal(); ref = composed(); torch.cuda.synchronize()
        gap = float(((c - ref).norm(dim=1) / ref.norm(dim=1)).max())
        pilot = max(window(modal, 3), window(composed, 3))
        calls = int(min(200, max(3, 2.0e4 / pilot)))
        a, b = [], []
        for _ in range(args.rounds):
            a.append(timed(modal, args.reps, calls)); b.append(timed(composed, args.reps, calls))
        bytes_ = 8 * (batch * npx + N * npx + batch * N)
        floor = bytes_ / HBM_COPY_RATE * 1e6
        per_screen_ws = pkg.modal_workspace_bytes(N, npx, 1) / 16
        r = {"npx": npx, "batch": batch, "calls_per_window": calls, "modal_vs_torch_rel": gap, "modal_us": a, "torch_us": b,
             "modal_spread": max(a) / min(a), "torch_spread": max(b) / min(b), "torch_over_modal": min(b) / min(a),
             "slower_beyond_spread": min(a) > max(b), "bytes": bytes_, "hbm_floor_us": floor, "hbm_roofline_fraction": floor / min(a),
             "workspace_bytes": ws.numel(), "workspace_share": 2.0 * per_screen_ws / (8.0 * npx)}
        out["shapes"][shape] = r
        print(shape, json.dumps(r), flush=True)
        del screens, ws, c, ref
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
