"""Timing of the science camera on one MI355X: fmpc_sci_expose_device against what it replaces.

    python scripts/science_timing.py [--rounds 3] [--reps 5] [--length 512] [--batches 1,256,2000] [--windows 32,64] [--samplings 1,2] [--out FILE]

The camera is reference_science_camera(d, s, length) (the README's pin-hole pupil); the screens are 0.5 rad of pixel noise.
  both / quality / image   ScienceCamera.expose with image=, quality= and workspace= given (nothing allocated per call), accumulating,
            in its three modes;
  torch     the composition it replaces, for the image and the six fields: the pupil field padded about its centre to s len,
            torch.fft.fft2, abs()**2, the window added to the image, and torch reductions for mean, rms, Strehl, Marechal, min
            and max -- in chunks of 64 screens, so that the padded field of 2000 screens need not exist at once;
  estimator at d = 32, s = 1 only: PhaseDiversityEstimator(ndiv = 1, zd = 0).apply_device(want_Y=True) plus the add: the window
            the estimator computes anyway (31 x 31, one sample per lambda / D), without accumulation or statistics;
  floor     one read of the screens, 8 batch len^2 bytes at the 6.3 TB/s measured copy rate of the part.
The workspace traffic of a call is reported next to the 8 len^2 bytes per screen it has to read: T is written once and read once
(16 len d bytes each way per screen in the standard form, twice that in the few-screens form).
Times are medians over --reps windows of back-to-back calls between two device events (the calls per window sized from a pilot so
that a window lasts about 20 ms), after a warm-up window, in one process, the sides alternating for --rounds rounds; every
round's median is listed and the best of each side is compared.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_RATE = 6.3e12
CHUNK = 64


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


def rounds(fns, n_rounds, reps):
    got, calls = {k: [] for k in fns}, {}
    for k, f in fns.items():
        calls[k] = int(min(200, max(2, 2.0e4 / window(f, 2))))
    for _ in range(n_rounds):
        for k, f in fns.items():
            got[k].append(timed(f, reps, calls[k]))
    return got, calls


def torch_composition(torch, A, scrn, image, quality, d, s, scale):
    """A: (len, len) [column, row]; scrn (batch, len, len) the same way; image (batch, d, d); quality (batch, 6)."""
    L = A.shape[0]
    N = s * L
    o = N // 2 - L // 2
    c = N // 2
    inside = A != 0
    W = A.sum()
    for b0 in range(0, scrn.shape[0], CHUNK):
        ph = scrn[b0:b0 + CHUNK]
        field = torch.polar(A.expand_as(ph), ph)
        if s > 1:
            big = torch.zeros((ph.shape[0], N, N), dtype=torch.complex128, device=ph.device)
            big[:, o:o + L, o:o + L] = field
        else:
            big = field
        I = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(big, dim=(-2, -1))), dim=(-2, -1))
        image[b0:b0 + CHUNK] += scale * I[:, c - d // 2:c + d // 2, c - d // 2:c + d // 2].abs() ** 2
        q = quality[b0:b0 + CHUNK]
        mu = (A * ph).sum(dim=(-2, -1)) / W
        var = (A * (ph - mu[:, None, None]) ** 2).sum(dim=(-2, -1)) / W
        q[:, 0] = mu; q[:, 1] = var.sqrt()
        q[:, 2] = field.sum(dim=(-2, -1)).abs() ** 2 / W ** 2
        q[:, 3] = torch.exp(-var)
        q[:, 4] = torch.where(inside, ph, float("inf")).amin(dim=(-2, -1))
        q[:, 5] = torch.where(inside, ph, float("-inf")).amax(dim=(-2, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--batches", default="1,256,2000")
    ap.add_argument("--windows", default="32,64")
    ap.add_argument("--samplings", default="1,2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    L = args.length
    out = {"device": torch.cuda.get_device_name(0), "length": L, "rounds": args.rounds, "reps": args.reps, "cases": []}
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    for batch in (int(v) for v in args.batches.split(",")):
        scrn = 0.5 * torch.randn((batch, L, L), dtype=torch.float64, device=dev, generator=gen)
        floor = 8.0 * batch * L * L / HBM_COPY_RATE * 1e6
        for d in (int(v) for v in args.windows.split(",")):
            for s in (int(v) for v in args.samplings.split(",")):
                cam = pkg.reference_science_camera(d, float(s), L)
                A = torch.from_numpy(np.ascontiguousarray(pkg.reference_pupil(L).T)).to(dev)
                ws = torch.empty(cam.workspace_bytes(batch), dtype=torch.uint8, device=dev)
                img = torch.zeros((batch, d, d), dtype=torch.float64, device=dev); q = torch.zeros((batch, 6), dtype=torch.float64, device=dev)
                timg = torch.zeros_like(img); tq = torch.zeros_like(q)
                fns = {"both": lambda: cam.expose(scrn, image=img, accumulate=True, quality=q, colmajor=True, workspace=ws),
                       "quality": lambda: cam.expose(scrn, want_image=False, quality=q, colmajor=True, workspace=ws),
                       "image": lambda: cam.expose(scrn, image=img, accumulate=True, want_quality=False, colmajor=True, workspace=ws),
                       "torch": lambda: torch_composition(torch, A, scrn, timg, tq, d, s, cam.scale)}
                est = None
                if d == 32 and s == 1:
                    opt = pkg.reference_optics(L)
                    one = pkg.EstimatorOptics(opt.pupil, opt.Z[4].t(), [0.0], opt.dx, opt.range_min, opt.range_max, AU=opt.AU)
                    est = one.estimator(opt.Z, skip=1)
                    eimg = torch.zeros((batch, est.p), dtype=torch.float64, device=dev); eout = torch.zeros((batch, est.nx), dtype=torch.float64, device=dev)

                    def estimator():
                        Y = est.apply_device(scrn, None, colmajor=True, out=eout, want_Y=True)[1]
                        eimg.add_(Y)
                    fns["estimator"] = estimator
                # agreement before anything is timed
                img.zero_(); timg.zero_()
                fns["both"](); fns["torch"](); torch.cuda.synchronize()
                gap_i = float(((img - timg).flatten(1).norm(dim=1) / timg.flatten(1).norm(dim=1)).max())
                gap_q = float(((q - tq).abs() / tq.abs().clamp_min(1e-300)).max())
                form = cam.last_form
                got, calls = rounds(fns, args.rounds, args.reps)
                best = {k: min(v) for k, v in got.items()}
                halves = 2 if form == pkg.FMPC_SCI_FORM_FEW else 1
                case = {"batch": batch, "d": d, "s": s, "form": form, "calls_per_window": calls, "us": got, "best_us": best,
                        "image_vs_torch_rel": gap_i, "quality_vs_torch_rel": gap_q, "hbm_floor_us": floor,
                        "floor_fraction_both": floor / best["both"], "torch_over_both": best["torch"] / best["both"],
                        "slower_than_torch_beyond_spread": min(got["both"]) > max(got["torch"]),
                        "screen_bytes": 8 * L * L, "workspace_bytes_written_per_screen": 16 * L * d * halves + 64 * (L // 16) * 8,
                        "workspace_bytes_read_per_screen": 16 * L * d * halves * (d // 16) + 64 * (L // 16) * 8, "workspace_bytes": ws.numel()}
                if est is not None:
                    case["estimator_over_image"] = best["estimator"] / best["image"]
                    est.close(); one.close(); opt.close()
                print(json.dumps(case), flush=True)
                out["cases"].append(case)
                cam.close()
                del ws, img, q, timg, tq
                torch.cuda.empty_cache()
        del scrn
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
