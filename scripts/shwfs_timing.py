"""Timing of the Shack-Hartmann sensor on one MI355X: fmpc_sh_measure_device against what it replaces.

    python scripts/shwfs_timing.py [--rounds 3] [--reps 5] [--length 512] [--batches 1,256,2000] [--cases 32:2:16,16:2:16] [--nmode 27] [--out FILE]

The sensor is ShackHartmann(reference_pupil(length), npl, pad, s) with a random reconstructor of --nmode rows; the screens are 1 rad
of pixel noise.  A case is npl:pad:s.
  slopes / coef / frame   ShackHartmann.measure with every output given (nothing allocated per call): slopes only, slopes with
            coefficients, slopes with the frame;
  torch_*   the same computation composed in torch: the screen cut into lenslets (a view), the field times the half-pixel
            phasor, torch.fft.fft2 zero-padded to nOut, the crop, abs()**2, the three sums of the centroid, (R @ slopes), (the
            frame assembled) -- in chunks of 32 screens, so that the padded spectra of 2000 screens need not exist at once;
  estimator PhaseDiversityEstimator.apply_device (fmpc_est_apply_device) of reference_optics(length) on the same screens;
  floors    one read of the screens, 8 batch len^2 bytes at the 6.3 TB/s measured copy rate of the part, and the nominal flops
            of the two small complex products, 8 npl s (npl + s) per lit lenslet, at the 78.6 TFLOP/s fp64 matrix peak.
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
FP64_MATRIX_PEAK = 78.6e12
CHUNK = 32


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


class TorchSensor:
    """The composition in torch.  A: (len, len) [column, row], as the screens are."""

    def __init__(self, torch, sen, A, R):
        self.t, self.npl, self.nL, self.s, self.nout = torch, sen.npl, sen.nL, sen.s, sen.pad * sen.npl
        dev = A.device
        self.A = A.view(self.nL, self.npl, self.nL, self.npl)                              # [j, x, i, y]
        u = torch.arange(self.npl, dtype=torch.float64, device=dev) * (1 - self.nout) / self.nout
        self.phasor = torch.exp(-1j * np.pi * (u[:, None] + u[None, :])) / self.nout      # [x, y]
        self.k0 = self.nout // 2 - self.s // 2 if self.nout > self.s else 0
        self.idx = torch.arange(self.s, dtype=torch.float64, device=dev)
        v = torch.from_numpy(np.flatnonzero(sen.valid.ravel(order="F"))).to(dev)          # l = i + nL j
        self.vj, self.vi = v // self.nL, v % self.nL
        self.R = R

    def run(self, scrn, slopes, coef=None, frame=None):
        t, s, k0 = self.t, self.s, self.k0
        for b0 in range(0, scrn.shape[0], CHUNK):
            ph = scrn[b0:b0 + CHUNK].view(-1, self.nL, self.npl, self.nL, self.npl)       # [b, j, x, i, y]
            field = t.polar(self.A.expand_as(ph), ph).permute(0, 1, 3, 2, 4) * self.phasor   # [b, j, i, x, y]
            W = t.fft.fft2(field, s=(self.nout, self.nout))[..., k0:k0 + s, k0:k0 + s]    # [b, j, i, column freq, row freq]
            I = W.real ** 2 + W.imag ** 2
            if frame is not None:
                frame[b0:b0 + CHUNK] = I.permute(0, 1, 3, 2, 4).reshape(-1, self.nL * s, self.nL * s)
            b = I[:, self.vj, self.vi]                                                    # [b, valid, column, row]
            m = b.sum(dim=(-2, -1))
            slopes[b0:b0 + CHUNK, :m.shape[1]] = (b.sum(dim=-1) * self.idx).sum(dim=-1) / m
            slopes[b0:b0 + CHUNK, m.shape[1]:] = (b.sum(dim=-2) * self.idx).sum(dim=-1) / m
        if coef is not None:
            t.matmul(slopes, self.R.t(), out=coef)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--batches", default="1,256,2000")
    ap.add_argument("--cases", default="32:2:16,16:2:16")
    ap.add_argument("--nmode", type=int, default=27)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    L = args.length
    out = {"device": torch.cuda.get_device_name(0), "length": L, "rounds": args.rounds, "reps": args.reps, "cases": []}
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    pupil = pkg.reference_pupil(L)
    A = torch.from_numpy(np.ascontiguousarray(pupil.T)).to(dev)
    opt = pkg.reference_optics(L)
    est = opt.estimator(opt.Z, skip=1)
    f64 = dict(dtype=torch.float64, device=dev)
    for batch in (int(v) for v in args.batches.split(",")):
        scrn = torch.randn((batch, L, L), generator=gen, **f64)
        eout = torch.zeros((batch, est.nx), **f64)
        floor = 8.0 * batch * L * L / HBM_COPY_RATE * 1e6
        for npl, pad, s in (tuple(int(v) for v in c.split(":")) for c in args.cases.split(",")):
            sen = pkg.ShackHartmann(pupil, npl, pad=pad, spot=s)
            R = torch.randn((args.nmode, 2 * sen.nvalid), generator=gen, **f64)
            sen.set_reconstructor(R)
            ts = TorchSensor(torch, sen, A, R)
            nlit = int((pupil.reshape(sen.nL, npl, sen.nL, npl) > 0).any(axis=(1, 3)).sum())
            fl = sen.frame_len
            sl = torch.zeros((batch, 2 * sen.nvalid), **f64); cf = torch.zeros((batch, args.nmode), **f64); fr = torch.zeros((batch, fl, fl), **f64)
            tsl = torch.zeros_like(sl); tcf = torch.zeros_like(cf); tfr = torch.zeros_like(fr)
            fns = {"slopes": lambda: sen.measure(scrn, colmajor=True, out=dict(slopes=sl)),
                   "coef": lambda: sen.measure(scrn, colmajor=True, out=dict(slopes=sl, coef=cf)),
                   "frame": lambda: sen.measure(scrn, want_coef=False, colmajor=True, out=dict(slopes=sl, frame=fr)),
                   "torch_slopes": lambda: ts.run(scrn, tsl),
                   "torch_coef": lambda: ts.run(scrn, tsl, coef=tcf),
                   "torch_frame": lambda: ts.run(scrn, tsl, frame=tfr),
                   "estimator": lambda: est.apply_device(scrn, None, colmajor=True, out=eout)}
            # agreement before anything is timed
            fns["coef"](); fns["frame"](); fns["torch_coef"](); fns["torch_frame"](); torch.cuda.synchronize()
            gap_s = float((sl - tsl).abs().max()); gap_f = float((fr - tfr).abs().max() / tfr.abs().max())
            gap_c = float((cf - tcf).abs().max() / tcf.abs().max())
            got, calls = rounds(fns, args.rounds, args.reps)
            best = {k: min(v) for k, v in got.items()}
            flops = float(batch) * nlit * 8.0 * npl * s * (npl + s)
            case = {"batch": batch, "npl": npl, "pad": pad, "s": s, "nvalid": sen.nvalid, "lit": nlit, "nmode": args.nmode, "calls_per_window": calls,
                    "us": got, "best_us": best, "slopes_vs_torch_px": gap_s, "frame_vs_torch_rel": gap_f, "coef_vs_torch_rel": gap_c,
                    "hbm_floor_us": floor, "hbm_fraction_slopes": floor / best["slopes"], "nominal_flops": flops,
                    "matrix_floor_us": flops / FP64_MATRIX_PEAK * 1e6, "matrix_peak_fraction_slopes": flops / FP64_MATRIX_PEAK * 1e6 / best["slopes"],
                    "torch_over_slopes": best["torch_slopes"] / best["slopes"], "torch_over_coef": best["torch_coef"] / best["coef"],
                    "torch_over_frame": best["torch_frame"] / best["frame"], "estimator_over_slopes": best["estimator"] / best["slopes"],
                    "estimator_over_coef": best["estimator"] / best["coef"],
                    "slower_than_torch_beyond_spread": {k: min(got[k]) > max(got["torch_" + k]) for k in ("slopes", "coef", "frame")}}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            sen.close()
            del sl, cf, fr, tsl, tcf, tfr, ts
            torch.cuda.empty_cache()
        del scrn, eout
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
