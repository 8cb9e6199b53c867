"""Timing of the atmosphere on one MI355X: one step of `Atmosphere` -- advance + screen -- against the same
arithmetic composed in torch and against the copy it replaces.

    python scripts/atm_timing.py [--rounds 3] [--reps 3] [--steps 20] [--batches 1,256,2000] [--lens 128,512] [--out FILE]
    python scripts/atm_timing.py --build 129,512          # the one-time host build of the operands (needs no device)

The atmosphere is reference_atmosphere (README.md:24-75: W = 129, the default stencil of 8 lines, three layers; 18.4 lines per
step on average), the screens are masked by the pupil disk and have their mean removed.
  device    `advance(1)` then `screen(out_len, mask, out=)` into a preallocated tensor.
  torch     the same process in torch on the device, windows (layers, batch, W, W): per extrusion the gather of the q lines,
            torch.randn for xi, two matmuls with A' and B', the shift by torch.cat; per screen an indexed bilinear gather per
            layer, the layer sum, the masked mean and the scale.  The line counts per step follow the same displacement rule.
  copy      the pinned host-to-device copy of batch x out_len^2 doubles: what a host-side generator costs per step at the least.
A window is --steps consecutive steps between two device events (the line count of a step varies, its average over 20 steps does
not); the figure is the median over --reps windows divided by the steps, after a warm-up window, the sides alternating for
--rounds rounds; the best round of each side is compared.
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_times(pkg, sizes):
    """Wall time of fmpc_atm_create for one layer and one realisation: the host build dominates (on a machine without a device the
    call returns FMPC_E_NO_DEVICE after the build)."""
    lib = pkg.load()
    out = {}
    one, zero = (C.c_double * 1)(1.0), (C.c_double * 1)(0.0)
    for W in sizes:
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.fmpc_atm_create(C.byref(h), W, 1.0 / (W - 2), 0.2, 42.0, 1, one, one, zero, 0.005, 0, None, 1, 0, 0, 0)
        dt = time.perf_counter() - t0
        if h.value:
            lib.fmpc_atm_destroy(h)
        q = len(pkg.atm_default_stencil(W))
        out[W] = dict(seconds=dt, rc=rc, q=q, qW=q * W)
        print(f"build W = {W} (q = {q}, q W = {q * W}): {dt:.2f} s (rc {rc})", flush=True)
    return out


class TorchAtmosphere:
    """The process composed of torch operators (not bit-compatible: torch.randn, float64 matmul)."""

    def __init__(self, atm, A, B, device):
        import torch
        self.W, self.s, self.layers, self.batch = atm.W, atm.stencil, atm.layers, atm.batch
        self.At = torch.from_numpy(A.T.copy()).to(device)                  # (q W, W)
        self.Bt = torch.from_numpy(B.T.copy()).to(device)
        self.sf = [math.sqrt(f) for f in atm.fractional_r0]
        self.vpx = [float(v) * math.cos(float(d)) * atm.dt / atm.pitch for v, d in zip(atm.wind_speed, atm.wind_direction)]
        self.vpy = [float(v) * math.sin(float(d)) * atm.dt / atm.pitch for v, d in zip(atm.wind_speed, atm.wind_direction)]
        self.win = torch.randn((self.layers, self.batch, self.W, self.W), dtype=torch.float64, device=device)
        self.k = 0
        self.device = device

    def extrude(self, l, axis, side):
        import torch
        W = self.W
        w = self.win[l] if axis == 0 else self.win[l].transpose(1, 2)
        z = torch.cat([w[:, :, s - 1] if side > 0 else w[:, :, W - s] for s in self.s], dim=1)
        xi = torch.randn((self.batch, W), dtype=torch.float64, device=self.device)
        line = (z @ self.At + self.sf[l] * (xi @ self.Bt)).unsqueeze(2)
        w = torch.cat([line, w[:, :, :-1]] if side > 0 else [w[:, :, 1:], line], dim=2)
        self.win[l] = w if axis == 0 else w.transpose(1, 2)

    def advance(self):
        for l in range(self.layers):
            for axis, v in ((0, self.vpx[l]), (1, self.vpy[l])):
                n = math.floor(abs((self.k + 1) * v)) - math.floor(abs(self.k * v))
                for _ in range(n):
                    self.extrude(l, axis, 1 if v > 0 else -1)
        self.k += 1

    def screen(self, out_len, mask, scale):
        import torch
        S = None
        t = torch.arange(out_len, dtype=torch.float64, device=self.device) * ((self.W - 2) / (out_len - 1))
        for l in range(self.layers):
            idx = []
            for v in (self.vpy[l], self.vpx[l]):
                d = abs(self.k * v)
                f = d - math.floor(d)
                c = t + (1.0 - f if v > 0 else f)
                i0 = torch.clamp(torch.floor(c), max=self.W - 2)
                idx.append((i0.long(), c - i0))
            (y0, wy), (x0, wx) = idx
            w = self.win[l]
            top, bot = w[:, y0], w[:, y0 + 1]
            wy, wx = wy[None, :, None], wx[None, None, :]
            b = (1 - wy) * ((1 - wx) * top[:, :, x0] + wx * top[:, :, x0 + 1]) + wy * ((1 - wx) * bot[:, :, x0] + wx * bot[:, :, x0 + 1])
            S = b if S is None else S + b
        mu = (S * mask).sum(dim=(1, 2)) / mask.sum()
        return scale * (mask * (S - mu[:, None, None]))


def window(fn, steps):
    import torch
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def timed(fn, reps, steps):
    window(fn, steps)
    return float(np.median([window(fn, steps) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="1,256,2000")
    ap.add_argument("--lens", default="128,512")
    ap.add_argument("--build", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    res = {}
    if args.build:
        res["build"] = build_times(pkg, [int(v) for v in args.build.split(",")])
    else:
        import torch
        dev = torch.device("cuda:0")
        A = B = None
        for batch in (int(v) for v in args.batches.split(",")):
            t0 = time.perf_counter()
            atm = pkg.reference_atmosphere(batch, 1)
            res.setdefault("create_seconds", time.perf_counter() - t0)
            atm.reset()
            if A is None:
                A, B = atm.extruder()
            tat = TorchAtmosphere(atm, A, B, dev)
            for n in (int(v) for v in args.lens.split(",")):
                x = (np.arange(n) - (n - 1) / 2.0) / ((n - 1) / 2.0)
                mask = torch.from_numpy((x[:, None] ** 2 + x[None, :] ** 2 <= 1.0).astype(np.float64)).to(dev)
                out = torch.empty((batch, n, n), dtype=torch.float64, device=dev)
                host = torch.empty((batch, n, n), dtype=torch.float64).pin_memory()
                fns = dict(device=lambda: (atm.advance(1), atm.screen(n, mask, 1.0, out)),
                           advance=lambda: atm.advance(1),
                           screen=lambda: atm.screen(n, mask, 1.0, out),
                           torch=lambda: (tat.advance(), tat.screen(n, mask, 1.0)),
                           copy=lambda: out.copy_(host, non_blocking=True))
                got = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for k, f in fns.items():
                        got[k].append(timed(f, args.reps, args.steps))
                best = {k: min(v) for k, v in got.items()}
                key = f"batch{batch}_len{n}"
                res[key] = dict(rounds_us=got, best_us=best, screen_bytes=batch * n * n * 8,
                                copy_GBps=batch * n * n * 8 / best["copy"] / 1e3,
                                screen_write_GBps=batch * n * n * 8 / best["screen"] / 1e3,
                                torch_over_device=best["torch"] / best["device"], copy_over_device=best["copy"] / best["device"])
                print(key, json.dumps({k: round(v, 1) for k, v in best.items()}),
                      f"torch/device {best['torch'] / best['device']:.2f} copy/device {best['copy'] / best['device']:.2f}", flush=True)
                del out, host
            del tat
            atm.close()
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
