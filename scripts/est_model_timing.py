"""Timing of the estimator's optics on one MI355X: the linearised image model A_s, b_s built on the device
(fmpc_est_model_device) against the same model composed from torch.fft.fft2 on the device and from numpy on the host, and
against the estimator itself on as many screens as the model has fields; the Zernike grid kernel against its bytes.

    python scripts/est_model_timing.py [--rounds 5] [--reps 5] [--sizes 512,64] [--out FILE]

Per size (len; N = 6: 28 modes, 3 diversities, the README's window: d = 31):
  model     EstimatorOptics.model with out= and workspace= at the recommended size (nothing allocated per call), phi0 = None
  model_phi the same about an operating point (one sincos per pixel and k-step)
  torch     fftshift(fft2(fftshift(.))) of the 29 x 3 fields on the device, window, |I|^2 and 2 Re(conj(I) dI); the largest
            relative gap to `model` (b_s; A_s against its largest column norm) is reported before anything is timed
  numpy     the same on the host, in the manner of synthetic.estimator_optics (one run: it takes seconds at 512)
  apply29   the yardstick: fmpc_est_apply_device on a batch of 29 screens -- the same number of partial DFTs, plus a sincos per
            pixel and the product with G
  zernike   fmpc_zernike_grid_device of the 28 maps; its floor is the 8 x 28 x len^2 bytes it writes at the 6.3 TB/s copy rate
Times are medians over --reps windows of back-to-back calls between two device events (calls per window sized from a pilot so
that a window lasts about 20 ms), after a warm-up window, in one process, the sides alternating for --rounds rounds; every
round's median is listed and the best of each side is compared.  The matrix-core roofline of the model is its nominal work --
per field and diversity 6 len^2 32 (three real 16 x 4 x 32 products per k-step, all k-steps) + 8 x 32 x 32 len (the second
factor) -- over the fp64 matrix peak of 78.6 TFLOP/s; the k-steps outside the pupil (21 % at the README's geometry) are not
issued, so the fraction is an upper estimate of the rate the kernel sustains."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_RATE = 6.3e12
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


def numpy_model(pupil, W, zd_list, dx, rmin, rmax, Z, AU):
    d = rmax - rmin + 1
    ft = lambda P_: (np.fft.fftshift(np.fft.fft2(np.fft.fftshift(P_))) * dx ** 2)[rmin:rmax + 1, rmin:rmax + 1]
    b_s = np.zeros(len(zd_list) * d * d); A_s = np.zeros((len(zd_list) * d * d, len(Z)))
    for k, zd in enumerate(zd_list):
        P0 = pupil * np.exp(1j * zd * W)
        I0 = ft(P0)
        b_s[k * d * d:(k + 1) * d * d] = (np.abs(I0) ** 2 * AU).reshape(-1, order="F")
        for j in range(len(Z)):
            A_s[k * d * d:(k + 1) * d * d, j] = (2.0 * AU * np.real(np.conj(I0) * ft(1j * Z[j] * P0))).reshape(-1, order="F")
    return A_s, b_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="512,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "sizes": {}}
    for L in (int(s) for s in args.sizes.split(",")):
        opt = pkg.reference_optics(L)
        Z, nmode, nd, d, p = opt.Z, int(opt.Z.shape[0]), opt.ndiv, opt.d, opt.p
        ws = torch.empty(opt.workspace_bytes(nmode), dtype=torch.uint8, device=dev)
        res = (torch.empty((nmode, p), dtype=torch.float64, device=dev).t(), torch.empty(p, dtype=torch.float64, device=dev))
        gen = torch.Generator(device=dev); gen.manual_seed(77)
        phi = 0.25 * torch.randn((L, L), dtype=torch.float64, device=dev, generator=gen)
        model = lambda: opt.model(Z, workspace=ws, out=res)
        model_phi = lambda: opt.model(Z, phi0=phi, workspace=ws, out=res)
        # the same from torch.fft, in the maps' own [column, row] order (the transform of a transpose is the transpose)
        zd = torch.from_numpy(opt.zd_list).to(dev)
        pup = torch.from_numpy(np.ascontiguousarray(opt.pupil.T)).to(dev)
        D = pup[None] * torch.exp(1j * zd[:, None, None] * Z[4][None])
        lo, hi = opt.range_min - 1, opt.range_max
        scale = opt.dx ** 4 * opt.AU

        def composed():
            fields = torch.cat([D[:, None], 1j * Z[None] * D[:, None]], dim=1)                       # (nd, 1 + nmode, L, L)
            F = torch.fft.fftshift(torch.fft.fft2(torch.fft.fftshift(fields, dim=(-2, -1))), dim=(-2, -1))[..., lo:hi, lo:hi]
            I0 = F[:, 0]
            b = (scale * (I0.real ** 2 + I0.imag ** 2)).reshape(-1)
            A = (2.0 * scale * (I0[:, None].conj() * F[:, 1:]).real).permute(1, 0, 2, 3).reshape(nmode, -1)
            return A, b

        model(); A_t, b_t = composed(); torch.cuda.synchronize()
        gap_b = float((res[1] - b_t).norm() / b_t.norm())
        gap_A = float(((res[0].t() - A_t).norm(dim=1)).max() / A_t.norm(dim=1).max())
        # the host
        Zh = np.ascontiguousarray(np.swapaxes(Z.cpu().numpy(), -1, -2))
        t0 = time.perf_counter()
        A_h, b_h = numpy_model(opt.pupil, Zh[4], opt.zd_list, opt.dx, lo, hi - 1, Zh, opt.AU)
        numpy_s = time.perf_counter() - t0
        gap_h = float(np.linalg.norm(res[1].cpu().numpy() - b_h) / np.linalg.norm(b_h))
        # the yardstick: the estimator on nmode + 1 screens
        est = opt.estimator(Z, skip=1)
        scr = 0.25 * torch.randn((nmode + 1, L, L), dtype=torch.float64, device=dev, generator=gen)
        ad = torch.empty((nmode + 1, est.nx), dtype=torch.float64, device=dev)
        apply29 = lambda: est.apply_device(scr, colmajor=True, out=ad)
        # the maps
        n_, m_ = pkg.zernike_modes(6)
        Zbuf = torch.empty_like(Z)
        lib, ip = pkg.load(), pkg._lib._ip
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        zern = lambda: lib.fmpc_zernike_grid_device(nmode, n_.ctypes.data_as(ip), m_.ctypes.data_as(ip), L, 0, C.c_void_p(Zbuf.data_ptr()), stream)
        sides = {"model": model, "model_phi": model_phi, "torch": composed, "apply29": apply29, "zernike": zern}
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(Zbuf, Z)
        calls = {k: int(min(200, max(3, 2.0e4 / window(fn, 3)))) for k, fn in sides.items()}
        t = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                t[k].append(timed(fn, args.reps, calls[k]))
        best = {k: min(v) for k, v in t.items()}
        flops = (nmode + 1) * nd * (6.0 * L * L * 32 + 8.0 * 32 * 32 * L)
        zbytes = 8.0 * nmode * L * L
        r = {"len": L, "nmode": nmode, "ndiv": nd, "d": d, "calls_per_window": calls, "us": t, "best_us": best,
             "spread": {k: max(v) / min(v) for k, v in t.items()},
             "model_vs_torch_rel_b": gap_b, "model_vs_torch_rel_A": gap_A, "model_vs_numpy_rel_b": gap_h, "numpy_s": numpy_s,
             "model_over_apply29": best["model"] / best["apply29"], "model_phi_over_apply29": best["model_phi"] / best["apply29"],
             "torch_over_model": best["torch"] / best["model"], "numpy_over_model": numpy_s * 1e6 / best["model"],
             "model_nominal_flops": flops, "model_matrix_roofline_fraction": flops / FP64_MATRIX_PEAK * 1e6 / best["model"],
             "zernike_bytes": zbytes, "zernike_hbm_floor_us": zbytes / HBM_COPY_RATE * 1e6,
             "zernike_hbm_roofline_fraction": zbytes / HBM_COPY_RATE * 1e6 / best["zernike"], "workspace_bytes": ws.numel()}
        out["sizes"][str(L)] = r
        print(L, json.dumps(r), flush=True)
        est.close(); opt.close()
        del ws, res, scr, Zbuf, D
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
