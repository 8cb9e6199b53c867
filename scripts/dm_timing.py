"""Timing of the mirror of Gaussian actuators on one MI355X: fmpc_dm_matrix_device and fmpc_dm_surface_device
against what they replace.

    python scripts/dm_timing.py [--rounds 5] [--reps 5] [--length 512] [--batches 1,256,2000] [--out FILE]

The mirror is reference_dm(length) (README.md:194-263, 144 actuators), the modes zernike_grid(6, length) (n = 28), skip = 1.
  matrix    GaussianDM.influence_matrix with out= and workspace= at the recommended size (nothing allocated per call), against
            composed  GaussianDM.influence into a preallocated (m, length, length) tensor followed by ModalFit.influence_matrix
                      with its workspace preallocated: the same build, the maps in memory;
            numpy     the maps and pinv(Z Z') Z I' on the host, one run by the wall clock.
            The largest relative gap per column between matrix and composed is reported before anything is timed.  The HBM
            roofline is on the compulsory bytes, the n mode maps, at the 6.3 TB/s measured copy rate of the part.
  surface   GaussianDM.surface with phase= and out= per batch size, against
            modal     fmpc_phase_residual_device on the same screens (27 modes, the handle's B: less arithmetic, another surface);
            einsum    phase + (Ex' o u_b) Ey as one batched torch matmul over device ex / ey tables (the tables precomputed).
            The roofline is one read and one write per pixel.
Times are medians over --reps windows of back-to-back calls between two device events (the calls per window sized from a pilot so
that a window lasts about 20 ms), after a warm-up window, in one process, the sides alternating for --rounds rounds; every
round's median is listed and the best of each side is compared.
"""
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
ORDER, N, SKIP = 6, 28, 1
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


def rounds(fns, n_rounds, reps):
    pilot = max(window(f, 3) for f in fns.values())
    calls = int(min(200, max(3, 2.0e4 / pilot)))
    got = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, f in fns.items():
            got[k].append(timed(f, reps, calls))
    return got, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--batches", default="1,256,2000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    L = args.length
    dm = pkg.reference_dm(L, 6.5e-6 * 512 / L)
    m, npx = dm.m, L * L
    Z = pkg.zernike_grid(ORDER, L)
    mf = pkg.ModalFit(Z)
    out = {"device": torch.cuda.get_device_name(0), "n": N, "m": m, "length": L, "skip": SKIP, "rounds": args.rounds, "reps": args.reps}

    # ---- B
    ws = torch.empty(pkg.dm_matrix_workspace_bytes(N, m, L, L), dtype=torch.uint8, device=dev)
    B = torch.empty((m, N - SKIP), dtype=torch.float64, device=dev).t()
    maps = torch.empty((m, L, L), dtype=torch.float64, device=dev)
    mws = torch.empty(pkg.modal_workspace_bytes(N, npx, m), dtype=torch.uint8, device=dev)
    fused = lambda: dm.influence_matrix(mf, skip=SKIP, workspace=ws, out=B)
    composed = lambda: mf.influence_matrix(dm.influence(out=maps), skip=SKIP, workspace=mws)
    fused(); ref = composed(); torch.cuda.synchronize()
    gap = float(((B - ref).norm(dim=0) / ref.norm(dim=0)).max())
    got, calls = rounds({"matrix": fused, "composed": composed}, args.rounds, args.reps)
    g = dm.geometry
    Zh = np.ascontiguousarray(np.swapaxes(Z.cpu().numpy(), -1, -2)).reshape(N, -1)
    t0 = time.perf_counter()
    al = np.log(g["coupling"]) / g["pitch"] ** 2
    I = np.exp(al * ((g["x"][None, None, :] - g["cx"][:, None, None]) ** 2 + (g["y"][None, :, None] - g["cy"][:, None, None]) ** 2))
    Bh = (np.linalg.pinv(Zh @ Zh.T) @ Zh @ I.reshape(m, -1).T)[SKIP:]
    numpy_us = (time.perf_counter() - t0) * 1e6
    gap_np = float((np.linalg.norm(B.cpu().numpy() - Bh, axis=0) / np.linalg.norm(Bh, axis=0)).max())
    floor = 8.0 * N * npx / HBM_COPY_RATE * 1e6
    a, b = got["matrix"], got["composed"]
    out["matrix"] = {"calls_per_window": calls, "matrix_vs_composed_rel": gap, "matrix_vs_numpy_rel": gap_np, "matrix_us": a, "composed_us": b,
                     "numpy_us": numpy_us, "matrix_spread": max(a) / min(a), "composed_spread": max(b) / min(b),
                     "composed_over_matrix": min(b) / min(a), "numpy_over_matrix": numpy_us / min(a), "slower_beyond_spread": min(a) > max(b),
                     "hbm_floor_us": floor, "hbm_roofline_fraction": floor / min(a), "workspace_bytes": ws.numel(), "maps_bytes": 8 * m * npx}
    print("matrix", json.dumps(out["matrix"]), flush=True)
    del maps, mws, ws, I
    torch.cuda.empty_cache()

    # ---- surface
    md = pkg.synthetic.make_model(N - 1, m, 10)
    h = pkg.FastMPCHandle(md["A1"], md["A2"], md["B"], md["Q"], md["R"], md["Qf"], md["u_min"], md["u_max"], md["x_min"], md["x_max"], md["T"])
    Zc = Z[1:].contiguous()
    al_t = float(np.log(dm.coupling) / dm.pitch ** 2)
    ex = torch.exp(al_t * (dm.x[None, :] - dm.cx[:, None]) ** 2)                         # (m, cols)
    ey = torch.exp(al_t * (dm.y[None, :] - dm.cy[:, None]) ** 2)                         # (m, rows)
    exT = ex.t().contiguous()
    vp = lambda t: C.c_void_p(t.data_ptr())
    out["surface"] = {}
    for batch in (int(v) for v in args.batches.split(",")):
        gen = torch.Generator(device=dev); gen.manual_seed(99 + batch)
        phase = torch.randn((batch, L, L), dtype=torch.float64, device=dev, generator=gen)
        u = torch.rand((batch, m), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        o = torch.empty_like(phase); o2 = torch.empty_like(phase)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        zonal = lambda: dm.surface(u, phase=phase, out=o)

        def modal():
            rc = h._lib.fmpc_phase_residual_device(h._h, batch, npx, vp(phase), vp(u), vp(Zc), vp(o2), stream)
            assert rc == 0
        einsum = lambda: phase + torch.matmul(exT[None] * u[:, None, :], ey)
        zonal(); ref = einsum(); torch.cuda.synchronize()
        gap = float((o - ref).abs().max() / ref.abs().max())
        del ref
        got, calls = rounds({"surface": zonal, "modal": modal, "einsum": einsum}, args.rounds, args.reps)
        floor = 16.0 * batch * npx / HBM_COPY_RATE * 1e6
        a = got["surface"]
        r = {"batch": batch, "calls_per_window": calls, "surface_vs_einsum_rel_to_max": gap, "surface_us": a, "modal_us": got["modal"],
             "einsum_us": got["einsum"], "surface_spread": max(a) / min(a), "modal_over_surface": min(got["modal"]) / min(a),
             "einsum_over_surface": min(got["einsum"]) / min(a), "hbm_floor_us": floor, "hbm_roofline_fraction": floor / min(a),
             "fp64_matrix_tflops": 2.0 * batch * npx * m / min(a) * 1e-6}
        out["surface"][str(batch)] = r
        print("surface", batch, json.dumps(r), flush=True)
        del phase, u, o, o2
        torch.cuda.empty_cache()
    h.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
