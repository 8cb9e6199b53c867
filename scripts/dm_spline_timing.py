"""Timing of the mirror of spline actuators on one MI355X: fmpc_dm_spline_surface_device with its tile lists
against its own FMPC_DM_DENSE walk and against the Gaussian mirror's surface at the same m, fmpc_dm_spline_prepare_device, and
fmpc_dm_spline_matrix_device against fmpc_dm_matrix_device.

    python scripts/dm_spline_timing.py [--rounds 5] [--reps 30] [--batches 1,256,2000] [--out profiles/dm_spline_timing.json]

Geometries, all on the 512 x 512 pupil grid of reference_dm_geometry (README.md:194-263):
  ref-0.1, ref-0.3   its 12 x 12 actuators (pitch 61.5 px) with OOMAO's profile at mechanical coupling 0.1 and 0.3;
  32x32-0.1          32 x 32 actuators over the same extent (pitch 21.8 px), coupling 0.1.
Per geometry and batch size the candidates alternate in one process for --rounds rounds; a round's figure is the median over
--reps windows of back-to-back calls between two device events (the calls per window sized from a pilot so that a window lasts
about 2 ms, at least one call), after a warm-up window.  The best round of each side is compared and every round is listed.
For the sparse surface the script also reports the matrix instructions it issues (64 v_mfma_f64_16x16x4_f64 per screen, tile and
stage of 16 list entries, from the list lengths), the HBM floor on one read and one write per pixel at the 6.3 TB/s measured copy
rate of the part, the matrix floor at 78.6 TFLOP/s, and which of the two is the larger.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ORDER, N, SKIP, L = 6, 28, 1, 512
HBM_COPY_RATE = 6.3e12
FP64_MATRIX_PEAK = 78.6e12
MFMA_FLOP = 2 * 16 * 16 * 4


def window(fn, calls):
    import torch
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def rounds(fns, n_rounds, reps):
    """{name: [median microseconds of one call, per round]}, the sides alternating."""
    pilot = {k: window(f, 2) for k, f in fns.items()}
    calls = {k: int(min(100, max(1, 2.0e3 / p))) for k, p in pilot.items()}
    got = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, f in fns.items():
            window(f, calls[k])
            got[k].append(float(np.median([window(f, calls[k]) for _ in range(reps)])))
    return got


def geometry(pkg, name):
    g = pkg.reference_dm_geometry(L)
    if name.startswith("ref"):
        return dict(x=g["x"], y=g["y"], cx=g["cx"], cy=g["cy"], pitch=g["pitch"]), float(name.split("-")[1])
    m1 = 32
    lo, hi = g["cx"].min(), g["cx"].max()
    x0 = np.linspace(lo, hi, m1)
    return dict(x=g["x"], y=g["y"], cx=np.tile(x0, m1), cy=np.repeat(-x0, m1), pitch=(hi - lo) / (m1 - 1)), 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batches", default="1,256,2000")
    ap.add_argument("--geometries", default="ref-0.1,ref-0.3,32x32-0.1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    npx = L * L
    Z = pkg.zernike_grid(ORDER, L)
    mf = pkg.ModalFit(Z)
    out = {"device": torch.cuda.get_device_name(0), "length": L, "n": N, "skip": SKIP, "rounds": args.rounds, "reps": args.reps, "geometries": {}}
    batches = [int(v) for v in args.batches.split(",")]
    for name in args.geometries.split(","):
        g, mech = geometry(pkg, name)
        prof = pkg.oomao_profile(mech)
        sdm = pkg.SplineDM(g["x"], g["y"], g["cx"], g["cy"], g["pitch"], prof)
        gdm = pkg.GaussianDM(g["x"], g["y"], g["cx"], g["cy"], mech, g["pitch"])
        m = sdm.m
        lens = np.array([len(s) for s in sdm.tile_lists()])
        stages = int(np.sum(-(-lens // 16)))
        rec = {"m": m, "mech": mech, "pitch_px": float(g["pitch"] / abs(g["x"][1] - g["x"][0])), "support_pitches": prof.support[1],
               "list_min": int(lens.min()), "list_max": int(lens.max()), "stages_per_screen": stages, "dense_stages_per_screen": int(len(lens) * -(-m // 16)),
               "mfma_per_screen": 64 * stages, "mfma_share_of_dense": stages / (len(lens) * -(-m // 16)), "workspace_bytes": int(sdm.ws.numel())}
        # ---- prepare and B
        ws2 = torch.empty(pkg.dm_spline_matrix_workspace_bytes(N, m, L, L), dtype=torch.uint8, device=dev)
        wsg = torch.empty(pkg.dm_matrix_workspace_bytes(N, m, L, L), dtype=torch.uint8, device=dev)
        B = torch.empty((m, N - SKIP), dtype=torch.float64, device=dev).t()
        Bg = torch.empty((m, N - SKIP), dtype=torch.float64, device=dev).t()
        got = rounds({"prepare": sdm.prepare, "matrix": lambda: sdm.influence_matrix(mf, skip=SKIP, workspace=ws2, out=B),
                      "gauss_matrix": lambda: gdm.influence_matrix(mf, skip=SKIP, workspace=wsg, out=Bg)}, args.rounds, args.reps)
        rec["setup"] = {k + "_us": v for k, v in got.items()}
        rec["setup"]["gauss_matrix_over_matrix"] = min(got["gauss_matrix"]) / min(got["matrix"])
        print(name, "setup", json.dumps(rec["setup"]), flush=True)
        del ws2, wsg
        # ---- surface
        rec["surface"] = {}
        for batch in batches:
            gen = torch.Generator(device=dev); gen.manual_seed(99 + batch)
            phase = torch.randn((batch, L, L), dtype=torch.float64, device=dev, generator=gen)
            u = torch.rand((batch, m), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
            o = torch.empty_like(phase)
            fns = {"sparse": lambda: sdm.surface(u, phase=phase, out=o), "dense": lambda: sdm.surface(u, phase=phase, out=o, dense=True),
                   "gauss": lambda: gdm.surface(u, phase=phase, out=o)}
            a = sdm.surface(u, phase=phase); b = sdm.surface(u, phase=phase, dense=True)
            gap = float((a - b).abs().max() / b.abs().max())
            del a, b
            got = rounds(fns, args.rounds, args.reps)
            t = min(got["sparse"])
            hbm = 16.0 * batch * npx / HBM_COPY_RATE * 1e6
            mat = 64.0 * stages * batch * MFMA_FLOP / FP64_MATRIX_PEAK * 1e6
            r = {"batch": batch, "sparse_vs_dense_rel_to_max": gap, "sparse_us": got["sparse"], "dense_us": got["dense"], "gauss_us": got["gauss"],
                 "sparse_spread": max(got["sparse"]) / t, "gauss_over_sparse": min(got["gauss"]) / t, "dense_over_sparse": min(got["dense"]) / t,
                 "us_per_screen": t / batch, "mfma_issued": 64 * stages * batch, "hbm_floor_us": hbm, "hbm_roofline_fraction": hbm / t,
                 "matrix_floor_us": mat, "matrix_peak_fraction": mat / t, "bound": "hbm" if hbm >= mat else "matrix",
                 "not_slower_than_gauss_5pct": t <= 1.05 * min(got["gauss"]), "not_slower_than_dense_5pct": t <= 1.05 * min(got["dense"])}
            rec["surface"][str(batch)] = r
            print(name, "surface", batch, json.dumps(r), flush=True)
            del phase, u, o
            torch.cuda.empty_cache()
        out["geometries"][name] = rec
    gs = out["geometries"]
    if "ref-0.1" in gs and "32x32-0.1" in gs:
        ratio = gs["32x32-0.1"]["stages_per_screen"] / gs["ref-0.1"]["stages_per_screen"]
        cmp_ = {"stage_ratio": ratio}
        for bs in gs["ref-0.1"]["surface"]:
            tr = gs["32x32-0.1"]["surface"][bs]["us_per_screen"] / gs["ref-0.1"]["surface"][bs]["us_per_screen"]
            cmp_[bs] = {"time_ratio": tr, "within_stage_ratio_plus_25pct": tr <= 1.25 * ratio, "within_1.25": tr <= 1.25}
        out["m1024_over_m144"] = cmp_
        print("m1024_over_m144", json.dumps(cmp_), flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
