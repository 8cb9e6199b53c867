"""Timing of the bank's closed-loop step with and without the stored cold-start factor on one MI355X:
nothing is asserted.

    python scripts/bank_prefactor_timing.py [--reps 10] [--legs step,build]
    FMPC_LIB=/path/to/older/libfastmpc.so python scripts/bank_prefactor_timing.py --legs step       # an older build: composed step only

Legs at (n, m, T) = (27, 144, 30), one model per realisation, n_newton = 1, first moves only, from the cold start:
  step   one closed-loop step at 256 and 2048 realisations
           composed   fmpc_loop_inputs_bank_device + fmpc_solve_bank_device (all an older build has)
           plain      fmpc_loop_step_bank_device without a stored factor
           stored     fmpc_loop_step_bank_device with the stored factors (fmpc_bank_prefactor_device for the same k)
  build  fmpc_bank_prefactor_device for 256 and 4096 models, and the store's device memory per model (by the layout, and as the
         change of free device memory with no store allocated before: the allocator's rounding included)
Times are medians over --reps calls after 3 warm-up calls, device events around the enqueue; boxes differ by up to 10 %, so compare
builds in ONE session, alternating (the caller runs this script under each library in turn, twice).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, M, T, K = 27, 144, 30, 1e-2


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    import ctypes
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--legs", default="step,build")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    probe = ctypes.CDLL(pkg._lib.LIB_PATH)                  # an older build (FMPC_LIB): leave what it does not export unbound
    missing = [k for k in pkg._lib.SIGNATURES if not hasattr(probe, k)]
    for name in missing:
        del pkg._lib.SIGNATURES[name]
    has_store = "fmpc_bank_prefactor_device" not in missing
    dev = torch.device("cuda:0")
    base = pkg.synthetic.make_model(N, M, T)
    rng = np.random.default_rng(0)
    out = {"has_store": has_store}

    def models(count):
        A1 = np.empty((count, N, N)); A2 = np.empty((count, N, N))
        for p in range(min(count, 256)):
            mp_ = pkg.synthetic.make_model(N, M, T, seed=1000 + p)
            A1[p], A2[p] = mp_["A1"], mp_["A2"]
        for p in range(256, count):                          # (more models than 256: the same matrices again, the work is the same)
            A1[p], A2[p] = A1[p % 256], A2[p % 256]
        t = lambda A: torch.from_numpy(A).to(dev).transpose(1, 2).contiguous().transpose(1, 2)
        return t(A1), t(A2)

    h = handle_from_model(pkg, base)
    if "step" in legs:
        for batch in (256, 2048):
            h.set_model_bank(*models(batch))
            f64 = dict(dtype=torch.float64, device=dev)
            a = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
            xl = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
            u1 = torch.from_numpy(0.1 * rng.standard_normal((batch, M))).to(dev); u2 = torch.from_numpy(0.1 * rng.standard_normal((batch, M))).to(dev)
            x0 = torch.empty((batch, N), **f64); x0p = torch.empty((batch, N), **f64); w = torch.empty((batch, T * N), **f64)
            u0 = torch.empty((batch, M), **f64)
            st = torch.empty(batch, dtype=torch.int32, device=dev); it = torch.empty(batch, dtype=torch.int32, device=dev)

            def composed():
                h.loop_inputs_bank(a, xl, u1, u2, x0, x0p, w)
                h.solve_bank_device(x0, x0p, w, None, None, 1, K, status=st, iters=it, u0_out=u0, want_z=False)

            def one_call():
                h.loop_step_bank(a, xl, u1, u2, x0, x0p, w, None, 1, K, status=st, iters=it, u0_out=u0)

            out[f"step_composed_{batch}_ms"] = timed(composed, args.reps)
            if has_store:
                out[f"step_plain_{batch}_ms"] = timed(one_call, args.reps)
                ref = u0.clone()
                h.prefactor_model_bank(K)
                out[f"step_stored_{batch}_ms"] = timed(one_call, args.reps)
                out[f"step_stored_{batch}_used"] = bool(h.last_bank_stored_factor())
                out[f"step_stored_{batch}_u0_rel_diff"] = float((u0 - ref).norm() / ref.norm())
                h.release_bank_prefactor()
    if "build" in legs and has_store:
        for count in (256, 4096):
            h.set_model_bank(*models(count))
            h.release_bank_prefactor()
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            h.prefactor_model_bank(K)
            torch.cuda.synchronize()
            out[f"store_bytes_per_model_{count}_allocated"] = (free0 - torch.cuda.mem_get_info()[0]) / count
            out[f"store_build_{count}_ms"] = timed(lambda: h.prefactor_model_bank(K), args.reps)
            out[f"store_models_{count}"] = h.bank_prefactor_count
        NB = N // 16 + 1
        out["store_bytes_per_model_layout"] = 8 * T * 3 * NB * NB * 256     # nb * 3 NB^2 tiles of 256 fp64 entries
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
