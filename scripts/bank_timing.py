"""Timing of the model bank on one MI355X: nothing is asserted.

    python scripts/bank_timing.py [--reps 20] [--legs bank,handles,shared,build]

Legs at (n, m, T) = (27, 144, 30), one model per problem, explicit mid-box start (so that every leg is the per-problem-factor
tiled kernel and they differ in nothing but where the model comes from):
  bank     fmpc_solve_bank_device, 256 and 2048 problems, Newton budgets 1 and 5
  handles  what a caller could do without a bank: 256 handles, one fmpc_solve_u0_device each, back to back on one stream
           (this leg needs no bank entry point: run it against an older build with FMPC_LIB=... to compare builds)
  shared   the same batch with ONE shared model, forced onto the tiled kernel (FMPC_TILED=1): what the per-problem operands cost
  build    fmpc_bank_set_device for 256 and 4096 models, and the bank's device memory per model (by the layout, and as the change of
           free device memory with no bank allocated before: the allocator's rounding included)
The bank leg also times fmpc_loop_inputs_bank_device on the same batches.
Times are medians over --reps calls after 3 warm-up calls, device events around the enqueue; boxes differ by up to 10 %.
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", default="bank,handles,shared,build")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch
    if "shared" in legs:
        os.environ["FMPC_TILED"] = "1"                      # read by fmpc_create (the shared-model handle below)
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    if "bank" not in legs and "build" not in legs:          # an older build (FMPC_LIB) has no bank entry points to bind
        for name in [k for k in pkg._lib.SIGNATURES if "_bank" in k]:
            del pkg._lib.SIGNATURES[name]
    dev = torch.device("cuda:0")
    base = pkg.synthetic.make_model(N, M, T)
    rng = np.random.default_rng(0)
    out = {}

    def models(count):
        A1 = np.empty((count, N, N)); A2 = np.empty((count, N, N))
        for p in range(min(count, 256)):
            mp_ = pkg.synthetic.make_model(N, M, T, seed=1000 + p)
            A1[p], A2[p] = mp_["A1"], mp_["A2"]
        for p in range(256, count):                          # (more models than 256: the same matrices again, the work is the same)
            A1[p], A2[p] = A1[p % 256], A2[p % 256]
        return A1, A2

    def data(batch):
        x0 = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
        x0p = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
        nu0 = torch.from_numpy(rng.random((batch, T * N))).to(dev)
        s = np.concatenate([(base["u_min"] + base["u_max"]) / 2, (base["x_min"] + base["x_max"]) / 2])
        zi = torch.from_numpy(np.tile(s, T)[None, :].repeat(batch, 0)).to(dev).contiguous()
        return x0, x0p, nu0, zi

    if "shared" in legs:
        h = handle_from_model(pkg, base)
        for batch in (256, 2048):
            x0, x0p, nu0, zi = data(batch)
            z = torch.empty((batch, h.nz), dtype=torch.float64, device=dev)
            st = torch.empty(batch, dtype=torch.int32, device=dev); it = torch.empty(batch, dtype=torch.int32, device=dev)
            for budget in (1, 5):
                out[f"shared_{batch}_nw{budget}_ms"] = timed(lambda: h.solve_device(x0, x0p, None, zi, nu0, budget, K, z_out=z, status=st, iters=it), args.reps)
        h.close()
        os.environ.pop("FMPC_TILED", None)
    if "bank" in legs or "build" in legs:
        h = handle_from_model(pkg, base)
        for count in (256, 4096) if "build" in legs else (256,):
            A1, A2 = models(count)
            tA1 = torch.from_numpy(A1).to(dev).transpose(1, 2).contiguous().transpose(1, 2)
            tA2 = torch.from_numpy(A2).to(dev).transpose(1, 2).contiguous().transpose(1, 2)
            h.release_model_bank()                           # (an earlier, smaller bank would be freed inside the interval)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            h.set_model_bank(tA1, tA2)
            torch.cuda.synchronize()
            out[f"bank_bytes_per_model_{count}_allocated"] = (free0 - torch.cuda.mem_get_info()[0]) / count
            out[f"bank_build_{count}_ms"] = timed(lambda: h.set_model_bank(tA1, tA2), args.reps)
        # by the layout (csrc/fmpc_bank.h): A1 | A2 | A1' | A2' plain and padded to 16 NB, (blocks + 1) NB^2 tiles of 256 fp64 entries
        NB, nblk = N // 16 + 1, 7                            # (7 constant Y blocks at T >= 4, VAR(2), Qf == Q)
        out["bank_bytes_per_model_layout"] = 8 * (4 * N * N + 4 * (16 * NB) ** 2 + (nblk + 1) * NB * NB * 256)
        if "bank" in legs:
            A1, A2 = models(2048)
            h.set_model_bank(torch.from_numpy(A1).to(dev), torch.from_numpy(A2).to(dev))
            for batch in (256, 2048):
                x0, x0p, nu0, zi = data(batch)
                z = torch.empty((batch, h.nz), dtype=torch.float64, device=dev)
                st = torch.empty(batch, dtype=torch.int32, device=dev); it = torch.empty(batch, dtype=torch.int32, device=dev)
                for budget in (1, 5):
                    out[f"bank_{batch}_nw{budget}_ms"] = timed(lambda: h.solve_bank_device(x0, x0p, None, zi, nu0, budget, K, z_out=z, status=st, iters=it), args.reps)
                # the loop inputs of the same batch with each problem's own model (fmpc_loop_inputs_bank_device)
                u1 = torch.from_numpy(rng.standard_normal((batch, M))).to(dev); u2 = torch.from_numpy(rng.standard_normal((batch, M))).to(dev)
                xo = torch.empty_like(x0); xpo = torch.empty_like(x0); w = torch.empty((batch, T * N), dtype=torch.float64, device=dev)
                out[f"bank_loop_inputs_{batch}_ms"] = timed(lambda: h.loop_inputs_bank(x0, x0p, u1, u2, xo, xpo, w), args.reps)
        h.close()
    if "handles" in legs:
        batch = 256
        A1, A2 = models(batch)
        hs = []
        for p in range(batch):
            mdl = dict(base); mdl["A1"], mdl["A2"] = A1[p], A2[p]
            hs.append(handle_from_model(pkg, mdl))
        x0, x0p, nu0, zi = data(batch)
        z = torch.empty((batch, hs[0].nz), dtype=torch.float64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev); it = torch.empty(batch, dtype=torch.int32, device=dev)
        u0 = torch.empty((batch, M), dtype=torch.float64, device=dev)
        rows = [(x0[p:p + 1], x0p[p:p + 1], nu0[p:p + 1], zi[p:p + 1], z[p:p + 1], st[p:p + 1], it[p:p + 1], u0[p:p + 1]) for p in range(batch)]
        for budget in (1, 5):
            def run():
                for hh, (a, b, c, d, e, f, g, u) in zip(hs, rows):
                    hh.solve_device(a, b, None, d, c, budget, K, z_out=e, status=f, iters=g, u0_out=u)
            out[f"handles_{batch}_nw{budget}_ms"] = timed(run, max(3, args.reps // 4))
        for hh in hs:
            hh.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
