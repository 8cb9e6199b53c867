"""Timing of the bank's closed-loop step in its per-model first-move form against the stored-factor step on one MI355X
(DESIGN.md section 6): nothing is asserted.

    python scripts/bank_first_move_timing.py [--reps 10]

At (n, m, T) = (27, 144, 30), one model per realisation, n_newton = 1, first moves only, from the cold start, at 256 and 2048
realisations, in ONE run on one box:
  stored   fmpc_loop_step_bank_device with the stored factors, the form not built: the yardstick
  form     the same call after fmpc_bank_first_move_device for the same k
  build    fmpc_bank_first_move_device itself
and the bytes per second the form achieves against its traffic count (the 222624 bytes of operands per realisation).
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
OPERAND_BYTES = 8 * (4 * N * M + M + 2 * (2 * N + 1) * 4 * N + 2 * 4 * N + (N + 1) + 8)


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
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    dev = torch.device("cuda:0")
    base = pkg.synthetic.make_model(N, M, T)
    rng = np.random.default_rng(0)
    out = {"operand_bytes_per_model": OPERAND_BYTES}

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
    for batch in (256, 2048):
        h.set_model_bank(*models(batch))
        h.prefactor_model_bank(K)
        f64 = dict(dtype=torch.float64, device=dev)
        a = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
        xl = torch.from_numpy(0.3 * rng.standard_normal((batch, N))).to(dev)
        u1 = torch.from_numpy(0.1 * rng.standard_normal((batch, M))).to(dev); u2 = torch.from_numpy(0.1 * rng.standard_normal((batch, M))).to(dev)
        x0 = torch.empty((batch, N), **f64); x0p = torch.empty((batch, N), **f64); w = torch.empty((batch, T * N), **f64)
        u0 = torch.empty((batch, M), **f64)
        st = torch.empty(batch, dtype=torch.int32, device=dev); it = torch.empty(batch, dtype=torch.int32, device=dev)

        def one_call():
            h.loop_step_bank(a, xl, u1, u2, x0, x0p, w, None, 1, K, status=st, iters=it, u0_out=u0)

        def inputs_only():
            h.loop_inputs_bank(a, xl, u1, u2, x0, x0p, w)

        t_st = timed(one_call, args.reps)
        assert h.last_bank_stored_factor() and not h.last_bank_first_move()
        ref = u0.clone()
        out[f"loop_inputs_{batch}_ms"] = timed(inputs_only, args.reps)
        h.first_move_model_bank(K)
        torch.cuda.synchronize()
        t_fm = timed(one_call, args.reps)
        out[f"step_stored_{batch}_ms"] = t_st
        out[f"step_form_{batch}_ms"] = t_fm
        out[f"step_form_{batch}_used"] = bool(h.last_bank_first_move())
        out[f"step_form_{batch}_handed_over"] = h.last_dispatch()[1]
        out[f"step_form_{batch}_models"] = h.bank_first_move_count
        out[f"ratio_{batch}"] = t_st / t_fm
        out[f"step_form_{batch}_GBps"] = OPERAND_BYTES * batch / (t_fm * 1e-3) / 1e9
        out[f"step_form_{batch}_u0_rel_diff"] = float((u0 - ref).norm() / ref.norm())
        out[f"build_{batch}_ms"] = timed(lambda: h.first_move_model_bank(K), max(2, args.reps // 3))
        h.release_bank_first_move()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
