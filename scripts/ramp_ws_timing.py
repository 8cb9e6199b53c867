"""Device time of the workspace ramp kernel (fmpc_newton_ramp_ws, FMPC_PATH_RAMP_WS): VAR(1) with ramp rows at (n, m, T) =
(65, 144, 10) -- BASELINE configs[0]'s shape at radial order 10 -- batch 256, Newton budgets 1 and 5, diagonal and dense R.
Prints ms per call and the share of the fp64 peak (78.6 TFLOP/s) on a FLOP model per problem-step:
  diagonal R: (T n)^3 / 3 (Cholesky of Y) + T (T + 1) / 2 * 2 n^2 m (the blocks B diag(g) B')
  dense R:    + T (m^3 / 3 + m^2 (m + (j + 1) n) per stage j for the factor and its substitution, 2 m^3 + 2 m^2 j n for the
              next stage's inputs) + sum over the block pairs of 2 n^2 m (T - I) for V'V
Not part of bench.py."""
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

pkg = importlib.import_module("mpc-sensorlessao_amd")
from tests.util import handle_from_model

PEAK = 78.6e12


def flops(n, m, T, dense_r):
    f = (T * n) ** 3 / 3.0
    if not dense_r:
        return f + T * (T + 1) / 2 * 2.0 * n * n * m
    for j in range(T):
        f += m ** 3 / 3.0 + m * m * (m + (j + 1) * n)                 # factor of A_j, substitution against [I | V sources]
        if j + 1 < T:
            f += 2.0 * m ** 3 + 2.0 * m * m * (j + 1) * n             # Z_j' [Z_j | V_j*]
    f += sum(2.0 * n * n * m * (T - I) for I in range(T) for J in range(I + 1))   # V'V, lower block triangle
    return f


def main():
    n, m, T, B = 65, 144, 10, 256
    dev = torch.device("cuda:0")
    for dense_r in (False, True):
        md = pkg.synthetic.make_model(n, m, T, var_order=1)
        if dense_r:
            N = np.random.default_rng(36).standard_normal((m, m)) / np.sqrt(m)
            md["R"] = np.eye(m) + 0.15 * (N + N.T)
        data = pkg.synthetic.make_replay_batch(md, r=2, steps=B)
        du = 0.2121 * np.ones(m)
        u_prev = 0.1 * np.random.default_rng(8).standard_normal((B, m))
        h = handle_from_model(pkg, md)
        h.set_ramp(-du, du)
        x0 = torch.tensor(data["x0"], device=dev)
        nu0 = torch.tensor(np.ascontiguousarray(data["nu0"][:, :T * n]), device=dev)
        up = torch.tensor(u_prev, device=dev)
        z = torch.empty((B, T * (n + m)), device=dev, dtype=torch.float64)
        for nw in (1, 5):
            it = torch.empty(B, dtype=torch.int32, device=dev)
            for _ in range(2):
                h.solve_device(x0, None, None, None, nu0, nw, 1e-2, z_out=z, iters=it, u_prev=up)
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            reps = 3
            e0.record()
            for _ in range(reps):
                h.solve_device(x0, None, None, None, nu0, nw, 1e-2, z_out=z, iters=it, u_prev=up)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            steps = int(it.sum().item())
            f = flops(n, m, T, dense_r) * steps
            print("(%d, %d, %d) %s R  batch %d  budget %d: %.2f ms per call, %d Newton steps, %.0f MFLOP per problem-step, "
                  "%.3f of the fp64 peak  path %d" % (n, m, T, "dense" if dense_r else "diagonal", B, nw, ms, steps,
                                                       flops(n, m, T, dense_r) / 1e6, f / (ms * 1e-3) / PEAK, h.last_dispatch()[0]),
                  flush=True)
        h.close()


if __name__ == "__main__":
    main()
