"""Timing of the KKT report on one MI355X: the kernel against the same six quantities composed in torch.

    python scripts/kkt_report_timing.py [--reps 20] [--calls 20] [--batches 256,2000] [--out FILE]

At (n, m, T) = (27, 144, 30), per batch size, with z, nu of a one-step solve from the cold start (solve_device, budget 1, k = 1e-2):
  kkt      fmpc_kkt_report_device, the full report with nu (the panel kernel and its fold)
  torch    the yardstick: unpack_device for U, X, then torch products (U B', X A1', X A2', nu B, nu A1, nu A2 as batched matmuls) and
           elementwise kernels for the slacks, the logarithms, the diagonal terms and the six reductions; the largest absolute gap
           to `kkt` per field is reported before anything is timed
  solve    the solve that produced z and nu
Times are medians over --reps windows of --calls back-to-back calls between two device events, after 3 warm-up windows, in one
process, the two sides alternating (two rounds each, the smaller median is reported).  The HBM floor is the bytes a problem must
move (z, nu, x0, x0_pre, w, the report row) over the 8.0 TB/s peak of the part.  The script exits non-zero when the kernel is
slower than the composition at any batch size.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, M, T = 27, 144, 30
K = 1e-2
HBM_PEAK = 8.0e12


def timed(fn, reps, calls, warm=3):
    """Median time of one call in microseconds."""
    import torch
    for _ in range(warm):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", default="256,2000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from tests.util import handle_from_model
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    md = pkg.synthetic.make_model(N, M, T)
    rng = np.random.default_rng(1)
    md["q"] = 0.1 * rng.standard_normal(N); md["r"] = 0.1 * rng.standard_normal(M); md["qf"] = 0.1 * rng.standard_normal(N)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    tB, tBt, tA1, tA1t, tA2, tA2t = (t(v) for v in (md["B"], md["B"].T, md["A1"], md["A1"].T, md["A2"], md["A2"].T))
    q2 = np.tile(2.0 * np.diag(md["Q"]), (T, 1)); q2[T - 1] = 2.0 * np.diag(md["Qf"])
    ql = np.tile(md["q"], (T, 1)); ql[T - 1] = md["qf"]
    tQ2, tql, tR2, trl, tumin, tumax = t(q2), t(ql), t(2.0 * np.diag(md["R"])), t(md["r"]), t(md["u_min"]), t(md["u_max"])
    out = {"device": torch.cuda.get_device_name(0), "shape": [N, M, T], "reps": args.reps, "calls_per_window": args.calls}
    slower = False
    for batch in (int(b) for b in args.batches.split(",")):
        h = handle_from_model(pkg, md)
        data = pkg.synthetic.make_replay_batch(md, r=0, steps=batch)
        x0, x0p = t(data["x0"]), t(data["x0_pre"])
        w = t(0.01 * np.random.default_rng(2).standard_normal((batch, T * N)))
        nu0 = t(np.random.default_rng(3).random((batch, h.nu_len)))
        nu = torch.empty_like(nu0)
        z, status, iters = h.solve_device(x0, x0p, w, nu0=nu0, n_newton=1, k=K, nu_out=nu)
        solve = lambda: h.solve_device(x0, x0p, w, nu0=nu0, n_newton=1, k=K, z_out=z, nu_out=nu, status=status, iters=iters)
        rep = torch.empty((batch, 6), dtype=torch.float64, device=dev); flags = torch.empty(batch, dtype=torch.int32, device=dev)
        kkt = lambda: h.kkt_report_device(x0, x0p, w, z=z, nu=nu, k=K, out=rep, flags=flags)
        U = torch.empty((batch, T, M), dtype=torch.float64, device=dev); X = torch.empty((batch, T, N), dtype=torch.float64, device=dev)
        NU = nu.view(batch, T, N); W = w.view(batch, T, N)

        def composed():
            h.unpack_device(z, U=U, X=X)
            hi, lo = tumax - U, U - tumin
            mn = torch.minimum(hi, lo).amin(dim=(1, 2))
            bar = -(torch.log(hi) + torch.log(lo)).sum(dim=(1, 2))
            r2u = U * tR2
            gu = r2u + trl + K * (1.0 / hi - 1.0 / lo) - torch.matmul(NU, tB)
            q2x = X * tQ2
            gx = q2x + tql + NU
            gx[:, :-1] -= torch.matmul(NU[:, 1:], tA1)
            gx[:, :-2] -= torch.matmul(NU[:, 2:], tA2)
            xj = torch.cat([x0[:, None], X[:, :-1]], dim=1)
            xjm = torch.cat([x0p[:, None], x0[:, None], X[:, :-2]], dim=1)
            rp_ = X - torch.matmul(U, tBt) - torch.matmul(xj, tA1t) - torch.matmul(xjm, tA2t) - W
            rd2 = (gu * gu).sum(dim=(1, 2)) + (gx * gx).sum(dim=(1, 2))
            rp2 = (rp_ * rp_).sum(dim=(1, 2))
            cost = (U * (0.5 * r2u + trl)).sum(dim=(1, 2)) + (X * (0.5 * q2x + tql)).sum(dim=(1, 2))
            return torch.stack([rd2.sqrt(), rp2.sqrt(), (rd2 + rp2).sqrt(), cost, bar, mn], dim=1)

        ref = composed(); kkt(); torch.cuda.synchronize()
        # (rd, rp, nr of a converged problem are differences of terms of order 1e2 that cancel to 1e-9 and below: the absolute gap counts)
        r = {"kkt_vs_torch_abs": [float((rep[:, f] - ref[:, f]).abs().max()) for f in range(6)],
             "torch_abs_max": [float(ref[:, f].abs().max()) for f in range(6)],
             "infeasible": int((flags & 2).ne(0).sum()), "converged": int((flags & 1).ne(0).sum())}
        a1 = timed(kkt, args.reps, args.calls); b1 = timed(composed, args.reps, args.calls)
        a2 = timed(kkt, args.reps, args.calls); b2 = timed(composed, args.reps, args.calls)
        r["kkt_us"], r["torch_us"] = [a1, a2], [b1, b2]
        r["solve_us"] = timed(solve, args.reps, args.calls)
        bytes_ = batch * 8 * (h.nz + h.nu_len + 2 * N + T * N + 6)
        r["bytes"] = bytes_
        r["hbm_floor_us"] = bytes_ / HBM_PEAK * 1e6
        r["hbm_roofline_fraction"] = r["hbm_floor_us"] / min(a1, a2)
        r["torch_over_kkt"] = min(b1, b2) / min(a1, a2)
        r["kkt_share_of_solve"] = min(a1, a2) / r["solve_us"]
        slower = slower or min(a1, a2) > min(b1, b2)
        out["batch_%d" % batch] = r
        h.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
