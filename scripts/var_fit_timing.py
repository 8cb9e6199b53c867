"""Timing of the VAR identification and validation entries on one MI355X: nothing is asserted.

    python scripts/var_fit_timing.py [--reps 20] [--legs small,large,validate]

Legs (series of num_train = 1000 samples of the synthetic model, one realisation per series):
  small     (n, order) = (27, 2) at batch 1, 256, 2048: the LDS kernel of fmpc_var_identify_device (what fmpc_var_fit_device
            hands these sizes to) against the blocked kernels forced onto the same input (FMPC_VARFIT_BLOCKED=1, read at call
            time), with the relative difference of the two results
  large     (65, 2) and (111, 2) at batch 1, 256, 2048 and (27, 1) at 256 through the blocked kernels, against a plain torch
            formulation on the same device: torch.bmm Gram matrices, torch.linalg.cholesky, torch.cholesky_solve
  validate  fmpc_var_validate_device at (65, 2), count 500, batch 256
Every figure comes with its batch and the workspace the fit used.  Times are medians over --reps calls after 3 warm-up calls,
device events around the enqueue; boxes differ by up to 10 %.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NUM_TRAIN = 1000


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
    ap.add_argument("--legs", default="small,large,validate")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}

    def series(n, order, batch, steps=NUM_TRAIN - 1):
        model = pkg.synthetic.make_model(n, 16, 4, var_order=order)
        uniq = np.stack([pkg.synthetic.make_realisation(model, r=b + 1, steps=steps) for b in range(min(batch, 16))])
        return torch.from_numpy(uniq[np.arange(batch) % len(uniq)].copy()).to(dev)   # (more series than 16: the same again, the work is the same)

    def fit_ms(t, order, tag):
        batch, _, n = t.shape
        ws = torch.empty(pkg.var_fit_workspace_bytes(n, order, batch), dtype=torch.uint8, device=dev)
        res = pkg.identify_var_device(t, order=order, workspace=ws)
        out[f"{tag}_ms"] = timed(lambda: pkg.identify_var_device(t, order=order, workspace=ws, out=res), args.reps)
        out[f"{tag}_workspace_bytes"] = ws.numel()
        return res

    def torch_fit(t, order):
        ns, n = t.shape[1], t.shape[2]
        AA = torch.cat([t[:, order - j:ns - j] for j in range(1, order + 1)], dim=2)
        BB = t[:, order:]
        L = torch.linalg.cholesky(torch.bmm(AA.transpose(1, 2), AA))
        return torch.cholesky_solve(torch.bmm(AA.transpose(1, 2), BB), L)

    if "small" in legs:
        for batch in (1, 256, 2048):
            t = series(27, 2, batch)
            os.environ.pop("FMPC_VARFIT_BLOCKED", None)
            old = fit_ms(t, 2, f"lds_n27_o2_b{batch}")
            os.environ["FMPC_VARFIT_BLOCKED"] = "1"
            new = fit_ms(t, 2, f"blocked_n27_o2_b{batch}")
            os.environ.pop("FMPC_VARFIT_BLOCKED", None)
            torch.cuda.synchronize()
            out[f"blocked_vs_lds_n27_o2_b{batch}_rel"] = max(float((a - b).norm() / b.norm()) for a, b in zip(new[:2], old[:2]))
    if "large" in legs:
        for n, order, batches in ((65, 2, (1, 256, 2048)), (111, 2, (1, 256, 2048)), (27, 1, (256,))):
            for batch in batches:
                t = series(n, order, batch)
                os.environ["FMPC_VARFIT_BLOCKED"] = "1"                              # ((27, 1) is blocked anyway)
                res = fit_ms(t, order, f"blocked_n{n}_o{order}_b{batch}")
                os.environ.pop("FMPC_VARFIT_BLOCKED", None)
                out[f"torch_n{n}_o{order}_b{batch}_ms"] = timed(lambda: torch_fit(t, order), max(3, args.reps // 2))
                para = torch_fit(t, order)
                torch.cuda.synchronize()
                out[f"blocked_vs_torch_n{n}_o{order}_b{batch}_rel"] = float((res[0] - para[:, :n].transpose(1, 2)).norm() / res[0].norm())
    if "validate" in legs:
        n, order, batch, count = 65, 2, 256, 500
        t = series(n, order, batch, steps=NUM_TRAIN + count - 1)
        A1, A2, _ = pkg.identify_var_device(t, order=order, num_train=NUM_TRAIN)
        res = pkg.validate_var_device(t, A1, A2, first=NUM_TRAIN, count=count)
        out[f"validate_n{n}_o{order}_c{count}_b{batch}_ms"] = timed(
            lambda: pkg.validate_var_device(t, A1, A2, first=NUM_TRAIN, count=count, out=res), args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
