"""Gram-form closure against the streaming closure: wall time of whole fits, and the two new kernels on their own.

    python tests/perf/gram_fit.py [--out profiles/gram_fit.json]

  * fits (best of 3, wall time including the one-pass statistics): the 64-seed L-BFGS sweep of bench.py's seed_sweeps leg
    (64 seeds x 50 000 points x 2, order 3, 60 epochs) and the single 50x2500x2 fit (train_SIGED_lbfgs's device trainer
    shape) at orders 3 and 5, each with closure "stream" and "gram";
  * symode_quad_closure at statistics built from 125 000, 2^20 and 2^24 points (its cost cannot depend on N: event timing);
  * symode_symreg_reversed_gram at 2^24 points, d = 2, orders 3 and 5, n_g = 1, priced at d p (d p + 1) / 2 * d FMAs per point
    against the 33.9 T FMA/s fp64 rate of profiles/r03_mfma_f64_probe.txt.
Kernel times for the record come from a separate rocprofv3 --kernel-trace --stats run of this script.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F64_FMA_RATE = 33.9e12


def _best(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def _events(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3                    # us per call


def sweep(eng, dev):
    from symode_amd import data
    from symode_amd.batched import BatchedClosure
    from symode_amd.sweep import SeedSweepLBFGS
    X, DX = data.make_dataset("dosc", 50, 1000, dt=0.02, noise=0.0, seed=10, device=dev, n_problems=64)
    torch.manual_seed(0)
    inits = torch.randn(64, 20, device=dev)
    out = {"shape": "64 seeds x 50000 points x 2, order 3, 60 epochs"}
    masks = {}
    for mode in ("stream", "gram"):
        sw = SeedSweepLBFGS(BatchedClosure(X, DX, 3, engine=eng), 0.1, 0.05, 50, gram_closure=mode == "gram")
        dt, fit = _best(lambda: sw.fit(inits, 60))
        out[f"{mode}_ms"] = dt * 1e3
        out[f"{mode}_epochs_max"] = int(fit["epochs"].max())
        masks[mode] = fit["mask"].cpu()
    out["masks_equal"] = bool(torch.equal(masks["stream"], masks["gram"]))
    return out


def single(eng, dev, order):
    from oracle import sindy_oracle as O
    import numpy as np
    from symode_amd.device_lbfgs import DeviceTrainer
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(50, np.random.RandomState(0)), 0.02, 2500)
    x = torch.from_numpy(xs.reshape(1, -1, 2)).float().to(dev)
    dx = torch.from_numpy(dxs.reshape(1, -1, 2)).float().to(dev)
    p = eng.lib_size(2, order, 0)
    P0 = (torch.randn(1, 2 * p, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    out = {"shape": f"50x2500x2, order {order}, 100 epochs"}
    for mode in ("stream", "gram"):
        def fit():
            tr = DeviceTrainer(x, dx, order, 0, lr=0.1, threshold=0.05, st_freq=50, closure=mode, engine=eng, detail=False)
            return tr.fit(P0, 100)
        dt, res = _best(fit)
        out[f"{mode}_ms"] = dt * 1e3
        out[f"{mode}_epochs"] = int(res["epochs"].max())
        out[f"{mode}_mask"] = res["mask"].flatten().int().tolist()
    out["masks_equal"] = out["stream_mask"] == out["gram_mask"]
    return out


def quad_vs_n(eng, dev):
    out = {}
    for n in (125000, 1 << 20, 1 << 24):
        x = torch.rand(1, n, 2, device=dev) * 2 - 1
        dx = torch.rand(1, n, 2, device=dev) * 2 - 1
        G = eng.aug_gram(x, dx, 3)
        xi = torch.randn(1, 2, 10, device=dev)
        m = torch.ones(1, 2, 10, device=dev)
        out[str(n)] = _events(lambda: eng.quad_closure(G, None, xi, m, 1.0 / (2 * n)))
        del x, dx
    return out


def rev_gram_rate(eng, dev):
    out = {}
    n = 1 << 24
    x = torch.rand(1, n, 2, device=dev) * 2 - 1
    th = torch.tensor(0.01)
    rot = torch.tensor([[torch.cos(th), torch.sin(th)], [-torch.sin(th), torch.cos(th)]], device=dev)
    gx = (x @ rot.T)[:, None].contiguous()
    jgx = rot.expand(1, 1, n, 2, 2).contiguous()
    for order in (3, 5):
        dp = 2 * eng.lib_size(2, order, 0)
        us = _events(lambda: eng.symreg_reversed_gram(x, gx, jgx, order), reps=5)
        fma = dp * (dp + 1) / 2 * 2 * n
        out[f"order{order}"] = {"us": us, "fma_per_point": dp * (dp + 1) // 2 * 2, "T_fma_per_s": fma / us / 1e6,
                                "fraction_of_f64_rate": fma / (us * 1e-6) / F64_FMA_RATE}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="sweep,single,quad,rev")
    a = ap.parse_args()
    import symode_amd
    eng = symode_amd.get_engine()
    dev = "cuda:0"
    legs = a.only.split(",")
    res = {}
    if "sweep" in legs:
        res["seed_sweep"] = sweep(eng, dev)
    if "single" in legs:
        res["single_order3"] = single(eng, dev, 3)
        res["single_order5"] = single(eng, dev, 5)
    if "quad" in legs:
        res["quad_closure_us_vs_points"] = quad_vs_n(eng, dev)
    if "rev" in legs:
        res["symreg_reversed_gram_2p24"] = rev_gram_rate(eng, dev)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
