"""EquivSINDy-c seed sweep: the device STLSQ fit under the equivariance constraint (SeedSweepSTLSQ.solve(device=True, coef=...),
symode_stlsq_sweep_constrained) against the route the parent commit has for these configs, and its grid.

    python tests/perf/stlsq_constrained.py [--out FILE] [--parent_lib PATH/libsymode_hip.so]

Data: the shape of dosc/noise20_esindy.cfg -- dosc, 50 trajectories x 100 samples x 2 at dt 0.2, noise 0.2, so(2) constraint,
64 seeds x 50 % subsample (2 500 points each), threshold 0.01, w_sindy_reg 0 -- at order 2 (p = 6, r' = 4) and at order 5 as
the bench uses it (p = 21).  Every figure is wall time around the call with the results on the host at the end, the median
of 20 runs after 3 warm-up runs, with min, max and half the interquartile range; paths that are compared alternate run by
run in one process.
  (a) one constrained device solve of the 64 seeds (matrices on the device; and with the gather-Gram launch in front of it)
      and the launch alone with its results left on the device (what is between the two is the host's: one copy, and the
      numpy replay of every seed that met a near-threshold coefficient or was flagged as possibly rank deficient)
      against the same seeds' EquivSINDy-c fit through SeedSweepLBFGS with the Gram closure on the same library build (100
      epochs x 20 L-BFGS iterations at most, lr 1, st_freq 100): the only route the parent commit has for these configs.
  (b) G = 1, 2, 4, 8 points x 64 seeds in one solve against G scalar solves in sequence.
  (c) the unconstrained symode_stlsq_sweep on the same matrices, this build; with --parent_lib also the parent commit's
      library, loaded beside it, run by run in turn (the kernel's code is untouched: stlsq.hpp has no line changed).
No threshold: the file records what was measured."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS, SEEDS = 3, 20, 64
W_REG, THRESHOLD, MAX_ITER = 0.0, 0.01, 100          # dosc/noise20_esindy.cfg (num_epochs 100 is the pass limit)
LR, ST_FREQ, EPOCHS = 1.0, 100, 100
DEV = "cuda:0"


def spread(times):
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), min(times), max(times), (q[2] - q[0]) / 2


def fmt(times):
    w = spread(times)
    return f"wall {w[0]:.3f} ms (min {w[1]:.3f}, max {w[2]:.3f}, +-{w[3]:.3f})"


def timed(call):
    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    return window


def alternate(*windows, reps=REPS):
    out = [[] for _ in windows]
    for k in range(WARMUP + reps):
        for which, window in enumerate(windows):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    ap.add_argument("--parent_lib", default=None, help="the parent commit's libsymode_hip.so, for (c)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import data, engine as E, lstsq
    from symode_amd.batched import BatchedClosure
    from symode_amd.sindy import SINDyRegression
    from symode_amd.sweep import SeedSweepLBFGS, SeedSweepSTLSQ
    X, DX = data.make_dataset("dosc", 50, 100, dt=0.2, noise=0.2, seed=0, device=DEV)
    x, dx = X[0].reshape(-1, 2).contiguous(), DX[0].reshape(-1, 2).contiguous()
    lines = [f"device: {torch.cuda.get_device_name(0)}; dosc 50 x 100 x 2, noise 0.2, so(2) constraint, {SEEDS} seeds x 50 % subsample; "
             f"w_sindy_reg {W_REG}, threshold {THRESHOLD}, max_iter {MAX_ITER}; {WARMUP} warm-up runs, median of {REPS} (min, max, +- half "
             f"the interquartile range), wall time"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        res, argtypes = E._SIGNATURES["symode_stlsq_sweep"]
        parent.symode_stlsq_sweep.restype, parent.symode_stlsq_sweep.argtypes = res, argtypes
        assert not hasattr(parent, "symode_stlsq_sweep_constrained")

    so2 = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
    for order in (2, 5):
        template = SINDyRegression(2, order, False, False, L_list=[so2], threshold=THRESHOLD, device=DEV, constrain_constant=False)
        coef = template.coef
        sw = SeedSweepSTLSQ(x, dx, order, n_seeds=SEEDS, subsample=0.5, seed0=0)
        eng, S, d, p = sw.engine, sw.S, sw.d, sw.p
        Gd = sw.grams(device=True)
        say(f"== order {order}: p = {p}, r = {coef.r}, r' = {coef.r + d}, {sw.m_local} points per seed")

        def device(thr=THRESHOLD, hyper=None):
            return sw.solve(W_REG, thr, max_iter=MAX_ITER, device=True, hyper=hyper, coef=coef)

        def gather_and_device():
            sw._gram_dev = None
            return device()

        rows = sw.idx.long()
        clos = BatchedClosure(x[rows].contiguous(), dx[rows].contiguous(), order, False, False, coef=coef)
        P0 = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in range(S)]).to(DEV)

        def lbfgs():
            sweep = SeedSweepLBFGS(clos, LR, THRESHOLD, ST_FREQ, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=W_REG, gram_closure=True)
            out = sweep.fit(P0, EPOCHS)
            return out["Xi"].cpu(), out["mask"].cpu(), out["epochs"].cpu()

        q_solve, q_xi = (torch.from_numpy(q).to(DEV) for q in (coef.solve_matrix(), coef.xi_matrix()))

        def launch(to_host=False):
            return eng.stlsq_sweep_constrained(Gd, sw.n_points, W_REG, float(np.float32(THRESHOLD)), MAX_ITER, q_solve, q_xi,
                                               coef.allow_constant, d=d, pivot_floor=lstsq.SINGULAR_RCOND ** 2, to_host=to_host)

        alone = launch(to_host=True)
        dev, ref = device(), lbfgs()
        say(f"    the launch: {int((alone[4] != 0).sum())} of {S} problems flagged (solved by the host loop, minimum-norm rule), "
            f"{int(((alone[3] != 0) & (alone[4] == 0)).sum())} more with a near-threshold coefficient (replayed on the host for the record)")
        agree = int((dev[1].bool() == ref[1].bool()).all(dim=(1, 2)).sum())
        say(f"    device: passes per seed {int(dev[2].min())}-{int(dev[2].max())}, near-threshold records {len(sw.near_threshold)}; L-BFGS: "
            f"epochs {int(ref[2].min())}-{int(ref[2].max())}; seeds whose two masks agree {agree}/{S}; "
            f"max |Xi_stlsq - Xi_lbfgs| on the common support {float(((dev[0] - ref[0]) * dev[1] * ref[1]).abs().max()):.3g}")
        got = alternate(timed(device), timed(gather_and_device), timed(lbfgs), timed(launch))
        med = [spread(t)[0] for t in got]
        say(f"(a) symode_stlsq_sweep_constrained alone, results on the device: {fmt(got[3])}",
            f"(a) constrained device solve, matrices on the device:          {fmt(got[0])}",
            f"(a) gather-Gram launch + constrained device solve:             {fmt(got[1])}",
            f"(a) SeedSweepLBFGS, Gram closure (the parent's route):         {fmt(got[2])}   L-BFGS / (gather + solve) {med[2] / med[1]:.1f}")
        # (b) a grid of G points on the 64 seeds
        for G in (1, 2, 4, 8):
            thr = [THRESHOLD * (1 + g) for g in range(G)]
            hyper = {"threshold": [t for t in thr for _ in range(S)]}
            whole = device(hyper=hyper)
            parts = [device(t) for t in thr]
            same = all(whole[0][g * S:(g + 1) * S].numpy().tobytes() == parts[g][0].numpy().tobytes() for g in range(G))
            g_t, s_t = alternate(timed(lambda: device(hyper=hyper)), timed(lambda: [device(t) for t in thr]))
            say(f"(b) G {G} x {SEEDS} seeds, one solve of {G * S} problems:              {fmt(g_t)}   bit for bit the scalar solves: {same}",
                f"(b) G {G} x {SEEDS} seeds, {G} scalar solve(s) in sequence:             {fmt(s_t)}   sequence / grid "
                f"{spread(s_t)[0] / spread(g_t)[0]:.2f}")
        # (c) the unconstrained entry on the same matrices
        outs = [torch.empty(S * d * p, dtype=torch.float32, device=DEV), torch.empty(S * d * p, dtype=torch.uint8, device=DEV)] + \
               [torch.empty(S, dtype=torch.int32, device=DEV) for _ in range(3)]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def raw(lib):
            def call():
                rc = lib.symode_stlsq_sweep(ctypes.c_void_p(Gd.data_ptr()), S, S, d, p, int(sw.n_points), None, W_REG, THRESHOLD, MAX_ITER,
                                            1e-4, *[ctypes.c_void_p(t.data_ptr()) for t in outs], stream)
                assert rc == 0, rc
                return [t.cpu() for t in outs]
            return call

        if parent is None:
            got = alternate(timed(raw(eng.lib)))
            say(f"(c) symode_stlsq_sweep (unconstrained), this build:            {fmt(got[0])}")
        else:
            mine, theirs = raw(eng.lib)(), raw(parent)()
            same = all(u.numpy().tobytes() == v.numpy().tobytes() for u, v in zip(mine, theirs))
            got = alternate(timed(raw(eng.lib)), timed(raw(parent)))
            say(f"(c) symode_stlsq_sweep (unconstrained), this build:            {fmt(got[0])}",
                f"(c) symode_stlsq_sweep (unconstrained), the parent's library:  {fmt(got[1])}   equal bytes: {same}; this / parent "
                f"{spread(got[0])[0] / spread(got[1])[0]:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
