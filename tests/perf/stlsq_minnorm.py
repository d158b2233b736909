"""EquivSINDy-c seed sweep: the constrained device STLSQ fit in its rank-revealing mode (SeedSweepSTLSQ.solve(device=True,
coef=..., min_norm=True), symode_stlsq_sweep_minnorm) against the same build without it -- the flag-and-host route of the
parent commit -- and against the L-BFGS sweep.

    python tests/perf/stlsq_minnorm.py [--out FILE] [--parent_lib PATH/libsymode_hip.so]

Data: the shape of tests/perf/stlsq_constrained.py (dosc/noise20_esindy.cfg) -- dosc, 50 trajectories x 100 samples x 2 at dt 0.2,
noise 0.2, so(2) constraint, 64 seeds x 50 % subsample (2 500 points each), threshold 0.01, w_sindy_reg 0 -- at orders 2 and 5.
Every figure is wall time around the call with the results on the host at the end, the median of 20 runs after 3 warm-up
runs, with min, max and half the interquartile range; the paths that are compared alternate run by run in one process.
  (a) gather-Gram launch + solve with min_norm=True; the same without it (the parent's route: flagged seeds replayed by the
      numpy host loop); SeedSweepLBFGS with the Gram closure (100 epochs x 20 iterations at most, lr 1, st_freq 100); and the
      new launch alone with its results left on the device.  How many of the 64 masks of the new route equal the old
      route's and L-BFGS's.
  (b) symode_stlsq_sweep_constrained (the unchanged path) through this build's library and, with --parent_lib, the parent
      commit's, run by run in turn: equal bytes, and the two times.
No threshold: the file records what was measured."""
import argparse
import ctypes
import os
import statistics
import sys
import time
import warnings

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
    ap.add_argument("--parent_lib", default=None, help="the parent commit's libsymode_hip.so, for (b)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    warnings.simplefilter("ignore", RuntimeWarning)         # the minimum-norm warning of both routes, once per solve
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
        res, argtypes = E._SIGNATURES["symode_stlsq_sweep_constrained"]
        parent.symode_stlsq_sweep_constrained.restype, parent.symode_stlsq_sweep_constrained.argtypes = res, argtypes
        assert not hasattr(parent, "symode_stlsq_sweep_minnorm")

    so2 = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
    for order in (2, 5):
        template = SINDyRegression(2, order, False, False, L_list=[so2], threshold=THRESHOLD, device=DEV, constrain_constant=False)
        coef = template.coef
        sw = SeedSweepSTLSQ(x, dx, order, n_seeds=SEEDS, subsample=0.5, seed0=0)
        eng, S, d, p = sw.engine, sw.S, sw.d, sw.p
        Gd = sw.grams(device=True)
        R = coef.r + d
        say(f"== order {order}: p = {p}, r = {coef.r}, r' = {R}, {sw.m_local} points per seed")

        def solve(min_norm):
            sw._gram_dev = None                                # the gather-Gram launch is part of the figure
            return sw.solve(W_REG, THRESHOLD, max_iter=MAX_ITER, device=True, coef=coef, **(dict(min_norm=True) if min_norm else {}))

        rows = sw.idx.long()
        clos = BatchedClosure(x[rows].contiguous(), dx[rows].contiguous(), order, False, False, coef=coef)
        P0 = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in range(S)]).to(DEV)

        def lbfgs():
            sweep = SeedSweepLBFGS(clos, LR, THRESHOLD, ST_FREQ, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=W_REG, gram_closure=True)
            out = sweep.fit(P0, EPOCHS)
            return out["Xi"].cpu(), out["mask"].cpu(), out["epochs"].cpu()

        q_solve, q_xi = (torch.from_numpy(q).to(DEV) for q in (coef.solve_matrix(), coef.xi_matrix()))
        thr32 = float(np.float32(THRESHOLD))

        def launch(to_host=False):
            return eng.stlsq_sweep_minnorm(Gd, sw.n_points, W_REG, thr32, MAX_ITER, q_solve, q_xi, coef.allow_constant, d=d,
                                           rcond=lstsq.SINGULAR_RCOND, to_host=to_host)

        def launch_old(to_host=False):
            return eng.stlsq_sweep_constrained(Gd, sw.n_points, W_REG, thr32, MAX_ITER, q_solve, q_xi, coef.allow_constant, d=d,
                                               pivot_floor=lstsq.SINGULAR_RCOND ** 2, to_host=to_host)

        alone, alone_old = launch(to_host=True), launch_old(to_host=True)
        say(f"    the new launch: {int((alone[6] != 0).sum())} of {S} problems with rank-truncated passes (ranks of the last solve "
            f"{int(alone[7].min())}-{int(alone[7].max())}), {int((alone[4] != 0).sum())} flagged, {int((alone[3] != 0).sum())} with a "
            f"near-threshold coefficient (replayed on the host for the record); passes {int(alone[2].min())}-{int(alone[2].max())}",
            f"    the existing launch: {int((alone_old[4] != 0).sum())} of {S} problems flagged (solved by the host loop)")
        new, old, ref = solve(True), solve(False), lbfgs()
        same_old = int((new[1].bool() == old[1].bool()).all(dim=(1, 2)).sum())
        same_ref = int((new[1].bool() == ref[1].bool()).all(dim=(1, 2)).sum())
        say(f"    masks of the new route equal to the old route's: {same_old}/{S}; to L-BFGS's: {same_ref}/{S} (old route to L-BFGS's: "
            f"{int((old[1].bool() == ref[1].bool()).all(dim=(1, 2)).sum())}/{S}); max |Xi_new - Xi_old| on the common support "
            f"{float(((new[0] - old[0]) * new[1] * old[1]).abs().max()):.3g}")
        got = alternate(timed(lambda: solve(True)), timed(lambda: solve(False)), timed(lbfgs), timed(launch), timed(launch_old))
        med = [spread(t)[0] for t in got]
        say(f"(a) symode_stlsq_sweep_minnorm alone, results on the device:      {fmt(got[3])}",
            f"(a) symode_stlsq_sweep_constrained alone, results on the device:  {fmt(got[4])}",
            f"(a) gather-Gram launch + solve(min_norm=True):                    {fmt(got[0])}",
            f"(a) gather-Gram launch + solve() (the parent's route):            {fmt(got[1])}   old / new {med[1] / med[0]:.2f}",
            f"(a) SeedSweepLBFGS, Gram closure:                                 {fmt(got[2])}   L-BFGS / new {med[2] / med[0]:.2f}")
        # (b) the unchanged entry through both libraries
        outs = [torch.empty(S * d * p, dtype=torch.float32, device=DEV), torch.empty(S * R, dtype=torch.float32, device=DEV),
                torch.empty(S * d * p, dtype=torch.uint8, device=DEV)] + [torch.empty(S, dtype=torch.int32, device=DEV) for _ in range(3)]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def raw(lib):
            def call():
                rc = lib.symode_stlsq_sweep_constrained(ctypes.c_void_p(Gd.data_ptr()), S, S, d, p, int(sw.n_points),
                                                        ctypes.c_void_p(q_solve.data_ptr()), ctypes.c_void_p(q_xi.data_ptr()), coef.r, 1, None,
                                                        W_REG, thr32, MAX_ITER, 1e-4, lstsq.SINGULAR_RCOND ** 2,
                                                        *[ctypes.c_void_p(t.data_ptr()) for t in outs], stream)
                assert rc == 0, rc
                return [t.cpu() for t in outs]
            return call

        def defined(o):
            """The outputs a flagged problem leaves unspecified (xi, var) are compared on the others."""
            keep = o[5].numpy() == 0
            return [o[0].numpy().reshape(S, -1)[keep].tobytes(), o[1].numpy().reshape(S, -1)[keep].tobytes()] + [t.numpy().tobytes() for t in o[2:]]

        if parent is None:
            got = alternate(timed(raw(eng.lib)))
            say(f"(b) symode_stlsq_sweep_constrained, this build:                   {fmt(got[0])}")
        else:
            same = defined(raw(eng.lib)()) == defined(raw(parent)())
            got = alternate(timed(raw(eng.lib)), timed(raw(parent)))
            say(f"(b) symode_stlsq_sweep_constrained, this build:                   {fmt(got[0])}",
                f"(b) symode_stlsq_sweep_constrained, the parent's library:         {fmt(got[1])}   equal bytes: {same}; this / parent "
                f"{spread(got[0])[0] / spread(got[1])[0]:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
