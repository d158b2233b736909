"""Weak-SINDy seed sweep: 50 in-process per-seed fits (WSINDyWrapper + train_WSINDy on each window: main_wsindy's route,
whose code this build leaves untouched) against one SeedSweepWSINDy normals + solve, and a grid of G points on the windows'
shared matrices against G scalar sweeps.

    python tests/perf/wsindy_sweep.py [--out FILE]

Data: the shape of dosc/noise20_wsindy.cfg -- dosc at noise 0.2 as dataset.py generates it (50 trajectories x 100 samples at dt 0.2, no GP
smoothing), 50 seeds, each a window of 80 % of one trajectory, K = 50 test functions, order 3 (p = 10), w_sindy_reg 0, threshold 0.05, at most 10 passes.  Every
figure is the median of 20 runs after 3 warm-up runs, with min, max and half the interquartile range; paths that are compared
alternate run by run in one process.  Two clocks per run: wall time around the call (both routes end with the results on the
host) and HIP-event time between the same two points of the stream.
  (a) the 50 per-seed fits in sequence, regressor and wrapper built once per seed outside the window (a per-seed PROCESS
      pays for them, the interpreter, the import and the data set as well; none of that is counted here).
  (b) one sweep: normals (symode_weak_normal_windows: two launches) + solve (symode_stlsq_sweep + one copy back), then the
      three launches on their own: window contraction + normal matrices with and without z_out, and the threshold loop with
      its results left on the device.
  (c) G = 1, 2, 4, 8 points x 50 seeds: one solve with a table against G scalar solves in sequence, on the same matrices.
No threshold: the file records what was measured."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.perf.stlsq_grid import REPS, WARMUP, alternate, fmt, spread, timed  # noqa: E402

SEEDS, K, ORDER = 50, 50, 3
W_REG, THRESHOLD, MAX_ITER = 0.0, 0.05, 10               # dosc/noise20_wsindy.cfg
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    a = ap.parse_args()
    import symode_amd  # noqa: F401
    from symode_amd import data, sindy
    from symode_amd import train as T
    from symode_amd.dataset import _RECIPES, ode_dt_dict
    from symode_amd.sweep import SeedSweepWSINDy
    n_ics, _, steps, sub, step = _RECIPES["dosc"]
    dt = ode_dt_dict["dosc"]
    x, _ = data.gen_data("dosc", n_ics, dt=step, num_steps=steps, subsample_rate=sub, noise=0.2, seed=0, device=DEV)   # (no GP smoothing)
    x3 = x.to(torch.float32).to(DEV).contiguous()
    n_ics, n_steps = x3.shape[:2]
    sw = SeedSweepWSINDy(x3, ORDER, dt=dt, seeds=range(SEEDS), num_test_funcs=K)
    eng, n_t = sw.engine, sw.n_t
    lines = [f"device: {torch.cuda.get_device_name(0)}; dosc {n_ics} x {n_steps} x 2, noise 0.2, {SEEDS} seeds x {n_t} time points of one "
             f"trajectory each, K = {K}, order {ORDER} (p = {sw.p}); w_sindy_reg {W_REG}, threshold {THRESHOLD}, max_iter {MAX_ITER}; "
             f"{WARMUP} warm-up runs, median of {REPS} (min, max, +- half the interquartile range)"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    # (a) the per-seed route
    windows = [x3[tr, st:st + n_t].contiguous() for tr, st in sw.windows.tolist()]
    fits = []
    for xw in windows:
        reg = sindy.SINDyRegression(2, ORDER, False, False, threshold=THRESHOLD, device=DEV, lstsq_driver="gels")
        fits.append((reg, sindy.WSINDyWrapper(reg, torch.arange(n_t) * dt, n_t * dt, num_test_funcs=K, device=DEV), xw))

    def per_seed(w=W_REG, thr=THRESHOLD):
        devnull = open(os.devnull, "w")
        out, sys.stdout = sys.stdout, devnull                          # train_WSINDy prints its convergence line per seed
        try:
            for reg, wrapper, xw in fits:
                with torch.no_grad():
                    reg.mask.fill_(1.0)                                 # every run starts from the full support
                T.train_WSINDy(wrapper=wrapper, train_x=xw, num_epochs=MAX_ITER, device=DEV, log_interval=10 ** 9,
                               save_interval=10 ** 9, save_dir="t", w_sindy_reg=w, threshold=thr, lstsq_driver="gels")
        finally:
            sys.stdout = out
            devnull.close()
        return (torch.stack([f[0].Xi.detach() for f in fits]).cpu(), torch.stack([f[0].mask.detach() for f in fits]).cpu())

    def sweep(w=W_REG, thr=THRESHOLD, hyper=None, fresh=True):
        if fresh:
            sw._normal_dev = sw._normal = None                          # the data pass belongs to the sweep
        return sw.solve(w, thr, max_iter=MAX_ITER, hyper=hyper)

    ref, got = per_seed(), sweep()
    same = bool(torch.equal(ref[1] > 0, got[1] > 0))
    err = float(((ref[0] - got[0]).abs() / ref[0].abs().amax(dim=-1, keepdim=True)).max())
    say(f"    passes per seed {int(got[2].min())}-{int(got[2].max())} ({int(got[2].sum())} in all), near-threshold records "
        f"{len(sw.near_threshold)}; the sweep's masks equal the per-seed route's: {same}; max |dXi| / largest of the row {err:.3g}")
    M = torch.from_numpy(np.ascontiguousarray(sw._VVt)).to(DEV)
    Nd = sw.normals(device=True)
    normals = lambda z: (lambda: eng.weak_normal_windows(sw.x, sw.windows, n_t, sw.V, sw.V_drv, M, ORDER, 0, want_z=z))   # noqa: E731
    launch = lambda: eng.stlsq_sweep(Nd, n_t, 0.0, THRESHOLD, MAX_ITER, d=2)                                            # noqa: E731
    t = alternate(timed(per_seed), timed(sweep), timed(normals(False)), timed(normals(True)), timed(launch))
    say(f"(a) {SEEDS} per-seed fits in sequence (WSINDyWrapper + train_WSINDy):     {fmt(t[0])}",
        f"(b) one sweep, normals + solve, results on the host:               {fmt(t[1])}   per-seed / sweep (wall) "
        f"{spread([v[0] for v in t[0]])[0] / spread([v[0] for v in t[1]])[0]:.1f}",
        f"(b) symode_weak_normal_windows alone (contraction + normal matrices): {fmt(t[2])}",
        f"(b) the same with z_out:                                            {fmt(t[3])}",
        f"(b) symode_stlsq_sweep alone, results left on the device:           {fmt(t[4])}")

    # (c) a grid of G points on the 50 windows' matrices
    S = SEEDS
    for G in (1, 2, 4, 8):
        points = [(1e-4 * (g % 3), THRESHOLD * (1 + 0.5 * g)) for g in range(G)]
        hyper = {"w_reg": [w for w, _ in points for _ in range(S)], "threshold": [thr for _, thr in points for _ in range(S)]}
        whole = sweep(hyper=hyper, fresh=False)
        parts = [sweep(w, thr, fresh=False) for w, thr in points]
        same = all(torch.equal(whole[0][g * S:(g + 1) * S], parts[g][0]) and np.array_equal(whole[2][g * S:(g + 1) * S], parts[g][2])
                   for g in range(G))
        g_t, s_t = alternate(timed(lambda: sweep(hyper=hyper, fresh=False)),
                             timed(lambda: [sweep(w, thr, fresh=False) for w, thr in points]))
        say(f"(c) G {G} x {S} seeds, one solve of {G * S} problems:                    {fmt(g_t)}   bit for bit the scalar solves: {same}",
            f"(c) G {G} x {S} seeds, {G} scalar solve(s) in sequence:                  {fmt(s_t)}   sequence / grid (wall) "
            f"{spread([v[0] for v in s_t])[0] / spread([v[0] for v in g_t])[0]:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
