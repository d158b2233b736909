"""STLSQ seed sweep: the threshold loop on the host (SeedSweepSTLSQ.solve) against the one device launch
(solve(device=True)), and a hyper-parameter grid of G x 64 problems on the 64 seeds' shared Gram matrices against G host solves
in sequence.

    python tests/perf/stlsq_grid.py [--out FILE]

Data: BASELINE config[3]'s shape -- selkov, 10 trajectories x 10 000 samples x 2 at dt 0.002, noise 0.2, 64 seeds x 50 % subsample (50 000
points each), order 3 (p = 10).  Every figure is the median of 20 runs after 3 warm-up runs, with min, max and half the
interquartile range; paths that are compared alternate run by run in one process.  Two clocks per run: wall time around the
call (the caller's view: both routes end with the results on the host) and HIP-event time between the same two points of the
stream.
  (1) the gather-Gram launch alone (no copy).
  (2) one solve of the 64 seeds, matrices already on the device: the host route of this build (copy of the matrices to the host
      + symode_host_stlsq_sweep, gels), the parent commit's host route restated here call for call (so the unchanged path is
      shown unchanged), the device route (one launch, one copy back), and the launch alone with its results left on the device.
  (3) G = 1, 2, 4, 8 points x 64 seeds: one device solve with a table against G host solves in sequence, each with its own
      copy of the matrices (what G runs of the sweep do today, their G Gram passes not counted).
No threshold: the file records what was measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS, SEEDS = 3, 20, 64
W_REG, THRESHOLD, MAX_ITER = 0.0, 0.075, 10          # selkov/noise20_eq_sindy.cfg
DEV = "cuda:0"


def spread(times):
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), min(times), max(times), (q[2] - q[0]) / 2


def fmt(pairs):
    wall, event = spread([p[0] for p in pairs]), spread([p[1] for p in pairs])
    return (f"wall {wall[0]:.3f} ms (min {wall[1]:.3f}, max {wall[2]:.3f}, +-{wall[3]:.3f}) | "
            f"events {event[0]:.3f} ms (min {event[1]:.3f}, max {event[2]:.3f}, +-{event[3]:.3f})")


def timed(call):
    """``call`` between two events and two readings of the wall clock: (wall ms, event ms)."""
    def window():
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        b.synchronize()
        return 1e3 * (time.perf_counter() - t0), a.elapsed_time(b)
    return window


def alternate(*windows):
    out = [[] for _ in windows]
    for k in range(WARMUP + REPS):
        for which, window in enumerate(windows):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import data, lstsq
    from symode_amd.sindy import NEAR_THRESHOLD_BAND
    from symode_amd.sweep import SeedSweepSTLSQ
    X, DX = data.make_dataset("selkov", 10, 10000, dt=0.002, noise=0.2, seed=0, device=DEV)
    x, dx = X[0].reshape(-1, 2).contiguous(), DX[0].reshape(-1, 2).contiguous()
    sw = SeedSweepSTLSQ(x, dx, 3, n_seeds=SEEDS, subsample=0.5, seed0=0)
    eng, lib = sw.engine, lstsq._native()
    S, d, p = sw.S, sw.d, sw.p
    lines = [f"device: {torch.cuda.get_device_name(0)}; selkov 10 x 10000 x 2, noise 0.2, {SEEDS} seeds x {sw.m_local} points, order 3 (p = {p}); "
             f"w_sindy_reg {W_REG}, threshold {THRESHOLD}, max_iter {MAX_ITER}; {WARMUP} warm-up runs, median of {REPS} (min, max, +- half the "
             f"interquartile range)"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    # (1) the Gram pass alone
    got, = alternate(timed(lambda: eng.aug_gram_gather(sw.x, sw.dx, sw.idx, sw.order, sw.flags)))
    say(f"(1) gather-Gram launch, {SEEDS} x {sw.m_local} points:                 {fmt(got)}")
    sw.grams(device=True)

    # (2) one solve of the 64 seeds
    def host(w=W_REG, thr=THRESHOLD):
        sw._gram = None                                      # the copy of the matrices belongs to the host route
        return sw.solve(w, thr, max_iter=MAX_ITER, lstsq_driver="gels")

    def parent(w=W_REG, thr=THRESHOLD):
        """The parent commit's grams() + solve() on the native route, call for call."""
        G = sw._gram_dev
        n = torch.tensor([float(sw.m_local)], dtype=torch.float64, device=G.device)
        Gh, n_points = G.cpu().numpy(), int(n.item())
        Xi = np.zeros((S, d, p), dtype=np.float32)
        Gc = np.ascontiguousarray(Gh, dtype=np.float64)
        m8 = np.ones((S, d, p), dtype=np.uint8)
        p32, near, fell = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        rc = lib.symode_host_stlsq_sweep(Gc.ctypes.data, S, d, p, n_points, float(w), float(thr), MAX_ITER, 1, float(NEAR_THRESHOLD_BAND),
                                         Xi.ctypes.data, m8.ctypes.data, p32.ctypes.data, near.ctypes.data, fell.ctypes.data)
        assert rc == 0, rc
        return torch.from_numpy(Xi), torch.from_numpy(m8.astype(bool).astype(np.float32)), p32.astype(np.int64)

    def device(w=W_REG, thr=THRESHOLD, hyper=None):
        return sw.solve(w, thr, max_iter=MAX_ITER, device=True, hyper=hyper)

    ref, par, dev = host(), parent(), device()
    near = len(sw.near_threshold)                            # (a seed that meets one is replayed in numpy by both routes)
    same = bool(torch.equal(ref[1], dev[1]) and np.array_equal(ref[2], dev[2]) and torch.equal(ref[0], par[0]) and torch.equal(ref[1], par[1]))
    say(f"    passes per seed {int(ref[2].min())}-{int(ref[2].max())} ({int(ref[2].sum())} in all), near-threshold records {near}; device masks and passes equal the host's, "
        f"this build's host route equals the parent's bit for bit: {same}; "
        f"max |Xi_dev - Xi_host| {float((ref[0] - dev[0]).abs().max()):.3g}")
    Gd = sw.grams(device=True)
    launch = lambda: eng.stlsq_sweep(Gd, sw.n_points, W_REG, THRESHOLD, MAX_ITER, d=d)      # noqa: E731
    got = alternate(timed(host), timed(parent), timed(device), timed(launch))
    say(f"(2) solve, host route (this build):                             {fmt(got[0])}",
        f"(2) solve, host route (the parent commit's calls):              {fmt(got[1])}",
        f"(2) solve, device route:                                        {fmt(got[2])}   host / device (wall) "
        f"{spread([t[0] for t in got[0]])[0] / spread([t[0] for t in got[2]])[0]:.2f}",
        f"(2) symode_stlsq_sweep alone, results left on the device:       {fmt(got[3])}")

    # (3) a grid of G points on the 64 seeds
    for G in (1, 2, 4, 8):
        points = [(0.05 * (g % 3), THRESHOLD * (1 + 0.5 * g)) for g in range(G)]
        hyper = {"w_reg": [w for w, _ in points for _ in range(S)], "threshold": [t for _, t in points for _ in range(S)]}
        whole = device(hyper=hyper)
        parts = [host(w, t) for w, t in points]
        same = all(np.array_equal(whole[2][g * S:(g + 1) * S], parts[g][2]) and torch.equal(whole[1][g * S:(g + 1) * S], parts[g][1])
                   for g in range(G))
        g_t, s_t = alternate(timed(lambda: device(hyper=hyper)), timed(lambda: [host(w, t) for w, t in points]))
        say(f"(3) G {G} x {SEEDS} seeds, one device solve of {G * S} problems:       {fmt(g_t)}   masks and passes equal the host's: {same}",
            f"(3) G {G} x {SEEDS} seeds, {G} host solve(s) in sequence:              {fmt(s_t)}   sequence / grid (wall) "
            f"{spread([t[0] for t in s_t])[0] / spread([t[0] for t in g_t])[0]:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
