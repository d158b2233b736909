"""Device Adam trainer: a hyper-parameter grid in one epoch launch (symode_adam_run with a per-problem table) against one
scalar launch per grid point, and the scalar launches themselves against another build of the library.

    python tests/perf/adam_grid.py [--part a|b|all] [--tree OTHER_CHECKOUT] [--label NAME] [--out FILE]

Data: the damped oscillator by the reference's recipe size (250 trajectories x 500 samples = 125 000 rows, 20 % noise),
d = 2, order 3, batch 256 (489 steps per epoch) and 4096 (31 steps), 64 seeds.  Every figure is HIP-event time around the
launches of one window of 16 epochs, per epoch; 3 warm-up windows per path, then the median of 20 with the spread of those
20 (min, max, half the interquartile range).  Paths that are compared alternate window by window in one process.
  (a) the 64-seed scalar launch, symode_adam_epochs on a prebuilt table (4 launches of 4 epochs: the table of 16 would be
      512 MB) and symode_adam_epochs_keyed (the same cut).  ``--tree`` names another checkout WITH its built library (the
      parent commit's): the same script then measures that build, and the two files are laid side by side -- run the two
      alternately, twice each, and read the difference against the spread the repeats themselves show.
  (b) G = 1, 2, 4, 8 grid points x 64 common seeds: ONE keyed launch of G x 64 problems with the table (16 epochs) against G
      keyed scalar launches of 64 problems in sequence (16 epochs each), per epoch of the whole grid, and the ratio.  Keyed
      only: an index table of 512 problems' own orders would be 256 MB per epoch.  A build without symode_adam_run skips it.
No threshold: the file records what was measured."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORDER, LR, W_X, W_REG, THRESHOLD = 3, 1e-3, 1.0, 1e-3, 0.05
WARMUP, REPS, EPOCHS, LAUNCH_EPOCHS, SEEDS = 3, 20, 16, 4, 64
DEV = "cuda:0"


def spread(times):
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), min(times), max(times), (q[2] - q[0]) / 2


def fmt(times):
    med, lo, hi, hiqr = spread(times)
    return f"{med:.4f} ms per epoch (min {lo:.4f}, max {hi:.4f}, +-{hiqr:.4f})"


def alternate(*windows):
    """WARMUP + REPS windows of each path, a b a b ...; returns one list of REPS figures per path."""
    out = [[] for _ in windows]
    for k in range(WARMUP + REPS):
        for which, window in enumerate(windows):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def timed(launches):
    """HIP events around ``launches()``, which enqueues EPOCHS epochs: ms per epoch."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launches()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / EPOCHS


def state(coef, n_problems, seeds):
    p = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in seeds]).repeat(n_problems // len(seeds), 1).to(DEV)
    return (p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(n_problems, dtype=torch.int32, device=DEV),
            torch.ones(n_problems, 2, coef.p, device=DEV))


def scalar_launches(eng, coef, x, dx, batch, seeds):
    """(a): the table launch and the keyed launch of len(seeds) problems."""
    table = eng.adam_order_table(x.shape[0], batch, seeds, LAUNCH_EPOCHS, device=torch.device(DEV))
    seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    kw = dict(lr=LR, w_x=W_X, w_reg=W_REG, threshold=THRESHOLD, st_freq=100)

    def window(keyed):
        st = state(coef, len(seeds), seeds)

        def launches():
            for _ in range(EPOCHS // LAUNCH_EPOCHS):
                if keyed:
                    eng.adam_epochs_keyed(x, dx, seeds_dev, LAUNCH_EPOCHS, batch, *st, ORDER, 0, **kw)
                else:
                    eng.adam_epochs(x, dx, table, *st, ORDER, 0, **kw)
        return lambda: timed(launches)

    return alternate(window(False), window(True))


def grid_launches(eng, coef, x, dx, batch, seeds, G):
    """(b): one launch of G x len(seeds) problems with the table against G scalar launches in sequence."""
    n = len(seeds)
    points = [(LR * (1 + g), W_REG * (1 + g % 3), THRESHOLD * (1 + g % 2), 0.0) for g in range(G)]
    hyper = torch.tensor([pt for pt in points for _ in seeds], dtype=torch.float32, device=DEV)
    grid_seeds = torch.tensor(seeds * G, dtype=torch.int64, device=DEV)
    seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    whole, parts = state(coef, G * n, seeds), [state(coef, n, seeds) for _ in range(G)]

    def grid():
        eng.adam_epochs_keyed(x, dx, grid_seeds, EPOCHS, batch, *whole, ORDER, 0, lr=LR, w_x=W_X, st_freq=100, hyper=hyper)

    def sequence():
        for (lr, w_reg, threshold, _), st in zip(points, parts):
            eng.adam_epochs_keyed(x, dx, seeds_dev, EPOCHS, batch, *st, ORDER, 0, lr=lr, w_x=W_X, w_reg=w_reg, threshold=threshold,
                                  st_freq=100)

    return alternate(lambda: timed(grid), lambda: timed(sequence))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("a", "b", "all"))
    ap.add_argument("--tree", default=ROOT, help="the checkout (with its built library) whose symode_amd is measured")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from tests.perf.e2e_adam import dosc_rows                # the data recipe of this checkout, whichever build is measured
    sys.path.insert(0, os.path.abspath(a.tree))
    import symode_amd as S
    from symode_amd.coef_map import CoefMap
    eng = S.get_engine()
    assert os.path.abspath(S.__file__).startswith(os.path.abspath(a.tree)), (S.__file__, a.tree)
    coef = CoefMap(2, eng.lib_size(2, ORDER, 0))
    x, dx = (t.to(DEV).contiguous() for t in dosc_rows())
    seeds = list(range(SEEDS))
    lines = [f"[{a.label}] device: {torch.cuda.get_device_name(0)}; rows {x.shape[0]}, d = 2, order {ORDER}, {SEEDS} seeds; HIP events, "
             f"windows of {EPOCHS} epochs, {WARMUP} warm-up windows, median of {REPS} (min, max, +- half the interquartile range)"]
    print(lines[0], flush=True)
    for batch in (256, 4096):
        steps = (x.shape[0] + batch - 1) // batch
        head = f"[{a.label}] batch {batch} ({steps} steps per epoch)"
        if a.part in ("a", "all"):
            table, keyed = scalar_launches(eng, coef, x, dx, batch, seeds)
            lines += [f"{head}: (a) {SEEDS}-seed scalar launch, table: {fmt(table)}",
                      f"{head}: (a) {SEEDS}-seed scalar launch, keyed: {fmt(keyed)}"]
            print("\n".join(lines[-2:]), flush=True)
        if a.part in ("b", "all") and hasattr(eng.lib, "symode_adam_run"):
            for G in (1, 2, 4, 8):
                grid, sequence = grid_launches(eng, coef, x, dx, batch, seeds, G)
                lines += [f"{head}: (b) G {G} x {SEEDS} seeds, one grid launch:      {fmt(grid)}",
                          f"{head}: (b) G {G} x {SEEDS} seeds, {G} scalar launch(es): {fmt(sequence)}   "
                          f"sequence / grid {spread(sequence)[0] / spread(grid)[0]:.2f}"]
                print("\n".join(lines[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
