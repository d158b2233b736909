"""Device Adam trainer: the epoch order drawn with tensor ops between the launches against the order computed inside them.

    python tests/perf/adam_shuffle.py [--out profiles/adam_device_shuffle.txt]

Data: the damped oscillator by the reference's recipe size (250 trajectories x 500 samples = 125 000 rows, 20 % noise),
d = 2, order 3, batch 256 (489 steps per epoch) and 4096 (31 steps), S = 64 seeds (main_sweep --sindy_optimizer adam) and
S = 1 (main --device_adam), in one process on one build, the two paths alternating window by window:
  (a) DeviceAdam.fit(orders=...) with the order generation main_sweep._fit_adam runs per epoch (one torch.rand per seed into
      a key matrix, one stable argsort of it; S = 1: the loader's randperm) -- wall time per epoch, tables, cuts by
      TABLE_BYTES and read-back of the log included;
  (b) DeviceAdam.fit(order_seeds=...) -- the same wall time with nothing between the launches;
  (c) the epoch launch ALONE, HIP events around symode_adam_epochs on a prebuilt table and around symode_adam_epochs_keyed,
      per minibatch step: what the index arithmetic in the prefetch slot costs the step.
A window is 16 epochs and ends in a synchronise ((c): 4 epochs per launch, the table of 16 would be 512 MB); 2 warm-up
windows per path, then the median of 20 with the spread of those 20 (min, max, half the interquartile range).  The file
also records the uniformity statistic of tests/test_host_adam_order.py for 1-4 Feistel rounds.  No threshold: the file
records what was measured; everything from the line `== kept as written` on (the reading of the figures, the comparison
with the parent's library, the kernels' resources) is kept as it stands when the file is rewritten."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.perf.e2e_adam import DEV, dosc_rows  # noqa: E402

ORDER, LR, W_X, W_REG = 3, 1e-3, 1.0, 1e-3
WARMUP, REPS, EPOCHS, LAUNCH_EPOCHS = 2, 20, 16, 4
KEEP = "== kept as written (tests/perf/adam_shuffle.py rewrites the lines above only)"


def spread(times):
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), min(times), max(times), (q[2] - q[0]) / 2


def fmt(times, unit):
    med, lo, hi, hiqr = spread(times)
    return f"{med:.3f} {unit} (min {lo:.3f}, max {hi:.3f}, +-{hiqr:.3f})"


def alternate(first, second):
    """WARMUP + REPS windows of each, a b a b ...; returns the two lists of REPS figures."""
    out = ([], [])
    for k in range(WARMUP + REPS):
        for which, window in enumerate((first, second)):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def trainer(S, x, dx, batch):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    coef = CoefMap(2, S.get_engine().lib_size(2, ORDER, 0))
    return DeviceAdam(x, dx, ORDER, False, False, coef, LR, W_X, W_REG, 0.05, 100, batch), coef


def wall_ms_per_epoch(S, x, dx, batch, seeds):
    """(a), (b): wall time of fit() over EPOCHS epochs, per epoch."""
    tr, coef = trainer(S, x, dx, batch)
    n, n_seeds = x.shape[0], len(seeds)
    P0 = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in seeds]).to(DEV)
    gens = [torch.Generator(device=DEV).manual_seed(s) for s in seeds]
    keys = torch.empty(n_seeds, n, device=DEV)

    def orders():                                              # main_sweep._fit_adam; S = 1: DeviceBatches.epoch_order
        for _ in range(EPOCHS):
            if n_seeds == 1:
                yield torch.randperm(n, device=DEV)[None]
                continue
            for k, g in enumerate(gens):
                torch.rand(n, generator=g, out=keys[k])
            yield torch.argsort(keys, dim=1, stable=True)

    def window(**how):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.fit(P0, EPOCHS, **{k: v() if callable(v) else v for k, v in how.items()})
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / EPOCHS
        return run

    return alternate(window(orders=orders), window(order_seeds=seeds))


def launch_us_per_step(S, x, dx, batch, seeds):
    """(c): HIP events around one launch of LAUNCH_EPOCHS epochs, per minibatch step."""
    eng = S.get_engine()
    tr, coef = trainer(S, x, dx, batch)
    n, n_seeds = x.shape[0], len(seeds)
    table = eng.adam_order_table(n, batch, seeds, LAUNCH_EPOCHS, device=torch.device(DEV))
    seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    P0 = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in seeds]).to(DEV)
    kw = dict(lr=LR, w_x=W_X, w_reg=W_REG, threshold=0.05, st_freq=100)

    def window(keyed):
        p = P0.clone()
        m, v, step = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(n_seeds, dtype=torch.int32, device=DEV)
        mask = torch.ones(n_seeds, 2, coef.p, device=DEV)

        def run():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if keyed:
                eng.adam_epochs_keyed(x, dx, seeds_dev, LAUNCH_EPOCHS, batch, p, m, v, step, mask, ORDER, 0, **kw)
            else:
                eng.adam_epochs(x, dx, table, p, m, v, step, mask, ORDER, 0, **kw)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / (LAUNCH_EPOCHS * tr.steps)
        return run

    return alternate(window(False), window(True))


def uniformity_lines():
    from symode_amd.device_adam import ORDER_ROUNDS, epoch_order

    def chi(orders):
        c = np.zeros((16, 16))
        for o in orders:
            c[np.arange(16), o] += 1
        return float(((c - 1024.0) ** 2 / 1024.0).sum())

    rng = np.random.default_rng(20261019)
    lines = ["(position, row) chi-square of 16 384 orders of 16 rows (64 seeds x 256 epochs) against 1024 per cell; the 99.9 % "
             "quantile of chi-square(225) is 296.1 (tests/test_host_adam_order.py)",
             f"  numpy.random.Generator.permutation: {chi(rng.permutation(16) for _ in range(16384)):.1f}"]
    for rounds in (1, 2, 3, 4):
        value = chi(epoch_order(s, e, 16, rounds=rounds) for s in range(64) for e in range(256))
        lines.append(f"  twin, {rounds} Feistel round(s): {value:.1f}" + ("   <- ORDER_ROUNDS, the smallest count below the bound"
                                                                        if rounds == ORDER_ROUNDS else ""))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_device_shuffle.txt"))
    a = ap.parse_args()
    import symode_amd as S
    x, dx = (t.to(DEV).contiguous() for t in dosc_rows())
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"rows {x.shape[0]}, d = 2, order {ORDER}; windows of {EPOCHS} epochs ((c): launches of {LAUNCH_EPOCHS}), the two paths "
             f"alternating, {WARMUP} warm-up windows, median of {REPS} (min, max, +- half the interquartile range of the {REPS})"]
    lines += uniformity_lines()
    for n_seeds in (64, 1):
        seeds = list(range(n_seeds))
        for batch in (256, 4096):
            steps = (x.shape[0] + batch - 1) // batch
            wa, wb = wall_ms_per_epoch(S, x, dx, batch, seeds)
            ca, cb = launch_us_per_step(S, x, dx, batch, seeds)
            head = f"S {n_seeds} batch {batch} ({steps} steps per epoch)"
            lines += [f"{head}: (a) table path, order generation included: {fmt(wa, 'ms per epoch')}",
                      f"{head}: (b) keyed path:                              {fmt(wb, 'ms per epoch')}   (a) / (b) {spread(wa)[0] / spread(wb)[0]:.2f}",
                      f"{head}: (c) launch alone, table: {fmt(ca, 'us per step')}",
                      f"{head}: (c) launch alone, keyed: {fmt(cb, 'us per step')}   keyed / table {spread(cb)[0] / spread(ca)[0]:.3f}"]
            print("\n".join(lines[-4:]), flush=True)
    kept = []
    if os.path.exists(a.out):
        old = open(a.out).read().splitlines()
        kept = old[old.index(KEEP):] if KEEP in old else []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
    print("\n".join(lines[:8]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
