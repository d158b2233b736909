"""Device L-BFGS trainer: a hyper-parameter grid on shared Gram matrices (symode_trainer_grid_run, G x 64 problems on 64 sets
of matrices) against G scalar Gram fits of 64 problems in sequence, and the 64-seed scalar fit of this build against
another build of the library.

    python tests/perf/lbfgs_grid.py [--part a|b|all] [--other-lib PATH/libsymode_hip.so] [--out FILE]

Data: 64 seeds x 2000 random points with the reversed regulariser's operands (2 group elements), d = 2, order 3 and 5; the
Gram form never looks at the points again, so N does not enter a fit's time.  A fit is 8 epochs of max_iter = 20 (8 x 41
launches) enqueued by ONE symode_trainer_run call from a freshly initialised state (the initialisation is outside the
events); no tolerance can end an iteration or an epoch early (all 0, st_freq 0), so every fit is the same work -- the line
of a path also says how many problems ended NaN, which would be empty launches.  Every figure is HIP-event time around one
fit in ms; 3 warm-up fits per path, then the median of 20 with their spread (min, max, half the interquartile range).  Paths
that are compared alternate fit by fit in one process.
  (a) the 64-seed scalar fit through this build's symode_trainer_run and, with ``--other-lib``, through that library's (the
      parent commit's: ``symode_trainer`` is the same struct, so both take the same descriptor and state block).
  (b) G = 1, 2, 4, 8 points x 64 seeds: one grid fit of G x 64 problems against G scalar fits in sequence, and the ratio.
No threshold: the file records what was measured."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS, EPOCHS, MAX_ITER, SEEDS, POINTS_PER_SEED = 3, 20, 8, 20, 64, 2000
LR, W_REG, THRESHOLD, W_SYM = 0.1, 1e-3, 0.05, 0.1
DEV = "cuda:0"


def spread(times):
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), min(times), max(times), (q[2] - q[0]) / 2


def fmt(times):
    med, lo, hi, hiqr = spread(times)
    return f"{med:.3f} ms per fit (min {lo:.3f}, max {hi:.3f}, +-{hiqr:.3f})"


def alternate(*windows):
    """WARMUP + REPS fits of each path, a b a b ...; returns one list of REPS figures per path."""
    out = [[] for _ in windows]
    for k in range(WARMUP + REPS):
        for which, window in enumerate(windows):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def statistics_of(S, order):
    """GramStatistics of 64 seeds with R: points around a sparse polynomial system, a rotation-like group action."""
    g = torch.Generator().manual_seed(order)
    p = S.get_engine().lib_size(2, order, 0)
    x = 0.6 * torch.randn(SEEDS, POINTS_PER_SEED, 2, generator=g)
    truth = torch.randn(2, p, generator=g) * (torch.rand(2, p, generator=g) < 0.3)
    theta = torch.stack([S.get_engine().theta(x[s].to(DEV), order, 0).cpu() for s in range(SEEDS)])
    dx = theta @ truth.T + 0.05 * torch.randn(SEEDS, POINTS_PER_SEED, 2, generator=g)
    A = torch.eye(2) + 0.2 * torch.randn(2, 2, 2, generator=g)
    gx = torch.einsum("gij,snj->sgni", A, x).contiguous()
    jgx = A[None, :, None].expand(SEEDS, 2, POINTS_PER_SEED, 2, 2).contiguous()
    st = S.gram_closure.GramStatistics(SEEDS, 2, order, 0, regulariser=True, device=DEV)
    return st.add(x.to(DEV), dx.to(DEV), gx.to(DEV), jgx.to(DEV)), p


def trainer(S, st, order, hyper=None, **scalars):
    s = dict(lr=LR, w_reg=W_REG, threshold=THRESHOLD, w_sym=W_SYM)
    s.update(scalars)
    return S.device_lbfgs.DeviceTrainer(None, None, order, 0, reversed_sym=(None, None, s["w_sym"]), lr=s["lr"], threshold=s["threshold"],
                                        st_freq=0, w_reg=s["w_reg"], l1=True, tol=0.0, max_iter=MAX_ITER, tol_grad=0.0, tol_change=0.0,
                                        detail=False, closure="gram", statistics=st, hyper=hyper)


def fit(tr, P0, run=None, init=None):
    """One fit of ``tr`` from P0: the state is initialised outside the events, the EPOCHS epochs are one run call."""
    lib = tr.engine.lib
    init, run = init or lib.symode_trainer_init, run or tr._run_fn
    desc = tr._Gp if run is tr._run_fn else tr._Tp

    def window():
        rc = init(tr._Tp, ctypes.c_void_p(P0.data_ptr()), None, tr._st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = run(desc, 0, EPOCHS, 0, tr._st())
        b.record()
        b.synchronize()
        assert rc == 0, rc
        return a.elapsed_time(b)
    return window


def nan_count(*trainers):
    return sum(int(tr.field("nan").sum()) + int(torch.isnan(tr.field("params")).any(dim=1).sum()) for tr in trainers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("a", "b", "all"))
    ap.add_argument("--other-lib", default=None, help="another build of libsymode_hip.so (the parent commit's) for part (a)")
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import symode_amd as S
    from symode_amd import device_lbfgs, gram_closure  # noqa: F401
    from symode_amd.engine import _SIGNATURES
    other = None
    if a.other_lib:
        other = ctypes.CDLL(os.path.abspath(a.other_lib))
        for name in ("symode_trainer_init", "symode_trainer_run"):
            getattr(other, name).restype, getattr(other, name).argtypes = _SIGNATURES[name]
    lines = [f"device: {torch.cuda.get_device_name(0)}; {SEEDS} seeds, d = 2, Gram form with R; a fit = {EPOCHS} epochs x max_iter {MAX_ITER} "
             f"({EPOCHS * (2 * MAX_ITER + 1)} launches); HIP events, {WARMUP} warm-up fits, median of {REPS} (min, max, +- half the "
             f"interquartile range)"]
    print(lines[0], flush=True)
    for order in (3, 5):
        st, p = statistics_of(S, order)
        P0 = (0.1 * torch.randn(SEEDS, 2 * p, generator=torch.Generator().manual_seed(1))).to(DEV)
        head = f"order {order} (d p = {2 * p})"
        if a.part in ("a", "all"):
            tr = trainer(S, st, order)
            paths = [fit(tr, P0)] + ([fit(tr, P0, other.symode_trainer_run, other.symode_trainer_init)] if other else [])
            got = alternate(*paths)
            lines.append(f"{head}: (a) {SEEDS}-seed scalar fit, this build:  {fmt(got[0])}   NaN problems {nan_count(tr)}")
            if other:
                lines.append(f"{head}: (a) {SEEDS}-seed scalar fit, other build: {fmt(got[1])}   this / other "
                             f"{spread(got[0])[0] / spread(got[1])[0]:.3f}")
            print("\n".join(lines[-(2 if other else 1):]), flush=True)
        if a.part in ("b", "all"):
            for G in (1, 2, 4, 8):
                points = [(LR * (1 + 0.25 * g), W_REG * (1 + g % 3), THRESHOLD * (1 + g % 2), W_SYM * (1 + g)) for g in range(G)]
                cols = list(zip(*[pt for pt in points for _ in range(SEEDS)]))
                grid = trainer(S, st, order, hyper=dict(zip(("lr", "w_reg", "threshold", "w_sym"), cols)))
                parts = [trainer(S, st, order, lr=pt[0], w_reg=pt[1], threshold=pt[2], w_sym=pt[3]) for pt in points]
                whole = fit(grid, P0.repeat(G, 1).contiguous())
                singles = [fit(tr, P0) for tr in parts]
                g_t, s_t = alternate(whole, lambda: sum(w() for w in singles))
                lines += [f"{head}: (b) G {G} x {SEEDS} seeds, one grid fit:      {fmt(g_t)}   NaN problems {nan_count(grid)}",
                          f"{head}: (b) G {G} x {SEEDS} seeds, {G} scalar fit(s):   {fmt(s_t)}   NaN problems {nan_count(*parts)}   "
                          f"sequence / grid {spread(s_t)[0] / spread(g_t)[0]:.2f}"]
                print("\n".join(lines[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
