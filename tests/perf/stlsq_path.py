"""The sparsity path of the device STLSQ sweep (symode_stlsq_path, SeedSweepSTLSQ.solve_path) beside the threshold loop and
its grid, and the two sibling entries through this build and the parent commit's library.

    python tests/perf/stlsq_path.py [--out FILE] [--parent_lib PATH/libsymode_hip.so] [--workdir DIR]

Shapes: (1) selkov, noise 0.2 with GP smoothing, order 3 (p = 10, d = 2), 64 seeds x 50 000 points: BASELINE config[3];
(2) dosc, noise 0.2 with GP smoothing, order 5 (p = 21, d = 2), 64 seeds x 2 500 points; (3) 64 random positive-definite
problems at p = 64, d = 4 (no compiled library: synthetic matrices, so no gather).  The held-out matrix is the validation
set's (1) (2), or from further rows (3).
Every figure is wall time around the call, the median of 20 runs after 3 warm-up runs, with min, max and half the
interquartile range; the routes of a shape alternate run by run in one process.
  (a) the path launch alone (results stay on the device); solve_path on resident matrices (one copy back); gather + solve_path.
  (b) for context: ONE symode_stlsq_sweep launch at the config's threshold, and an 8-point threshold grid (8 x 64 problems
      on the same matrices, one launch) -- through the parent's library when --parent_lib is given, else this build's.
  (c) symode_stlsq_sweep and symode_stlsq_sweep_constrained on shape (1)'s matrices through this build, the parent's library and
      this build AGAIN, run by run in turn: equal bytes, and the ratio this / parent beside the ratio of the two runs of this
      build (the spread that repeats of one path show in the session).
No threshold on any time: the file records what was measured."""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS, SEEDS = 3, 20, 64
DEV = "cuda:0"
COMMON = ["--noise", "0.2", "--smoothing", "gp", "--sindy_optimizer", "lbfgs", "--w_sindy_reg", "0.0", "--w_sym_reg", "0.0",
          "--lbfgs_subsample", "0.5", "--num_epochs", "10", "--ae_arch", "none"]
SHAPES = [("selkov", 3, 0.075), ("dosc", 5, 0.01)]


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
    ap.add_argument("--parent_lib", default=None, help="the parent commit's libsymode_hip.so, for (b) and (c)")
    ap.add_argument("--workdir", default=None, help="data files go here (default: a temp dir)")
    a = ap.parse_args()
    out_file = os.path.abspath(a.out) if a.out else None
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import dataset as D, engine as E, lstsq
    from symode_amd.coef_map import CoefMap
    from symode_amd.main_sweep import PATH_TOL
    from symode_amd.parser_utils import get_args
    from symode_amd.sweep import SeedSweepSTLSQ, seeded_subsamples
    work = a.workdir or tempfile.mkdtemp(prefix="stlsq_path_")
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    S = SEEDS
    eng = symode_amd.get_engine()
    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        for entry in ("symode_stlsq_sweep", "symode_stlsq_sweep_constrained"):
            getattr(parent, entry).restype, getattr(parent, entry).argtypes = E._SIGNATURES[entry]
        assert not hasattr(parent, "symode_stlsq_path")
    grid_lib, grid_name = (parent, "the parent's library") if parent is not None else (eng.lib, "this build")
    lines = [f"device: {torch.cuda.get_device_name(0)}; {S} seeds; path_tol {PATH_TOL}, floor_rel 1e-10, w_sindy_reg 0; {WARMUP} warm-up runs, "
             f"median of {REPS} (min, max, +- half the interquartile range), wall time"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32

    def sweep_call(lib, G, d, p, n_points, thr, n_problems, table=None):
        """One raw symode_stlsq_sweep launch through ``lib``; the outputs stay on the device."""
        out = [torch.empty(n_problems * d * p, dtype=f32, device=DEV), torch.empty(n_problems * d * p, dtype=u8, device=DEV)] + \
              [torch.empty(n_problems, dtype=i32, device=DEV) for _ in range(3)]

        def call():
            rc = lib.symode_stlsq_sweep(ptr(G), G.shape[0], n_problems, d, p, int(n_points), None if table is None else ptr(table), 0.0,
                                        float(np.float32(thr)), 10, 1e-4, *[ptr(t) for t in out], stream)
            assert rc == 0, rc
            return out
        return call

    def report(tag, G, V, d, n_points, thr, sw=None, gather=None):
        """``sw``: the sweep whose solve_path is timed too (the synthetic deck has none: no compiled library at d = 4)."""
        p = G.shape[1] - d
        launch = lambda: eng.stlsq_path(G, V, n_points, 0.0, PATH_TOL, 1e-10, d=d)                      # noqa: E731
        solve = (lambda: sw.solve_path(0.0, V, PATH_TOL)) if sw is not None else (                       # noqa: E731
            lambda: eng.stlsq_path(G, V, n_points, 0.0, PATH_TOL, 1e-10, d=d, to_host=True))
        o = eng.stlsq_path(G, V, n_points, 0.0, PATH_TOL, 1e-10, d=d, to_host=True)
        size = p - o["best"]
        say(f"{tag}: p = {p}, d = {d}, {n_points} points per seed; {int(o['fell'].sum())} of {S} problems flagged, near-tie eliminations in "
            f"{int((o['near'] > 0).sum())}; chosen support sizes per row " + ", ".join(f"{int(size[:, j].min())}-{int(size[:, j].max())}" for j in range(d)))
        thrs = [thr * f for f in (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)]
        table = torch.tensor([[0.0, t] for t in thrs for _ in range(S)], dtype=f32, device=DEV)
        one = sweep_call(eng.lib, G, d, p, n_points, thr, S)
        grid = sweep_call(grid_lib, G, d, p, n_points, thr, 8 * S, table)
        windows = [timed(launch), timed(solve), timed(one), timed(grid)]
        if gather is not None:
            windows.append(timed(lambda: (gather(), solve())))
        got = alternate(*windows)
        say(f"(a) {tag}: symode_stlsq_path alone, results on the device:        {fmt(got[0])}",
            f"(a) {tag}: {'solve_path' if sw is not None else 'engine.stlsq_path'}, matrices on the device, one copy back: {fmt(got[1])}")
        if gather is not None:
            say(f"(a) {tag}: gather launch + solve_path:                            {fmt(got[4])}")
        say(f"(b) {tag}: ONE symode_stlsq_sweep launch (threshold {thr:g}), this build: {fmt(got[2])}",
            f"(b) {tag}: 8-point threshold grid, 8 x {S} problems, one launch, {grid_name}: {fmt(got[3])}   "
            f"path launch / grid launch {spread(got[0])[0] / spread(got[3])[0]:.2f}")

    first = None
    for task, order, thr in SHAPES:
        args = vars(get_args(argv=COMMON + ["--task", task, "--poly_order", str(order), "--threshold", str(thr)]))
        tr, va, args = D.get_dataset(args)
        x, dx = tr.x.to(DEV), tr.dx.to(DEV)
        m = int(x.shape[0] * args["lbfgs_subsample"])
        rows = seeded_subsamples(x.shape[0], m, list(range(S)), DEV)
        sw = SeedSweepSTLSQ(x, dx, order, n_seeds=S, idx=rows, idx_sorted=True)
        V = sw.val_grams(va.x.to(DEV), va.dx.to(DEV))

        def gather(sw=sw):
            sw._gram, sw._gram_dev = None, None
            return sw.grams(device=True)

        report(f"{task} order {order}", sw.grams(device=True), V, sw.d, sw.n_points, thr, sw, gather)
        first = sw if first is None else first
    rng = np.random.RandomState(0)
    A = rng.randn(S, 400, 68)
    xi = rng.randn(S, 4, 64) * (rng.rand(S, 4, 64) < 0.1)
    A[:, :, 64:] = np.einsum("snp,sjp->snj", A[:, :, :64], xi) + 0.05 * rng.randn(S, 400, 4)
    B = rng.randn(1, 200, 68)
    B[:, :, 64:] = np.einsum("snp,sjp->snj", B[:, :, :64], xi[:1]) + 0.05 * rng.randn(1, 200, 4)
    report("random positive-definite deck", torch.from_numpy(np.einsum("sna,snb->sab", A, A)).to(DEV),
           torch.from_numpy(np.einsum("sna,snb->sab", B, B)).to(DEV), 4, 400, 0.1)
    # (c) the two sibling entries on shape (1)'s matrices: this build, the parent's library, this build again
    sw = first
    Gd, d, p = sw.grams(device=True), sw.d, sw.p
    coef = CoefMap(d, p, torch.eye(d * p), True, False)         # Q = I without constants: no support leaves collinear columns
    q_solve, q_xi = (torch.from_numpy(q).to(DEV) for q in (coef.solve_matrix(), coef.xi_matrix()))
    cons_out = [torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * q_solve.shape[1], dtype=f32, device=DEV),
                torch.empty(S * d * p, dtype=u8, device=DEV)] + [torch.empty(S, dtype=i32, device=DEV) for _ in range(3)]
    thr32 = float(np.float32(SHAPES[0][2]))

    def plain(lib):
        inner = sweep_call(lib, Gd, d, p, sw.n_points, thr32, S)
        return lambda: [t.cpu() for t in inner()]

    def constrained(lib):
        def call():
            rc = lib.symode_stlsq_sweep_constrained(ptr(Gd), S, S, d, p, int(sw.n_points), ptr(q_solve), ptr(q_xi), coef.r, 1 if coef.allow_constant else 0,
                                                    None, 0.0, thr32, 10, 1e-4, lstsq.SINGULAR_RCOND ** 2, *[ptr(t) for t in cons_out], stream)
            assert rc == 0, rc
            return [t.cpu() for t in cons_out]
        return call

    for label, entry in (("symode_stlsq_sweep", plain), ("symode_stlsq_sweep_constrained", constrained)):
        if parent is None:
            got = alternate(timed(entry(eng.lib)), timed(entry(eng.lib)))
            say(f"(c) {label}, this build:       {fmt(got[0])}",
                f"(c) {label}, this build again: {fmt(got[1])}   again / first {spread(got[1])[0] / spread(got[0])[0]:.3f}; the parent's library: not run")
            continue
        mine, theirs = entry(eng.lib)(), entry(parent)()
        flagged = mine[-1].numpy() != 0                                             # a flagged problem's other outputs are unspecified
        same = all(u.numpy().reshape(S, -1)[~flagged].tobytes() == v.numpy().reshape(S, -1)[~flagged].tobytes() for u, v in zip(mine, theirs))
        got = alternate(timed(entry(eng.lib)), timed(entry(parent)), timed(entry(eng.lib)))
        say(f"(c) {label}, this build:           {fmt(got[0])}",
            f"(c) {label}, the parent's library: {fmt(got[1])}   equal bytes in every output: {same} ({int(flagged.sum())} flagged); this / parent "
            f"{spread(got[0])[0] / spread(got[1])[0]:.3f}",
            f"(c) {label}, this build again:     {fmt(got[2])}   again / first {spread(got[2])[0] / spread(got[0])[0]:.3f} (the spread of one path)")
    if out_file:
        os.makedirs(os.path.dirname(out_file), exist_ok=True)
        with open(out_file, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
