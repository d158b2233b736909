"""Block-bootstrap bagging of the device STLSQ sweep (symode_gram_resample, symode_stlsq_bag, SeedSweepSTLSQ.solve_bagged)
beside what the existing entries alone can do for the same result, and the two sibling entries through this build and the
parent commit's library.

    python tests/perf/stlsq_bag.py [--out FILE] [--parent_lib PATH/libsymode_hip.so] [--workdir DIR]

Shape: selkov, noise 0.2 with GP smoothing, order 3 (p = 10, d = 2), 64 seeds x 50 000 points: BASELINE config[3]; B = 32
replicas of C = 128 chunks, the inclusion ladder 0.5 / 0.6 / 0.8 / 0.9 / 1.0 as the grid.
Every figure is wall time around the call, the median of 20 runs after 3 warm-up runs, with min, max and half the
interquartile range; the routes alternate run by run in one process.
  (a) the four launches one by one (results stay on the device) -- chunk matrices (symode_aug_gram_gather on the (S C, L)
      table), replicas (symode_gram_resample), replica fits (symode_stlsq_sweep, S B problems), aggregation and refit
      (symode_stlsq_bag, 5 x S problems) -- and together: solve_bagged, one copy back.
  (b) the same result from existing entries only: a with-replacement (S B, m) row table from torch (row-level bootstrap of each
      seed's subsample), ONE symode_aug_gram_gather on it, ONE symode_stlsq_sweep, aggregation and refit in numpy
      (sindy.stlsq_bag_from_gram per problem).  Timed in three parts and together, 5 runs (it takes seconds).
  (c) symode_stlsq_sweep and symode_stlsq_path on the shape's matrices through this build, the parent's library and this build
      AGAIN, run by run in turn: equal bytes, and the ratio this / parent beside the ratio of the two runs of this build.
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
WARMUP, REPS, SEEDS, B, C = 3, 20, 64, 32, 128
LADDER = [0.5, 0.6, 0.8, 0.9, 1.0]
DEV = "cuda:0"
ARGV = ["--task", "selkov", "--poly_order", "3", "--threshold", "0.075", "--noise", "0.2", "--smoothing", "gp", "--sindy_optimizer", "lbfgs",
        "--w_sindy_reg", "0.0", "--w_sym_reg", "0.0", "--lbfgs_subsample", "0.5", "--num_epochs", "10", "--ae_arch", "none"]


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


def alternate(*windows, reps=REPS, warmup=WARMUP):
    out = [[] for _ in windows]
    for k in range(warmup + reps):
        for which, window in enumerate(windows):
            t = window()
            if k >= warmup:
                out[which].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    ap.add_argument("--parent_lib", default=None, help="the parent commit's libsymode_hip.so, for (c)")
    ap.add_argument("--workdir", default=None, help="data files go here (default: a temp dir)")
    a = ap.parse_args()
    out_file = os.path.abspath(a.out) if a.out else None
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import dataset as D, engine as E
    from symode_amd.parser_utils import get_args
    from symode_amd.sindy import stlsq_bag_from_gram
    from symode_amd.sweep import SeedSweepSTLSQ, inclusion_milli, seeded_subsamples
    work = a.workdir or tempfile.mkdtemp(prefix="stlsq_bag_")
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    S = SEEDS
    eng = symode_amd.get_engine()
    lines = [f"device: {torch.cuda.get_device_name(0)}; {S} seeds, B = {B} replicas, C = {C} chunks, inclusion ladder {LADDER}; {WARMUP} "
             f"warm-up runs, median of {REPS} (min, max, +- half the interquartile range), wall time"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    args = vars(get_args(argv=list(ARGV)))
    tr, va, args = D.get_dataset(args)
    x, dx = tr.x.to(DEV), tr.dx.to(DEV)
    m = int(x.shape[0] * args["lbfgs_subsample"])
    rows = seeded_subsamples(x.shape[0], m, list(range(S)), DEV)
    sw = SeedSweepSTLSQ(x, dx, 3, n_seeds=S, idx=rows, idx_sorted=True)
    G, d, p, thr = sw.grams(device=True), sw.d, sw.p, float(np.float32(args["threshold"]))
    tau = torch.tensor([t for t in inclusion_milli(LADDER) for _ in range(S)], dtype=torch.int32, device=DEV)
    seeds = torch.tensor(sw.seeds, dtype=torch.int64, device=DEV)
    chunk = sw.chunk_grams(C)
    rep = eng.gram_resample(chunk, seeds, B)
    fits = eng.stlsq_sweep(rep, sw.n_points, 0.0, thr, 10, d=d)
    Xi, mask, record = sw.solve_bagged(0.0, thr, B, n_chunks=C, inclusion=LADDER)
    size = (mask.numpy() > 0).sum(axis=(1, 2)).reshape(len(LADDER), S)
    say(f"selkov order 3: p = {p}, d = {d}, {sw.n_points} points per seed, chunks of {m // C} rows; valid replicas "
        f"{record['valid'].min()}-{record['valid'].max()} of {B}; refits flagged {int(record['fell'].sum())}; support sizes "
        + ", ".join(f"{size[g].min()}-{size[g].max()} at {LADDER[g]}" for g in range(len(LADDER))))
    got = alternate(timed(lambda: sw.chunk_grams(C)), timed(lambda: eng.gram_resample(chunk, seeds, B)),
                    timed(lambda: eng.stlsq_sweep(rep, sw.n_points, 0.0, thr, 10, d=d)),
                    timed(lambda: eng.stlsq_bag(G, fits[0], fits[1], fits[4], B, 0.0, tau_table=tau, d=d)),
                    timed(lambda: sw.solve_bagged(0.0, thr, B, n_chunks=C, inclusion=LADDER)),
                    timed(lambda: sw.solve(0.0, thr, max_iter=10, device=True)))
    say(f"(a) chunk matrices, symode_aug_gram_gather on the ({S * C}, {m // C}) table:   {fmt(got[0])}",
        f"(a) replicas, symode_gram_resample ({S * B} x {p + d} x {p + d}):                  {fmt(got[1])}",
        f"(a) replica fits, symode_stlsq_sweep ({S * B} problems):                  {fmt(got[2])}",
        f"(a) aggregation and refit, symode_stlsq_bag ({len(LADDER) * S} problems):          {fmt(got[3])}",
        f"(a) together, solve_bagged (seed matrices resident, one copy back):     {fmt(got[4])}",
        f"(a) for context, solve(device=True): ONE fit per seed, one copy back:   {fmt(got[5])}")
    together = spread(got[4])[0]

    # (b) the same result with the entries the parent has: row-level bootstrap through one big gather
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    state = {}

    def table():
        pick = torch.randint(0, m, (S * B, m), device=DEV, generator=gen)
        state["idx"] = torch.sort(torch.gather(sw.idx.repeat_interleave(B, dim=0).long(), 1, pick), dim=1).values.to(torch.int32)

    def gather():
        state["rep"] = eng.aug_gram_gather(x, dx, state["idx"], 3, 0)

    def fit():
        state["fits"] = eng.stlsq_sweep(state["rep"], m, 0.0, thr, 10, d=d, to_host=True)

    def aggregate():
        rxi, rmask, _, _, rfell = state["fits"]
        Gh = sw.grams()
        for g, t in enumerate(inclusion_milli(LADDER)):
            for k in range(S):
                at = slice(k * B, (k + 1) * B)
                stlsq_bag_from_gram(Gh[k], rxi[at], rmask[at], rfell[at], t, 0.0, d, m)

    def parent_route():
        table(), gather(), fit(), aggregate()

    table(), gather(), fit()
    old = alternate(timed(table), timed(gather), timed(fit), timed(aggregate), timed(parent_route), reps=5, warmup=1)
    say(f"(b) existing entries only: with-replacement ({S * B}, {m}) row table from torch: {fmt(old[0])}",
        f"(b) ONE symode_aug_gram_gather on it:                                   {fmt(old[1])}",
        f"(b) ONE symode_stlsq_sweep ({S * B} problems), one copy back:             {fmt(old[2])}",
        f"(b) aggregation and refit in numpy ({len(LADDER) * S} problems):                   {fmt(old[3])}",
        f"(b) together:                                                           {fmt(old[4])}   existing entries / solve_bagged "
        f"{spread(old[4])[0] / together:.1f}")
    state.clear()

    # (c) the sibling entries through this build, the parent's library and this build again
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    V = sw.val_grams(va.x.to(DEV), va.dx.to(DEV))
    sweep_out = [torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=u8, device=DEV)] + \
                [torch.empty(S, dtype=i32, device=DEV) for _ in range(3)]
    path_out = [torch.empty(S * d * (p + 1) * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=i32, device=DEV),
                torch.empty(S * d * (p + 1), dtype=f64, device=DEV), torch.empty(S * d * (p + 1), dtype=f64, device=DEV),
                torch.empty(S * d, dtype=i32, device=DEV), torch.empty(S * d * p, dtype=f32, device=DEV),
                torch.empty(S * d * p, dtype=u8, device=DEV), torch.empty(S, dtype=i32, device=DEV), torch.empty(S, dtype=i32, device=DEV)]

    def plain(lib):
        def call():
            rc = lib.symode_stlsq_sweep(ptr(G), S, S, d, p, int(sw.n_points), None, 0.0, thr, 10, 1e-4, *[ptr(t) for t in sweep_out], stream)
            assert rc == 0, rc
            return [t.cpu() for t in sweep_out]
        return call

    def path(lib):
        def call():
            rc = lib.symode_stlsq_path(ptr(G), ptr(V), S, 1, S, d, p, int(sw.n_points), 0.0, 0.02, 1e-10, 1e-4, *[ptr(t) for t in path_out], stream)
            assert rc == 0, rc
            return [t.cpu() for t in path_out]
        return call

    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        for entry in ("symode_stlsq_sweep", "symode_stlsq_path"):
            getattr(parent, entry).restype, getattr(parent, entry).argtypes = E._SIGNATURES[entry]
        assert not hasattr(parent, "symode_stlsq_bag") and not hasattr(parent, "symode_gram_resample")
    for label, entry in (("symode_stlsq_sweep", plain), ("symode_stlsq_path", path)):
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
