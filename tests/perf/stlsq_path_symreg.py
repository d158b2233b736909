"""The sparsity path with the reversed symmetry regulariser (symode_stlsq_path_symreg, SeedSweepSTLSQ.solve_path(rev=...))
beside the threshold loop it replaces, and the two kernels it touches or builds on through this build and the parent's.

    python tests/perf/stlsq_path_symreg.py [--out FILE] [--parent_lib PATH/libsymode_hip.so] [--workdir DIR]

Every figure is wall time around the call with the results on the host at the end (the launches alone: results on the
device, synchronised), the median of 20 runs after 3 warm-up runs, with min, max and half the interquartile range; all routes
in one process, 64 seeds.
  (a) lv/noise99_eq_rsymreg.cfg's shape -- LV, 200 x 10^4 x 2, noise 0.99 (gp), order 2 + exp: n = d p = 16, 64 seeds x 20 000
      points, a frozen random LaLiGAN as tests/perf/stlsq_symreg.py builds one; validation matrix from the whole validation
      set: the launch alone, solve_path, [G | R] gather + solve_path; beside them one symode_stlsq_sweep_symreg launch and an
      8-point threshold grid of it (the route a user had: a threshold ladder), through the parent's library when given.
  (b) dosc order 5 (n = 42): the 64 draws of tests/stlsq_symreg_cases' osc_o5 (400 points each; matrices handed in, no gather),
      validation = draw + 100: the launch alone and solve_path.
  (c) the lane limit (n = 64): spd_d4_p16 and spd_d1_p64, 64 draws each, likewise.
  (d) the pass mark, on the UNCHANGED kernels only: symode_stlsq_sweep_symreg (whose pass now comes from stlsqs_pass_solve)
      and symode_stlsq_path on (a)'s matrices through this build, the parent's library, and this build again.  Required:
      equal bytes in every output, and a this / parent ratio of medians inside the spread the two runs of this build show
      (the three alternate run by run; the spread is again / first, the distance of the two runs' medians, as earlier entries
      of README judged; run-to-run spread is the only noise source).  The exit status says whether both held.
      The new launch's time is recorded, not judged."""
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
TOL, FLOOR_REL = 0.02, 1e-10


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


def run(window, reps=REPS):
    return [window() for k in range(WARMUP + reps)][WARMUP:]


def alternate(*windows, reps=REPS):
    """The windows in turn, run by run, so that a drift of the machine meets all of them alike."""
    out = [[] for _ in windows]
    for k in range(WARMUP + reps):
        for which, window in enumerate(windows):
            t = window()
            if k >= WARMUP:
                out[which].append(t)
    return out


def flops(n):
    """sum_t (n - t)^3 / 3: the factorisations of the chain."""
    return sum((n - t) ** 3 / 3 for t in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print only)")
    ap.add_argument("--parent_lib", default=None, help="the parent commit's libsymode_hip.so, for (a) and (d)")
    ap.add_argument("--workdir", default=None, help="data / saved_models go here (default: a temp dir)")
    a = ap.parse_args()
    out_file = os.path.abspath(a.out) if a.out else None
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import dataset as D, engine as E, lstsq
    from symode_amd.gram_closure import GramStatistics
    from symode_amd.main_sweep import _load_laligan, symmetry_operands
    from symode_amd.parser_utils import get_args
    from symode_amd.sindy import SINDyRegression
    from symode_amd.sweep import SeedSweepSTLSQ, seeded_subsamples
    from tests import stlsq_symreg_cases as C
    from tests.perf.sym_sweep import _argv, _laligan
    work = a.workdir or tempfile.mkdtemp(prefix="stlsq_path_symreg_")
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    name = "perf-laligan-lv"
    args = vars(get_args(argv=_argv("lv", name, "perf-lv")))
    tr, va, args = D.get_dataset(args)
    x, dx = tr.x.to(DEV), tr.dx.to(DEV)
    if not os.path.exists(os.path.join("saved_models", name, "generator_mask.pt")):
        _laligan("lv", args, x, dx)
    laligan = _load_laligan(args, torch.device(DEV))
    S = SEEDS
    m = int(x.shape[0] * args["lbfgs_subsample"])
    rows = seeded_subsamples(x.shape[0], m, list(range(S)), DEV)
    x_used, gx, jgx, table, used = symmetry_operands(x, rows, *laligan)
    dx_used = dx[used].contiguous()
    template = SINDyRegression(**args).to(DEV)
    order, flags, d, p = template.poly_order, template.flags, template.latent_dim, template.coef.p
    thr, max_iter, w_reg = args["threshold"], max(1, args["num_epochs"]), args["w_sindy_reg"]
    w_sym = args["w_sym_reg"] / args["w_sindy_x"]
    floor = lstsq.SINGULAR_RCOND ** 2
    lines = [f"device: {torch.cuda.get_device_name(0)}; {S} seeds; path_tol {TOL}; {WARMUP} warm-up runs, median of {REPS} (min, max, +- half the "
             f"interquartile range), wall time"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    eng = symode_amd.get_engine()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())              # noqa: E731
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        for entry in ("symode_stlsq_sweep_symreg", "symode_stlsq_path"):
            getattr(parent, entry).restype, getattr(parent, entry).argtypes = E._SIGNATURES[entry]
        assert not hasattr(parent, "symode_stlsq_path_symreg")

    # ---- (a) the LV shape
    sw = SeedSweepSTLSQ(x, dx, order, template.include_sine, template.include_exp, n_seeds=S, idx=rows, idx_sorted=True)

    def gather():
        return GramStatistics(S, d, order, flags, regulariser=True, device=DEV).add_gathered(x_used, dx_used, table, gx, jgx)

    stats = gather()
    sw.set_grams(stats.G, stats.count)
    V = sw.val_grams(va.x.to(DEV), va.dx.to(DEV))
    n_points = int(stats.count)
    gamma = float(np.sqrt(w_reg))

    def solve_path(st=stats):
        return sw.solve_path(w_reg, V, TOL, rev=(st.R, w_sym))

    def gather_and_solve_path():
        st = gather()
        sw.set_grams(st.G, st.count)
        return solve_path(st)

    def launch(G, R, Vd, dd, g=gamma, w=w_sym):
        return eng.stlsq_path_symreg(G, R, Vd, n_points, g, w, TOL, FLOOR_REL, d=dd, pivot_floor=floor)

    sym_out = [torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=u8, device=DEV)] + \
              [torch.empty(S, dtype=i32, device=DEV) for _ in range(3)]
    grid_out = [torch.empty(8 * S * d * p, dtype=f32, device=DEV), torch.empty(8 * S * d * p, dtype=u8, device=DEV)] + \
               [torch.empty(8 * S, dtype=i32, device=DEV) for _ in range(3)]
    ladder = [thr * f for f in (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)]
    table8 = torch.tensor([[gamma, t, w_sym] for t in ladder for _ in range(S)], dtype=f32, device=DEV)
    path_out = [torch.empty(S * d * (p + 1) * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=i32, device=DEV),
                torch.empty(S * d * (p + 1), dtype=f64, device=DEV), torch.empty(S * d * (p + 1), dtype=f64, device=DEV),
                torch.empty(S * d, dtype=i32, device=DEV), torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=u8, device=DEV),
                torch.empty(S, dtype=i32, device=DEV), torch.empty(S, dtype=i32, device=DEV)]

    def symreg(lib, hyper=None, outs=sym_out):
        n_problems = S if hyper is None else hyper.shape[0]

        def call():
            rc = lib.symode_stlsq_sweep_symreg(ptr(stats.G), ptr(stats.R), S, n_problems, d, p, n_points, ptr(hyper), gamma, thr, w_sym, max_iter,
                                               1e-4, floor, *[ptr(t) for t in outs], stream)
            assert rc == 0, rc
        return call

    def plain_path(lib):
        def call():
            rc = lib.symode_stlsq_path(ptr(stats.G), ptr(V), S, 1, S, d, p, n_points, gamma, TOL, FLOOR_REL, 1e-4, *[ptr(t) for t in path_out], stream)
            assert rc == 0, rc
        return call

    o = launch(stats.G, stats.R, V, d)
    Xi, mask, rec = solve_path()
    size = d * p - rec["best"]
    say(f"(a) lv 200 x 10^4 x 2, noise 0.99 (gp), order {order} + exp: d = {d}, p = {p}, n = {d * p}; {S} seeds x {m} points, {int(gx.shape[0])} group "
        f"element(s), {va.x.shape[0]} validation points; w_sindy_reg {w_reg}, w_sym {w_sym}",
        f"    the launch: {int(o['fell'].sum())} of {S} problems flagged; chosen support size {int(size.min())}-{int(size.max())} of {d * p}; "
        f"near-tie eliminations in {int((rec['near'] > 0).sum())} problems; LDS {E_lds(d, p)} B per workgroup")
    say(f"(a) symode_stlsq_path_symreg alone, results on the device:      {fmt(run(timed(lambda: launch(stats.G, stats.R, V, d))))}",
        f"(a) solve_path(rev=...), matrices on the device:                {fmt(run(timed(solve_path)))}",
        f"(a) [G | R] gather launches + solve_path(rev=...):              {fmt(run(timed(gather_and_solve_path)))}")
    sw.set_grams(stats.G, stats.count)
    for label, lib in (("this build", eng.lib),) + ((("the parent's library", parent),) if parent else ()):
        say(f"(a) one symode_stlsq_sweep_symreg launch (threshold {thr}), {label}: {fmt(run(timed(symreg(lib))))}",
            f"(a) an 8-point threshold grid of it ({8 * S} problems), {label}:  {fmt(run(timed(symreg(lib, table8, grid_out))))}")

    # ---- (b), (c) the decks: matrices handed in
    for tag, case in (("(b) dosc order 5", "osc_o5"), ("(c) lane limit", "spd_d4_p16"), ("(c) lane limit", "spd_d1_p64")):
        pairs = [C.pair(case, v) for v in range(S)]
        dd = pairs[0][2]
        G = torch.from_numpy(np.stack([q[0] for q in pairs])).to(DEV)
        R = torch.from_numpy(np.stack([q[1] for q in pairs])).to(DEV)
        Vd = torch.from_numpy(np.stack([C.pair(case, v + 100)[0] for v in range(S)])).to(DEV)
        pp = G.shape[1] - dd
        n = dd * pp
        deck = SeedSweepSTLSQ(torch.zeros(8, 2, device=DEV), torch.zeros(8, 2, device=DEV), 1, n_seeds=S, engine=eng,
                              idx=torch.zeros(S, 4, dtype=torch.int32))
        deck.d, deck.p = dd, pp                                 # the deck has no compiled library behind it: only the matrices' shape counts
        deck.set_grams(G, C.N_POINTS)
        o = launch(G, R, Vd, dd, 0.0, 1.0)
        alone = run(timed(lambda: launch(G, R, Vd, dd, 0.0, 1.0)))
        whole = run(timed(lambda: deck.solve_path(0.0, Vd, TOL, rev=(R, 1.0))))
        say(f"{tag}, {case}: d = {dd}, p = {pp}, n = {n}, {n + 1} steps, {S} draws, ridge 0, w_sym 1; {int(o['fell'].sum())} flagged; LDS "
            f"{E_lds(dd, pp)} B per workgroup; sum_t (n - t)^3 / 3 = {flops(n):.3g} multiply-adds per problem",
            f"{tag}, {case}: symode_stlsq_path_symreg alone:   {fmt(alone)}   = {1e3 * spread(alone)[0] / (n + 1):.1f} us per step",
            f"{tag}, {case}: solve_path(rev=...):              {fmt(whole)}")

    # ---- (d) the pass mark: the unchanged kernels, this build / parent / this build
    ok = True
    if parent is None:
        say("(d) no --parent_lib: the pass mark was not taken")
    else:
        for label, entry, outs in (("symode_stlsq_sweep_symreg", symreg, sym_out), ("symode_stlsq_path", plain_path, path_out)):
            entry(eng.lib)()
            torch.cuda.synchronize()
            mine = [t.cpu().numpy().copy() for t in outs]
            entry(parent)()
            torch.cuda.synchronize()
            theirs = [t.cpu().numpy().copy() for t in outs]
            flagged = mine[-1] != 0                                                 # a flagged problem's other outputs are unspecified
            same = all(u.reshape(S, -1)[~flagged].tobytes() == v.reshape(S, -1)[~flagged].tobytes() for u, v in zip(mine, theirs))
            first, theirs_t, second = alternate(timed(entry(eng.lib)), timed(entry(parent)), timed(entry(eng.lib)))
            m1, mp_, m2 = spread(first)[0], spread(theirs_t)[0], spread(second)[0]
            width = abs(m2 / m1 - 1.0)                              # the spread the two runs of this build show: again / first
            ratio = m1 / mp_
            inside = same and abs(ratio - 1.0) <= width
            ok &= inside
            say(f"(d) {label}, this build:           {fmt(first)}",
                f"(d) {label}, the parent's library: {fmt(theirs_t)}   equal bytes in every output: {same} ({int(flagged.sum())} flagged)",
                f"(d) {label}, this build again:     {fmt(second)}   again / first {m2 / m1:.3f}",
                f"(d) {label}: this / parent {ratio:.4f} ({1e3 * (m1 - mp_):+.2f} us); again / first {m2 / m1:.4f}; this / parent inside what the two runs "
                f"of this build show, and equal bytes: {inside}")
    if out_file:
        os.makedirs(os.path.dirname(out_file), exist_ok=True)
        with open(out_file, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def E_lds(d, p):
    """stlsqps_lds_bytes of csrc/stlsq_path_symreg.hpp."""
    F, n = p + d, d * p
    return (2 * F * F + 2 * n * n) * 8 + 4 * 8 + n * 8


if __name__ == "__main__":
    sys.exit(main())
