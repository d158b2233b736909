"""EquivSINDy-r seed sweep: the device STLSQ fit with the reversed symmetry regulariser (SeedSweepSTLSQ.solve(device=True,
rev=...), symode_stlsq_sweep_symreg) against the route the parent commit has for these configs, and its grid.

    python tests/perf/stlsq_symreg.py [--out FILE] [--parent_lib PATH/libsymode_hip.so] [--workdir DIR]

Data: the shape of lv/noise99_eq_rsymreg.cfg -- LV, 200 trajectories x 10^4 steps x 2, noise 0.99 with GP smoothing, order 2
plus exp (p = 8, d p = 16), 64 seeds x 1 % subsample (20 000 points each), threshold 0.15, w_sindy_reg 0, w_sym_reg 0.1 -- with a
frozen random LaLiGAN built as tests/perf/sym_sweep.py builds one.  g(x), J_g(x) are computed once, outside every window.
Every figure is wall time around the call with the results on the host at the end, the median of 20 runs after 3 warm-up
runs, with min, max and half the interquartile range; paths that are compared alternate run by run in one process.
  (a) [G | R] of the 64 seeds (GramStatistics.add_gathered: one gather launch each) plus one device solve, and the solve and the
      launch alone, against the same seeds' fit through SeedSweepLBFGS with the Gram closure on the same library build (the
      config's 100 epochs x 20 L-BFGS iterations at most, lr 0.1, st_freq 100) on the same statistics: the only route the
      parent commit has for these configs.  Seeds whose two masks agree are counted.
  (b) G = 1, 2, 4, 8 values of w_sym x 64 seeds in one solve against G scalar solves in sequence.
  (c) symode_stlsq_sweep and symode_stlsq_sweep_constrained on the same matrices, this build; with --parent_lib also the parent
      commit's library, loaded beside it, run by run in turn.
No threshold: the file records what was measured."""
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
    ap.add_argument("--workdir", default=None, help="data / saved_models go here (default: a temp dir)")
    a = ap.parse_args()
    out_file = os.path.abspath(a.out) if a.out else None
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd import dataset as D, engine as E, lstsq
    from symode_amd.coef_map import CoefMap
    from symode_amd.gram_closure import GramStatistics
    from symode_amd.main_sweep import _load_laligan, symmetry_operands
    from symode_amd.parser_utils import get_args
    from symode_amd.sindy import SINDyRegression
    from symode_amd.sweep import GramClosure, SeedSweepLBFGS, SeedSweepSTLSQ, seeded_subsamples
    from tests.perf.sym_sweep import _argv, _laligan
    work = a.workdir or tempfile.mkdtemp(prefix="stlsq_symreg_")
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    name = "perf-laligan-lv"
    args = vars(get_args(argv=_argv("lv", name, "perf-lv")))
    tr, _, args = D.get_dataset(args)
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
    lines = [f"device: {torch.cuda.get_device_name(0)}; lv 200 x 10^4 x 2, noise 0.99 (gp), order {order} + exp: p = {p}, d p = {d * p}; {S} seeds x "
             f"{m} points, {int(gx.shape[0])} group elements; w_sindy_reg {w_reg}, threshold {thr}, w_sym {w_sym}, max_iter {max_iter}; {WARMUP} "
             f"warm-up runs, median of {REPS} (min, max, +- half the interquartile range), wall time"]
    print(lines[0], flush=True)

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    sw = SeedSweepSTLSQ(x, dx, order, template.include_sine, template.include_exp, n_seeds=S, idx=rows, idx_sorted=True)
    eng = sw.engine

    def gather():
        return GramStatistics(S, d, order, flags, regulariser=True, device=DEV).add_gathered(x_used, dx_used, table, gx, jgx)

    stats = gather()
    sw.set_grams(stats.G, stats.count)

    def solve(w=w_sym, hyper=None, st=stats):
        return sw.solve(w_reg, thr, max_iter=max_iter, device=True, hyper=hyper, rev=(st.R, w))

    def gather_and_solve():
        st = gather()
        sw.set_grams(st.G, st.count)
        return solve(st=st)

    def launch(to_host=False):
        return eng.stlsq_sweep_symreg(stats.G, stats.R, stats.count, w_reg, thr, w_sym, max_iter, d=d, pivot_floor=lstsq.SINGULAR_RCOND ** 2,
                                      to_host=to_host)

    P0 = torch.stack([template.coef.draw(torch.Generator().manual_seed(s)) for s in range(S)]).to(DEV)

    def lbfgs(st=None):
        st = gather() if st is None else st
        clos = GramClosure(st, w_sym=w_sym, coef=template.coef)
        sweep = SeedSweepLBFGS(clos, args["lr_sindy"], thr, args["st_freq"], w_sindy_x=args["w_sindy_x"], sindy_reg_type=args["sindy_reg_type"],
                               w_sindy_reg=w_reg, gram_closure=True, statistics=st)
        out = sweep.fit(P0, args["num_epochs"])
        return out["Xi"].cpu(), out["mask"].cpu(), out["epochs"].cpu()

    alone = launch(to_host=True)
    dev, ref = solve(), lbfgs(stats)
    say(f"    the launch: {int((alone[4] != 0).sum())} of {S} problems flagged (solved by the host loop, minimum-norm rule), "
        f"{int(((alone[3] != 0) & (alone[4] == 0)).sum())} more with a near-threshold coefficient (replayed on the host for the record)")
    agree = int((dev[1].bool() == ref[1].view(S, d, p).bool()).all(dim=(1, 2)).sum())
    common = dev[1] * ref[1].view(S, d, p)
    say(f"    device: passes per seed {int(dev[2].min())}-{int(dev[2].max())}, near-threshold records {len(sw.near_threshold)}; L-BFGS: "
        f"epochs {int(ref[2].min())}-{int(ref[2].max())}; seeds whose two masks agree {agree}/{S}; "
        f"max |Xi_stlsq - Xi_lbfgs| on the common support {float(((dev[0] - ref[0].view(S, d, p)) * common).abs().max()):.3g}")
    got = alternate(timed(solve), timed(gather_and_solve), timed(lambda: lbfgs(stats)), timed(lbfgs), timed(launch))
    med = [spread(t)[0] for t in got]
    say(f"(a) symode_stlsq_sweep_symreg alone, results on the device:    {fmt(got[4])}",
        f"(a) regularised device solve, matrices on the device:          {fmt(got[0])}",
        f"(a) [G | R] gather launches + regularised device solve:        {fmt(got[1])}",
        f"(a) SeedSweepLBFGS, Gram closure, matrices on the device:      {fmt(got[2])}   L-BFGS / solve {med[2] / med[0]:.1f}",
        f"(a) [G | R] gather launches + SeedSweepLBFGS (parent's route): {fmt(got[3])}   L-BFGS / (gather + solve) {med[3] / med[1]:.1f}")
    # (b) a grid of G values of w_sym on the 64 seeds
    for G in (1, 2, 4, 8):
        ws = [w_sym * (1 + g) for g in range(G)]
        hyper = {"w_sym": [w for w in ws for _ in range(S)]}
        whole = solve(hyper=hyper)
        parts = [solve(w) for w in ws]
        same = all(whole[0][g * S:(g + 1) * S].numpy().tobytes() == parts[g][0].numpy().tobytes() for g in range(G))
        g_t, s_t = alternate(timed(lambda: solve(hyper=hyper)), timed(lambda: [solve(w) for w in ws]))
        say(f"(b) G {G} x {S} seeds, one solve of {G * S} problems:              {fmt(g_t)}   bit for bit the scalar solves: {same}",
            f"(b) G {G} x {S} seeds, {G} scalar solve(s) in sequence:             {fmt(s_t)}   sequence / grid "
            f"{spread(s_t)[0] / spread(g_t)[0]:.2f}")
    # (c) the two sibling entries on the same matrices, this build and the parent's
    Gd = stats.G
    # (Q = I without constants: the constrained fit is then the unconstrained one, so no support leaves collinear columns and
    # no problem is flagged -- every output of every problem is compared)
    coef = CoefMap(d, p, torch.eye(d * p), True, False)
    q_solve, q_xi = (torch.from_numpy(q).to(DEV) for q in (coef.solve_matrix(), coef.xi_matrix()))
    R_ = q_solve.shape[1]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    plain_out = [torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * d * p, dtype=u8, device=DEV)] + \
                [torch.empty(S, dtype=i32, device=DEV) for _ in range(3)]
    cons_out = [torch.empty(S * d * p, dtype=f32, device=DEV), torch.empty(S * R_, dtype=f32, device=DEV),
                torch.empty(S * d * p, dtype=u8, device=DEV)] + [torch.empty(S, dtype=i32, device=DEV) for _ in range(3)]
    thr32 = float(np.float32(thr))

    def plain(lib):
        def call():
            rc = lib.symode_stlsq_sweep(ptr(Gd), S, S, d, p, int(stats.count), None, w_reg, thr32, max_iter, 1e-4, *[ptr(t) for t in plain_out],
                                        stream)
            assert rc == 0, rc
            return [t.cpu() for t in plain_out]
        return call

    def constrained(lib):
        def call():
            rc = lib.symode_stlsq_sweep_constrained(ptr(Gd), S, S, d, p, int(stats.count), ptr(q_solve), ptr(q_xi), coef.r, 1 if coef.allow_constant else 0, None, w_reg,
                                                    thr32,
                                                    max_iter, 1e-4, lstsq.SINGULAR_RCOND ** 2, *[ptr(t) for t in cons_out], stream)
            assert rc == 0, rc
            return [t.cpu() for t in cons_out]
        return call

    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        for entry in ("symode_stlsq_sweep", "symode_stlsq_sweep_constrained"):
            getattr(parent, entry).restype, getattr(parent, entry).argtypes = E._SIGNATURES[entry]
        assert not hasattr(parent, "symode_stlsq_sweep_symreg")
    for label, entry in (("symode_stlsq_sweep", plain), ("symode_stlsq_sweep_constrained", constrained)):
        if parent is None:
            got = alternate(timed(entry(eng.lib)))
            say(f"(c) {label}, this build: {fmt(got[0])}")
        else:
            mine, theirs = entry(eng.lib)(), entry(parent)()
            flagged = mine[-1].numpy() != 0                                             # a flagged problem's other outputs are unspecified
            same = all(u.numpy().reshape(S, -1)[~flagged].tobytes() == v.numpy().reshape(S, -1)[~flagged].tobytes() for u, v in zip(mine, theirs))
            got = alternate(timed(entry(eng.lib)), timed(entry(parent)))
            say(f"(c) {label}, this build:           {fmt(got[0])}",
                f"(c) {label}, the parent's library: {fmt(got[1])}   equal bytes: {same} ({int(flagged.sum())} flagged); this / parent "
                f"{spread(got[0])[0] / spread(got[1])[0]:.3f}")
    if out_file:
        os.makedirs(os.path.dirname(out_file), exist_ok=True)
        with open(out_file, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
