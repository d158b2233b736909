"""What the regularised sparsity path buys over the regularised threshold fit, and how it depends on --path_tol: seeds that end
on the true support, on the CPU with the fp64 host twin (sindy.stlsq_path_symreg_from_gram) -- no GPU.

    python tests/perf/stlsq_path_symreg_tol.py [N_VARIANTS] [--out FILE]

Data: the oscillator deck of tests/stlsq_symreg_cases.py (400 seeded points, 50 % noise, two rotations as group elements) at
orders 2, 3 and 5; draw ``variant`` trains, draw ``variant + 100`` of the same case validates.  Ridge weight 0.  Per case and
w_sym the chain of a draw is computed ONCE (it does not depend on the tolerance), the selection rule
(sindy.stlsq_path_symreg_select) is applied per ladder value.  Beside each: the threshold fit --symreg_stlsq performs
(sindy.stlsq_symreg_from_gram, strict > 0.05 in fp32 on the active entries until the mask repeats) and the draws whose chain
passes through the true support at all.  The table is recorded in profiles/stlsq_path_symreg.txt."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LADDER = (0.0, 0.01, 0.02, 0.05, 0.1)
W_SYMS = (0.0, 0.1, 1.0, 10.0)
CASES = ("osc_o2", "osc_o3", "osc_o5")
THRESHOLD, MAX_ITER, FLOOR_REL, BAND = 0.05, 10, 1e-10, 1e-4


def threshold_fit(G, R, d, w_sym, n_points):
    """The host loop of SeedSweepSTLSQ.solve(rev=...): the final mask."""
    from symode_amd.sindy import stlsq_symreg_from_gram
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    for _ in range(MAX_ITER):
        xi = stlsq_symreg_from_gram(G, R, n_points, mask, 0.0, w_sym, d, "gels")[0]
        new = mask & (np.abs(xi) > np.float32(THRESHOLD))
        if np.array_equal(new, mask):
            break
        mask = new
    return mask


def main():
    argv = sys.argv[1:]
    out_file = os.path.abspath(argv.pop(argv.index("--out") + 1)) if "--out" in argv else None
    if "--out" in argv:
        argv.remove("--out")
    S = int(argv[0]) if argv else 64
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from symode_amd.sindy import stlsq_path_symreg_from_gram, stlsq_path_symreg_select
    from tests import stlsq_symreg_cases as C
    f32 = lambda v: float(np.float32(v))                                        # noqa: E731  (as the launch holds w_sym)
    lines = [f"oscillator deck of tests/stlsq_symreg_cases.py, {C.N_POINTS} points, noise {C.NOISE}, variants 0..{S - 1} train, variant + 100 "
             f"validates; ridge 0; threshold fit at {THRESHOLD}; seeds ending on the true support of {S}",
             "case      n   w_sym  threshold fit  truth in chain  chosen at tol " + "  ".join(f"{t:<5g}" for t in LADDER)]
    print("\n".join(lines), flush=True)
    for name in CASES:
        truth = C.truth(name)
        n_true = int(truth.sum())
        for w in W_SYMS:
            thr_ok, in_chain, chosen = 0, 0, {t: 0 for t in LADDER}
            for v in range(S):
                G, R, d = C.pair(name, v)
                V = C.pair(name, v + 100)[0]
                n0 = R.shape[0]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    thr_ok += bool(np.array_equal(threshold_fit(G, R, d, f32(w), C.N_POINTS), truth))
                    _, _, rec = stlsq_path_symreg_from_gram(G, R, V, 0.0, f32(w), 0.0, FLOOR_REL, BAND, d, C.N_POINTS)
                at = np.zeros(n0, dtype=bool)
                at[rec["order"][n0 - n_true:]] = True
                in_chain += bool(np.array_equal(at.reshape(truth.shape), truth))
                for t in LADDER:
                    best = stlsq_path_symreg_select(rec["mse_val"], V, d, t, FLOOR_REL)
                    m = np.zeros(n0, dtype=bool)
                    m[rec["order"][best:]] = True
                    chosen[t] += bool(np.array_equal(m.reshape(truth.shape), truth))
            line = f"{name:<9} {truth.size:<3} {w:<6g} {thr_ok:<14} {in_chain:<15} " + " " * 14 + "  ".join(f"{chosen[t]:<5}" for t in LADDER)
            lines.append(line)
            print(line, flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
