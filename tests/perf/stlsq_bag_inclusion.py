"""How main_sweep's default --bag_inclusion was chosen: the success count of the bagged threshold fit against
evaluation.truth_table over a ladder of inclusion levels, beside the plain threshold fit's, on the CPU with the host twin
(sweep.resample_grams, symode_host_stlsq_sweep with the full-rank driver, sindy.stlsq_bag_from_gram) -- no GPU.

    python tests/perf/stlsq_bag_inclusion.py [N_SEEDS] [--workdir DIR]      (from symmetry-ode-discovery_amd/, where run_configs/ is)

Data: the training sets the generators make for the three plain configs below; each seed's subsample as main_sweep draws it on
the CPU, its chunks as SeedSweepSTLSQ.chunk_grams cuts them (ascending rows, L = m // C per chunk), ridge weight and threshold
each config's own.  The replica fits of a seed are computed ONCE (they do not depend on the level), aggregation and refit per
ladder value.  The table is recorded in profiles/stlsq_bag.txt."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LADDER = (0.5, 0.6, 0.8, 0.9, 1.0)
CONFIGS = ("growth/noise05_sindy.cfg", "dosc/noise20_sindy.cfg", "selkov/noise20_eq_sindy.cfg")
B, C = 32, 128


def main():
    argv = sys.argv[1:]
    if "--workdir" in argv:
        os.chdir(argv.pop(argv.index("--workdir") + 1))
        argv.remove("--workdir")
    S = int(argv[0]) if argv else 64
    sys.path.insert(0, ROOT)
    import symode_amd  # noqa: F401
    from oracle import sindy_oracle as O
    from symode_amd.dataset import get_dataset
    from symode_amd.evaluation import score_coefficients, truth_table
    from symode_amd.parser_utils import get_args
    from symode_amd.sindy import stlsq_bag_from_gram
    from symode_amd.sweep import inclusion_milli, resample_grams, seeded_subsamples
    from tests.stlsq_cases import host_sweep
    total = {t: 0 for t in LADDER}
    for cfg in CONFIGS:
        args = vars(get_args(argv=["--config", cfg]))
        train, _, args = get_dataset(args)
        order, sine, exp = args["poly_order"], args["include_sine"], args["include_exp"]
        x, dx = train.x.cpu(), train.dx.cpu()
        d = x.shape[1]
        A = torch.cat([O.theta(x, order, sine, exp).double(), dx.double()], 1).numpy()
        p = A.shape[1] - d
        m = int(x.shape[0] * args["lbfgs_subsample"])
        L = m // C
        idx = seeded_subsamples(x.shape[0], m, list(range(S)), "cpu").numpy()
        truth = truth_table(args["task"], p, sine, exp)
        w, thr, passes = float(np.float32(args["w_sindy_reg"])), float(np.float32(args["threshold"])), max(1, args["num_epochs"])
        seeds = [1_000_003 * s for s in range(S)]
        G = np.stack([A[idx[s]].T @ A[idx[s]] for s in range(S)])
        chunk = np.stack([[A[idx[s, c * L:(c + 1) * L]].T @ A[idx[s, c * L:(c + 1) * L]] for c in range(C)] for s in range(S)])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = host_sweep(G, d, w, thr, passes, n_points=m)
            rep, _ = resample_grams(chunk, seeds, B)
            fits = host_sweep(rep, d, w, thr, passes, n_points=C * L)
        plain_ok = sum(bool(score_coefficients(plain[0][s], plain[1][s], truth)[3]) for s in range(S))
        ok, sizes, valid = {t: 0 for t in LADDER}, {t: [] for t in LADDER}, []
        for s in range(S):
            rows = slice(s * B, (s + 1) * B)
            for t in LADDER:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    Xi, mask, rec = stlsq_bag_from_gram(G[s], fits[0][rows], fits[1][rows], fits[4][rows], inclusion_milli(t)[0], w, d, m)
                ok[t] += bool(score_coefficients(Xi, mask, truth)[3])
                sizes[t].append(int(mask.sum()))
            valid.append(rec["valid"])
        print(f"{cfg}: d = {d}, p = {p}, {S} seeds x {m} of {x.shape[0]} points, B = {B} replicas of C = {C} chunks x {L} rows, "
              f"w_sindy_reg {args['w_sindy_reg']}, threshold {args['threshold']}, valid replicas {min(valid)}-{max(valid)}")
        print(f"   threshold fit     : success {plain_ok}/{S}   support size {int(plain[1].sum(axis=(1, 2)).min())}-"
              f"{int(plain[1].sum(axis=(1, 2)).max())} (truth {int((truth != 0).sum())})")
        for t in LADDER:
            total[t] += ok[t]
            print(f"   inclusion {t:<7}: success {ok[t]}/{S}   support size {min(sizes[t])}-{max(sizes[t])}", flush=True)
    best = max(LADDER, key=lambda t: (total[t], t))                     # ties go to the larger value
    print("summed over the configs: " + ", ".join(f"{t}: {total[t]}" for t in LADDER) + f"   -> default --bag_inclusion {best}")


if __name__ == "__main__":
    main()
