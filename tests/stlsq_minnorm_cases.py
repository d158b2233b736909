"""The cases of the rank-revealing device sweep's tests, with no GPU in it: tests/stlsq_constrained_cases.py's deck read for
the other purpose -- the problems that entry FLAGS are the ones this mode is for.  The smallest shapes at which each part can
go wrong:
  rankdef     so2_o3_cc1 on ``rankdef_gram`` (d = 2, p = 10, r' = 4): pass 1 of rank 4, pass 2 with n = 4 and rank 2;
  FLAGGED     negdet_o2_cc1, so3a_o2 (d = 3), so3a_o2_cc: up to four passes, three of them truncated, ranks 1 .. 7;
  dup64       the lane limit with a deficiency: 40 orthonormal columns followed by exact copies of the first 24 (d = 2, p = 41,
              n = 64 and rank 40 on both passes), data as ``orthonormal_case``;
  zero        an all-zero matrix: rank 0, Xi = 0, a mask that empties;
  FULL        three SOLVED deck names and r64, full rank on every pass: the mode must then be the existing entry.
``python -m tests.stlsq_minnorm_cases`` prints per pass what tests/test_host_stlsq_minnorm_model.py asserts."""
import functools

import numpy as np
import torch

from symode_amd.coef_map import CoefMap
from tests import stlsq_constrained_cases as C

THRESHOLD, GAMMAS, MAX_ITERS, BAND, COND_BOUND, N_POINTS = C.THRESHOLD, C.GAMMAS, C.MAX_ITERS, C.BAND, C.COND_BOUND, C.N_POINTS
FLAGGED = C.FLAGGED
FULL = ("negdet_o3_cc0", "scaling2_o2_cc0", "so2_o3_cc1", "r64")
TRUNCATED = ("rankdef",) + FLAGGED + ("dup64",)
ALL = TRUNCATED + ("zero",) + FULL
# n -> rank per pass at THRESHOLD, gamma 0 (an empty support: (0, 0))
RANKS = {"rankdef": [(4, 4), (4, 2)],
         "negdet_o2_cc1": [(2, 2), (2, 1), (0, 0), (0, 0)],
         "so3a_o2": [(11, 11), (8, 7), (7, 5), (7, 4)],
         "so3a_o2_cc": [(8, 8), (8, 7), (7, 6)],
         "dup64": [(64, 40), (64, 40)],
         "zero": [(4, 0), (0, 0)]}


@functools.lru_cache(maxsize=None)
def dup64():
    """(G, coef): Q = 40 orthonormal columns and exact copies of the first 24 behind them."""
    d, p, r = 2, 41, 40
    rng = np.random.RandomState(5)
    Q = np.linalg.qr(rng.randn(d * p, r))[0].astype(np.float32)
    coef = CoefMap(d, p, torch.from_numpy(np.concatenate([Q, Q[:, :24]], axis=1)), True, False)
    A = rng.randn(600, p + d)
    A[:, 0] = 1.0
    beta = rng.uniform(0.5, 1.5, coef.r) * rng.choice([-1.0, 1.0], coef.r)
    beta[::3] *= 0.02
    xi = coef.xi(beta.astype(np.float32), np.full(d, 0.7, dtype=np.float32)).astype(np.float64)
    A[:, p:] = A[:, :p] @ xi.T + C.NOISE * rng.randn(600, d)
    return A.T @ A, coef


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(G (p+d, p+d) fp64, CoefMap) of a case."""
    if key == "rankdef":
        return C.rankdef_gram(), C.coef_map("so2_o3_cc1")
    if key == "dup64":
        return dup64()
    if key == "zero":
        return np.zeros((12, 12)), C.coef_map("so2_o3_cc1")
    if key == "r64":
        return C.orthonormal_case()
    return C.gram(key)[0], C.coef_map(key)


if __name__ == "__main__":
    from tests import stlsq_minnorm_model as M
    for key in ALL:
        G, coef = inputs(key)
        qs, qx = C.matrices(coef)
        for gamma in GAMMAS:
            trace = []
            out = M.sweep(G, coef.d, gamma, THRESHOLD, 10, qs, qx, coef.allow_constant, band=BAND, trace=trace)
            print(key, "gamma", gamma, "passes", out["passes"], "near", out["near"], "fell", out["fell"], "trunc", out["trunc"], "rank",
                  out["rank"])
            for t in trace:
                info = t[5]
                n, rank, R = info["n"], info["rank"], info["R"]
                line = f"   n {n} fact {info['fact']} rank {rank}"
                if 0 < rank < n:
                    dropped = abs(R[rank, rank]) if rank < info["fact"] else 0.0
                    line += (f" dropped/cut {dropped / (M.RCOND * abs(R[0, 0])):.3g} kept/R00 {abs(R[rank - 1, rank - 1]) / abs(R[0, 0]):.3g}"
                             f" cond {M.truncated_cond(info):.3g}")
                print(line)
