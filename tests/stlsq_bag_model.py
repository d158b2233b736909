"""numpy model of ``symode_stlsq_bag``, written from what include/symode.h documents at that entry, not from the kernel, and
knowing nothing of waves or LDS: statistics term by term in Python floats (fp64) in the documented order, the inclusion rule in
Python integers, the refit as a DENSE solve (numpy.linalg.solve on the support's ridge system) rounded to fp32.  Also the inputs
the GPU and the CPU tests of the entry share."""
import math

import numpy as np

COND_BOUND = 1e6            # what the bound on the refit rests on (tests/test_gpu_stlsq_device.py derives it)


def statistics(rep_xi, rep_mask, rep_fell):
    """(count (d, p) int32, valid, mean, std (d, p) fp64) of one seed's replicas (B, d, p)"""
    B, d, p = rep_xi.shape
    ok = [b for b in range(B) if rep_fell[b] == 0]
    count, mean, std = np.zeros((d, p), dtype=np.int32), np.zeros((d, p)), np.zeros((d, p))
    for j in range(d):
        for k in range(p):
            xs = [float(rep_xi[b, j, k]) for b in ok if rep_mask[b, j, k]]
            count[j, k] = len(xs)
            if xs:
                total = 0.0
                for x in xs:
                    total = total + x
                mean[j, k] = total / len(xs)
                ss = 0.0
                for x in xs:
                    ss = ss + (x - mean[j, k]) * (x - mean[j, k])
                std[j, k] = math.sqrt(ss / len(xs))
    return count, len(ok), mean, std


def bag(G, rep_xi, rep_mask, rep_fell, tau, gamma):
    """All problems of a launch.  G (S, p+d, p+d), rep_* (S B, ...), tau (n_problems,) thousandths, problem s on seed s % S.
    Returns dict(xi (n_problems, d, p) fp32, mask uint8, fell int32 (a support whose system is not positive definite), count
    (S, d, p) int32, valid (S,) int32, mean, std (S, d, p) fp64)."""
    S = G.shape[0]
    B, d, p = rep_xi.shape[0] // S, rep_xi.shape[1], rep_xi.shape[2]
    stats = [statistics(rep_xi[k * B:(k + 1) * B], rep_mask[k * B:(k + 1) * B], rep_fell[k * B:(k + 1) * B]) for k in range(S)]
    n = len(tau)
    xi, mask, fell = np.zeros((n, d, p), dtype=np.float32), np.zeros((n, d, p), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    for s in range(n):
        k = s % S
        count, valid = stats[k][0], stats[k][1]
        Gtt = G[k, :p, :p] + gamma * gamma * np.eye(p)
        for j in range(d):
            sel = [c for c in range(p) if valid > 0 and 1000 * int(count[j, c]) >= int(tau[s]) * valid]
            mask[s, j, sel] = 1
            if sel:
                A = Gtt[np.ix_(sel, sel)]
                try:
                    np.linalg.cholesky(A)
                except np.linalg.LinAlgError:
                    fell[s] = 1
                    continue
                xi[s, j, sel] = np.linalg.solve(A, G[k, sel, p + j]).astype(np.float32)
    return dict(xi=xi, mask=mask, fell=fell, count=np.stack([t[0] for t in stats]),
                valid=np.array([t[1] for t in stats], dtype=np.int32), mean=np.stack([t[2] for t in stats]),
                std=np.stack([t[3] for t in stats]))


def statistic_bounds(rep_xi, rep_mask, B, std):
    """How far mean and std of a launch may lie from the model's, per seed-term, derived from the arithmetic: both add the same
    <= B fp64 terms in the same order, so the sums agree to the last bit unless the device's division or square root rounds
    differently from the host's (either is within 1 ulp).  Not relying on that: a sum of B terms of size <= X = max |x| carries
    at most (B - 1) u X, the division one more rounding, so |mean - mean'| <= (B + 1) 2^-52 X.  std is the 2-norm of (x - mean)
    / sqrt(count), so a shift of the mean moves it by at most that shift (triangle inequality), and its own B + 2 roundings
    (subtract, square, B adds, divide, root) by at most (B + 4) 2^-52 std: |std - std'| <= mean bound + (B + 4) 2^-52 std."""
    S = std.shape[0]
    X = np.abs(np.where(rep_mask != 0, rep_xi, 0).astype(np.float64)).reshape(S, B, *std.shape[1:]).max(axis=1)
    mean_bound = (B + 1) * 2.0 ** -52 * X
    return mean_bound, mean_bound + (B + 4) * 2.0 ** -52 * std


def row_bound(xi):
    """spacing(fp32(max |Xi| over the row)): tests/test_gpu_stlsq_device.py's bound on a coefficient of an fp64 solve rounded
    once to fp32, for n <= 64 unknowns and cond <= COND_BOUND"""
    return np.spacing(np.abs(xi).max(axis=-1, keepdims=True).astype(np.float32)).astype(np.float64)


def random_grams(S, d, p, n_rows=400, seed=0, noise=0.05):
    """(S, p+d, p+d) fp64 augmented Gram matrices of random well-conditioned data with a sparse truth, and that truth"""
    rng = np.random.RandomState(seed)
    th = rng.randn(S, n_rows, p)
    xi = np.zeros((S, d, p))
    for s in range(S):
        for j in range(d):
            cols = rng.choice(p, size=min(3, p), replace=False)
            xi[s, j, cols] = rng.uniform(0.5, 1.5, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))
    y = np.einsum("snp,sjp->snj", th, xi) + noise * rng.randn(S, n_rows, d)
    a = np.concatenate([th, y], axis=2)
    return np.einsum("sna,snb->sab", a, a), xi


def random_replicas(S, B, d, p, seed=0, keep=0.6, n_fell=0):
    """replica outputs that no fit produced: random fp32 coefficients, a random mask (a term kept in ~``keep`` of the
    replicas, some in all, some in none) and ``n_fell`` flagged replicas per seed"""
    rng = np.random.RandomState(seed + 100)
    xi = (rng.randn(S * B, d, p) * 10.0 ** rng.uniform(-2, 1, size=(S * B, d, p))).astype(np.float32)
    share = rng.choice([0.0, keep, 1.0], size=(S, 1, d, p), p=[0.2, 0.6, 0.2])
    mask = (rng.uniform(size=(S, B, d, p)) < share).reshape(S * B, d, p).astype(np.uint8)
    fell = np.zeros((S, B), dtype=np.int32)
    for k in range(S):
        fell[k, rng.choice(B, size=min(n_fell, B), replace=False)] = 1
    return xi, mask, fell.reshape(-1)
