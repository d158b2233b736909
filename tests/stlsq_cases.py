"""Inputs and the host reference of tests/test_gpu_stlsq_device.py, with no GPU in them: 3 sets of 200 random points in
[-1, 1]^d per library, targets from a sparse true Xi plus small noise, and symode_host_stlsq_sweep (driver 1, gels) on
whatever Gram matrices it is handed.  ``python -m tests.stlsq_cases`` prints, for Gram matrices formed on the CPU from the
oracle's Theta, the conditions the GPU test asserts on its inputs -- the generator seeds below were chosen with it."""
import functools

import numpy as np
import torch

from symode_amd import lstsq
from symode_amd.engine import FLAG_EXP, FLAG_SINE

N_SETS, N_POINTS = 3, 200
THRESHOLD, BAND, NOISE = 0.1, 1e-4, 0.02
GAMMAS = (0.0, 0.1)
MAX_ITERS = (1, 2, 10)
COND_BOUND = 1e6
# (d, order, flags): p = 2 the smallest, 10, 21, a flagged d = 3 library (exp: p = 13), and the largest compiled p (41)
SHAPES = ((1, 1, 0), (2, 3, 0), (2, 5, 0), (3, 2, FLAG_EXP), (3, 4, FLAG_SINE | FLAG_EXP))
# generator seed per shape: with it the host reports near == 0 and fell == 0 for every problem, gamma and max_iter
SEEDS = {(1, 1, 0): 0, (2, 3, 0): 0, (2, 5, 0): 0, (3, 2, FLAG_EXP): 0, (3, 4, FLAG_SINE | FLAG_EXP): 0}
# Where cond(Gtt) <= COND_BOUND cannot hold whatever the seed: sin and exp on [-1, 1] lie within ~1e-5 of the span of the
# polynomials up to order 4, so without a ridge the Gram matrix of the largest library has cond >= 5e10 (40 seeds tried:
# 5.0e10 .. 7.9e10).  The GPU test asserts that this IS the case there, and asserts everything else as for the other cases.
COND_UNATTAINABLE = {((3, 4, FLAG_SINE | FLAG_EXP), 0.0)}


def theta(x, order, flags):
    from oracle import sindy_oracle as O
    return O.theta(x, order, bool(flags & FLAG_SINE), bool(flags & FLAG_EXP))


@functools.lru_cache(maxsize=None)
def points(shape):
    """(x, dx) (N_SETS, N_POINTS, d) fp32 and the true Xi (N_SETS, d, p) of a shape.  Every row of the truth has two
    coefficients of size 0.5 .. 1.5; set 1 also holds one of 0.13, just above the threshold; the last row of set 2 is
    zero, so its support empties."""
    d, order, flags = shape
    rng = np.random.RandomState(1000 * SEEDS[shape] + 7)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (N_SETS, N_POINTS, d)).astype(np.float32))
    th = theta(x.reshape(-1, d), order, flags).double().numpy().reshape(N_SETS, N_POINTS, -1)
    p = th.shape[-1]
    xi = np.zeros((N_SETS, d, p))
    for s in range(N_SETS):
        for j in range(d):
            cols = rng.choice(p, size=min(2, p), replace=False)
            xi[s, j, cols] = rng.uniform(0.5, 1.5, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))
    if p > 2:
        xi[1, 0, rng.choice(np.nonzero(xi[1, 0] == 0)[0])] = 0.13
    xi[2, d - 1] = 0.0
    dx = np.einsum('snp,sjp->snj', th, xi) + NOISE * rng.randn(N_SETS, N_POINTS, d)
    return x, torch.from_numpy(dx.astype(np.float32)), xi


def gram_cpu(shape):
    """[Theta | dx]^T [Theta | dx] in fp64 from the oracle's fp32 Theta: what symode_aug_gram computes, up to summation order."""
    d, order, flags = shape
    x, dx, _ = points(shape)
    a = torch.cat([theta(x.reshape(-1, d), order, flags).reshape(N_SETS, N_POINTS, -1), dx], dim=2).double().numpy()
    return np.einsum('sna,snb->sab', a, a)


def host_sweep(G, d, gamma, threshold, max_iter, band=BAND, n_points=N_POINTS):
    """symode_host_stlsq_sweep(driver = 1) on G (S, p+d, p+d): Xi (S, d, p) fp32, mask bool, passes, near, fell."""
    lib = lstsq._native()
    assert lib, "libsymode_hip.so must be built for this test"
    G = np.ascontiguousarray(G, dtype=np.float64)
    S, p = G.shape[0], G.shape[1] - d
    xi, m8 = np.zeros((S, d, p), dtype=np.float32), np.ones((S, d, p), dtype=np.uint8)
    passes, near, fell = (np.zeros(S, dtype=np.int32) for _ in range(3))
    rc = lib.symode_host_stlsq_sweep(G.ctypes.data, S, d, p, int(n_points), float(gamma), float(threshold), int(max_iter), 1,
                                     float(band), xi.ctypes.data, m8.ctypes.data, passes.ctypes.data, near.ctypes.data,
                                     fell.ctypes.data)
    assert rc == 0, rc
    return xi, m8.astype(bool), passes, near, fell


def row_solve(A, c):
    """The kernel's solve of ONE equation row's system, statement by statement in numpy fp64 (csrc/stlsq.hpp): position t of
    the pivot order holds (orig, running diagonal, right-hand side), the factor's row replaces the pivot's row of A, forward
    substitution inside the factor loop, back substitution row by row.  None at a pivot that is not > 0."""
    n = len(c)
    A, c = A.copy(), c.copy()
    orig, dg = list(range(n)), [A[t, t] for t in range(n)]
    for kk in range(n):
        jp = kk
        for t in range(kk + 1, n):                           # largest remaining diagonal, the lowest position of equals
            if dg[t] > dg[jp]:
                jp = t
        if jp != kk:
            orig[kk], orig[jp] = orig[jp], orig[kk]
            dg[kk], dg[jp] = dg[jp], dg[kk]
            c[kk], c[jp] = c[jp], c[kk]
        if not dg[kk] > 0.0:
            return None
        r, jo = np.sqrt(dg[kk]), orig[kk]
        R = np.zeros(n)
        for t in range(kk + 1, n):
            R[t] = A[jo, orig[t]] / r
            A[jo, orig[t]] = R[t]
        A[jo, jo] = r
        for a in range(kk + 1, n):
            for t in range(kk + 1, n):
                A[orig[a], orig[t]] -= R[a] * R[t]
        q = c[kk] / r
        for t in range(kk + 1, n):
            c[t] -= R[t] * q
            dg[t] -= R[t] * R[t]
        c[kk] = q
    for i in range(n - 1, -1, -1):
        acc = c[i]
        for t in range(i + 1, n):
            acc -= A[orig[i], orig[t]] * c[t]
        c[i] = acc / A[orig[i], orig[i]]
    w = np.zeros(n)
    for t in range(n):
        w[orig[t]] = c[t]
    return w


def per_row_sweep(G, d, gamma, threshold, max_iter, band=BAND):
    """The kernel's loop in numpy: every equation row solved alone on its support (``row_solve``), the host's thresholding,
    the problem stopped when its whole (d, p) mask repeats.  Xi fp32, mask, passes, near, fell as ``host_sweep``."""
    S, p = G.shape[0], G.shape[1] - d
    xi, mask = np.zeros((S, d, p), dtype=np.float32), np.ones((S, d, p), dtype=bool)
    passes, near, fell = (np.zeros(S, dtype=np.int32) for _ in range(3))
    for s in range(S):
        Gtt = G[s, :p, :p] + np.where(np.eye(p) > 0, gamma * gamma, 0.0)
        Gty = G[s, :p, p:]
        for it in range(max_iter):
            changed = False
            for j in range(d):
                sel = np.nonzero(mask[s, j])[0]
                row = np.zeros(p)
                if len(sel):
                    w = row_solve(Gtt[np.ix_(sel, sel)], Gty[sel, j])
                    if w is None:
                        fell[s] = 1
                        break
                    row[sel] = w
                v = row.astype(np.float32)
                av = np.abs(v)
                near[s] += int((mask[s, j] & (np.abs(av.astype(np.float64) - threshold) < band)).sum())
                new = mask[s, j] & (av > np.float32(threshold))
                changed |= bool((new != mask[s, j]).any())
                xi[s, j], mask[s, j] = v, new
            passes[s] = it + 1
            if fell[s] or not changed:
                break
    return xi, mask, passes, near, fell


def conditions(G, d, gamma):
    """What the test asserts on its inputs: (largest cond(Gtt) over the sets, and per max_iter the host's outputs)."""
    p = G.shape[1] - d
    cond = max(np.linalg.cond(G[s, :p, :p] + gamma * gamma * np.eye(p)) for s in range(G.shape[0]))
    return cond, {m: host_sweep(G, d, gamma, THRESHOLD, m) for m in MAX_ITERS}


if __name__ == "__main__":
    for shape in SHAPES:
        G = gram_cpu(shape)
        for gamma in GAMMAS:
            cond, ref = conditions(G, shape[0], gamma)
            full = ref[MAX_ITERS[-1]]
            print(shape, "p", G.shape[1] - shape[0], "gamma", gamma, "cond %.3g" % cond, "passes", full[2].tolist(),
                  "near", [int(ref[m][3].sum()) for m in MAX_ITERS], "fell", [int(ref[m][4].sum()) for m in MAX_ITERS],
                  "empty rows", int((~full[1].any(axis=2)).sum()), "max |Xi| %.3g" % np.abs(full[0]).max())
