"""The deck of the sparsity-path tests, with no GPU in it, and the dense fp64 reference they are held against.

Library cases reuse tests/stlsq_cases.py: where that module holds a shape (orders 3 and 5 at d = 2, order 2 + exp at d = 3) the
training matrices are its ``gram_cpu`` and the truth its ``points``; orders 2 and 2 + exp at d = 2 are drawn here by the same
recipe (its ``theta``, N_POINTS, NOISE).  Every library case gets a held-out matrix from SEPARATE rows with the same truth.
Then random positive-definite pairs at p = 64, p = 1, p = 2, a diagonal matrix with two bit-equal coefficients and a row
whose right-hand side is zero.  ``python -m tests.stlsq_path_cases`` prints the conditions test_host_stlsq_path_model.py
asserts for every case and step; the seeds below were chosen with it (a draw that fails a condition is replaced, not excused).
"""
import functools

import numpy as np
import torch

from tests import stlsq_cases as C

BAND = 1e-4                       # near_band of every launch (sindy.NEAR_THRESHOLD_BAND)
FLOOR_REL = 1e-10                 # solve_path's default
TOL_DEFAULT = 0.02                # main_sweep's --path_tol default (profiles/stlsq_path.txt)
GAMMAS = (0.0, 0.1)
TOLS = (0.0, TOL_DEFAULT)
COND_BOUND = 1e6
DECIDED_BY = 100.0                # every elimination and every comparison behind `best` is decided by this many bounds
N_VAL = 100                       # held-out rows per set
U53, U24 = 2.0 ** -53, 2.0 ** -24


def _library_rows(shape, xi, n_rows, rng):
    """(n_sets, n_rows, p + d) rows [Theta(x) | dx] in fp64 of fresh points under the truth xi (n_sets, d, p), C.points' recipe."""
    d, order, flags = shape
    n_sets = xi.shape[0]
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (n_sets, n_rows, d)).astype(np.float32))
    th = C.theta(x.reshape(-1, d), order, flags).double().numpy().reshape(n_sets, n_rows, -1)
    dx = (np.einsum('snp,sjp->snj', th, xi) + C.NOISE * rng.randn(n_sets, n_rows, d)).astype(np.float32).astype(np.float64)
    return np.concatenate([th, dx], axis=2)


def _truth(shape, p, rng):
    """C.points' truth: two coefficients of size 0.5 .. 1.5 per row, one of 0.13 in set 1, the last row of set 2 zero."""
    d = shape[0]
    xi = np.zeros((C.N_SETS, d, p))
    for s in range(C.N_SETS):
        for j in range(d):
            cols = rng.choice(p, size=min(2, p), replace=False)
            xi[s, j, cols] = rng.uniform(0.5, 1.5, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))
    if p > 2:
        xi[1, 0, rng.choice(np.nonzero(xi[1, 0] == 0)[0])] = 0.13
    xi[2, d - 1] = 0.0
    return xi


def _library_case(shape, seed):
    d, order, flags = shape
    rng = np.random.RandomState(seed)
    if shape in C.SEEDS:
        G, xi = C.gram_cpu(shape), C.points(shape)[2]
    else:
        p = C.theta(torch.zeros(1, d), order, flags).shape[1]
        xi = _truth(shape, p, rng)
        rows = _library_rows(shape, xi, C.N_POINTS, rng)
        G = np.einsum('sna,snb->sab', rows, rows)
    rows = _library_rows(shape, xi, N_VAL, rng)
    return G, np.einsum('sna,snb->sab', rows, rows), xi != 0


def _random_pd(p, d, n_sets, seed, n_rows=400, noise=0.05):
    """[B | Y]^T [B | Y] for Gaussian B (n_rows, p), Y = B xi + noise with three coefficients of size 0.5 .. 1.5 per row; the
    held-out pair from 200 further rows.  cond(B^T B) ~ 5 at p = 64."""
    rng = np.random.RandomState(seed)
    xi = np.zeros((n_sets, d, p))
    for s in range(n_sets):
        for j in range(d):
            cols = rng.choice(p, size=min(3, p), replace=False)
            xi[s, j, cols] = rng.uniform(0.5, 1.5, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))
    out = []
    for n in (n_rows, n_rows // 2):
        B = rng.randn(n_sets, n, p)
        rows = np.concatenate([B, np.einsum('snp,sjp->snj', B, xi) + noise * rng.randn(n_sets, n, d)], axis=2)
        out.append(np.einsum('sna,snb->sab', rows, rows))
    return out[0], out[1], xi != 0


def _diagonal_tie():
    """A diagonal system (p = 4, d = 1) whose columns 1 and 2 have bit-equal coefficients 0.25 = 0.5 / 2 = 1 / 4, the smallest:
    column 1 must leave first.  Every quotient is exact, at ridge 0; the ridge 0.1 breaks the tie and is not run here."""
    G = np.zeros((1, 5, 5))
    diag, c = np.array([1.0, 2.0, 4.0, 1.0]), np.array([1.0, 0.5, 1.0, 0.5])
    G[0, :4, :4], G[0, :4, 4], G[0, 4, :4], G[0, 4, 4] = np.diag(diag), c, c, 2.0
    V = G.copy()
    V[0, 4, 4] = 2.5
    return G, V, None


def _zero_rhs():
    """Order 3 at d = 2 with the targets of row 1 set to zero in every set, training and held-out: that row's coefficients are
    exact zeros at every step (ties, the lowest index leaves first), every error is 0 and the empty model must win."""
    G, V, truth = _library_case((2, 3, 0), 11)
    G, V, truth = G.copy(), V.copy(), truth.copy()
    p = G.shape[1] - 2
    for H in (G, V):
        H[:, p + 1, :] = 0.0
        H[:, :, p + 1] = 0.0
    truth[:, 1] = False
    return G, V, truth


# The p = 64 cases run fewer (ridge, tol) pairs for the time the pure-Python model takes (2-3 s per run at d = 4), not for a failed
# draw: their conditions hold at every pair.
# name -> (d, builder, gammas, tols, exact ties allowed).  G (n_sets, p+d, p+d), V (n_val_sets, p+d, p+d), truth (n_sets, d, p) or None
DECK = {
    'o2': (2, lambda: _library_case((2, 2, 0), 2), GAMMAS, TOLS, False),
    'o3': (2, lambda: _library_case((2, 3, 0), 3), GAMMAS, TOLS, False),
    'o5': (2, lambda: _library_case((2, 5, 0), 3), GAMMAS, TOLS, False),
    'o2_exp': (2, lambda: _library_case((2, 2, C.FLAG_EXP), 1), GAMMAS, TOLS, False),
    'd3_o2_exp': (3, lambda: _library_case((3, 2, C.FLAG_EXP), 5), GAMMAS, TOLS, False),
    'pd_p64_d4': (4, lambda: _random_pd(64, 4, 1, 6), (0.1,), (TOL_DEFAULT,), False),
    'pd_p64_d1': (1, lambda: _random_pd(64, 1, 1, 7), GAMMAS, (0.0,), False),
    'p1': (2, lambda: _random_pd(1, 2, 3, 8), GAMMAS, TOLS, False),
    'p2': (1, lambda: _random_pd(2, 1, 3, 9), GAMMAS, TOLS, False),
    'diag_tie': (1, _diagonal_tie, (0.0,), TOLS, True),
    'zero_rhs': (2, _zero_rhs, GAMMAS, TOLS, True),
}
RUNS = [(name, g, t) for name, c in DECK.items() for g in c[2] for t in c[3]]


@functools.lru_cache(maxsize=None)
def case(name):
    d, build, _, _, ties = DECK[name]
    G, V, truth = build()
    return d, np.ascontiguousarray(G), np.ascontiguousarray(V), truth, ties


@functools.lru_cache(maxsize=None)
def model(name, gamma, tol):
    """tests/stlsq_path_model.py on a case: computed once, shared by the tests, never modified."""
    from tests import stlsq_path_model as M
    d, G, V, _, _ = case(name)
    return M.path(G, V, d, gamma, tol, FLOOR_REL, BAND)


def _quad(H, p, j, w):
    """Hyy - 2 w^T c + w^T H w in np.longdouble."""
    Hl, wl = H.astype(np.longdouble), w.astype(np.longdouble)
    return Hl[p + j, p + j] - 2 * (wl @ Hl[:p, p + j]) + wl @ Hl[:p, :p] @ wl


def err_bound(H, p, j, w):
    """(n + 2)^2 2^-53 (Hyy + 2 |w|^T |c| + |w|^T |H| |w|): n + 2 terms per sum, two nested sums."""
    n = int(np.count_nonzero(w))
    a = np.abs(w)
    return (n + 2) ** 2 * U53 * (abs(H[p + j, p + j]) + 2 * a @ np.abs(H[:p, p + j]) + a @ np.abs(H[:p, :p]) @ a)


@functools.lru_cache(maxsize=None)
def reference(name, gamma, tol):
    """The dense reference of a case: per support np.linalg.solve in fp64, elimination by |coefficient| (the lowest index of
    equals), v = (float) of the solution, errors of v in np.longdouble, the same selection rule.  Beside its answers it
    returns what the tests' bounds and conditions are made of, per (problem, row, step):
      cond       cond_2 of the step's system;
      coef_bound 4 n^2 cond 2^-53 |v|_max + 2^-24 |v| per coefficient (the solve's backward error times the condition number,
                 then the rounding to fp32);
      gap        runner-up |x| minus smallest |x| of the step, and its two coefficient bounds summed;
      val_bound  the error bound of rss_val at the step PLUS the first-order effect of the coefficient bounds on it,
                 sum_k |2 (V w - c)_k| coef_bound_k: two implementations within the coefficient bounds differ by no more;
      margin     per step |rss_val[t] - cut|, and the bound of that difference (val_bound[t] + (1 + tol) val_bound[argmin])."""
    d, G, V, _, _ = case(name)
    S, p = G.shape[0], G.shape[1] - d
    nv = V.shape[0]
    r = dict(order=np.zeros((S, d, p), dtype=np.int32), best=np.zeros((S, d), dtype=np.int32), mask=np.zeros((S, d, p), dtype=bool),
             x=np.zeros((S, d, p + 1, p)), rss_train=np.zeros((S, d, p + 1), dtype=np.longdouble),
             rss_val=np.zeros((S, d, p + 1), dtype=np.longdouble), cond=np.ones((S, d, p + 1)), coef_bound=np.zeros((S, d, p + 1, p)),
             gap=np.full((S, d, p), np.inf), gap_bound=np.zeros((S, d, p)), val_bound=np.zeros((S, d, p + 1)),
             margin=np.zeros((S, d, p + 1)), margin_bound=np.zeros((S, d, p + 1)))
    for s in range(S):
        Gs, Vs = G[s], V[s % nv]
        Gtt = Gs[:p, :p] + gamma * gamma * np.eye(p)
        for j in range(d):
            active = np.ones(p, dtype=bool)
            for t in range(p + 1):
                sel = np.nonzero(active)[0]
                n = len(sel)
                if n:
                    A = Gtt[np.ix_(sel, sel)]
                    r['x'][s, j, t, sel] = np.linalg.solve(A, Gs[sel, p + j])
                    r['cond'][s, j, t] = np.linalg.cond(A)
                x = r['x'][s, j, t]
                v = x.astype(np.float32).astype(np.float64)
                cb = np.where(active, 4 * n * n * r['cond'][s, j, t] * U53 * np.abs(x).max() + U24 * np.abs(x), 0.0)
                r['coef_bound'][s, j, t] = cb
                r['rss_train'][s, j, t], r['rss_val'][s, j, t] = _quad(Gs, p, j, v), _quad(Vs, p, j, v)
                r['val_bound'][s, j, t] = err_bound(Vs, p, j, v) + np.abs(2 * (Vs[:p, :p] @ v - Vs[:p, p + j])) @ cb
                if n:
                    ax = np.where(active, np.abs(x), np.inf)
                    out = int(np.argmin(ax))
                    if n > 1:
                        ax[out] = np.inf
                        up = int(np.argmin(ax))
                        r['gap'][s, j, t] = abs(x[up]) - abs(x[out])
                        r['gap_bound'][s, j, t] = cb[up] + cb[out]
                    r['order'][s, j, t] = out
                    active[out] = False
            ev = r['rss_val'][s, j]
            at = int(np.argmin(ev))
            cut = (1 + np.longdouble(tol)) * max(ev[at], 0) + np.longdouble(FLOOR_REL) * Vs[p + j, p + j]
            best = max(t for t in range(p + 1) if ev[t] <= cut)
            r['best'][s, j] = best
            r['mask'][s, j, r['order'][s, j, best:]] = True
            r['margin'][s, j] = np.abs(ev - cut).astype(np.float64)
            r['margin_bound'][s, j] = r['val_bound'][s, j] + (1 + tol) * r['val_bound'][s, j, at]
            r['margin_bound'][s, j, at] = 0.0          # the argmin passes its own cut whatever the rounding
    return r


def conditions(name, gamma, tol):
    """(largest cond, smallest gap / gap_bound over the eliminations that are no exact tie, number of exact ties, smallest
    margin / margin_bound over the comparisons with a non-zero bound, number of comparisons whose bound AND margin are 0)."""
    r = reference(name, gamma, tol)
    tie = r['gap'] == 0.0
    fin = np.isfinite(r['gap']) & ~tie
    with np.errstate(divide='ignore', invalid='ignore'):
        g = (r['gap'][fin] / r['gap_bound'][fin]).min() if fin.any() else np.inf
        live = r['margin_bound'] > 0
        m = (r['margin'][live] / r['margin_bound'][live]).min() if live.any() else np.inf
    return r['cond'].max(), g, int(tie.sum()), m, int(((r['margin_bound'] == 0) & (r['margin'] == 0)).sum())


if __name__ == "__main__":
    for name, gamma, tol in RUNS:
        cond, g, ties, m, exact = conditions(name, gamma, tol)
        r = reference(name, gamma, tol)
        truth = case(name)[3]
        on_truth = '-' if truth is None else str(bool(np.array_equal(r['mask'], truth)))
        print(f"{name:10s} gamma {gamma} tol {tol}: cond {cond:.3g}  gap/bound {g:.3g}  exact ties {ties}  margin/bound {m:.3g}  "
              f"exact-zero comparisons {exact}  best {r['best'].tolist()}  on the true support: {on_truth}")
