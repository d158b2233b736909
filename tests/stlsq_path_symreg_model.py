"""csrc/stlsq_path_symreg.hpp in numpy, statement by statement, with no GPU in it: fp64 for the system, the solve and the
scores, fp32 where the kernel rounds (gamma, w_sym, the coefficients, the elimination's compare), the same order of sums -- so
that the GPU test can expect equal bytes while it asserts derived bounds.  The system is tests.stlsq_symreg_model.build_system
(the two kernels share stlsqs_pass_solve); the solve is tests.stlsq_constrained_model.solve with its rank-one update written
as one array statement (one product and one subtraction per entry, as there: the same bits, which the CPU test checks)."""
import numpy as np

from tests.stlsq_path_model import rss
from tests.stlsq_symreg_model import PIVOT_FLOOR, U32, U64, build_system, f32, support, xi_bound  # noqa: F401


def solve(A, c, pivot_floor):
    """csrc/stlsq_joint.hpp: pivoted Cholesky with fused forward substitution, back substitution; None at a flagged pivot."""
    n = len(c)
    A, c = A.copy(), c.copy()
    orig, dg = np.arange(n), A.diagonal().copy()
    first = 0.0
    for kk in range(n):
        jp = kk + int(np.argmax(dg[kk:]))                       # largest remaining diagonal, the lowest position of equals
        if jp != kk:
            orig[[kk, jp]] = orig[[jp, kk]]
            dg[[kk, jp]] = dg[[jp, kk]]
            c[[kk, jp]] = c[[jp, kk]]
        if kk == 0:
            first = dg[0]
        if not dg[kk] > pivot_floor * first or not dg[kk] > 0.0:
            return None
        r, jo, rest = np.sqrt(dg[kk]), orig[kk], orig[kk + 1:]
        R = A[jo, rest] / r
        A[jo, rest] = R
        A[jo, jo] = r
        A[np.ix_(rest, rest)] -= np.multiply.outer(R, R)
        q = c[kk] / r
        c[kk + 1:] -= R * q
        dg[kk + 1:] -= R * R
        c[kk] = q
    for i in range(n - 1, -1, -1):
        acc = c[i]
        prod = A[orig[i], orig[i + 1:]] * c[i + 1:]
        for t in range(len(prod)):
            acc -= prod[t]
        c[i] = acc / A[orig[i], orig[i]]
    w = np.zeros(n)
    w[orig] = c
    return w


def mse(H, d, p, active, w64):
    """stlsqps_mse: from 0.0, rows ascending, each row's term stlsq_path_rss."""
    e = 0.0
    for j in range(d):
        e += rss(H, p, j, np.nonzero(active[j])[0], w64[j])
    return e


def form(R, flat, v):
    """stlsqps_form: q_b over the support ascending from 0.0, r_b = v_b q_b, then the r_b ascending from 0.0."""
    r = []
    for b in flat:
        q = 0.0
        for a in flat:
            q += R[b, a] * v[a]
        r.append(v[b] * q)
    e = 0.0
    for x in r:
        e += x
    return e


def smallest(active, av):
    """stlsq_path_smallest over the flat index: (index, |v|) of the smallest fp32 |v|, the lowest index of equals."""
    idx = np.nonzero(active)[0]
    k = idx[int(np.argmin(av[idx]))]
    return int(k), av[k]


def select(ev, vyy, n0, tol, floor_rel):
    """The kernel's selection: lanes t < n0 hold ev[t], the empty model's error is vyy itself."""
    e_min = vyy
    for t in range(n0):
        if ev[t] < e_min:
            e_min = ev[t]
    cut = (1.0 + tol) * (e_min if e_min > 0.0 else 0.0) + floor_rel * vyy
    ok = [t for t in range(n0) if ev[t] <= cut]
    return (n0 if (vyy <= cut or not ok) else ok[-1]), cut


def chain(G, R, V, d, gamma, w_sym, near_band, pivot_floor=PIVOT_FLOOR, trace=None):
    """Steps t = 0 .. d p of one problem (everything of the kernel but the selection, which alone reads tol): a dict of
    path_xi (n0+1, d, p) fp32, order (n0,), mse_train, reg_train, mse_val (n0+1,), near, fell, rem (n0,).  gamma and w_sym
    are rounded to fp32 here, as the entry rounds them.  ``trace`` receives (active (d, p), A, b, sel) per step with a solve."""
    gamma, w_sym = f32(gamma), f32(w_sym)
    p = G.shape[0] - d
    n0 = d * p
    o = dict(path_xi=np.zeros((n0 + 1, d, p), dtype=np.float32), order=np.zeros(n0, dtype=np.int32), mse_train=np.zeros(n0 + 1),
             reg_train=np.zeros(n0 + 1), mse_val=np.zeros(n0 + 1), near=0, fell=0, rem=np.full(n0, -1))
    active = np.ones((d, p), dtype=bool)
    for t in range(n0 + 1):
        sel = support(active)
        xi = np.zeros((d, p), dtype=np.float32)
        if sel:
            A, b = build_system(G, R, d, gamma, w_sym, sel)
            w = solve(A, b, pivot_floor)
            if w is None:
                o['fell'] = 1
                return o
            if trace is not None:
                trace.append((active.copy(), A, b, sel))
            for (j, k), v in zip(sel, w):
                xi[j, k] = np.float32(v)
        o['path_xi'][t] = xi
        w64 = xi.astype(np.float64)
        flat = np.nonzero(active.reshape(-1))[0]
        o['mse_train'][t] = mse(G, d, p, active, w64)
        o['reg_train'][t] = form(R, flat, w64.reshape(-1))
        o['mse_val'][t] = mse(V, d, p, active, w64)
        if sel:
            av = np.abs(xi).reshape(-1)
            fa = active.reshape(-1).copy()
            out, lo = smallest(fa, av)
            if len(sel) > 1:
                fa[out] = False
                _, up = smallest(fa, av)
                o['near'] += int(np.float64(up) - np.float64(lo) < near_band)
            o['order'][t] = out
            o['rem'][out] = t
            active[out // p, out % p] = False
    return o


def path(G, R, V, d, gamma, w_sym, tol, floor_rel, near_band, pivot_floor=PIVOT_FLOOR, trace=None, chained=None):
    """stlsq_path_symreg_kernel for one problem: G (p+d, p+d), R (d p, d p), V (p+d, p+d).  A dict of the entry's outputs
    (Xi, mask, best beside ``chain``'s); a problem that fell keeps zeros there (unspecified by the entry).  ``chained``: the
    result of ``chain`` on the same arguments, to select on it again with another tol."""
    p = G.shape[0] - d
    n0 = d * p
    o = dict(chain(G, R, V, d, gamma, w_sym, near_band, pivot_floor, trace) if chained is None else chained)
    o.update(Xi=np.zeros((d, p), dtype=np.float32), mask=np.zeros((d, p), dtype=bool), best=n0)
    if o['fell']:
        return o
    vyy = 0.0
    for j in range(d):
        vyy += V[p + j, p + j]
    best, _ = select(o['mse_val'], vyy, n0, tol, floor_rel)
    m = (o['rem'] >= best).reshape(d, p)
    xi = np.zeros((d, p), dtype=np.float32)
    sel = support(m)
    if sel:
        A, b = build_system(G, R, d, f32(gamma), f32(w_sym), sel)
        for (j, k), v in zip(sel, solve(A, b, pivot_floor)):
            xi[j, k] = np.float32(v)
    o.update(Xi=xi, mask=m, best=best)
    return o
