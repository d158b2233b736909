"""The rank-revealing mode of the constrained device sweep (symode_stlsq_sweep_minnorm, the MINNORM branch of
csrc/stlsq_constrained.hpp) restated in numpy, statement by statement and with no GPU in it.  Columns, system and Xi are
tests/stlsq_constrained_model.py's; what is added is the factorisation without the pivot floor, xGELSY's rank loop over
xLAIC1 estimates, the truncated minimum-norm solve and the loop around them -- the same operations in the same order, so
the GPU test can expect equal bytes while it asserts the bound derived below."""
import numpy as np

from symode_amd import lstsq as L
from tests.stlsq_constrained_model import U32, U64, build_system, effective_columns, xi_of

RCOND = L.SINGULAR_RCOND                 # what the sweep passes: the cut on the triangular factor


def factor(A, c):
    """The kernel's pivoted Cholesky with the fused forward substitution and NO pivot floor: a pivot that is not > 0 ends it.
    Returns (R (n, n) in pivot-position order, upper triangular, rows fact.. zero; q (n) the forward substitution (entries
    fact.. are not part of it); orig, the pivot order; fact)."""
    n = len(c)
    A, c = A.copy(), c.copy()
    orig, dg = list(range(n)), [A[t, t] for t in range(n)]
    fact = n
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
            fact = kk
            break
        r, jo = np.sqrt(dg[kk]), orig[kk]
        Rt = np.zeros(n)
        for t in range(kk + 1, n):
            Rt[t] = A[jo, orig[t]] / r
            A[jo, orig[t]] = Rt[t]
        A[jo, jo] = r
        for a in range(kk + 1, n):
            for t in range(kk + 1, n):
                A[orig[a], orig[t]] -= Rt[a] * Rt[t]
        q = c[kk] / r
        for t in range(kk + 1, n):
            c[t] -= Rt[t] * q
            dg[t] -= Rt[t] * Rt[t]
        c[kk] = q
    R = np.zeros((n, n))
    for a in range(fact):
        for t in range(a, n):
            R[a, t] = A[orig[a], orig[t]]
    return R, c, orig, fact


def _laic1(job, alpha, sest, gamma):
    """lstsq._laic1 on an alpha that is already summed (its x^T w is then the product alpha * 1, which is exact)."""
    return L._laic1(job, np.array([alpha]), sest, np.array([1.0]), gamma)


def rank_of(R, fact, rcond):
    """xGELSY's loop (host_lstsq.cpp's driver 0): alpha summed in ascending position order."""
    n = R.shape[0]
    if fact == 0:
        return 0
    smax = smin = abs(R[0, 0])
    xmin, xmax = np.zeros(n), np.zeros(n)
    xmin[0] = xmax[0] = 1.0
    rank = 1
    while rank < n:
        gam = R[rank, rank] if rank < fact else 0.0
        amin = amax = 0.0
        for i in range(rank):
            amin += xmin[i] * R[i, rank]
            amax += xmax[i] * R[i, rank]
        sminpr, s1, c1 = _laic1(2, amin, smin, gam)
        smaxpr, s2, c2 = _laic1(1, amax, smax, gam)
        if not smaxpr * rcond <= sminpr:
            break
        xmin[:rank] *= s1
        xmax[:rank] *= s2
        xmin[rank], xmax[rank] = c1, c2
        smin, smax = sminpr, smaxpr
        rank += 1
    return rank


def back_substitution(R, q):
    n = len(q)
    y = q.copy()
    for i in range(n - 1, -1, -1):
        acc = y[i]
        for t in range(i + 1, n):
            acc -= R[i, t] * y[t]
        y[i] = acc / R[i, i]
    return y


def min_norm(R, q, rank):
    """Y = Wm^T (Wm Wm^T)^-1 q[:rank], Wm = R[:rank, :], in the kernel's (= the host's) order; None where a diagonal of the
    factor of Wm Wm^T is not > 0."""
    n = R.shape[0]
    M = np.zeros((rank, rank))
    for a in range(rank):
        for b in range(rank):
            acc = 0.0
            for t in range(a, n):
                acc += R[a, t] * (R[b, t] if b <= t else 0.0)
            M[a, b] = acc
    Lc = np.zeros((rank, rank))
    for b in range(rank):
        acc = np.zeros(rank)
        for a in range(b, rank):
            acc[a] = M[a, b]
            for t in range(b):
                acc[a] -= Lc[a, t] * Lc[b, t]
        if not acc[b] > 0.0:
            return None
        lbb = np.sqrt(acc[b])
        for a in range(b, rank):
            Lc[a, b] = lbb if a == b else acc[a] / lbb
    z = q[:rank].copy()
    for i in range(rank):
        acc = z[i]
        for t in range(i):
            acc -= Lc[i, t] * z[t]
        z[i] = acc / Lc[i, i]
    for i in range(rank - 1, -1, -1):
        acc = z[i]
        for t in range(i + 1, rank):
            acc -= Lc[t, i] * z[t]
        z[i] = acc / Lc[i, i]
    Y = np.zeros(n)
    for t in range(n):
        acc = 0.0
        for a in range(rank):
            acc += (R[a, t] if a <= t else 0.0) * z[a]
        Y[t] = acc
    return Y


def solve(Gq, cq, rcond=RCOND):
    """One pass's solve: (w (n) in the order of the effective columns or None when flagged, info) with info = dict(n, fact, rank,
    R, q, orig)."""
    n = len(cq)
    R, q, orig, fact = factor(Gq, cq)
    rank = rank_of(R, fact, rcond)
    info = dict(n=n, fact=fact, rank=rank, R=R, q=q, orig=orig)
    if rank == n:
        Y = back_substitution(R, q)
    elif rank > 0:
        Y = min_norm(R, q, rank)
        if Y is None:
            return None, info
    else:
        Y = np.zeros(n)
    w = np.zeros(n)
    for t in range(n):
        w[orig[t]] = Y[t]
    return w, info


def truncated_cond(info):
    """cond(R11)^2 cond(Wm Wm^T) of a truncated pass (1 at rank 0)."""
    rank, R = info["rank"], info["R"]
    if rank == 0:
        return 1.0
    Wm = R[:rank, :]
    return float(np.linalg.cond(R[:rank, :rank]) ** 2 * np.linalg.cond(Wm @ Wm.T))


def pass_cond(info, Gq):
    """The condition number the bounds take: cond(Gq) of a full-rank pass, ``truncated_cond`` of a truncated one."""
    if info["n"] == 0:
        return 1.0
    return float(np.linalg.cond(Gq)) if info["rank"] == info["n"] else truncated_cond(info)


def var_bound(var32, cond, n):
    """Bound on |var - exact| per variable for a TRUNCATED pass, in the form of stlsq_constrained_model.var_bound with cond(Gq)
    replaced by kappa = cond(R11)^2 cond(Wm Wm^T).  The minimum-norm solution is Y = Wm^T (Wm Wm^T)^-1 R11^-T c1 with
    Wm = [R11 R12] the first `rank` rows of the Cholesky factor in the pivot order, a function of G11, G12 and c1 alone.  Its
    computation is three backward-stable steps in fp64 (Higham, Accuracy and Stability): the factor rows (thm 10.3:
    R^T R = G + dG, |dG| <= (n + 1) u |R^T| |R|), whose effect on R11 is amplified by cond(G11) = cond(R11)^2 (Sun's bound on the
    Cholesky factor, Higham 10.8); the two triangular solves with R11^T inside the factor loop and with the factor of Wm Wm^T
    (thm 8.5: n u cond each, and cond(R11) <= cond(R11)^2, cond(Lc)^2 = cond(Wm Wm^T)); and the Cholesky solve of Wm Wm^T (thm
    10.4: about 3 n^2 u cond(Wm Wm^T) normwise).  To first order the relative errors add; each of the factors cond(R11)^2 and
    cond(Wm Wm^T) is >= 1, so their sum -- and the n-term products that form Wm Wm^T and Wm^T z, (n + 1) u each -- is below
    their product times the number of steps, and 4 n^2 kappa 2^-53 max|var| covers it with the constant of thm 10.4 rounded up
    exactly as the full-rank bound rounds it.  Plus the rounding of the variable to fp32."""
    v = np.abs(np.asarray(var32, dtype=np.float64))
    return 4.0 * max(n, 1) ** 2 * cond * U64 * (v.max() if v.size else 0.0) + U32 * v + np.finfo(np.float64).tiny


def xi_bound(q_xi, var32, cond, n, d, p, allow_constant):
    """Bound on |Xi - exact| per entry (d, p) of a truncated pass: ``var_bound``'s solve term mapped through |q_xi| (and 1 for
    the constant), plus the fp32 steps of stlsq_constrained_model.xi_bound, which are the same steps."""
    q = np.abs(np.asarray(q_xi, dtype=np.float64))
    r = q.shape[1]
    v = np.abs(np.asarray(var32, dtype=np.float64))
    solve_ = 4.0 * max(n, 1) ** 2 * cond * U64 * (v.max() if v.size else 0.0)
    mag = (q @ v[:r]).reshape(d, p)
    through = q.sum(axis=1).reshape(d, p)
    if allow_constant:
        mag[:, 0] += v[r:r + d]
        through[:, 0] += 1.0
    return solve_ * through + (len(v) + 2) * U32 * mag + np.finfo(np.float64).tiny


def one_pass(G, d, gamma, q_solve, q_xi, allow_constant, mask, rcond=RCOND):
    """One pass on ``mask`` (d, p) bool: (Xi (d, p) fp32 or None when flagged, var (r') fp32, Gq, cq, cols, info)."""
    p = G.shape[0] - d
    r = q_xi.shape[1]
    cols = effective_columns(q_solve, mask)
    var = np.zeros(q_solve.shape[1], dtype=np.float32)
    Gq, cq = build_system(G, d, gamma, q_solve, mask, cols)
    info = dict(n=0, fact=0, rank=0, R=np.zeros((0, 0)), q=np.zeros(0), orig=[])
    if cols:
        w, info = solve(Gq, cq, rcond)
        if w is None:
            return None, var, Gq, cq, cols, info
        var[cols] = w.astype(np.float32)
    return xi_of(var, np.asarray(q_xi, dtype=np.float32), d, p, r, allow_constant), var, Gq, cq, cols, info


def sweep(G, d, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, band=1e-4, rcond=RCOND, trace=None):
    """The kernel's loop for one problem; gamma and threshold as the launch holds them.  Returns dict(xi, var, mask, passes,
    near, fell, trunc, rank); ``trace``: a list that receives (mask before the pass, Xi, Gq, cq, cols, info) per pass."""
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    xi = np.zeros((d, p), dtype=np.float32)
    var = np.zeros(q_solve.shape[1], dtype=np.float32)
    near, passes, fell, trunc, rank = 0, 0, 0, 0, 0
    for it in range(max_iter):
        passes = it + 1
        out = one_pass(G, d, gamma, q_solve, q_xi, allow_constant, mask, rcond)
        info = out[5]
        rank = info["rank"]
        if info["rank"] < info["n"]:
            trunc += 1
        if out[0] is None:
            fell = 1
            break
        xi, var = out[0], out[1]
        if trace is not None:
            trace.append((mask.copy(),) + out[:1] + out[2:])
        av = np.abs(xi)
        near += int((mask & (np.abs(av.astype(np.float64) - threshold) < band)).sum())
        new = mask & (av > np.float32(threshold))
        changed = bool((new != mask).any())
        mask = new
        if not changed:
            break
    return dict(xi=xi, var=var, mask=mask, passes=passes, near=near, fell=fell, trunc=trunc, rank=rank)
