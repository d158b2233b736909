"""The per-pass algorithm of symode_stlsq_sweep_constrained (csrc/stlsq_constrained.hpp) restated in numpy, with no GPU in it:
the same operations in the same order -- fp64 loops for the system and the solve, fp32 where the kernel rounds -- so that the
GPU test can expect equal bytes while it asserts a derived bound, and the CPU tests can pin the algorithm itself against
``solve_SINDy_one_step`` and against an extended-precision solve."""
import numpy as np

PIVOT_FLOOR = 1e-7 ** 2                  # lstsq.SINGULAR_RCOND ** 2, what the sweep passes


def effective_columns(q_solve, mask):
    """The columns of q_solve (d p, r') with a non-zero entry in a row the mask keeps, ascending (the host's sindy.py:284)."""
    rows = np.nonzero(mask.reshape(-1))[0]
    return [c for c in range(q_solve.shape[1]) if np.any(q_solve[rows, c] != 0.0)]


def build_system(G, d, gamma, q_solve, mask, cols):
    """Gq (n, n), cq (n) in the kernel's order: for j, active k ascending, u_b = sum over active l ascending, Gq[a, b] for
    a <= b, the lower triangle mirrored."""
    p = G.shape[0] - d
    n = len(cols)
    g2 = gamma * gamma
    Gq, cq = np.zeros((n, n)), np.zeros(n)
    for j in range(d):
        act = np.nonzero(mask[j])[0]
        for k in act:
            u = np.zeros(n)
            for l in act:
                g = G[k, l] + (g2 if k == l else 0.0)
                for b in range(n):
                    u[b] += g * q_solve[j * p + l, cols[b]]
            qk = q_solve[j * p + k, cols]
            cq += qk * G[k, p + j]
            for a in range(n):
                Gq[a, a:] += qk[a] * u[a:]
    for b in range(n):
        Gq[b, :b] = Gq[:b, b]
    return Gq, cq


def solve(A, c, pivot_floor):
    """tests.stlsq_cases.row_solve with the kernel's pivot floor: None at a pivot that is not > pivot_floor * (first pivot)."""
    n = len(c)
    A, c = A.copy(), c.copy()
    orig, dg = list(range(n)), [A[t, t] for t in range(n)]
    first = 0.0
    for kk in range(n):
        jp = kk
        for t in range(kk + 1, n):                           # largest remaining diagonal, the lowest position of equals
            if dg[t] > dg[jp]:
                jp = t
        if jp != kk:
            orig[kk], orig[jp] = orig[jp], orig[kk]
            dg[kk], dg[jp] = dg[jp], dg[kk]
            c[kk], c[jp] = c[jp], c[kk]
        if kk == 0:
            first = dg[0]
        if not dg[kk] > pivot_floor * first or not dg[kk] > 0.0:
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


def xi_of(var32, q_xi, d, p, r, allow_constant):
    """Xi[j, k] = sum over c ascending of q_xi[j p + k, c] beta32[c] in fp32, + const32[j] at k = 0."""
    xi = np.zeros(d * p, dtype=np.float32)
    for c in range(r):
        xi = (xi + (q_xi[:, c] * var32[c]).astype(np.float32)).astype(np.float32)
    xi = xi.reshape(d, p)
    if allow_constant:
        xi[:, 0] = (xi[:, 0] + var32[r:r + d]).astype(np.float32)
    return xi


U64, U32 = 2.0 ** -53, 2.0 ** -24


def var_bound(var32, cond, n):
    """Bound on |var - exact| per variable: the fp64 Cholesky solve of an n x n system is backward stable, its normwise
    forward error at most 4 n^2 cond 2^-53 max|var| (Higham, Accuracy and Stability, thm 10.4 with the constant rounded up),
    plus the rounding of the variable to fp32."""
    v = np.abs(np.asarray(var32, dtype=np.float64))
    return 4.0 * max(n, 1) ** 2 * cond * U64 * (v.max() if v.size else 0.0) + U32 * v + np.finfo(np.float64).tiny


def xi_bound(q_xi, var32, cond, n, d, p, allow_constant):
    """Bound on |Xi - exact| per entry (d, p): the solve's error mapped through |q_xi| (and 1 for the constant), plus the
    fp32 steps -- the variables' rounding, r products and r + 1 additions per entry: (r' + 2) 2^-24 (|q_xi| |beta32| + |const32|)."""
    q = np.abs(np.asarray(q_xi, dtype=np.float64))
    r = q.shape[1]
    v = np.abs(np.asarray(var32, dtype=np.float64))
    solve = 4.0 * max(n, 1) ** 2 * cond * U64 * (v.max() if v.size else 0.0)
    mag = (q @ v[:r]).reshape(d, p)
    through = q.sum(axis=1).reshape(d, p)
    if allow_constant:
        mag[:, 0] += v[r:r + d]
        through[:, 0] += 1.0
    return solve * through + (len(v) + 2) * U32 * mag + np.finfo(np.float64).tiny


def one_pass(G, d, gamma, q_solve, q_xi, allow_constant, mask, pivot_floor=PIVOT_FLOOR):
    """One pass on ``mask`` (d, p) bool: (Xi (d, p) fp32, var (r') fp32, Gq, cq, cols), or None for a flagged pivot."""
    p = G.shape[0] - d
    r = q_xi.shape[1]
    cols = effective_columns(q_solve, mask)
    var = np.zeros(q_solve.shape[1], dtype=np.float32)
    Gq, cq = build_system(G, d, gamma, q_solve, mask, cols)
    if cols:
        w = solve(Gq, cq, pivot_floor)
        if w is None:
            return None
        var[cols] = w.astype(np.float32)
    return xi_of(var, np.asarray(q_xi, dtype=np.float32), d, p, r, allow_constant), var, Gq, cq, cols


def sweep(G, d, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, band=1e-4, pivot_floor=PIVOT_FLOOR, trace=None):
    """The kernel's loop for one problem.  gamma and threshold as the launch holds them (the caller rounds to fp32 where a
    table would).  Returns dict(xi, var, mask, passes, near, fell); ``trace``: a list that receives (mask before the pass,
    Xi, Gq, cq, cols) per pass."""
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    xi = np.zeros((d, p), dtype=np.float32)
    var = np.zeros(q_solve.shape[1], dtype=np.float32)
    near, passes, fell = 0, 0, 0
    for it in range(max_iter):
        passes = it + 1
        out = one_pass(G, d, gamma, q_solve, q_xi, allow_constant, mask, pivot_floor)
        if out is None:
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
    return dict(xi=xi, var=var, mask=mask, passes=passes, near=near, fell=fell)
