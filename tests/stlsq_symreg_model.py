"""The per-pass algorithm of symode_stlsq_sweep_symreg (csrc/stlsq_symreg.hpp) restated in numpy, with no GPU in it: the same
operations in the same order -- fp64 for the system and the solve, fp32 where the kernel rounds -- so that the GPU test can
expect equal bytes while it asserts a derived bound, and the CPU test can pin the algorithm itself against a dense solve.
The solve is the one statement the constrained kernel's model has (tests/stlsq_constrained_model.solve), as the two kernels
share csrc/stlsq_joint.hpp."""
import numpy as np

from tests.stlsq_constrained_model import PIVOT_FLOOR, U32, U64, solve  # noqa: F401  (PIVOT_FLOOR: what the sweep passes)


def f32(v):
    """The value as the launch holds it: gamma, threshold and w_sym arrive in fp32, with or without a table."""
    return float(np.float32(v))


def support(mask):
    """The entries (j, k) the mask keeps, in ascending (j, k)."""
    return [(int(j), int(k)) for j, k in zip(*np.nonzero(mask))]


def build_system(G, R, d, gamma, w_sym, sel):
    """A (n, n), b (n) in the kernel's order: for a <= b the bracket [j_a == j_b] (Gtt + gamma^2 [k_a == k_b]) first (an exact
    0.0 across rows), then the one addition of the one product w_sym R; the lower triangle mirrored."""
    p = G.shape[0] - d
    n = len(sel)
    g2 = gamma * gamma
    A, b = np.zeros((n, n)), np.zeros(n)
    for a, (ja, ka) in enumerate(sel):
        for c in range(a, n):
            jb, kb = sel[c]
            block = G[ka, kb] + (g2 if ka == kb else 0.0) if ja == jb else 0.0
            A[a, c] = block + w_sym * R[ja * p + ka, jb * p + kb]
    for c in range(n):
        A[c, :c] = A[:c, c]
        b[c] = G[sel[c][1], p + sel[c][0]]
    return A, b


def xi_bound(v32, cond, n):
    """Bound on |Xi - exact| per entry: the fp64 Cholesky solve of an n x n system is backward stable, its normwise forward
    error at most 4 n^2 cond 2^-53 max|v| (Higham, Accuracy and Stability, thm 10.4 with the constant rounded up), plus the
    rounding of the coefficient to fp32 -- tests/stlsq_constrained_model.xi_bound without the map through q_xi."""
    v = np.abs(np.asarray(v32, dtype=np.float64))
    return 4.0 * max(n, 1) ** 2 * cond * U64 * (v.max() if v.size else 0.0) + U32 * v + np.finfo(np.float64).tiny


def one_pass(G, R, d, gamma, w_sym, mask, pivot_floor=PIVOT_FLOOR):
    """One pass on ``mask`` (d, p) bool: (Xi (d, p) fp32, A, b, sel), or None for a flagged pivot."""
    p = G.shape[0] - d
    sel = support(mask)
    xi = np.zeros((d, p), dtype=np.float32)
    A, b = build_system(G, R, d, gamma, w_sym, sel)
    if sel:
        w = solve(A, b, pivot_floor)
        if w is None:
            return None
        for (j, k), v in zip(sel, w):
            xi[j, k] = np.float32(v)
    return xi, A, b, sel


def sweep(G, R, d, gamma, threshold, w_sym, max_iter, band=1e-4, pivot_floor=PIVOT_FLOOR, trace=None):
    """The kernel's loop for one problem; gamma, threshold and w_sym are rounded to fp32 here, as the entry rounds them.
    Returns dict(xi, mask, passes, near, fell); ``trace``: a list that receives (mask before the pass, Xi, A, b, sel) per pass."""
    gamma, threshold, w_sym = f32(gamma), f32(threshold), f32(w_sym)
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    xi = np.zeros((d, p), dtype=np.float32)
    near, passes, fell = 0, 0, 0
    for it in range(max_iter):
        passes = it + 1
        out = one_pass(G, R, d, gamma, w_sym, mask, pivot_floor)
        if out is None:
            fell = 1
            break
        xi = out[0]
        if trace is not None:
            trace.append((mask.copy(),) + out)
        av = np.abs(xi)
        near += int((mask & (np.abs(av.astype(np.float64) - threshold) < band)).sum())
        new = mask & (av > np.float32(threshold))
        changed = bool((new != mask).any())
        mask = new
        if not changed:
            break
    return dict(xi=xi, mask=mask, passes=passes, near=near, fell=fell)
