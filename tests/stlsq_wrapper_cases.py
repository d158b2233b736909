"""Synthetic operands for what the six engine.stlsq_* wrappers share (tests/test_gpu_stlsq_wrappers.py): S = 3 sets of
G = A^T A from 40 random rows, a validation matrix, a PSD R, Q from a random orthonormal basis with r = 2, and a grid of 6
problems behind a table.  ``modelled_fell`` runs the numpy models of the kernels on them: the GPU test compares real fits only
if none of them flags a problem (tests/test_host_stlsq_wrapper_cases.py)."""
import numpy as np

S, GRID, ROWS, R_FREE = 3, 6, 40, 2
SHAPES = ((1, 3), (2, 3))                       # (d, p)
N_POINTS, MAX_ITER, BAND, TOL, FLOOR_REL = ROWS, 10, 1e-4, 0.02, 1e-10
GAMMA, THRESHOLD, W_SYM = 0.1, 1e-3, 1.0
PIVOT_FLOOR, RCOND = 1e-14, 1e-7
# the table of the grid, one row per problem: problem s on set s % S
GAMMAS = [0.1, 0.1, 0.1, 0.3, 0.3, 0.3]
THRESHOLDS = [1e-3, 2e-3, 1e-3, 2e-3, 1e-3, 2e-3]
W_SYMS = [1.0, 1.0, 0.5, 0.5, 2.0, 2.0]


def operands(d, p, allow_constant):
    """dict(G (S, p+d, p+d), V (1, p+d, p+d), R (S, d p, d p), q_solve (d p, r') fp64, q_xi (d p, r) fp32)"""
    rng = np.random.RandomState(1000 * d + 10 * p + int(allow_constant))
    A = rng.standard_normal((S, ROWS, p + d))
    Av = rng.standard_normal((1, ROWS, p + d))
    B = rng.standard_normal((S, ROWS // 2, d * p))
    q = np.linalg.qr(rng.standard_normal((d * p, R_FREE)))[0]
    q_solve = q
    if allow_constant:                          # d unit columns behind Q: column r + j holds its 1 in row j p (CoefMap.solve_matrix)
        q_solve = np.concatenate([q, np.zeros((d * p, d))], axis=1)
        for j in range(d):
            q_solve[j * p, R_FREE + j] = 1.0
    T = lambda M: np.ascontiguousarray(np.swapaxes(M, 1, 2) @ M)                       # noqa: E731
    return dict(G=T(A), V=T(Av), R=T(B), q_solve=np.ascontiguousarray(q_solve), q_xi=np.ascontiguousarray(q.astype(np.float32)))


def f32(v):
    return float(np.float32(v))


def modelled_fell(d, p, allow_constant):
    """{wrapper: the ``fell`` flags the numpy model of its kernel gives, scalar call then grid}"""
    from tests import stlsq_cases, stlsq_constrained_model, stlsq_minnorm_model, stlsq_path_model, stlsq_path_symreg_model, \
        stlsq_symreg_model
    o = operands(d, p, allow_constant)
    G, V, R, qs, qx = o["G"], o["V"], o["R"], o["q_solve"], o["q_xi"]
    scalar = [(s, GAMMA, THRESHOLD, W_SYM) for s in range(S)]
    grid = [(s % S, GAMMAS[s], THRESHOLDS[s], W_SYMS[s]) for s in range(GRID)]
    both = scalar + grid
    return {
        "stlsq_sweep": [stlsq_cases.per_row_sweep(G[k][None], d, f32(g), f32(t), MAX_ITER, BAND)[-1][0] for k, g, t, _ in both],
        "stlsq_sweep_constrained": [stlsq_constrained_model.sweep(G[k], d, f32(g), f32(t), MAX_ITER, qs, qx, allow_constant, BAND,
                                                                  PIVOT_FLOOR)["fell"] for k, g, t, _ in both],
        "stlsq_sweep_minnorm": [stlsq_minnorm_model.sweep(G[k], d, f32(g), f32(t), MAX_ITER, qs, qx, allow_constant, BAND, RCOND)["fell"]
                                for k, g, t, _ in both],
        "stlsq_sweep_symreg": [stlsq_symreg_model.sweep(G[k], R[k], d, g, t, w, MAX_ITER, BAND, PIVOT_FLOOR)["fell"] for k, g, t, w in both],
        "stlsq_path": list(stlsq_path_model.path(G, V, d, GAMMA, TOL, FLOOR_REL, BAND, GRID)["fell"]),
        "stlsq_path_symreg": [stlsq_path_symreg_model.path(G[k], R[k], V[0], d, f32(g), f32(w), TOL, FLOOR_REL, BAND, PIVOT_FLOOR)["fell"]
                              for k, g, _, w in both],
    }
