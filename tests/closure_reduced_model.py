"""fp64 numpy model of the closure reduced to a quadratic form in the fit's variables (csrc/closure_reduced.hpp: symode_quad_reduce,
symode_quad_step), built on tests/closure_quad_model.py, one problem at a time.

    z = (beta, const), K = r + d_c numbers;   P z = (view(Q beta) + const on column 0) * mask on the live columns
    g(W) = 2 inv (W Gtt - Gty^T + w_sym T(W)) * mask on the live columns     (closure_quad_model's gradient, W NOT rounded to fp32)
    column i of H = 1/2 P^T (g(P e_i) - g(0)),   h = -1/2 P^T g(0),   c0 = inv tr(Gyy)
    B = 1/2 (B0 + B0^T),  B0 = [[H, -h], [-h^T, c0]]       (quad_reduce)
    loss = v^T B v,  d loss / d z = 2 (B v)[:K],  v = [z; 1]   (quad_step)
Nothing is rounded to fp32: the tests add the roundings to their tolerances."""
import numpy as np

from tests.closure_quad_model import map_grad
from tests.test_host_fold_gram_model import gram_term

# The largest deviation of this model from the fp64 point-wise closure that tests/test_host_closure_reduced_model.py measured over
# its cases, as a fraction of each output's scale (profiles/closure_reduced.txt: loss 7.7e-15, gradient by beta 3.4e-15, by
# const 6.5e-16; against the closure without a point loop on un-rounded coefficients 9.7e-16, 1.1e-15, 2.0e-16), the worst of
# them rounded up: the "fp64 reordering term" of the GPU tolerances, as closure_quad_model.REORDER is.
REORDER_REDUCED = 2e-14


def quad_closure64(A, M, J, W, mask, live, w_sym, inv):
    """closure_quad_model.quad_closure on fp64 coefficients W (d, p) that are NOT rounded to fp32 first:
    (mse, reg, loss, grad (d, p))"""
    A, M, J = (np.asarray(a, dtype=np.float64) for a in (A, M, J))
    d = J.shape[0]
    p = A.shape[0] - d
    live = np.asarray(live, dtype=bool)
    mk = np.ones((d, p)) if mask is None else np.asarray(mask, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64) * mk * live
    Gtt, Gty, Gyy = A[:p, :p], A[:p, p:], A[p:, p:]
    ssr = (W * (W @ Gtt)).sum() - 2.0 * (W * Gty.T).sum() + np.trace(Gyy)
    value, wT = gram_term(J, M, Gtt, W, None, live, float(w_sym))
    grad = 2.0 * inv * (W @ Gtt - Gty.T + wT) * mk * live
    mse, reg = inv * ssr, inv * value
    return mse, reg, mse + float(w_sym) * reg, grad


def map_xi64(Q, z, d, p, use_kron, allow_constant=True):
    """Xi (d, p) in fp64 from z = [beta; const] (const present iff allow_constant): the map without its rounding to fp32"""
    Q = np.asarray(Q, dtype=np.float64)
    r = Q.shape[1]
    z = np.asarray(z, dtype=np.float64)
    flat = Q @ z[:r]
    Xi = flat.reshape(d, p).copy() if use_kron else flat.reshape(p, d).T.copy()
    if allow_constant:
        Xi[:, 0] += z[r:r + d]
    return Xi


def map_grad64(Q, grad, use_kron, allow_constant=True):
    """P^T grad as one vector [g_beta; g_const] in fp64"""
    gb, gc = map_grad(Q, grad, use_kron, allow_constant)
    return gb if gc is None else np.concatenate([gb, gc])


def quad_reduce(A, M, J, Q, use_kron, allow_constant, mask, live, w_sym, inv):
    """B (K+1, K+1) in fp64 by the K + 1 states e_0 .. e_{K-1}, 0, as the kernel walks them"""
    A = np.asarray(A, dtype=np.float64)
    d = np.asarray(J).shape[0]
    p = A.shape[0] - d
    K = np.asarray(Q).shape[1] + (d if allow_constant else 0)

    def ptg(z):
        return map_grad64(Q, quad_closure64(A, M, J, map_xi64(Q, z, d, p, use_kron, allow_constant), mask, live, w_sym, inv)[3],
                          use_kron, allow_constant)
    g0 = ptg(np.zeros(K))
    B = np.zeros((K + 1, K + 1))
    for i in range(K):
        B[:K, i] = 0.5 * (ptg(np.eye(K)[i]) - g0)
    B[:K, K] = 0.5 * g0
    B[K, :K] = 0.5 * g0
    B[K, K] = inv * np.trace(A[p:, p:])
    return 0.5 * (B + B.T)


def quad_step(B, z):
    """(loss, d loss / d z (K,)) in fp64 from B (K+1, K+1) and z (K,)"""
    v = np.concatenate([np.asarray(z, dtype=np.float64), [1.0]])
    a = np.asarray(B, dtype=np.float64).T @ v
    return float(v @ a), 2.0 * a[:-1]
