"""fp64 numpy model of the closure without a point loop (csrc/closure_quad.hpp, symode_loss_grad_reversed_linear_quad): the
kernel's formulae on the kernel's tables, one problem at a time.

    A = [Gtt Gty; Gty^T Gyy] = sum_n [Theta | dx]^T [Theta | dx]   (p+d, p+d), raw sums
    W = fl32(xi * mask) on the live columns
    mse  = inv (tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy))
    R    = W Gtt - Gty^T
    reg  = inv sum_j c_j Gtt c_j^T,  C = J W - W M;   T = (J - I)^T U - U (M - I)^T,  U = C Gtt     (gram_term)
    grad = 2 inv (R + w_sym T) * mask on the live columns,      loss = mse + w_sym reg
and the coefficient map: Xi = fl32(view(Q beta) + const on column 0), g_beta = vec(grad) Q, g_const = grad[:, 0].
Nothing is rounded to fp32 on the way out: the tests add the roundings to their tolerances."""
import numpy as np

from tests.test_host_fold_gram_model import gram_term

# The largest deviation of this model from the fp64 point-wise closure that tests/test_host_closure_quad_model.py measured over
# its cases, as a fraction of each output's scale (profiles/closure_quad.txt: mse and loss 7.1e-15, regulariser 1.8e-14,
# gradient by Xi 2.2e-15, by beta 1.2e-15, by const 4.4e-16), the worst of them rounded up: the "fp64 reordering term" of the GPU
# tolerances.  The residual's share grows with (|tr(W Gtt W^T)| + 2 |tr(W Gty)| + tr(Gyy)) / sum r^2, which the host test prints
# and bounds (at most 6.7 over its cases); the regulariser's with |W| / |C|, large for a group element close to the identity.
REORDER = 2e-14


def exact_m(J, exponents):
    """M (p, p) with Theta(J x) = M Theta(x) for the d = 2 monomials x^a y^b of ``exponents`` (oracle.term_exponents), by
    expanding (J00 x + J01 y)^a (J10 x + J11 y)^b: products of fp64 coefficient vectors, no fit."""
    J = np.asarray(J, dtype=np.float64)
    col = {tuple(e): k for k, e in enumerate(exponents)}
    M = np.zeros((len(exponents), len(exponents)))
    for k, (a, b) in enumerate(exponents):
        c = np.ones(1)                                     # c[i]: coefficient of x^i y^(degree - i)
        for _ in range(a):
            c = np.convolve(c, [J[0, 1], J[0, 0]])
        for _ in range(b):
            c = np.convolve(c, [J[1, 1], J[1, 0]])
        for i, v in enumerate(c):
            M[k, col[(i, a + b - i)]] = v
    return M


def map_xi(Q, beta, const, d, p, use_kron, allow_constant=True):
    """fp32 Xi (d, p) of one problem from the variables: Q (d p, r) fp32, beta (r,), const (d,) or None"""
    flat = np.asarray(Q, dtype=np.float64) @ np.asarray(beta, dtype=np.float64)
    Xi = flat.reshape(d, p).copy() if use_kron else flat.reshape(p, d).T.copy()
    if allow_constant and const is not None:
        Xi[:, 0] += np.asarray(const, dtype=np.float64).reshape(d)
    return Xi.astype(np.float32)


def map_grad(Q, grad, use_kron, allow_constant=True):
    """(g_beta (r,), g_const (d,) or None) in fp64 from the fp64 gradient by Xi"""
    g = grad if use_kron else grad.T
    return g.reshape(-1) @ np.asarray(Q, dtype=np.float64), (grad[:, 0].copy() if allow_constant else None)


def quad_closure(A, M, J, xi, mask, live, w_sym, inv):
    """(mse, reg, loss, grad (d, p)) in fp64.  A (p+d, p+d), M (p, p), J (d, d); xi fp32 (d, p); mask fp32 (d, p) or None;
    live (p,) bool; w_sym and inv as the launch gets them (w_sym an fp32 value)."""
    A, M, J = (np.asarray(a, dtype=np.float64) for a in (A, M, J))
    d = J.shape[0]
    p = A.shape[0] - d
    live = np.asarray(live, dtype=bool)
    xi = np.asarray(xi, dtype=np.float32)
    mk = np.ones((d, p), dtype=np.float32) if mask is None else np.asarray(mask, dtype=np.float32)
    W = (xi * mk).astype(np.float64) * live
    Gtt, Gty, Gyy = A[:p, :p], A[:p, p:], A[p:, p:]
    ssr = (W * (W @ Gtt)).sum() - 2.0 * (W * Gty.T).sum() + np.trace(Gyy)
    R = W @ Gtt - Gty.T
    value, wT = gram_term(J, M, Gtt, W, None, live, float(w_sym))
    grad = 2.0 * inv * (R + wT) * mk.astype(np.float64) * live
    mse, reg = inv * ssr, inv * value
    return mse, reg, mse + float(w_sym) * reg, grad


def cancellation(A, xi, mask, live):
    """(|tr(W Gtt W^T)| + 2 |tr(W Gty)| + tr(Gyy)) / (the residual's sum of squares): how many digits the three terms lose"""
    A = np.asarray(A, dtype=np.float64)
    d, p = xi.shape
    W = (np.asarray(xi, dtype=np.float32) * (1.0 if mask is None else np.asarray(mask, dtype=np.float32))).astype(np.float64) * live
    a, b, c = (W * (W @ A[:p, :p])).sum(), (W * A[:p, p:].T).sum(), np.trace(A[p:, p:])
    return (abs(a) + 2.0 * abs(b) + c) / (a - 2.0 * b + c)
