"""The regulariser of the fold closure from the library Gram matrix (closure_fold.hpp, FoldGram), restated in fp64 numpy:
    C = J W - W M,  W = Xi * mask on the live columns,      U = C G,  G = sum_n Theta(x_n) Theta(x_n)^T,
    sum_n |u_n|^2 = sum_jk C_jk U_jk,      T = (J - I)^T U - U (M - I)^T  (zero outside the live columns),
against the fp64 closure (oracle.symreg_reversed_precomputed on g(x) = J x, autograd).  M is not taken from the library's
construction but from a least-squares fit of Theta(J x) on Theta(x), so that the identity the term rests on is checked too.
``gram_term`` is what tests/test_gpu_closure_fold_gram.py holds the kernel to."""
import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O

D = 2


def gram_term(J, M, G, xi, mask, live, w_sym):
    """(sum_n |u_n|^2, w_sym * T) of one problem in fp64: J (d, d), M (p, p), G (p, p) raw sums, xi / mask (d, p), live (p,)
    bool.  Unscaled: the closure's regulariser is inv_count * value, its share of the gradient 2 inv_count * mask * w_sym T."""
    J, M, G = (np.asarray(a, dtype=np.float64) for a in (J, M, G))
    live = np.asarray(live, dtype=bool)
    W = np.asarray(xi, dtype=np.float64) * (1.0 if mask is None else np.asarray(mask, dtype=np.float64)) * live
    p = W.shape[1]
    # a dead column has a zero coefficient; its C is formed like any other (h(J x) has a share in that monomial)
    C = J @ W - W @ M
    U = C @ G
    T = (J - np.eye(D)).T @ U - U @ (M - np.eye(p)).T
    return float((C * U).sum()), w_sym * T * live


def fitted_m(J, order, rng):
    """M with Theta(J x) = M Theta(x), by fp64 least squares over a few hundred points; the fit residual is asserted"""
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (400, D)))
    th, thg = O.theta(x, order).numpy(), O.theta(x @ torch.from_numpy(J).T, order).numpy()
    A, *_ = np.linalg.lstsq(th, thg, rcond=None)
    assert np.abs(th @ A - thg).max() < 1e-12
    return A.T


CASES = [(order, rot, masked) for order in (1, 2, 3, 4, 5) for rot in (False, True) for masked in (False, True)]


@pytest.mark.parametrize("order,rot,masked", CASES)
def test_gram_term_against_the_fp64_closure(order, rot, masked):
    rng = np.random.RandomState(100 * order + 10 * rot + masked)
    p, n, w = O.term_count(D, order), 257, 0.37
    if rot:
        t = 0.3
        J = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    else:
        J = np.eye(D) + 0.3 * rng.randn(D, D)
    M = fitted_m(J, order, rng)
    x = torch.from_numpy(rng.randn(n, D) * 0.5)
    xi0 = rng.randn(D, p) * 0.3
    mask = (rng.rand(D, p) > 0.25).astype(np.float64) if masked else np.ones((D, p))
    th = O.theta(x, order).numpy()
    value, T = gram_term(J, M, th.T @ th, xi0, mask, np.ones(p, dtype=bool), w)

    xi = torch.from_numpy(xi0).requires_grad_(True)
    mk, Jt = torch.from_numpy(mask), torch.from_numpy(J)

    def h(z):
        return O.theta(z, order) @ (xi * mk).T
    sym = O.symreg_reversed_precomputed(x, [x @ Jt.T], [Jt.expand(n, D, D)], h)
    g, = torch.autograd.grad(w * sym, xi)
    inv = 1.0 / (n * D)
    assert abs(inv * value - sym.item()) <= 1e-10 * abs(sym.item())
    got = 2.0 * inv * mask * T
    assert np.abs(got - g.numpy()).max() <= 1e-10 * np.abs(g.numpy()).max()


def test_dead_columns_count_as_zero_coefficients():
    """a live set that is a union of whole degrees (constant + odd degrees at order 5): the term of the coefficients with the
    other columns cleared, and no gradient there"""
    rng = np.random.RandomState(3)
    order = 5
    p = O.term_count(D, order)
    deg = np.array([sum(e) for e in O.term_exponents(D, order)])
    live = (deg == 0) | (deg % 2 == 1)
    J = np.eye(D) + 0.3 * rng.randn(D, D)
    M = fitted_m(J, order, rng)
    th = O.theta(torch.from_numpy(rng.randn(100, D) * 0.5), order).numpy()
    G, xi = th.T @ th, rng.randn(D, p) * 0.3
    a = gram_term(J, M, G, xi, None, live, 1.0)
    b = gram_term(J, M, G, xi * live, None, np.ones(p, dtype=bool), 1.0)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
    assert np.abs(a[1] - b[1] * live).max() <= 1e-12 * np.abs(b[1]).max() and (a[1][:, ~live] == 0).all()
