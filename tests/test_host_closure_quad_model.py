"""tests/closure_quad_model.py (the fp64 numpy model of the closure without a point loop) against the fp64 point-wise closure:
oracle.theta and oracle.symreg_reversed_precomputed in float64 on the same points, autograd for the gradient, Xi from the fp64
map rounded once to fp32 as the kernel rounds it.

S = 3 problems of n = 1030 points of the damped oscillator with noise 0.2 (the residual is then no cancellation to round-off
of the three terms of the quadratic form), orders 1-5, the dense library with free coefficients and the so2 constraint's map
with its live set, masked and unmasked, w_sym 0 and 0.37.

The bound: both sides are fp64.  The model's mse is a sum of three traces of magnitude kappa * (n d mse), kappa =
(|tr(W Gtt W^T)| + 2 |tr(W Gty)| + tr(Gyy)) / sum r^2; each trace is a (p+d)-term dot product of (p+d)-term dot products, and
the matrices themselves are n-term sums, so with gamma_k = k 2^-53 the deviation is at most about (n + 2 (p + d)) 2^-53 kappa
of the result; the point-wise side adds its own n-term mean.  The test asserts 4 (n + 2 (p + d)) 2^-53 kappa of each output's
scale -- 4.9e-13 kappa at order 5 -- and prints what it measured; the worst figures are recorded in profiles/closure_quad.txt
and closure_quad_model.REORDER, which the GPU test adds to its fp32 roundings."""
import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from symode_amd.coef_map import CoefMap
from symode_amd.constraint import constraint_Q
from tests.closure_quad_model import cancellation, exact_m, map_grad, map_xi, quad_closure
from tests.test_host_fold_gram_model import fitted_m

D, S, N_ICS, N_STEPS, NOISE = 2, 3, 10, 103, 0.2
SO2 = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
CASES = [(order, so2, masked, w) for order in (1, 2, 3, 4, 5) for so2 in (False, True) for masked in (False, True) for w in (0.0, 0.37)]


def problems(order, seed, n_problems=S):
    """n_problems problems: x, dx (n, 2) fp32 with noise, a rotation J each (an fp32 matrix), its M, the augmented matrix in fp64"""
    rng = np.random.RandomState(seed)
    out = []
    for s in range(n_problems):
        xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(N_ICS, rng), 0.02, N_STEPS)
        x = xs.reshape(-1, D).astype(np.float64)
        dx = dxs.reshape(-1, D).astype(np.float64)
        x = (x + NOISE * x.std(0) * rng.randn(*x.shape)).astype(np.float32)
        dx = (dx + NOISE * dx.std(0) * rng.randn(*dx.shape)).astype(np.float32)
        t = 0.01 + 0.3 * rng.rand()
        J = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]).astype(np.float32).astype(np.float64)
        M = exact_m(J, O.term_exponents(D, order))
        B = np.concatenate([O.theta(torch.from_numpy(x).double(), order).numpy(), dx.astype(np.float64)], axis=1)
        out.append((x, dx, J, M, B.T @ B))
    return out


def pointwise(x, dx, J, xi32, mask, order, w):
    """(mse, reg, loss, dloss/dXi) of one problem, fp64, point by point"""
    x, dx, Jt = torch.from_numpy(x).double(), torch.from_numpy(dx).double(), torch.from_numpy(J)
    mk = torch.ones(xi32.shape, dtype=torch.float64) if mask is None else torch.from_numpy(mask).double()
    xi = torch.from_numpy(xi32).double().requires_grad_(True)

    def h(z):
        return O.theta(z, order) @ (xi * mk).T
    mse = torch.mean((h(x) - dx) ** 2)
    sym = O.symreg_reversed_precomputed(x, [x @ Jt.T], [Jt.expand(x.shape[0], D, D)], h)
    loss = mse + w * sym
    g, = torch.autograd.grad(loss, xi)
    return mse.item(), sym.item(), loss.item(), g.numpy()


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_exact_m_is_the_fitted_one(order):
    rng = np.random.RandomState(order)
    J = np.eye(D) + 0.3 * rng.randn(D, D)
    assert np.abs(exact_m(J, O.term_exponents(D, order)) - fitted_m(J, order, rng)).max() < 1e-10


@pytest.mark.parametrize("order,so2,masked,w", CASES)
def test_model_against_the_pointwise_fp64_closure(order, so2, masked, w):
    p = O.term_count(D, order)
    n = N_ICS * N_STEPS
    assert n == 1030
    rng = np.random.RandomState(1000 * order + 100 * so2 + 10 * masked + int(w > 0))
    w32 = float(np.float32(w))
    inv = 1.0 / (n * D)
    if so2:
        Q, use_kron = constraint_Q([SO2], D, order)
        cmap = CoefMap(D, p, Q, use_kron, True)
        live = cmap.live_columns().any(axis=0)
        Qn = Q.numpy().astype(np.float32)
    else:
        live = np.ones(p, dtype=bool)
    worst = {}
    for s, (x, dx, J, M, A) in enumerate(problems(order, 7 * order + 1)):
        mask = (rng.rand(D, p) > 0.25).astype(np.float32) if masked else None
        if so2:
            beta, const = (rng.randn(Qn.shape[1]) * 0.3).astype(np.float32), (rng.randn(D) * 0.1).astype(np.float32)
            xi = map_xi(Qn, beta, const, D, p, use_kron)
        else:
            xi = (rng.randn(D, p) * 0.3).astype(np.float32)
        mse, reg, loss, grad = quad_closure(A, M, J, xi, mask, live, w32, inv)
        # the point-wise closure knows no live set: it gets the coefficients with the dead columns cleared, and its gradient
        # is compared on the live ones
        rm, rr, rl, rg = pointwise(x, dx, J, xi * live, mask, order, w32)
        rg = rg * live
        kappa = cancellation(A, xi, mask, live)
        tol = 4.0 * (n + 2 * (p + D)) * 2.0 ** -53 * kappa
        pairs = {"mse": (mse, rm), "reg": (reg, rr), "loss": (loss, rl), "grad": (grad, rg)}
        if so2:
            gb, gc = map_grad(Qn, grad, use_kron)
            rb, rc = map_grad(Qn, rg, use_kron)
            pairs.update({"g_beta": (gb, rb), "g_const": (gc, rc)})
        for name, (got, want) in pairs.items():
            scale = max(np.abs(want).max(), np.abs(rg).max() if name.startswith("g") else 0.0)
            dev = np.abs(np.asarray(got) - np.asarray(want)).max() / scale
            worst[name] = max(worst.get(name, 0.0), dev)
            assert dev <= tol, (name, s, dev, tol, kappa)
        assert (grad[:, ~live] == 0).all()
    print(f"closure_quad model: order={order} so2={so2} masked={masked} w={w} kappa<={kappa:.3g} tol={tol:.2e} "
          + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
