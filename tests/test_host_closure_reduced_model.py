"""tests/closure_reduced_model.py (the fp64 numpy model of quad_reduce / quad_step) against the fp64 point-wise closure and against
the closure without a point loop on un-rounded coefficients (closure_reduced_model.quad_closure64).

The cases of tests/test_host_closure_quad_model.py: S = 3 problems of n = 1030 points of the damped oscillator with noise 0.2,
orders 1-5, w_sym 0 and 0.37; the so2 constraint's map with its constants (K = r + 2) and "no map" -- Q the identity, the
variables are Xi (K = d p; the numpy model has no limit on K) --, each with every column live and with the odd-degree set.

The bound: both sides are fp64.  The point-wise side and the matrices are n-term sums and every entry of the form is a
(p+d)-term product of (p+d)-term products, as in the sibling test: (n + 2 (p + d)) 2^-53 kappa with kappa the cancellation of
the residual's three traces.  The form adds its own (K+1)^2-term sum v^T B v, whose terms cancel to the loss:
kappa_B = |v|^T |B| |v| / loss, and 2 (K + 1) 2^-53 for the two nested (K+1)-term sums.  Asserted: 4 (n + 2 (p + d) + 2 (K + 1))
2^-53 max(kappa, kappa_B) of each output's scale; the test prints what it measured, the worst figures are recorded in
profiles/closure_reduced.txt and closure_reduced_model.REORDER_REDUCED, which the GPU test adds to its fp32 rounding."""
import numpy as np
import pytest

from oracle import sindy_oracle as O
from symode_amd.coef_map import CoefMap
from symode_amd.constraint import constraint_Q
from tests.closure_quad_model import cancellation
from tests.closure_reduced_model import map_grad64, map_xi64, quad_closure64, quad_reduce, quad_step
from tests.test_host_closure_quad_model import D, SO2, pointwise, problems

CASES = [(order, so2, odd, w) for order in (1, 2, 3, 4, 5) for so2 in (False, True) for odd in (False, True) for w in (0.0, 0.37)]


@pytest.mark.parametrize("order,so2,odd,w", CASES)
def test_reduced_form_against_the_fp64_closures(order, so2, odd, w):
    p = O.term_count(D, order)
    n = 1030
    rng = np.random.RandomState(2000 * order + 100 * so2 + 10 * odd + int(w > 0))
    w32, inv = float(np.float32(w)), 1.0 / (n * D)
    Qs, use_kron = constraint_Q([SO2], D, order)
    live = CoefMap(D, p, Qs, use_kron, True).live_columns().any(axis=0) if odd else np.ones(p, dtype=bool)
    Q, allow_constant = (Qs.numpy().astype(np.float32), True) if so2 else (np.eye(D * p, dtype=np.float32), False)
    if not so2:
        use_kron = True
    K = Q.shape[1] + (D if allow_constant else 0)
    worst = {}
    for s, (x, dx, J, M, A) in enumerate(problems(order, 7 * order + 1)):
        B = quad_reduce(A, M, J, Q, use_kron, allow_constant, None, live, w32, inv)
        assert B.shape == (K + 1, K + 1) and np.abs(B - B.T).max() == 0.0
        z = np.concatenate([(rng.randn(Q.shape[1]) * 0.3).astype(np.float32), (rng.randn(D) * 0.1).astype(np.float32)[:K - Q.shape[1]]])
        loss, gz = quad_step(B, z)
        W = map_xi64(Q, z, D, p, use_kron, allow_constant) * live
        _, _, ql, qg = quad_closure64(A, M, J, W, None, live, w32, inv)
        _, _, rl, rg = pointwise(x, dx, J, W, None, order, w32)
        v = np.concatenate([z, [1.0]]).astype(np.float64)
        kappa = max(cancellation(A, W.astype(np.float32), None, live), float(np.abs(v) @ np.abs(B) @ np.abs(v)) / loss)
        tol = 4.0 * (n + 2 * (p + D) + 2 * (K + 1)) * 2.0 ** -53 * kappa
        r = Q.shape[1]
        for ref, (wl, wg) in (("quad", (ql, qg)), ("pointwise", (rl, rg * live))):
            wz = map_grad64(Q, wg, use_kron, allow_constant)
            gscale = np.abs(wg).max()
            pairs = {"loss": (loss, wl, abs(wl)), "g_beta": (gz[:r], wz[:r], max(np.abs(wz[:r]).max(), gscale))}
            if allow_constant:
                pairs["g_const"] = (gz[r:], wz[r:], max(np.abs(wz[r:]).max(), gscale))
            for name, (got, want, scale) in pairs.items():
                dev = np.abs(np.asarray(got) - np.asarray(want)).max() / scale
                worst[ref + " " + name] = max(worst.get(ref + " " + name, 0.0), dev)
                assert dev <= tol, (ref, name, s, dev, tol, kappa)
    print(f"closure_reduced model: order={order} so2={so2} odd={odd} w={w} K={K} kappa<={kappa:.3g} tol={tol:.2e} "
          + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


def test_b_as_built_is_symmetric_before_it_is_symmetrised():
    """the stored 1/2 (B + B^T) moves no entry by more than round-off: H = 1/2 P^T A P is symmetric where the closure's
    gradient is the gradient of its loss"""
    order, p = 5, O.term_count(D, 5)
    Qs, use_kron = constraint_Q([SO2], D, order)
    Q = Qs.numpy().astype(np.float32)
    live = CoefMap(D, p, Qs, use_kron, True).live_columns().any(axis=0)
    x, dx, J, M, A = problems(order, 36)[0]
    inv, K = 1.0 / (1030 * D), Q.shape[1] + D

    def ptg(z):
        return map_grad64(Q, quad_closure64(A, M, J, map_xi64(Q, z, D, p, use_kron), None, live, 0.37, inv)[3], use_kron)
    g0 = ptg(np.zeros(K))
    H = np.stack([0.5 * (ptg(np.eye(K)[i]) - g0) for i in range(K)], axis=1)
    print("asymmetry of H as built, fraction of max|H|:", np.abs(H - H.T).max() / np.abs(H).max())
    assert np.abs(H - H.T).max() <= 64 * 2.0 ** -53 * np.abs(H).max()
