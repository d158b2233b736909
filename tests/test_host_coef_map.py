"""coef_map.CoefMap -- the one map between the optimiser's variables and Xi -- against the oracle's ``xi_from_beta``, against
autograd (the gradient is the transpose of the map) and against a regressor's own parameters, for every layout:
unconstrained, Kronecker view, transposed view, transposed view with ``constrain_constant``.

Both generators the other tests use (so(2), scaling2) have det > 0, i.e. the Kronecker branch; the transposed layouts read
scaling2's Q with the other view (the map's arithmetic does not depend on where Q came from), and ``swap`` (det -1, the
generator of the negdet golden vectors) is a regressor that takes the transposed branch by itself.

Bounds.  eps = 2^-23.  Two fp32 evaluations of the same k-term dot product sum_j a_j b_j each lie within
k (eps / 2) sum_j |a_j b_j| of the exact value (Higham, Accuracy and Stability, section 3.1), so they differ by at most
k eps sum_j |a_j b_j|: that is ``_dot_bound``.  Where a constant is added after the product, each of the two fp32 additions
rounds once more (eps / 2 |result| each): the constant column gets ``+ eps |Xi|``.
"""
import numpy as np
import pytest
import torch

import symode_amd  # noqa: F401
from oracle import sindy_oracle as O
from symode_amd.coef_map import CoefMap
from symode_amd.constraint import constraint_Q
from symode_amd.sindy import SINDyRegression
from tests.oracle_engine import OracleEngine

torch.set_num_threads(1)
EPS = float(torch.finfo(torch.float32).eps)
SO2 = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
SCALING2 = torch.tensor([[2.0, 0.0], [0.0, 1.0]])
SWAP = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
S = 7


def _map(name):
    if name == "free":
        return CoefMap(2, 10)
    L, order, kron, allow = {"kron": (SO2, 2, True, True), "transposed": (SCALING2, 2, False, True),
                             "transposed_cc": (SCALING2, 2, False, False), "swap_o3": (SWAP, 3, None, True)}[name]
    Q, use_kron = constraint_Q([L], 2, order)
    assert use_kron is (name != "swap_o3")                     # so(2), scaling2: Kronecker branch; swap: transposed
    return CoefMap(2, O.term_count(2, order, False, False), Q, use_kron if kron is None else kron, allow)


LAYOUTS = ["free", "kron", "transposed", "transposed_cc", "swap_o3"]


def _view(c, flat):
    """|Q| @ |beta| laid out as Xi is (the bound of every coefficient sits where the coefficient does)."""
    return flat.view(c.d, c.p) if c.use_kron else flat.view(c.p, c.d).T


def _dot_bound(c, beta):
    return c.r * EPS * _view(c, c.Q.abs() @ beta.abs())


@pytest.mark.parametrize("name", LAYOUTS)
def test_layout_and_split_join(name):
    c = _map(name)
    assert c.n_params == (c.d * c.p if c.Q is None else c.Q.shape[1] + c.d) and c.r == (0 if c.Q is None else c.Q.shape[1])
    P = torch.randn(S, c.n_params, generator=torch.Generator().manual_seed(0))
    a, b = c.split(P)
    if c.Q is None:
        assert b is None and a.shape == (S, c.d, c.p) and a.data_ptr() == P.data_ptr()
        assert c.split(P[0])[0].shape == (c.d, c.p)
    else:
        assert torch.equal(a, P[:, :c.r]) and torch.equal(b, P[:, c.r:].reshape(S, c.d, 1))
        a1, b1 = c.split(P[0])
        assert torch.equal(a1, P[0, :c.r]) and torch.equal(b1, P[0, c.r:].view(c.d, 1))
    assert torch.equal(c.join(a, b), P)


@pytest.mark.parametrize("name", LAYOUTS)
def test_xi_one_problem_is_the_oracle_bit_for_bit_and_the_batched_rows_agree(name):
    c = _map(name)
    g = torch.Generator().manual_seed(1)
    for trial in range(20):
        P = torch.randn(S, c.n_params, generator=g)
        beta, const = c.split(P)
        Xi_b = c.xi(beta.contiguous(), const)
        assert Xi_b.shape == (S, c.d, c.p)
        if c.Q is None:
            assert Xi_b is beta and torch.equal(c.xi(c.split(P[0])[0]), P[0].view(c.d, c.p))
            continue
        zero = torch.zeros(S, c.d, 1)
        Xi_b0 = c.xi(beta.contiguous(), zero)                   # x + 0 is exact: the bare r-term products
        assert Xi_b.is_contiguous()
        for s in range(S):
            want = O.xi_from_beta(c.Q, beta[s], const[s], c.d, c.use_kron, c.allow_constant)
            got = c.xi(beta[s], const[s])
            assert torch.equal(got, want), (name, trial, s)
            bound = _dot_bound(c, beta[s])
            err0 = (Xi_b0[s] - c.xi(beta[s], zero[s])).abs()
            assert bool((err0 <= bound).all()), (name, trial, s, float((err0 - bound).max()))
            with_add = bound.clone()
            if c.allow_constant:
                with_add[:, 0] += EPS * want[:, 0].abs()       # the two additions of const round once each
            err = (Xi_b[s] - want).abs()
            assert bool((err <= with_add).all()), (name, trial, s, float((err - with_add).max()))
        if not c.allow_constant:                                # the unread constant changes nothing
            assert torch.equal(Xi_b, Xi_b0) and torch.equal(Xi_b, c.xi(beta.contiguous(), None))


@pytest.mark.parametrize("name", LAYOUTS)
def test_grad_is_the_transpose_of_xi(name):
    c = _map(name)
    g = torch.Generator().manual_seed(2)
    for trial in range(20):
        P = torch.randn(S, c.n_params, generator=g).requires_grad_(True)
        W = torch.randn(S, c.d, c.p, generator=g)
        beta, const = c.split(P)
        (want,) = torch.autograd.grad((c.xi(beta.contiguous(), const) * W).sum(), P)
        got = c.grad(W, flat=True)
        assert torch.equal(got, want), (name, trial, float((got - want).abs().max()))     # autograd runs the same g @ Q
        g_beta, g_const = c.grad(W)
        if c.Q is None:
            assert g_beta is W and g_const is None
        elif c.allow_constant:
            assert torch.equal(g_const, W[:, :, 0:1]) and torch.equal(got[:, c.r:], W[:, :, 0])
        else:
            assert g_const is None and torch.equal(got[:, c.r:], torch.zeros(S, c.d))     # exactly zero
        for s in range(S):                                       # numpy form: fp32 Q.T @ G on the host
            w = W[s].numpy()
            flat = c.grad(w, flat=True)
            assert flat.dtype == np.float32 and flat.shape == (c.n_params,)
            if c.Q is None:
                assert np.array_equal(flat, w.reshape(-1))
                continue
            laid = W[s] if c.use_kron else W[s].T
            bound = (c.d * c.p * EPS * (c.Q.abs().T @ laid.reshape(-1).abs())).numpy()
            assert (np.abs(flat[:c.r] - want[s, :c.r].numpy()) <= bound).all(), (name, trial, s)
            assert np.array_equal(flat[c.r:], want[s, c.r:].numpy())
            pieces = c.grad(w)
            assert np.array_equal(pieces[0], flat[:c.r]) and (pieces[1] is None) == (not c.allow_constant)


@pytest.mark.parametrize("name", LAYOUTS[1:])
def test_numpy_xi_and_effective_Q_reproduce_xi(name):
    c = _map(name)
    q_eff = c.effective_Q()
    assert q_eff.dtype == np.float32 and q_eff.flags["C_CONTIGUOUS"] and q_eff.shape == (c.d * c.p, c.r)
    bare = CoefMap(c.d, c.p, c.Q, c.use_kron, allow_constant=False)
    g = torch.Generator().manual_seed(3)
    for trial in range(20):
        beta, const = torch.randn(c.r, generator=g), torch.randn(c.d, 1, generator=g)
        bound = _dot_bound(c, beta).numpy()
        want = bare.xi(beta, None).numpy()
        got = (q_eff @ beta.numpy()).reshape(c.d, c.p)           # what the device trainer's XiMap computes
        assert (np.abs(got - want) <= bound).all(), (name, trial)
        host = c.xi(beta.numpy(), const.numpy().reshape(-1))     # the fp32 host form (STLSQ solution -> Xi)
        full = c.xi(beta, const).numpy()
        if c.allow_constant:
            bound[:, 0] += EPS * np.abs(full[:, 0])
        assert host.dtype == np.float32 and host.flags["C_CONTIGUOUS"] and (np.abs(host - full) <= bound).all(), (name, trial)


def _regressor(L_list, order, constrain_constant=False):
    return SINDyRegression(2, order, False, False, L_list=L_list, threshold=0.05, device="cpu",
                           constrain_constant=constrain_constant, engine=OracleEngine())


@pytest.mark.parametrize("L_list,order,cc", [([], 3, False), ([SO2], 2, False), ([SCALING2], 2, True), ([SWAP], 3, False)])
def test_pack_adopt_round_trip_and_regressor_delegation(L_list, order, cc):
    torch.manual_seed(4)
    src, dst = _regressor(L_list, order, cc), _regressor(L_list, order, cc)
    c = CoefMap.from_regressor(src)
    assert c.n_params == sum(q.numel() for q in src.parameters()) and (c.Q is None) == (not src.constraint)
    if src.constraint:
        first = dst.coef
        dst.Q = src.Q                                            # the regressor's map follows a replaced Q
        assert dst.coef is not first and dst.coef.Q is src.Q and dst.coef is dst.coef
        want = O.xi_from_beta(src.Q, src.beta, src.const, 2, src.use_kron_product, src.allow_constant)
        assert torch.equal(src.get_Xi(), want) and c.use_kron == bool(src.use_kron_product) and c.allow_constant == (not cc)
    src.mask.copy_((torch.rand(src.mask.shape) > 0.4).float())
    flat = c.pack(src)
    assert flat.shape == (c.n_params,)
    assert torch.equal(flat, torch.cat([q.detach().reshape(-1) for q in src.parameters()]))
    for params, mask in ((flat, src.mask), (flat.numpy().copy(), src.mask.numpy().reshape(-1).copy())):
        for q in dst.parameters():
            q.data.zero_()
        mask_tensor = dst.mask
        dst.coef.adopt(dst, params, mask)
        assert all(torch.equal(a, b) for a, b in zip(dst.parameters(), src.parameters()))
        assert dst.mask is mask_tensor and torch.equal(dst.mask, src.mask)       # the mask is written in place
        assert torch.equal(dst.get_Xi(), src.get_Xi())


@pytest.mark.parametrize("name", LAYOUTS)
def test_update_norm_and_draw(name):
    c = _map(name)
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(S, c.n_params, generator=g), torch.randn(S, c.n_params, generator=g)
    got = c.update_norm(A, B)
    pieces = [(a, b) for a, b in zip(c.split(A), c.split(B)) if a is not None]
    assert torch.equal(got, sum((a - b).reshape(S, -1).norm(dim=1) for a, b in pieces))
    for s in range(S):                                           # train.py:702-704, one problem, one tensor at a time
        want = sum(torch.norm(a[s] - b[s]) for a, b in pieces)
        assert abs(float(got[s]) - float(want)) <= (c.n_params + 2) * EPS * float(want)
    # initial variables: the constructor's draws, in its order, on the caller's generator
    g1, g2 = torch.Generator().manual_seed(6), torch.Generator().manual_seed(6)
    want = torch.randn(c.d * c.p, generator=g2) if c.Q is None else \
        torch.cat([torch.randn(c.r, generator=g2), torch.randn(c.d, generator=g2)])
    assert torch.equal(c.draw(g1), want)


def test_map_of_a_duck_typed_closure_and_shared_constants():
    class Bare:                                                  # what SeedSweepLBFGS needs of a closure without ``coef``
        S, d, p, Q, distributed = 2, 1, 3, None, False
    from symode_amd.sweep import SeedSweepLBFGS
    c = SeedSweepLBFGS(Bare(), 0.1, 0.05, 50).coef
    assert (c.d, c.p, c.Q, c.n_params) == (1, 3, None, 3)
    Bare.coef = _map("kron")
    assert SeedSweepLBFGS(Bare(), 0.1, 0.05, 50).coef is Bare.coef
    from symode_amd import device_lbfgs, sindy
    assert device_lbfgs.NEAR_THRESHOLD_BAND == sindy.NEAR_THRESHOLD_BAND
