"""The constant-Jacobian closures told which library columns can hold a coefficient (the _live entries; engine
``live_columns=``; BatchedClosure.evaluate): the kernels instantiated for "constant column + odd degrees" (d = 2 plain
polynomial libraries, orders 4 and 5) leave the other columns out.

With Xi exactly zero in the dead columns a dead column contributes fma(0, t, s) = s to every sum, so the sparse kernel is
held to torch.equal with the dense one in the loss pair and in every live gradient entry, and to zero in the dead ones.  With
the round-off of the constraint's Q left there (2e-7) it is held to the fp64 closure at the tolerances of
test_gpu_constj.py::test_compact_table_against_the_oracle (loss rtol 2e-5, gradient 3e-5 of its scale)."""
import os

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.test_gpu_constj import assert_close_scaled, expand, make_case

pytestmark = pytest.mark.gpu

D, S, W_SYM = 2, 3, 0.37
ALL = 0xFFFFFFFFFFFFFFFF
# constant column + odd degrees: the set the sparse kernels are instantiated for, and its dead columns
PATTERN = {4: 0x3C7, 5: 0x1F83C7}
DEAD = {4: [3, 4, 5, 10, 11, 12, 13, 14], 5: [3, 4, 5, 10, 11, 12, 13, 14]}
DENSE_BODY = {4: "scalar", 5: "packed"}


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


class env:
    """One SYMODE_* variable for the duration of a block (the library reads its variables once: engine.reload_env)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def _set(self, value):
        import symode_amd
        if value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = value
        symode_amd.engine.reload_env()

    def __enter__(self):
        self.old = os.environ.get(self.name)
        self._set(self.value)

    def __exit__(self, *exc):
        self._set(self.old)


def both_forms(eng, c, xi, mask, order, live):
    """(fused loss pair, fused gradient, regulariser loss, regulariser gradient) and the body each launch took"""
    x, dx, gx, table = c
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, 0, x.shape[0] if x.dim() == 3 else 1, x.shape[-2]))
    kw = {} if live is None else {"live_columns": live}
    fused = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, **kw)
    bodies = [eng.closure_body(ws)]
    alone = eng.symreg_reversed(x, gx, table, xi, mask, order, 0, ws=ws, **kw)
    bodies.append(eng.closure_body(ws))
    return (*fused, *alone), bodies


def columns(order, eng):
    p = eng.lib_size(D, order, 0)
    dead = torch.zeros(p, dtype=torch.bool)
    dead[DEAD[order]] = True
    assert sum(1 << k for k in range(p) if not dead[k]) == PATTERN[order]
    return dead.cuda()


def check_sparse_against_dense(got, want, dead, what):
    for (g, w, name) in zip(got, want, ("fused loss pair", "fused gradient", "regulariser loss", "regulariser gradient")):
        assert torch.isfinite(w).all() and w.abs().max() > 0, (what, name)
        if "gradient" in name:
            assert torch.equal(g[..., ~dead], w[..., ~dead]), f"{what}: {name}, live columns"
            assert (g[..., dead] == 0).all(), f"{what}: {name}, dead columns"
        else:
            assert torch.equal(g, w), f"{what}: {name}"


# n = 1032: the vector ring with a partial turn; 1031 (odd, S > 1): the per-point path; 5: a ring shorter than one turn
CASES = [(n, n_g, order, masked) for order in (5, 4) for n in (1032, 1031, 5) for n_g in (1, 2) for masked in (False, True)]


@pytest.mark.parametrize("n,n_g,order,masked", CASES)
def test_sparse_kernel_equals_the_dense_one_on_coefficients_that_are_zero_there(eng, n, n_g, order, masked):
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, D, order, eng)
    dead = columns(order, eng)
    xi = xi.clone()
    xi[..., dead] = 0.0
    mask = mask if masked else None
    c = (x, dx, gx, table)
    want, bodies = both_forms(eng, c, xi, mask, order, None)
    assert bodies == [DENSE_BODY[order]] * 2
    got, bodies = both_forms(eng, c, xi, mask, order, PATTERN[order])
    assert bodies == ["scalar-live"] * 2, "the launcher takes the sparse kernel for a set inside its pattern"
    check_sparse_against_dense(got, want, dead, "the pattern itself")
    # a strict subset (the constant column dead too, as without allow_constant): what Xi holds there counts as zero
    sub = PATTERN[order] & ~1
    dead0 = dead.clone()
    dead0[0] = True
    assert xi[..., 0].abs().min() > 0
    xi0 = xi.clone()
    xi0[..., 0] = 0.0
    want0, _ = both_forms(eng, c, xi0, mask, order, None)
    got0, bodies = both_forms(eng, c, xi, mask, order, sub)
    assert bodies == ["scalar-live"] * 2
    check_sparse_against_dense(got0, want0, dead0, "a subset of the pattern")


@pytest.mark.parametrize("order", [5, 4])
def test_one_aligned_problem(eng, order):
    x, dx, gx, table, xi, mask = make_case(1, 1031, 1, D, order, eng)
    dead = columns(order, eng)
    xi = xi.clone()
    xi[..., dead] = 0.0
    assert x.data_ptr() % 16 == 0
    for c, q, m in (((x, dx, gx, table), xi, mask), ((x[0], dx[0], gx[0], table[0]), xi[0], mask[0])):     # batched of one, and the one-problem form
        want, _ = both_forms(eng, c, q, m, order, None)
        got, bodies = both_forms(eng, c, q, m, order, PATTERN[order])
        assert bodies == ["scalar-live"] * 2
        check_sparse_against_dense(got, want, dead, "S = 1")


@pytest.mark.parametrize("order", [5, 4])
def test_a_set_outside_the_pattern_runs_the_dense_kernel(eng, order):
    n, n_g = 1032, 2
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, D, order, eng)
    c = (x, dx, gx, table)
    want, _ = both_forms(eng, c, xi, mask, order, None)
    for live in (PATTERN[order] | 1 << 3, PATTERN[order] | 1 << 14, ALL):            # one even-degree bit; everything
        got, bodies = both_forms(eng, c, xi, mask, order, live)
        assert bodies == [DENSE_BODY[order]] * 2, hex(live)
        for g, w in zip(got, want):
            assert torch.equal(g, w), hex(live)                                      # Xi as it is, every column
    # bits past the library's columns say nothing about it
    got, bodies = both_forms(eng, c, xi, mask, order, PATTERN[order] | 1 << 40)
    assert bodies == ["scalar-live"] * 2
    # libraries without a sparse kernel: the set is taken and the dense kernel runs (order 3; sine columns at order 5)
    x3, dx3, gx3, t3, xi3, m3 = make_case(S, n, 1, D, 3, eng)
    want3, b0 = both_forms(eng, (x3, dx3, gx3, t3), xi3, m3, 3, None)
    got3, b1 = both_forms(eng, (x3, dx3, gx3, t3), xi3, m3, 3, 0x3C7)
    assert b0 == b1 == ["scalar"] * 2 and all(torch.equal(g, w) for g, w in zip(got3, want3))
    # the materialised Jacobian has no sparse form either
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, 0, S, n))
    l2, g = eng.loss_grad_reversed(x, dx, gx, expand(table, n), xi, mask, order, 0, w_sym=W_SYM, ws=ws, live_columns=PATTERN[order])
    assert eng.closure_body(ws) == "scalar" and torch.equal(l2, want[0]) and torch.equal(g, want[1])
    # and the knob keeps the dense kernels
    with env("SYMODE_CLOSURE_LIVE", "0"):
        got, bodies = both_forms(eng, c, xi, mask, order, PATTERN[order])
    assert bodies == [DENSE_BODY[order]] * 2 and all(torch.equal(g, w) for g, w in zip(got, want))
    _, bodies = both_forms(eng, c, xi, mask, order, PATTERN[order])
    assert bodies == ["scalar-live"] * 2


def fp64_closure(x, dx, gx, table, xi, mask, order, w):
    """(mse, regulariser, d(mse + w regulariser)/dXi, d regulariser/dXi) of one problem in fp64, Xi as given."""
    x, dx, gx, table, mask = (t.detach().cpu().double() for t in (x, dx, gx, table, mask))
    xi = xi.detach().cpu().double().requires_grad_(True)

    def h(z):
        return O.theta(z, order) @ (xi * mask).T
    mse = torch.mean((h(x) - dx) ** 2)
    sym = O.symreg_reversed_precomputed(x, list(gx), [J.expand(x.shape[0], D, D) for J in table], h)
    g_sym, = torch.autograd.grad(sym, xi, retain_graph=True)
    g_all, = torch.autograd.grad(mse + w * sym, xi)
    return mse.item(), sym.item(), g_all, g_sym


@pytest.mark.parametrize("order", [5, 4])
def test_round_off_in_the_dead_columns_against_the_fp64_closure(eng, order):
    """What the constrained map really hands over: +-2e-7 where the constraint says zero.  The fp64 closure reads Xi as it is."""
    n, n_g = 1032, 2
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, D, order, eng)
    dead = columns(order, eng)
    g = torch.Generator().manual_seed(5)
    noise = (2e-7 * (2.0 * (torch.rand(xi.shape, generator=g) > 0.5).float() - 1.0)).cuda()
    xi = torch.where(dead, noise, xi)
    assert (xi[..., dead].abs() == 2e-7).all()
    (loss2, grad, l_s, g_s), bodies = both_forms(eng, (x, dx, gx, table), xi, mask, order, PATTERN[order])
    assert bodies == ["scalar-live"] * 2
    live = (~dead).cpu()
    for s in range(S):
        mse, sym, g_all, g_sym = fp64_closure(x[s], dx[s], gx[s], table[s], xi[s], mask[s], order, W_SYM)
        assert np.isclose(loss2[s, 0].item(), mse, rtol=2e-5) and np.isclose(loss2[s, 1].item(), sym, rtol=2e-5)
        assert np.isclose(l_s[s].item(), sym, rtol=2e-5)
        # the gradient in the columns the caller declared dead is not asked for: it comes back zero
        assert_close_scaled(grad[s].cpu()[:, live], g_all[:, live], 3e-5, f"fused closure grad, problem {s}")
        assert_close_scaled(g_s[s].cpu()[:, live], g_sym[:, live], 3e-5, f"regulariser grad, problem {s}")
        assert (grad[s][:, dead] == 0).all() and (g_s[s][:, dead] == 0).all()


def test_batched_closure_takes_the_sparse_kernel_from_its_map(eng):
    from symode_amd.batched import BatchedClosure
    from symode_amd.constraint import constraint_Q
    n, order = 1032, 5
    x, dx, gx, table, _, _ = make_case(S, n, 1, D, order, eng)
    Q, use_kron = constraint_Q([torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], D, order)
    Q = Q.cuda()
    g = torch.Generator().manual_seed(11)
    beta = (torch.randn(S, Q.shape[1], generator=g) * 0.3).cuda()
    const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda()

    def closure(**kw):
        return BatchedClosure(x, dx, order, Q=Q, use_kron_product=use_kron, allow_constant=True, engine=eng,
                              reversed_sym=(gx, expand(table, n), 0.1), **kw)

    def run(clos):
        out = tuple(t.clone() for t in clos.evaluate(beta, const))
        return out, eng.closure_body(clos._ws_kw["ws"])
    sparse, dense = closure(), closure(live_columns=False)
    assert sparse._live == 0x1F83C7 and dense._live is None
    # the map's Xi is NOT zero in the dead columns: that is why the set has to be told
    Xi = sparse.xi_from(beta, const)
    dead = columns(order, eng)
    assert 0 < Xi[..., dead].abs().max() < 1e-5
    want, body = run(dense)
    assert body == "packed"
    got, body = run(sparse)
    assert body == "scalar-live"
    assert np.allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=2e-5, atol=0)
    assert_close_scaled(got[1].cpu(), want[1].cpu(), 3e-5, "d/dbeta")
    assert_close_scaled(got[2].cpu(), want[2].cpu(), 3e-5, "d/dconst")
    with env("SYMODE_CLOSURE_LIVE", "0"):
        same, body = run(sparse)
    assert body == "packed" and all(torch.equal(a, b) for a, b in zip(same, want))
    # loss_grad_xi called directly keeps the dense launch
    l, gr = sparse.loss_grad_xi(Xi)
    assert eng.closure_body(sparse._ws_kw["ws"]) == "packed"
    ld, gd = dense.loss_grad_xi(Xi)
    assert torch.equal(l, ld) and torch.equal(gr, gd)
