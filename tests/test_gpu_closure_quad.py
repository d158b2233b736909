"""The fold closure without a point loop (csrc/closure_quad.hpp: closure_quad_kernel; symode_loss_grad_reversed_linear_quad;
engine ``aug=`` / ``coef=``; BatchedClosure ``residual_gram=``; SYMODE_FOLD_RESID_GRAM): residual AND regulariser of a problem are
quadratic forms of its augmented Gram matrix, one wave per problem, the coefficient map in the same launch.

Tolerances.  Against the fp64 numpy model of the kernel's formulae on the kernel's own tables (tests/closure_quad_model.py):
every output is formed in fp64 and rounded to fp32 ONCE, so the kernel is held to one fp32 rounding of the output's scale,
2^-24 max|.| per problem, plus the fp64 reordering term measured on the host (closure_quad_model.REORDER, from
tests/test_host_closure_quad_model.py; profiles/closure_quad.txt) -- the device sums its fp64 products in another order than
numpy.  The Xi the launch forms from (beta, const) is compared with the model's on the same terms and then handed to the model,
so that a rounding of Xi that falls the other way does not show up in every other output.
Against the point-loop Gram kernel (``gram=``) on the same inputs: the figures tests/test_gpu_closure_fold_gram.py holds the Gram
form to against the plain fold kernel, rtol 2e-5 on the loss pair and 3e-5 of its scale on the gradient (the point loop is fp32).
Two half shards: 16 * 2^-24 of scale, the figure and reasoning of that file's test (here the kernel's own sums are fp64; the
three roundings to fp32 remain).
S = 3 and S = 5 with four waves to a workgroup: an idle wave in the last workgroup, and two workgroups."""
import functools

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from symode_amd.coef_map import CoefMap
from symode_amd.constraint import constraint_Q
from tests.closure_quad_model import REORDER, map_grad, map_xi, quad_closure
from tests.test_gpu_closure_fold import columns_of, workspace
from tests.test_gpu_closure_fold_gram import batched_inputs
from tests.test_gpu_closure_live import env
from tests.test_gpu_constj import assert_close_scaled, expand
from tests.test_host_closure_quad_model import D, SO2, problems

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W_SYM = 0.37
ALL = 0xFFFFFFFFFFFFFFFF
N = 1030


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


@functools.lru_cache(maxsize=None)
def device_case(S, order):
    """S noisy damped-oscillator problems on the device with their tables from the engine: (x, dx, gx, table, M, A, ws)"""
    import symode_amd
    eng = symode_amd.get_engine()
    ps = problems(order, 7 * order + 1, S)
    x = torch.from_numpy(np.stack([q[0] for q in ps])).cuda()
    dx = torch.from_numpy(np.stack([q[1] for q in ps])).cuda()
    table = torch.from_numpy(np.stack([q[2] for q in ps])).float()[:, None].cuda().contiguous()
    gx = torch.einsum("sgab,snb->sgna", table.double(), x.double()).float().contiguous()
    M, linear = eng.linear_action(x, gx, table, order)
    assert linear
    A = eng.aug_gram(x, dx, order)
    return x, dx, gx, table, M, A, workspace(eng, x, order)


@functools.lru_cache(maxsize=None)
def so2_map(order, generator="so2", allow_constant=True):
    L = SO2 if generator == "so2" else torch.tensor([[0.0, 1.0], [0.0, 0.0]])
    Q, use_kron = constraint_Q([L], D, order)
    return CoefMap(D, O.term_count(D, order), Q.cuda(), use_kron, allow_constant)


def close(got, want, scale, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = U * np.abs(want).max() + REORDER * max(scale, np.abs(want).max())
    err = np.abs(got - want).max()
    print(f"{what}: {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, (what, err, tol)


def check_against_model(eng, S, order, cmap, masked, w, what):
    x, dx, gx, table, M, A, ws = device_case(S, order)
    p = eng.lib_size(D, order, 0)
    g = torch.Generator().manual_seed(100 * order + 10 * S + masked)
    mask = (torch.rand(S, D, p, generator=g) > 0.25).float().cuda() if masked else None
    w32, inv = float(np.float32(w)), 1.0 / (N * D)
    if cmap is None:
        live = ALL
        xi = (torch.randn(S, D, p, generator=g) * 0.3).cuda()
        l2, grad = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=w, ws=ws, linear_m=M, aug=A)
        loss = None
    else:
        live = cmap.live_mask()
        beta = (torch.randn(S, cmap.r, generator=g) * 0.3).cuda()
        const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda()
        xi = torch.full((S, D, p), float("nan"), device="cuda")
        g_beta = torch.full((S, cmap.r), float("nan"), device="cuda")
        g_const = torch.full((S, D, 1), float("nan"), device="cuda") if cmap.allow_constant else None
        loss = torch.full((S,), float("nan"), device="cuda")
        out = (torch.empty(S, 2, device="cuda"), torch.empty(S, D, p, device="cuda"), loss)
        l2, grad, gb, gc = eng.loss_grad_reversed(x, dx, gx, table, None, mask, order, 0, w_sym=w, ws=ws, linear_m=M, aug=A, out=out,
                                                  live_columns=live, coef=(cmap, beta, const), coef_out=(xi, g_beta, g_const))
        assert gb.data_ptr() == g_beta.data_ptr() and (gc is None) == (g_const is None)
    assert eng.closure_quad(ws) and eng.closure_gram(ws)
    keep = columns_of(order, live).numpy()
    for s in range(S):
        if cmap is not None:
            want_xi = map_xi(cmap.Q.cpu().numpy(), beta[s].cpu().numpy(), const[s].cpu().numpy() if cmap.allow_constant else None,
                             D, p, cmap.use_kron, cmap.allow_constant)
            close(xi[s].cpu().numpy(), want_xi, 0.0, f"{what} s={s}: Xi")
        mse, reg, tot, gr = quad_closure(A[s].cpu().numpy(), M[s, 0].cpu().numpy(), table[s, 0].cpu().double().numpy(),
                                         xi[s].cpu().numpy(), None if mask is None else mask[s].cpu().numpy(), keep, w32, inv)
        close(l2[s, 0].item(), mse, 0.0, f"{what} s={s}: mse")
        close(l2[s, 1].item(), reg, 0.0, f"{what} s={s}: regulariser")
        gscale = np.abs(gr).max()
        close(grad[s].cpu().numpy(), gr, gscale, f"{what} s={s}: gradient")
        assert (grad[s].cpu().numpy()[:, ~keep] == 0).all()
        if cmap is not None:
            close(loss[s].item(), tot, 0.0, f"{what} s={s}: loss")
            wb, wc = map_grad(cmap.Q.cpu().numpy(), gr, cmap.use_kron, cmap.allow_constant)
            close(g_beta[s].cpu().numpy(), wb, gscale, f"{what} s={s}: g_beta")
            if cmap.allow_constant:
                close(g_const[s].cpu().numpy().reshape(-1), wc, gscale, f"{what} s={s}: g_const")


@pytest.mark.parametrize("w", [0.0, W_SYM])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("so2", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("S", [3, 5])
def test_kernel_against_the_model(eng, S, order, so2, masked, w):
    check_against_model(eng, S, order, so2_map(order) if so2 else None, masked, w, f"S={S} order={order} so2={so2} masked={masked} w={w}")


@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("generator,allow_constant", [("so2", False), ("shear", True), ("shear", False)])
def test_map_variants_against_the_model(eng, order, generator, allow_constant):
    """the transposed (p, d) view (a generator without an inverse: use_kron_product is false) and a constant the model does not read"""
    cmap = so2_map(order, generator, allow_constant)
    assert cmap.use_kron == (generator == "so2") and 1 <= cmap.r <= D * cmap.p
    check_against_model(eng, 5, order, cmap, True, W_SYM, f"order={order} {generator} allow_constant={allow_constant}")


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("so2", [False, True])
def test_kernel_against_the_point_loop_gram_kernel(eng, order, so2):
    S = 5
    x, dx, gx, table, M, A, ws = device_case(S, order)
    p = eng.lib_size(D, order, 0)
    g = torch.Generator().manual_seed(order)
    live = so2_map(order).live_mask() if so2 else ALL
    xi = (torch.randn(S, D, p, generator=g) * 0.3).cuda() * columns_of(order, live).cuda()
    mask = (torch.rand(S, D, p, generator=g) > 0.25).float().cuda()
    G = A[:, None, :p, :p].contiguous()
    kw = {} if live == ALL else {"live_columns": live}
    want = tuple(t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, gram=G, **kw))
    assert not eng.closure_quad(ws)
    body = eng.closure_body(ws)
    got = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, aug=A, **kw)
    assert eng.closure_quad(ws) and eng.closure_body(ws) == body
    assert np.allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=2e-5, atol=0)
    # the gradient on the live columns: where the library has no point-loop kernel for the set (orders 1-3) the dense fold
    # kernel leaves its gradient in the dead columns as well, this kernel writes zeros there at every order
    keep = columns_of(order, live)
    for s in range(S):
        assert_close_scaled(got[1][s].cpu()[:, keep], want[1][s].cpu()[:, keep], 3e-5, f"gradient, problem {s}")
        assert (got[1][s].cpu()[:, ~keep] == 0).all()


# ------------------------------------------------------------------------------------------------ BatchedClosure
def make_closure(eng, x, dx, gx, table, Q, use_kron, **kw):
    from symode_amd.batched import BatchedClosure
    return BatchedClosure(x, dx, 5, Q=Q, use_kron_product=use_kron, allow_constant=True, engine=eng,
                          reversed_sym=(gx, expand(table, x.shape[1]), 0.1), **kw)


def test_rebuild_follows_x_and_dx(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng)
    x, dx, gx = x.clone(), dx.clone(), gx.clone()
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)

    def run(c):
        return tuple(t.clone() for t in c.evaluate(beta, const))

    def fresh():
        return run(make_closure(eng, x, dx, gx, table, Q, use_kron, residual_gram=False))

    def same(got, want, what):
        assert np.allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=2e-5, atol=0), what
        assert_close_scaled(got[1].cpu(), want[1].cpu(), 3e-5, what + ": d/dbeta")
        assert_close_scaled(got[2].cpu(), want[2].cpu(), 3e-5, what + ": d/dconst")
    first = run(clos)
    run(clos)
    assert clos.gram_builds == 1 and eng.closure_quad(clos._ws_kw["ws"])
    same(first, fresh(), "as built")
    dx.mul_(1.25)
    second = run(clos)
    run(clos)
    assert clos.gram_builds == 2
    same(second, fresh(), "after dx.mul_")
    assert not np.allclose(second[0].cpu().numpy(), first[0].cpu().numpy(), rtol=1e-3, atol=0)
    x.mul_(1.25)
    gx.copy_(torch.einsum("sgab,snb->sgna", table.double(), x.double()).float())
    third = run(clos)
    run(clos)
    assert clos.gram_builds == 3 and eng.closure_quad(clos._ws_kw["ws"])
    same(third, fresh(), "after x.mul_")
    assert not np.allclose(third[0].cpu().numpy(), second[0].cpu().numpy(), rtol=1e-3, atol=0)


def test_switches_give_the_point_loop_step_bit_for_bit_and_the_header_tells(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    ws = clos._ws_kw["ws"]
    clos.evaluate(beta, const)
    assert eng.closure_body(ws) == "fold-live" and eng.closure_gram(ws) and eng.closure_quad(ws)
    # the step with the point loop, spelt out: the map in torch, the Gram-form fold launch, the sum of the two slots, the transpose
    cmap = clos.coef
    Xi = cmap.xi(beta, const)
    G = eng.aug_gram(x, dx, 5)[:, None, :clos.p, :clos.p].contiguous()
    l2, grad = eng.loss_grad_reversed(x, dx, gx, table, Xi, None, 5, 0, w_sym=0.1, inv_count=clos.inv_count, ws=ws,
                                      live_columns=clos._live, linear_m=clos._lin_m, gram=G)
    want = (l2[:, 0] + 0.1 * l2[:, 1],) + tuple(cmap.grad(grad))
    assert not eng.closure_quad(ws) and eng.closure_gram(ws)
    with env("SYMODE_FOLD_RESID_GRAM", "0"):
        off = tuple(t.clone() for t in clos.evaluate(beta, const))
        assert eng.closure_body(ws) == "fold-live" and eng.closure_gram(ws) and not eng.closure_quad(ws)
    param = make_closure(eng, x, dx, gx, table, Q, use_kron, residual_gram=False)
    off2 = tuple(t.clone() for t in param.evaluate(beta, const))
    assert not eng.closure_quad(param._ws_kw["ws"]) and param.gram_builds == 1
    for a, b, c in zip(off, off2, want):
        assert torch.equal(a, c) and torch.equal(b, c)
    clos.evaluate(beta, const)
    assert eng.closure_quad(ws)


def test_returned_tensors_are_fresh_unless_aliased(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    a = clos.evaluate(beta, const)
    kept = tuple(t.clone() for t in a)
    b = clos.evaluate(beta * 1.5, const)
    assert all(torch.equal(p, q) for p, q in zip(a, kept)) and not torch.equal(a[0], b[0])
    c = clos.evaluate(beta, const, alias=True)
    assert all(torch.equal(p, q) for p, q in zip(c, kept))
    d = clos.evaluate(beta * 1.5, const, alias=True)
    assert all(p.data_ptr() == q.data_ptr() for p, q in zip(c, d))


def test_unconstrained_variables_are_xi(eng):
    """Q = None: beta is Xi and there is no map; the launch is the one on Xi, checked against the model"""
    S, order = 5, 5
    x, dx, gx, table, M, A, _ = device_case(S, order)
    from symode_amd.batched import BatchedClosure
    clos = BatchedClosure(x, dx, order, engine=eng, reversed_sym=(gx, expand(table, N), W_SYM))
    p = clos.p
    xi = (torch.randn(S, D, p, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
    loss, g, g_const = clos.evaluate(xi)
    assert g_const is None and eng.closure_quad(clos._ws_kw["ws"]) and eng.closure_body(clos._ws_kw["ws"]) == "fold"
    for s in range(S):
        _, _, tot, gr = quad_closure(A[s].cpu().numpy(), M[s, 0].cpu().numpy(), table[s, 0].cpu().double().numpy(), xi[s].cpu().numpy(),
                                     None, np.ones(p, dtype=bool), float(np.float32(W_SYM)), clos.inv_count)
        close(loss[s].item(), tot, 0.0, f"s={s}: loss")
        close(g[s].cpu().numpy(), gr, 0.0, f"s={s}: gradient")


def test_two_half_shards_sum_to_the_single_shard(eng):
    S, n = 3, 2060
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, S, n, 5)

    def shard(lo, hi, **kw):
        return make_closure(eng, x[:, lo:hi].contiguous(), dx[:, lo:hi].contiguous(), gx[:, :, lo:hi].contiguous(), table, Q, use_kron, **kw)
    whole = shard(0, n)
    want = tuple(t.clone() for t in whole.evaluate(beta, const))
    halves = [shard(0, n // 2, world_size=2), shard(n // 2, n, world_size=2)]
    parts = [tuple(t.clone().double() for t in h.evaluate(beta, const)) for h in halves]
    for h in halves:
        assert h.gram_builds == 1 and eng.closure_quad(h._ws_kw["ws"])
    for a, b, c, what in zip(parts[0], parts[1], want, ("loss", "d/dbeta", "d/dconst")):
        assert_close_scaled((a + b).cpu(), c.cpu(), 16 * U, what)


def test_two_chunks_equal_one_chunk_bit_for_bit(eng):
    """each wave sees its own problem alone: on the same Xi the chunking cannot show (``evaluate`` with more than one chunk forms
    Xi in torch, in fp32, so its outputs are compared through loss_grad_xi)"""
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng)
    one, two = make_closure(eng, x, dx, gx, table, Q, use_kron), make_closure(eng, x, dx, gx, table, Q, use_kron, n_chunks=2)
    Xi = one.xi_from(beta, const)
    a = one.loss_grad_xi(Xi, live_columns=one._live)
    b = two.loss_grad_xi(Xi, live_columns=two._live)
    assert len(two.chunks) == 2 and eng.closure_quad(one._ws_kw["ws"]) and eng.closure_quad(two._ws_kw["ws"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c, d = one.evaluate(beta, const), two.evaluate(beta, const)
    for p, q, what in zip(c, d, ("loss", "d/dbeta", "d/dconst")):
        assert_close_scaled(p.cpu(), q.cpu(), 16 * U, what)


def test_seed_sweep_lbfgs_takes_the_route(eng):
    """SeedSweepLBFGS(BatchedClosure(...)) with no change of its own: its tensor-op form (SYMODE_LBFGS_FUSED=0; by default a GPU fit
    goes to the device trainer, which streams the points itself and evaluates no BatchedClosure) reaches the kernel through
    ``evaluate``, aliased outputs and the captured iteration included, and descends"""
    from symode_amd.sweep import SeedSweepLBFGS
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    ref = make_closure(eng, x, dx, gx, table, Q, use_kron, residual_gram=False)
    init = clos.coef.join(beta, const)
    with env("SYMODE_LBFGS_FUSED", "0"):
        fit = SeedSweepLBFGS(clos, 0.1, 0.0, 50).fit(init.clone(), 2)
    assert eng.closure_quad(clos._ws_kw["ws"]) and clos.gram_builds == 1
    P = fit["params"]
    assert torch.isfinite(P).all()
    before = ref.evaluate(*clos.coef.split(init))[0].clone()
    after = ref.evaluate(*clos.coef.split(P.contiguous()))[0].clone()
    print("loss before", before.tolist(), "after", after.tolist())
    assert (after < before).all()
