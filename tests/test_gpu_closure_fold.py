"""The fused reversed closure under a linear group action, g(x) = J x (symode_linear_action, symode_loss_grad_reversed_linear;
engine ``linear_action`` / ``linear_m=``; BatchedClosure ``linear_action=``): Theta(J x) = M Theta(x) for the plain polynomial
libraries, so the kernel reads x and dx alone, evaluates the library once and applies [Xi; C], C = J Xi - Xi M.

The fold replaces g(x) by J x (the detector accepts 4 * 2^-24 per component) and forms u from C: not the streamed kernels' bits.
It is held to the fp64 closure at the bounds of test_gpu_constj.py::test_compact_table_against_the_oracle (loss rtol 2e-5,
gradient 3e-5 of its scale), to the streamed constant-J entry at the same bounds, and with SYMODE_CLOSURE_FOLD=0 to
torch.equal with that entry."""
import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.test_gpu_closure_live import PATTERN, env
from tests.test_gpu_constj import assert_close_scaled, expand

pytestmark = pytest.mark.gpu

D, W_SYM, U = 2, 0.37, 2.0 ** -24
ALL = 0xFFFFFFFFFFFFFFFF
# what the launcher routes to the fold kernels (closure_fold.hpp: closure_fold_dense_pays / closure_fold_live_pays) and what
# the streamed launch takes for the same call
FOLD_DENSE = {1: True, 2: True, 3: True, 4: True, 5: True}
FOLD_LIVE = {4: True, 5: True}
STREAMED_DENSE = {1: "scalar", 2: "scalar", 3: "scalar", 4: "scalar", 5: "packed"}


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def rotation(t):
    c, s = torch.cos(t), torch.sin(t)
    return torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)


def linear_case(S, n, order, eng, seed=0, rot=False):
    """x, dx (S, n, 2), a distinct J per problem (S, 1, 2, 2), gx = J x formed in fp64 and rounded once, Xi and a partial mask"""
    g = torch.Generator().manual_seed(977 * S + 13 * n + order + seed)
    p = eng.lib_size(D, order, 0)
    x = torch.randn(S, n, D, generator=g) * 0.5
    dx = torch.randn(S, n, D, generator=g)
    if rot:
        table = rotation(0.05 + 0.4 * torch.rand(S, generator=g).double()).float()[:, None]
    else:
        table = (torch.eye(D) + 0.3 * torch.randn(S, 1, D, D, generator=g))
    gx = torch.einsum("sgab,snb->sgna", table.double(), x.double()).float()
    xi = torch.randn(S, D, p, generator=g) * 0.3
    mask = (torch.rand(S, D, p, generator=g) > 0.25).float()
    return tuple(t.cuda().contiguous() for t in (x, dx, gx, table, xi, mask))


def workspace(eng, x, order):
    return eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, 0, x.shape[0], x.shape[-2]))


def fp64_closure(x, dx, table, xi, mask, order, w):
    """(mse, regulariser, d(mse + w regulariser)/dXi) of one problem in fp64 with gx = J x formed in fp64 here"""
    x, dx, table = (t.detach().cpu().double() for t in (x, dx, table))
    mask = torch.ones_like(xi).cpu().double() if mask is None else mask.detach().cpu().double()
    xi = xi.detach().cpu().double().requires_grad_(True)

    def h(z):
        return O.theta(z, order) @ (xi * mask).T
    mse = torch.mean((h(x) - dx) ** 2)
    sym = O.symreg_reversed_precomputed(x, [x @ J.T for J in table], [J.expand(x.shape[0], D, D) for J in table], h)
    g_all, = torch.autograd.grad(mse + w * sym, xi)
    return mse.item(), sym.item(), g_all


# ------------------------------------------------------------------------------------------------ M
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("rot", [False, True])
def test_substitution_matrix_against_numpy(eng, order, rot):
    S, n = 3, 50
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng, rot=rot)
    M, linear = eng.linear_action(x, gx, table, order)
    p = eng.lib_size(D, order, 0)
    assert linear and M.dtype == torch.float64 and M.shape == (S, 1, p, p)
    deg = np.array([sum(e) for e in O.term_exponents(D, order)])
    off_block = torch.from_numpy(deg[:, None] != deg[None, :])
    for s in range(S):
        xs, J = x[s].cpu().double(), table[s, 0].cpu().double()
        th, thg = O.theta(xs, order), O.theta(xs @ J.T, order)
        got = th @ M[s, 0].cpu().T
        assert (got - thg).abs().max() <= 1e-12 * max(thg.abs().max().item(), 1.0), (order, rot, s)
        assert (M[s, 0].cpu()[off_block] == 0).all(), "block diagonal by degree: exact zeros outside the blocks"


# ------------------------------------------------------------------------------------------------ detector
def products(x, table):
    """g(x) = J x formed three ways in fp32: torch on the GPU, torch on the CPU, explicit FMAs (fma(a, b, c) through fp64: the
    product is exact there and the sum is rounded to fp32 once more)"""
    Jt = table[:, 0].transpose(1, 2).contiguous()
    xc, Jc = x.cpu(), table[:, 0].cpu()
    a = (xc.double()[..., None, :] * Jc.double()[:, None])                     # (S, n, a, b): the exact products J_ab x_b
    fma = (a[..., 0] + a[..., 1].float().double()).float()                     # fma(J_a0, x_0, fl(J_a1 x_1))
    return {"torch, GPU": (x @ Jt)[:, None].contiguous(), "torch, CPU": (xc @ Jc.transpose(1, 2))[:, None].contiguous().cuda(),
            "explicit FMAs": fma[:, None].contiguous().cuda()}


def excess(x, gx, table):
    """max over components of |gx - J x| / sum |J| |x| in units of u = 2^-24, fp64 on the host"""
    x, gx, J = x.cpu().double(), gx[:, 0].cpu().double(), table[:, 0].cpu().double()
    exact = torch.einsum("sab,snb->sna", J, x)
    scale = torch.einsum("sab,snb->sna", J.abs(), x.abs())
    return ((gx - exact).abs() / scale).max().item() / U


@pytest.mark.parametrize("n", [6, 1031])
def test_detector_accepts_fp32_products(eng, n):
    S, order = 3, 3
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng)
    assert eng.linear_action(x, gx, table, order)[1], "gx rounded once from the fp64 product"
    for how, g in products(x, table).items():
        e = excess(x, g, table)
        print(f"n = {n}, {how}: max |gx - J x| / sum |J||x| = {e:.3f} u")
        assert e <= 4.0, f"{how}: the 4 u bound does not hold for this product ({e:.3f} u)"
        assert eng.linear_action(x, g, table, order)[1], how


@pytest.mark.parametrize("n", [6, 1031])
def test_detector_refuses_what_is_not_the_linear_image(eng, n):
    S, order = 3, 3
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng)
    scale = torch.einsum("sab,snb->sna", table[:, 0].double().abs(), x.double().abs())
    # one component of one point moved by 8 u sum |J| |x|: the first point, the last one, one of the ragged tail
    for s, i, a in ((0, 0, 0), (S - 1, n - 1, 1), (1, n - 2, 0), (2, n // 2, 1)):
        bad = gx.clone()
        bad[s, 0, i, a] = (gx[s, 0, i, a].double() + 8.0 * U * scale[s, i, a]).float()
        assert excess(x, bad, table) > 4.0
        assert not eng.linear_action(x, bad, table, order)[1], (s, i, a)
    assert not eng.linear_action(x, gx + 1e-3, table, order)[1], "an offset b = 1e-3: affine, not linear"
    for t in (gx, x):
        bad = t.clone()
        bad[1, ..., n - 1, 0] = float("nan")
        args = (x, bad, table) if t is gx else (bad, gx, table)
        assert not eng.linear_action(*args, order)[1], "a NaN"
    bad = gx.clone()
    bad[0, 0, 0, 0] = float("inf")
    assert not eng.linear_action(x, bad, table, order)[1], "an infinity"
    g = torch.Generator().manual_seed(3)
    assert not eng.linear_action(x, (torch.randn(gx.shape, generator=g) * 0.5).cuda(), table, order)[1], "random gx"
    assert eng.linear_action(x, gx, table, order)[1]


# ------------------------------------------------------------------------------------------------ the kernel
def columns_of(order, live):
    p = O.term_count(D, order)
    return torch.tensor([(live >> k) & 1 == 1 for k in range(p)])


KERNEL_CASES = [(S, n, order, live) for S in (1, 3) for n in (1, 6, 1030, 1031)
                for order, live in [(o, None) for o in (1, 2, 3, 4, 5)] + [(4, PATTERN[4]), (5, PATTERN[5])]]


@pytest.mark.parametrize("S,n,order,live", KERNEL_CASES)
def test_fold_kernel_against_the_fp64_closure_and_the_streamed_entry(eng, S, n, order, live):
    """n = 1: the tail alone; 6: fewer chunks than lanes; 1030: ring + tail; 1031 (odd): the per-point path where S > 1."""
    x, dx, gx, table, xi, mask = linear_case(S, n, order, eng)
    keep = columns_of(order, ALL if live is None else live).cuda()
    xi = xi * keep                                            # the caller's declaration holds: zero outside the set
    M, linear = eng.linear_action(x, gx, table, order)
    assert linear
    ws = workspace(eng, x, order)
    kw = {} if live is None else {"live_columns": live}
    l2, grad = (t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw))
    routed = FOLD_DENSE[order] if live is None else FOLD_LIVE[order]
    assert eng.closure_body(ws) == (("fold" if live is None else "fold-live") if routed else
                                    (STREAMED_DENSE[order] if live is None else "scalar-live"))
    ls, gs = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, **kw)
    assert eng.closure_body(ws) == (STREAMED_DENSE[order] if live is None else "scalar-live")
    keep = keep.cpu()
    for s in range(S):
        mse, sym, g_all = fp64_closure(x[s], dx[s], table[s], xi[s], mask[s], order, W_SYM)
        dev = [abs(t[s, 0].item() - mse) / mse for t in (l2, ls)] + [abs(t[s, 1].item() - sym) / sym for t in (l2, ls)]
        gdev = [(t[s].cpu().double()[:, keep] - g_all[:, keep]).abs().max().item() / g_all[:, keep].abs().max().item() for t in (grad, gs)]
        print(f"S={S} n={n} order={order} live={live} s={s}: mse fold {dev[0]:.2e} streamed {dev[1]:.2e}; reg fold {dev[2]:.2e} "
              f"streamed {dev[3]:.2e}; grad fold {gdev[0]:.2e} streamed {gdev[1]:.2e}")
        assert np.isclose(l2[s, 0].item(), mse, rtol=2e-5) and np.isclose(l2[s, 1].item(), sym, rtol=2e-5), (s, dev)
        assert_close_scaled(grad[s].cpu()[:, keep], g_all[:, keep], 3e-5, f"fold gradient, problem {s}")
        assert (grad[s].cpu()[:, ~keep] == 0).all()
    # the streamed constant-J entry on the same inputs
    assert np.allclose(l2.cpu().numpy(), ls.cpu().numpy(), rtol=2e-5, atol=0)
    for s in range(S):
        assert_close_scaled(grad[s].cpu(), gs[s].cpu(), 3e-5, f"fold against streamed gradient, problem {s}")


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [6, 1030])
def test_equivariant_coefficients_where_the_regulariser_is_round_off(eng, order, n):
    """Xi = Q beta + const with Q the rotation constraint and J a rotation: u is round-off in the streamed kernels and comes
    from C, whose Q part vanishes, in the fold.  Bounds on mse, mse + w * regulariser and the gradient; none on the regulariser."""
    from symode_amd.coef_map import CoefMap
    from symode_amd.constraint import constraint_Q
    S = 3
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng, seed=5, rot=True)
    Q, use_kron = constraint_Q([torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], D, order)
    coef = CoefMap(D, eng.lib_size(D, order, 0), Q.cuda(), use_kron, True)
    g = torch.Generator().manual_seed(11 + order)
    beta = (torch.randn(S, Q.shape[1], generator=g) * 0.3).cuda()
    const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda()
    xi = coef.xi(beta, const).contiguous()
    live = coef.live_mask()
    M, linear = eng.linear_action(x, gx, table, order)
    assert linear
    ws = workspace(eng, x, order)
    for kw in ({}, {"live_columns": live}):
        l2, grad = eng.loss_grad_reversed(x, dx, gx, table, xi, None, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw)
        keep = columns_of(order, ALL if not kw else live)
        for s in range(S):
            mse, sym, g_all = fp64_closure(x[s], dx[s], table[s], xi[s] * keep.cuda(), None, order, W_SYM)
            print(f"order={order} n={n} s={s} {kw}: mse {l2[s, 0].item():.6e} / {mse:.6e}; reg {l2[s, 1].item():.3e} / {sym:.3e}")
            assert np.isclose(l2[s, 0].item(), mse, rtol=2e-5)
            assert np.isclose(l2[s, 0].item() + W_SYM * l2[s, 1].item(), mse + W_SYM * sym, rtol=2e-5)
            assert_close_scaled(grad[s].cpu()[:, keep], g_all[:, keep], 3e-5, f"gradient, problem {s}")


@pytest.mark.parametrize("order,live", [(3, None), (4, None), (5, None), (4, PATTERN[4]), (5, PATTERN[5])])
def test_knob_keeps_the_streamed_step_bit_for_bit(eng, order, live):
    x, dx, gx, table, xi, mask = linear_case(3, 1030, order, eng, seed=2)
    M, _ = eng.linear_action(x, gx, table, order)
    ws = workspace(eng, x, order)
    kw = {} if live is None else {"live_columns": live}
    want = tuple(t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, **kw))
    streamed = eng.closure_body(ws)
    assert streamed == (STREAMED_DENSE[order] if live is None else "scalar-live")
    with env("SYMODE_CLOSURE_FOLD", "0"):
        got = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw)
        assert eng.closure_body(ws) == streamed
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw)
    routed = FOLD_DENSE[order] if live is None else FOLD_LIVE[order]
    assert eng.closure_body(ws) == (("fold" if live is None else "fold-live") if routed else streamed)


# ------------------------------------------------------------------------------------------------ BatchedClosure
def test_batched_closure_routing(eng):
    from symode_amd.batched import BatchedClosure
    from symode_amd.constraint import constraint_Q
    S, n, order = 3, 1030, 5
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng, seed=7, rot=True)
    Q, use_kron = constraint_Q([torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], D, order)
    Q = Q.cuda()
    g = torch.Generator().manual_seed(11)
    beta = (torch.randn(S, Q.shape[1], generator=g) * 0.3).cuda()
    const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda()

    def closure(gx_, n_g=1, **kw):
        tab = table.expand(S, n_g, D, D).contiguous()
        return BatchedClosure(x, dx, order, Q=Q, use_kron_product=use_kron, allow_constant=True, engine=eng,
                              reversed_sym=(gx_, expand(tab, n), 0.1), **kw)

    def run(clos):
        out = tuple(t.clone() for t in clos.evaluate(beta, const))
        return out, eng.closure_body(clos._ws_kw["ws"])
    # linear gx: one detection, the fold from then on
    gx_lin = gx.clone()
    fold, streamed = closure(gx_lin), closure(gx_lin, linear_action=False)
    got, body = run(fold)
    run(fold)
    assert fold.linear_detections == 1 and body == ("fold-live" if FOLD_LIVE[order] else "scalar-live")
    want, body = run(streamed)
    assert streamed.linear_detections == 0 and body == "scalar-live"
    assert np.allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=2e-5, atol=0)
    assert_close_scaled(got[1].cpu(), want[1].cpu(), 3e-5, "d/dbeta")
    assert_close_scaled(got[2].cpu(), want[2].cpu(), 3e-5, "d/dconst")
    with env("SYMODE_CLOSURE_FOLD", "0"):
        same, body = run(fold)
    assert body == "scalar-live" and all(torch.equal(a, b) for a, b in zip(same, want))
    # an in-place write to gx: detection runs again, and what is no longer linear is streamed
    gx_lin[1, 0, 517, 1] += 0.25
    got, body = run(fold)
    assert fold.linear_detections == 2 and body == "scalar-live"
    want, _ = run(streamed)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # random gx: the streamed path, bit for bit
    g = torch.Generator().manual_seed(4)
    gx_rnd = (torch.randn(gx.shape, generator=g) * 0.5).cuda()
    a, b = closure(gx_rnd), closure(gx_rnd, linear_action=False)
    (got, body), (want, _) = run(a), run(b)
    assert a.linear_detections == 1 and body == "scalar-live" and all(torch.equal(p, q) for p, q in zip(got, want))
    # two group elements: out of scope, streamed without a detection pass
    two = closure(gx.expand(S, 2, n, D).contiguous(), n_g=2)
    _, body = run(two)
    assert two.linear_detections == 0 and body == "scalar-live"
