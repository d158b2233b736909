"""The Gram form of the fold closure (closure_fold.hpp: symreg_fold_kernel<FoldGram<..>, ..>; symode_loss_grad_reversed_linear_gram;
engine ``gram=``; BatchedClosure ``regulariser_gram=``; SYMODE_FOLD_GRAM): the regulariser and its gradient come from the
library Gram matrix G = sum_n Theta Theta^T of each problem, once per problem and launch in fp64, and the point loop carries
the residual alone.

The point loop's sums are the plain fold kernel's statements on the same chunk-to-lane assignment, so loss2[:, 0], and with
w_sym = 0 the gradient, are held to torch.equal with symode_loss_grad_reversed_linear on the same grid.  With w_sym = 0.37 the
regulariser and the gradient are held to the fp64 closure at the bounds of tests/test_gpu_closure_fold.py (loss rtol 2e-5,
gradient 3e-5 of its scale) and to the fp64 numpy restatement of the term (tests/test_host_fold_gram_model.py: gram_term) on
the device's own G within two fp32 roundings of the output's scale:
  * loss2[:, 1] = fl32(value * inv32): value is formed in fp64 from the same fp32 inputs (its own error, a few 2^-53 of the
    products that make up C, is far below fp32), inv32 is the fp32 factor the launch was given and is used as such in the
    restatement: ONE rounding, to fp32 on the way out;
  * gradient = fl32((R + w T) * 2 inv32) * mask against  fl32(R * 2 inv32) * mask + 2 inv32 w T mask, the first term being the
    device's own gradient at w_sym = 0 (the same R bits): ONE rounding on each side of the comparison, TWO in all, each at
    most 2^-24 of the gradient's largest entry.
A further 1e-13 of scale covers the fp64 sums' own order (the device adds U and T in column order, numpy however it likes).

Every case runs on the launcher's grid, on ONE workgroup per problem and on three (tests/test_gpu_closure_fold_pk.py: the
ring's steady state, and the once-per-problem addition with one, two and three rows per problem).  SYMODE_FOLD_GRAM=2 brings
the Gram kernel to the instantiations the launcher's table leaves out."""
import numpy as np
import pytest
import torch

from tests.test_gpu_closure_fold import columns_of, fp64_closure, linear_case, workspace
from tests.test_gpu_closure_fold_pk import grid_cap
from tests.test_gpu_closure_live import PATTERN, env
from tests.test_gpu_constj import assert_close_scaled, expand
from tests.test_host_fold_gram_model import gram_term

pytestmark = pytest.mark.gpu

D, W_SYM, U = 2, 0.37, 2.0 ** -24
W32 = float(np.float32(W_SYM))
ALL = 0xFFFFFFFFFFFFFFFF
# the launcher's table (closure_fold.hpp: closure_fold_gram_pays), (order, odd set?) -> the Gram form by default
ROUTED = {(1, False): False, (2, False): False, (3, False): True, (4, False): True, (5, False): True, (4, True): False, (5, True): True}
SIZES = (1, 2, 7, 1023, 1026, 2048, 4099, 7834)
GRIDS = (None, 1, 3)
INSTANCES = [(o, None) for o in (1, 2, 3, 4, 5)] + [(4, PATTERN[4]), (5, PATTERN[5]), (4, PATTERN[4] & ~1), (5, PATTERN[5] & ~(1 | 1 << 7))]


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def library_gram(eng, x, dx, order):
    """(S, 1, p, p) fp64 raw sums: the top-left block of the augmented Gram matrix"""
    p = eng.lib_size(D, order, 0)
    return eng.aug_gram(x, dx, order)[:, None, :p, :p].contiguous()


def check(eng, case, order, live, masked, refs, G, M, what):
    """one grid: the Gram form against the plain fold kernel (bits) and against the two fp64 references"""
    x, dx, gx, table, xi, mask = case
    mask = mask if masked else None
    S, n = x.shape[0], x.shape[1]
    ws = workspace(eng, x, order)
    kw = {} if live is None else {"live_columns": live}
    body = "fold" if live is None else "fold-live"

    def run(w, **more):
        out = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=w, ws=ws, linear_m=M, **kw, **more)
        return tuple(t.clone() for t in out), eng.closure_body(ws), eng.closure_gram(ws), eng.closure_levers(ws)
    (pl, pg), b0, g0, lev0 = run(W_SYM)
    (pl0, pg0), _, _, _ = run(0.0)
    (gl, gg), b1, g1, lev1 = run(W_SYM, gram=G)
    (gl0, gg0), _, _, _ = run(0.0, gram=G)
    assert (b0, g0, b1, g1, lev1) == (body, False, body, True, (False, False)), (what, b0, g0, b1, g1, lev0, lev1)
    assert torch.isfinite(gl).all() and torch.isfinite(gg).all() and gg.abs().max() > 0, what
    assert torch.equal(gl[:, 0], pl[:, 0]) and torch.equal(gl0[:, 0], pl0[:, 0]), f"{what}: mse"
    assert torch.equal(gg0, pg0), f"{what}: gradient at w_sym = 0"
    again, _, _, _ = run(W_SYM, gram=G)
    assert torch.equal(again[0], gl) and torch.equal(again[1], gg), f"{what}: a second launch"
    inv32 = float(np.float32(1.0 / (n * D)))
    keep = refs["keep"]
    for s in range(S):
        mse, sym, g_all = refs["fp64"][s]
        rel = abs(gl[s, 1].item() - sym) / sym
        print(f"{what} s={s}: regulariser gram {rel:.2e} plain {abs(pl[s, 1].item() - sym) / sym:.2e} of the fp64 closure")
        assert np.isclose(gl[s, 1].item(), sym, rtol=2e-5), (what, s, gl[s, 1].item(), sym)
        assert_close_scaled(gg[s].cpu()[:, keep], g_all[:, keep], 3e-5, f"{what}: gradient, problem {s}")
        assert (gg[s].cpu()[:, ~keep] == 0).all()
        value, T = refs["term"][s]
        want = value * inv32
        assert abs(gl[s, 1].item() - want) <= (2 * U + 1e-13) * abs(want), (what, s, gl[s, 1].item(), want)
        m = np.ones((D, len(keep))) if mask is None else mask[s].cpu().double().numpy()
        want = gg0[s].cpu().double().numpy() + 2.0 * inv32 * m * T
        got = gg[s].cpu().double().numpy()
        scale = max(np.abs(got).max(), np.abs(want).max())
        assert np.abs(got - want).max() <= (2 * U + 1e-13) * scale, (what, s, np.abs(got - want).max() / scale)


def references(eng, case, order, live, masked, G, M):
    """per problem: the fp64 closure, and the numpy restatement of the term on the device's G (shared by the grids)"""
    x, dx, gx, table, xi, mask = case
    keep = columns_of(order, ALL if live is None else live)
    out = {"keep": keep, "fp64": [], "term": []}
    for s in range(x.shape[0]):
        out["fp64"].append(fp64_closure(x[s], dx[s], table[s], xi[s], mask[s] if masked else None, order, W_SYM))
        out["term"].append(gram_term(table[s, 0].cpu().double().numpy(), M[s, 0].cpu().numpy(), G[s, 0].cpu().numpy(),
                                     xi[s].cpu().double().numpy(), mask[s].cpu().double().numpy() if masked else None,
                                     keep.numpy(), W32))
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("order,live", INSTANCES)
def test_gram_form_against_the_plain_fold_kernel_and_fp64(eng, order, live, S, masked):
    with env("SYMODE_FOLD_GRAM", "2"):
        for n in SIZES:
            x, dx, gx, table, xi, mask = linear_case(S, n, order, eng)
            xi = xi * columns_of(order, ALL if live is None else live).cuda()
            case = (x, dx, gx, table, xi, mask)
            M, linear = eng.linear_action(x, gx, table, order)
            assert linear
            G = library_gram(eng, x, dx, order)
            refs = references(eng, case, order, live, masked, G, M)
            for gx_ in GRIDS:
                with grid_cap(gx_, S):
                    check(eng, case, order, live, masked, refs, G, M, f"order={order} live={live} S={S} n={n} masked={masked} grid={gx_}")


@pytest.mark.parametrize("order,live", [(5, None), (5, PATTERN[5]), (4, PATTERN[4]), (3, None)])
def test_x_offset_by_one_float(eng, order, live):
    """x starts 4 bytes past a 16-byte boundary: no 16-byte vectors, every point by per-lane loads"""
    with env("SYMODE_FOLD_GRAM", "2"):
        for n in (7, 1026):
            x, dx, gx, table, xi, mask = linear_case(1, n, order, eng, seed=3)
            xi = xi * columns_of(order, ALL if live is None else live).cuda()
            buf = torch.zeros(x.numel() + 1, dtype=torch.float32, device=x.device)
            buf[1:] = x.reshape(-1)
            xo = buf[1:].view(x.shape)
            assert xo.data_ptr() % 16 == 4 and torch.equal(xo, x)
            case = (xo, dx, gx, table, xi, mask)
            M, linear = eng.linear_action(xo, gx, table, order)
            assert linear
            G = library_gram(eng, xo, dx, order)
            refs = references(eng, case, order, live, True, G, M)
            for grid in (None, 1):
                with grid_cap(grid, 1):
                    check(eng, case, order, live, True, refs, G, M, f"offset x, order={order} live={live} n={n} grid={grid}")


@pytest.mark.parametrize("order,live", INSTANCES)
def test_table_and_knob(eng, order, live):
    """by default the launcher's table decides; SYMODE_FOLD_GRAM=0 is the entry without the table, bit for bit"""
    x, dx, gx, table, xi, mask = linear_case(3, 1026, order, eng, seed=2)
    xi = xi * columns_of(order, ALL if live is None else live).cuda()
    M, _ = eng.linear_action(x, gx, table, order)
    G = library_gram(eng, x, dx, order)
    ws = workspace(eng, x, order)
    kw = {} if live is None else {"live_columns": live}
    want = tuple(t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw))
    assert not eng.closure_gram(ws)
    got = tuple(t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, gram=G, **kw))
    routed = ROUTED[(order, live is not None)]
    assert eng.closure_gram(ws) == routed and eng.closure_body(ws) == ("fold" if live is None else "fold-live")
    if not routed:
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for knob in ("0",):
        with env("SYMODE_FOLD_GRAM", knob):
            off = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, gram=G, **kw)
            assert not eng.closure_gram(ws) and torch.equal(off[0], want[0]) and torch.equal(off[1], want[1])
    with env("SYMODE_CLOSURE_FOLD", "0"):
        streamed = tuple(t.clone() for t in eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, **kw))
        off = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, gram=G, **kw)
        assert torch.equal(off[0], streamed[0]) and torch.equal(off[1], streamed[1])


@pytest.mark.parametrize("order,live,S", [(5, PATTERN[5], 3), (5, None, 3), (3, None, 1), (4, PATTERN[4] & ~1, 1)])
def test_finalisation_modes_give_equal_bytes(eng, order, live, S):
    x, dx, gx, table, xi, mask = linear_case(S, 4099, order, eng, seed=4)
    xi = xi * columns_of(order, ALL if live is None else live).cuda()
    M, _ = eng.linear_action(x, gx, table, order)
    G = library_gram(eng, x, dx, order)
    kw = {} if live is None else {"live_columns": live}
    with env("SYMODE_FOLD_GRAM", "2"):
        for grid in GRIDS:
            outs = []
            for mode in ("1", "0", "2"):
                with env("SYMODE_FUSED_FINALIZE", mode), grid_cap(grid, S):
                    ws = workspace(eng, x, order)
                    out = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, gram=G, **kw)
                    outs.append(tuple(t.clone() for t in out))
                    assert eng.closure_gram(ws), (mode, grid)
            for mode, o in zip(("0", "2"), outs[1:]):
                assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), f"SYMODE_FUSED_FINALIZE={mode}, grid {grid}"
            assert outs[0][0][:, 1].abs().min() > 0


# ------------------------------------------------------------------------------------------------ BatchedClosure
def batched_inputs(eng, S=3, n=1030, order=5):
    from symode_amd.constraint import constraint_Q
    x, dx, gx, table, _, _ = linear_case(S, n, order, eng, seed=7, rot=True)
    Q, use_kron = constraint_Q([torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], D, order)
    g = torch.Generator().manual_seed(11)
    beta = (torch.randn(S, Q.shape[1], generator=g) * 0.3).cuda()
    const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda()
    return x, dx, gx, table, Q.cuda(), use_kron, beta, const


def test_batched_closure_routing_and_rebuild(eng):
    from symode_amd.batched import BatchedClosure
    S, n, order = 3, 1030, 5
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, S, n, order)
    x = x.clone()

    def closure(xs=x, dxs=dx, gxs=gx, **kw):
        return BatchedClosure(xs, dxs, order, Q=Q, use_kron_product=use_kron, allow_constant=True, engine=eng,
                              reversed_sym=(gxs, expand(table, xs.shape[1]), 0.1), **kw)

    def run(clos):
        out = tuple(t.clone() for t in clos.evaluate(beta, const))
        ws = clos._ws_kw["ws"]
        return out, eng.closure_body(ws), eng.closure_gram(ws)
    gram, plain = closure(), closure(regulariser_gram=False)
    got, body, took = run(gram)
    run(gram)
    assert gram.gram_builds == 1 and plain.gram_builds == 0 and (body, took) == ("fold-live", True)
    want, body, took = run(plain)                      # the parent's route: the fold closure given no Gram table
    assert (body, took) == ("fold-live", False)
    assert np.allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=2e-5, atol=0)
    assert_close_scaled(got[1].cpu(), want[1].cpu(), 3e-5, "d/dbeta")
    assert_close_scaled(got[2].cpu(), want[2].cpu(), 3e-5, "d/dconst")
    with env("SYMODE_FOLD_GRAM", "0"):
        off, body, took = run(gram)
    assert (body, took) == ("fold-live", False) and all(torch.equal(a, b) for a, b in zip(off, want))
    # an in-place write to x (gx follows it: the action stays linear): exactly one rebuild, and the result follows the new data
    x.mul_(1.25)
    gx.copy_(torch.einsum("sgab,snb->sgna", table.double(), x.double()).float())
    got2, body, took = run(gram)
    run(gram)
    assert gram.gram_builds == 2 and (body, took) == ("fold-live", True)
    fresh, _, _ = run(closure(regulariser_gram=False))
    assert np.allclose(got2[0].cpu().numpy(), fresh[0].cpu().numpy(), rtol=2e-5, atol=0)
    assert_close_scaled(got2[1].cpu(), fresh[1].cpu(), 3e-5, "d/dbeta on the new data")
    assert_close_scaled(got2[2].cpu(), fresh[2].cpu(), 3e-5, "d/dconst on the new data")
    assert not np.allclose(got2[0].cpu().numpy(), got[0].cpu().numpy(), rtol=1e-3, atol=0)


def test_two_half_shards_sum_to_the_single_shard(eng):
    from symode_amd.batched import BatchedClosure
    S, n, order = 3, 2060, 5
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, S, n, order)

    def closure(lo, hi, **kw):
        return BatchedClosure(x[:, lo:hi].contiguous(), dx[:, lo:hi].contiguous(), order, Q=Q, use_kron_product=use_kron,
                              allow_constant=True, engine=eng,
                              reversed_sym=(gx[:, :, lo:hi].contiguous(), expand(table, hi - lo), 0.1), **kw)
    whole = closure(0, n)
    want = tuple(t.clone() for t in whole.evaluate(beta, const))
    halves = [closure(0, n // 2, world_size=2), closure(n // 2, n, world_size=2)]
    parts = [tuple(t.clone().double() for t in h.evaluate(beta, const)) for h in halves]
    for h in halves:
        assert h.gram_builds == 1 and eng.closure_gram(h._ws_kw["ws"])
    # "within fp32 rounding": each shard's outputs are rounded to fp32 once and so is the single shard's, three roundings of
    # the result's scale; the split also regroups the kernels' fp32 sums over the points -- at 2060 points and the launcher's
    # grid a lane holds at most two chunks, so a sum's fp32 part is a handful of terms and the regrouping moves it by a few
    # units more; the Gram term itself is linear in G and fp64.  16 units of 2^-24 in all.
    for a, b, c, what in zip(parts[0], parts[1], want, ("loss", "d/dbeta", "d/dconst")):
        assert_close_scaled((a + b).cpu(), c.cpu(), 16 * U, what)
