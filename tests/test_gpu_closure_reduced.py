"""The closure without a point loop reduced to a quadratic form in (beta, const) (csrc/closure_reduced.hpp: quad_reduce_kernel,
quad_step_kernel; symode_quad_reduce / symode_quad_step; engine.quad_reduce / quad_step / quad_step_plan; BatchedClosure
``reduced=``; SYMODE_QUAD_REDUCED).

Tolerances.
B against the fp64 numpy model on the kernel's own tables (tests/closure_reduced_model.py): both sides are fp64 and sum in
different orders.  An entry of B is P^T (a d p-term sum) of a gradient whose longest chain of nested sums is W Gtt (p terms)
beside T (d + p) of U (p) of C (d + p): n_terms = d p + 3 p + 2 d.  Its two halves, P^T g(P e_i) and P^T g(0), are each of the
size of the entries of B (|B[:K, K]| is one of them), so the scale is 2 max|B| per problem and the bound
4 n_terms 2^-53 * 2 max|B| -- the factor 4 of tests/test_host_closure_reduced_model.py.
The step against the model's v^T B v on the kernel's OWN B: every output is formed in fp64 and rounded to fp32 once, 2^-24 of
the output's scale, plus the fp64 term of two nested (K+1)-term sums on the magnitudes, 2 (K + 1) 2^-53 |v|^T |B| |v| for the
loss and 2 (K + 1) 2^-53 * 2 max_i (|B|^T |v|)_i for the gradient.
``evaluate`` on the reduced route against ``reduced=False``: 16 * 2^-24 of scale per output, the figure the project holds the
fp32-map and fp64-map steps to (tests/test_gpu_closure_quad.py).
S = 5 and S = 17: with four waves (quad_reduce) and sixteen lane groups (quad_step) to a workgroup both are ragged last
workgroups, and S = 17 is a second workgroup of the step."""
import numpy as np
import pytest
import torch

from symode_amd.coef_map import CoefMap
from tests.closure_reduced_model import quad_reduce, quad_step
from tests.test_gpu_closure_fold import columns_of
from tests.test_gpu_closure_fold_gram import batched_inputs
from tests.test_gpu_closure_live import env
from tests.test_gpu_closure_quad import ALL, D, N, device_case, make_closure, so2_map
from tests.test_gpu_constj import assert_close_scaled

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E = 2.0 ** -53
STEP_GROUPS = 16                     # problems per workgroup of quad_step_kernel (closure_reduced.hpp: REDUCED_PER_BLOCK)
SIZES = (5, STEP_GROUPS + 1)


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def the_map(order, kron, allow_constant):
    """the so2 constraint's map in its (d, p) view, or the same map with Q's rows in the transposed (p, d) order"""
    cmap = so2_map(order, "so2", allow_constant)
    if kron:
        return cmap
    p = cmap.p
    rows = (np.arange(p)[:, None] + p * np.arange(D)[None, :]).reshape(-1)      # row k d + j of the (p, d) view is row j p + k
    return CoefMap(D, p, cmap.Q[torch.from_numpy(rows).cuda()].contiguous(), False, allow_constant)


@pytest.mark.parametrize("allow_constant", [True, False])
@pytest.mark.parametrize("kron", [True, False])
@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("S", SIZES)
def test_reduce_and_step_against_the_model(eng, S, order, kron, allow_constant):
    x, dx, gx, table, M, A, ws = device_case(S, order)
    cmap = the_map(order, kron, allow_constant)
    p, r = cmap.p, cmap.r
    dc = D if allow_constant else 0
    K = r + dc
    inv = 1.0 / (N * D)
    n_terms = D * p + 3 * p + 2 * D
    Qn = cmap.Q.cpu().numpy()
    g = torch.Generator().manual_seed(1000 * order + 10 * S + 2 * kron + allow_constant)
    beta = (torch.randn(S, r, generator=g) * 0.3).cuda()
    const = (torch.randn(S, D, 1, generator=g) * 0.1).cuda() if allow_constant else None
    state = torch.cat([beta, torch.zeros(S, D, device="cuda") if const is None else const.view(S, D)], dim=1).contiguous()
    for live in (ALL, so2_map(order).live_mask()):
        keep = columns_of(order, live).numpy()
        for w in (0.0, 0.37):
            what = f"S={S} order={order} kron={kron} const={allow_constant} live={live:#x} w={w}"
            B = eng.quad_reduce(A, M, table, order, cmap, w, inv, live_columns=live)
            assert B.shape == (S, K + 1, K + 1) and torch.equal(B, B.transpose(1, 2))
            Bn = B.cpu().numpy()
            worst = 0.0
            for s in range(S):
                want = quad_reduce(A[s].cpu().numpy(), M[s, 0].cpu().numpy(), table[s, 0].cpu().double().numpy(), Qn, cmap.use_kron,
                                   allow_constant, None, keep, float(np.float32(w)), inv)
                tol = 4.0 * n_terms * E * 2.0 * np.abs(want).max()
                err = np.abs(Bn[s] - want).max()
                worst = max(worst, err / tol)
                assert err <= tol, (what, s, err, tol)
            print(f"{what}: B worst error / bound {worst:.3f}")
            for strided in (False, True):
                if strided:
                    b_in, c_in = state[:, :r], (state[:, r:].unsqueeze(-1) if allow_constant else None)
                    assert b_in.stride(0) == r + D and not b_in.is_contiguous()
                else:
                    b_in, c_in = beta, const
                loss = torch.full((S,), float("nan"), device="cuda")
                g_beta = torch.full((S, r), float("nan"), device="cuda")
                g_const = torch.full((S, D, 1), float("nan"), device="cuda") if allow_constant else None
                out = eng.quad_step(B, b_in, c_in, order, live_columns=live, out=(loss, g_beta, g_const), ws=ws)
                assert out[0].data_ptr() == loss.data_ptr() and (out[2] is None) == (not allow_constant)
                assert eng.closure_reduced(ws) and eng.closure_quad(ws) and eng.closure_gram(ws)
                worst_l = worst_g = 0.0
                for s in range(S):
                    z = state[s, :K].cpu().double().numpy()
                    wl, wg = quad_step(Bn[s], z)
                    v = np.abs(np.concatenate([z, [1.0]]))
                    tol_l = U * abs(wl) + 2 * (K + 1) * E * float(v @ np.abs(Bn[s]) @ v)
                    tol_g = U * np.abs(wg).max() + 2 * (K + 1) * E * 2.0 * float((np.abs(Bn[s]).T @ v).max())
                    got_g = np.concatenate([g_beta[s].cpu().numpy().reshape(-1)] + ([g_const[s].cpu().numpy().reshape(-1)] if allow_constant else []))
                    el, eg = abs(loss[s].item() - wl), np.abs(got_g - wg).max()
                    worst_l, worst_g = max(worst_l, el / tol_l), max(worst_g, eg / tol_g)
                    assert el <= tol_l, (what, strided, s, "loss", el, tol_l)
                    assert eg <= tol_g, (what, strided, s, "gradient", eg, tol_g)
                print(f"{what} strided={strided}: step worst error / bound, loss {worst_l:.3f} gradient {worst_g:.3f}")


# ------------------------------------------------------------------------------------------------ BatchedClosure
def clones(out):
    return tuple(None if t is None else t.clone() for t in out)


@pytest.mark.parametrize("S", SIZES)
def test_evaluate_against_todays_step(eng, S):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, S)
    new, old = make_closure(eng, x, dx, gx, table, Q, use_kron), make_closure(eng, x, dx, gx, table, Q, use_kron, reduced=False)
    got, want = clones(new.evaluate(beta, const)), clones(old.evaluate(beta, const))
    ws, ws_old = new._ws_kw["ws"], old._ws_kw["ws"]
    assert new.reduced_builds == 1 and old.reduced_builds == 0
    assert eng.closure_reduced(ws) and eng.closure_quad(ws) and eng.closure_gram(ws) and eng.closure_body(ws) == "fold-live"
    assert not eng.closure_reduced(ws_old) and eng.closure_quad(ws_old) and eng.closure_body(ws_old) == "fold-live"
    for a, b, what in zip(got, want, ("loss", "d/dbeta", "d/dconst")):
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous()
        assert_close_scaled(a.cpu(), b.cpu(), 16 * U, what)
    # every column live: the header names the dense fold kernel, as today's step does
    dense = make_closure(eng, x, dx, gx, table, Q, use_kron, live_columns=False)
    dense_old = make_closure(eng, x, dx, gx, table, Q, use_kron, live_columns=False, reduced=False)
    got, want = clones(dense.evaluate(beta, const)), clones(dense_old.evaluate(beta, const))
    assert eng.closure_reduced(dense._ws_kw["ws"]) and eng.closure_body(dense._ws_kw["ws"]) == "fold" == eng.closure_body(dense_old._ws_kw["ws"])
    for a, b, what in zip(got, want, ("loss", "d/dbeta", "d/dconst")):
        assert_close_scaled(a.cpu(), b.cpu(), 16 * U, what + ", every column live")


def test_switches_give_todays_step_bit_for_bit_and_the_header_tells(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, 5)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    ws = clos._ws_kw["ws"]
    clos.evaluate(beta, const)
    assert eng.closure_reduced(ws) and clos.reduced_builds == 1
    # today's step, spelt out: the one launch with the map in it
    A = eng.aug_gram(x, dx, 5)
    loss = torch.empty(5, device="cuda")
    want = eng.loss_grad_reversed(x, dx, gx, table, None, None, 5, 0, w_sym=0.1, inv_count=clos.inv_count, ws=ws, live_columns=clos._live,
                                  linear_m=clos._lin_m, aug=A, coef=(clos.coef, beta, const),
                                  out=(torch.empty(5, 2, device="cuda"), torch.empty(5, D, clos.p, device="cuda"), loss))
    want = (loss,) + clones(want[2:])
    assert not eng.closure_reduced(ws) and eng.closure_quad(ws)
    with env("SYMODE_QUAD_REDUCED", "0"):
        assert not eng.closure_reduced_enabled() and eng.closure_quad_enabled()
        off = clones(clos.evaluate(beta, const))
        assert not eng.closure_reduced(ws) and eng.closure_quad(ws) and eng.closure_gram(ws) and eng.closure_body(ws) == "fold-live"
    param = make_closure(eng, x, dx, gx, table, Q, use_kron, reduced=False)
    off2 = clones(param.evaluate(beta, const))
    assert not eng.closure_reduced(param._ws_kw["ws"]) and param.reduced_builds == 0
    for a, b, c, what in zip(off, off2, want, ("loss", "d/dbeta", "d/dconst")):
        assert torch.equal(a, b) and torch.equal(a, c), what
    clos.evaluate(beta, const)
    assert eng.closure_reduced(ws) and clos.reduced_builds == 1


def test_rebuilds_follow_the_keys(eng):
    def fresh(x, dx, gx, w):
        c = make_closure(eng, x, dx, gx, table, Q, use_kron, reduced=False)
        c.sym = c.sym[:2] + (w,)
        return clones(c.evaluate(beta, const))

    def same(got, want, what):
        for a, b, name in zip(got, want, ("loss", "d/dbeta", "d/dconst")):
            assert_close_scaled(a.cpu(), b.cpu(), 16 * U, f"{what}: {name}")
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, 5)
    for change in ("dx", "x", "w_sym"):
        xs, dxs, gxs = x.clone(), dx.clone(), gx.clone()
        clos = make_closure(eng, xs, dxs, gxs, table, Q, use_kron)
        first = clones(clos.evaluate(beta, const))
        clos.evaluate(beta, const)
        assert clos.reduced_builds == 1, change
        same(first, fresh(xs, dxs, gxs, 0.1), "as built")
        w = 0.1
        if change == "dx":
            dxs.mul_(1.25)
        elif change == "x":
            xs.mul_(1.25)
            gxs.copy_(torch.einsum("sgab,snb->sgna", table.double(), xs.double()).float())
        else:
            w = 5.0                                        # the regulariser is about 1e-3 of these losses: a weight that shows
            clos.sym = clos.sym[:2] + (w,)
        second = clones(clos.evaluate(beta, const))
        clos.evaluate(beta, const)
        assert clos.reduced_builds == 2 and eng.closure_reduced(clos._ws_kw["ws"]), change
        same(second, fresh(xs, dxs, gxs, w), "after " + change)
        assert not np.allclose(second[0].cpu().numpy(), first[0].cpu().numpy(), rtol=1e-3, atol=0), change


def test_a_mask_and_a_capture_keep_todays_kernel(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, 5)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    old = make_closure(eng, x, dx, gx, table, Q, use_kron, reduced=False)
    ws = clos._ws_kw["ws"]
    mask = (torch.rand(5, D, clos.p, generator=torch.Generator().manual_seed(3)) > 0.25).float().cuda()
    got, want = clones(clos.evaluate(beta, const, mask=mask)), clones(old.evaluate(beta, const, mask=mask))
    assert clos.reduced_builds == 0 and not eng.closure_reduced(ws) and eng.closure_quad(ws)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # B is missing: a call under capture builds nothing and records today's launch
    want = clones(old.evaluate(beta, const))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = clos.evaluate(beta, const)
    assert clos.reduced_builds == 0
    graph.replay()
    torch.cuda.synchronize()
    assert not eng.closure_reduced(ws) and eng.closure_quad(ws)
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    # outside the capture the form is built, and a masked call after it still leaves the count alone
    clos.evaluate(beta, const)
    assert clos.reduced_builds == 1 and eng.closure_reduced(ws)
    clos.evaluate(beta, const, mask=mask)
    assert clos.reduced_builds == 1 and not eng.closure_reduced(ws)


def test_returned_tensors_are_fresh_unless_aliased(eng):
    x, dx, gx, table, Q, use_kron, beta, const = batched_inputs(eng, 5)
    clos = make_closure(eng, x, dx, gx, table, Q, use_kron)
    a = clos.evaluate(beta, const)
    kept = clones(a)
    b = clos.evaluate(beta * 1.5, const)
    assert all(torch.equal(p, q) for p, q in zip(a, kept)) and not torch.equal(a[0], b[0])
    c = clos.evaluate(beta, const, alias=True)
    assert all(torch.equal(p, q) for p, q in zip(c, kept))
    d = clos.evaluate(beta * 1.5, const, alias=True)
    assert all(p.data_ptr() == q.data_ptr() for p, q in zip(c, d))
    assert all(torch.equal(p, q) for p, q in zip(d, b))
    assert eng.closure_reduced(clos._ws_kw["ws"]) and clos.reduced_builds == 1
    # rows of a flat [beta | const] state, as the sweep passes them
    state = clos.coef.join(beta, const).contiguous()
    e = clos.evaluate(*clos.coef.split(state))
    assert all(torch.equal(p, q) for p, q in zip(e, kept))


def test_route_limits(eng):
    """K + 1 > 16: the variables are Xi itself, or a map with more than 13 columns beside the two constants"""
    from symode_amd.batched import BatchedClosure
    from tests.test_gpu_constj import expand
    S, order = 5, 5
    x, dx, gx, table, M, A, _ = device_case(S, order)
    free = BatchedClosure(x, dx, order, engine=eng, reversed_sym=(gx, expand(table, N), 0.37))
    xi = (torch.randn(S, D, free.p, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
    free.evaluate(xi)
    assert not free._reduced_on and free.reduced_builds == 0 and not eng.closure_reduced(free._ws_kw["ws"]) and eng.closure_quad(free._ws_kw["ws"])
    g = torch.Generator().manual_seed(6)
    Q = (torch.randn(D * free.p, 14, generator=g) * 0.3).cuda()
    beta, const = (torch.randn(S, 14, generator=g) * 0.3).cuda(), (torch.randn(S, D, 1, generator=g) * 0.1).cuda()
    kw = dict(Q=Q, use_kron_product=True, allow_constant=True, engine=eng, reversed_sym=(gx, expand(table, N), 0.37))
    wide, old = BatchedClosure(x, dx, order, **kw), BatchedClosure(x, dx, order, reduced=False, **kw)
    got, want = clones(wide.evaluate(beta, const)), clones(old.evaluate(beta, const))
    assert not wide._reduced_on and wide.reduced_builds == 0 and not eng.closure_reduced(wide._ws_kw["ws"]) and eng.closure_quad(wide._ws_kw["ws"])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # thirteen columns fit: K + 1 = 16
    kw["Q"] = Q[:, :13].contiguous()
    fits, old = BatchedClosure(x, dx, order, **kw), BatchedClosure(x, dx, order, reduced=False, **kw)
    got, want = clones(fits.evaluate(beta[:, :13].contiguous(), const)), clones(old.evaluate(beta[:, :13].contiguous(), const))
    assert fits.reduced_builds == 1 and eng.closure_reduced(fits._ws_kw["ws"])
    for a, b, what in zip(got, want, ("loss", "d/dbeta", "d/dconst")):
        assert_close_scaled(a.cpu(), b.cpu(), 16 * U, what + ", K + 1 = 16")
