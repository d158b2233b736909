"""Point-constant group Jacobian: the closure kernels' compact-table form (symode_loss_grad_reversed_constj /
symode_symreg_reversed_batched_constj), the detection pass (symode_jacobian_constant) and BatchedClosure's use of both.

The compact form keeps the arithmetic, its order and the chunk-to-lane assignment of the materialised form, so it is held
to BIT identity with the existing entries on the expanded (S, n_g, N, d, d) Jacobian; against the oracle it is held to
the tolerances of test_gpu_kernels.py::test_fused_closure_mse_plus_reversed_regulariser (loss rtol 2e-5, gradient 3e-5 of
its scale)."""
import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def assert_close_scaled(got, want, rtol, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max() / scale
    assert err <= rtol, f"{what}: max scaled error {err:.3e} > {rtol}"


def make_case(S, n, n_g, d, order, eng, seed=0, offset_points=0):
    """x, dx (S, n, d), gx (S, n_g, n, d), a distinct random matrix per (problem, group element), Xi and a non-trivial mask;
    ``offset_points``: every point array starts that many points into its allocation (an unaligned base)."""
    g = torch.Generator().manual_seed(1000 * S + 10 * n + n_g + d + seed)
    p = eng.lib_size(d, order, 0)
    m = n + offset_points
    x = (torch.randn(S, m, d, generator=g) * 0.5).cuda()[:, offset_points:]
    dx = torch.randn(S, m, d, generator=g).cuda()[:, offset_points:]
    gx = (torch.randn(S, n_g, m, d, generator=g) * 0.5).cuda()[:, :, offset_points:]
    table = (torch.eye(d) + 0.3 * torch.randn(S, n_g, d, d, generator=g)).cuda()
    xi = (torch.randn(S, d, p, generator=g) * 0.3).cuda()
    mask = (torch.rand(S, d, p, generator=g) > 0.25).float().cuda()
    return x, dx, gx, table, xi, mask


def expand(table, n):
    S, n_g, d, _ = table.shape
    return table[:, :, None].expand(S, n_g, n, d, d).contiguous()


# (S, n, n_g, d, order, offset_points)
BIT_CASES = (
    # the vector ring with a point tail (N even: slabs stay 16-byte aligned), and odd N with S > 1 (per-point path)
    [(3, n, n_g, 2, order, 0) for n in (1030, 1031) for order in (5, 3) for n_g in (1, 2)]
    + [(1, 1030, 1, 2, 3, 1),          # one problem whose base is offset by one point: unaligned, per-point path
       (2, 2052, 1, 3, 2, 0),          # d = 3: full-wave tile path, ragged last wave
       (2, 2052, 2, 3, 2, 0),
       (1, 1030, 2, 1, 3, 0),          # d = 1
       (3, 6, 2, 2, 3, 0)])            # fewer chunks than lanes


@pytest.mark.parametrize("S,n,n_g,d,order,off", BIT_CASES)
def test_compact_table_is_bit_identical_to_the_materialised_jacobian(eng, S, n, n_g, d, order, off):
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, d, order, eng, offset_points=off)
    if off:
        assert S == 1 and n_g == 1 and x.data_ptr() % 16 != 0 and x.is_contiguous() and gx.is_contiguous()
    jgx = expand(table, n)
    w = 0.37
    ref_l2, ref_g = eng.loss_grad_reversed(x, dx, gx, jgx, xi, mask, order, 0, w_sym=w)
    got_l2, got_g = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=w)
    assert got_l2.shape == (S, 2) and got_g.shape == ref_g.shape
    assert torch.isfinite(ref_l2).all() and ref_g.abs().max() > 0
    assert torch.equal(got_l2, ref_l2), "fused closure: loss"
    assert torch.equal(got_g, ref_g), "fused closure: gradient"
    ref_l, ref_gs = eng.symreg_reversed(x, gx, jgx, xi, mask, order, 0)
    got_l, got_gs = eng.symreg_reversed(x, gx, table, xi, mask, order, 0)
    assert torch.equal(got_l, ref_l), "regulariser alone: loss"
    assert torch.equal(got_gs, ref_gs), "regulariser alone: gradient"


def test_one_problem_form_takes_the_compact_table_too(eng):
    x, dx, gx, table, xi, mask = make_case(1, 1030, 2, 2, 3, eng)
    jgx = expand(table, 1030)
    ref = eng.loss_grad_reversed(x[0], dx[0], gx[0], jgx[0], xi[0], mask[0], 3, 0, w_sym=0.2)
    got = eng.loss_grad_reversed(x[0], dx[0], gx[0], table[0], xi[0], mask[0], 3, 0, w_sym=0.2)
    assert got[0].shape == (2,) and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    ref = eng.symreg_reversed(x[0], gx[0], jgx[0], xi[0], mask[0], 3, 0)
    got = eng.symreg_reversed(x[0], gx[0], table[0], xi[0], mask[0], 3, 0)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_compact_table_against_the_oracle(eng):
    S, n, n_g, d, order, w = 3, 1030, 2, 2, 5, 0.37
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, d, order, eng)
    loss2, grad = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=w)
    l_s, g_s = eng.symreg_reversed(x, gx, table, xi, mask, order, 0)
    jgx = expand(table, n).cpu()
    xc, dxc, gxc, xic, mc = x.cpu(), dx.cpu(), gx.cpu(), xi.cpu(), mask.cpu()
    for s in range(S):
        reg = O.OracleRegressor(d, order, False, False, Xi0=xic[s])
        reg.mask = mc[s]
        mse = torch.nn.functional.mse_loss(reg(xc[s]), dxc[s])
        sym = O.symreg_reversed_precomputed(xc[s], list(gxc[s]), list(jgx[s]), reg)
        g_sym, = torch.autograd.grad(sym, reg.Xi, retain_graph=True)
        (mse + w * sym).backward()
        assert np.isclose(loss2[s, 0].item(), mse.item(), rtol=2e-5) and np.isclose(loss2[s, 1].item(), sym.item(), rtol=2e-5)
        assert_close_scaled(grad[s].cpu(), reg.Xi.grad * mc[s], 3e-5, f"fused closure grad, problem {s}")
        assert np.isclose(l_s[s].item(), sym.item(), rtol=2e-5)
        assert_close_scaled(g_s[s].cpu(), g_sym * mc[s], 3e-5, f"regulariser grad, problem {s}")


# ---------------------------------------------------------------------------------------- the detection pass
def constant_jacobian(n, d, S=3, n_g=2, seed=0):
    g = torch.Generator().manual_seed(7 * n + d + seed)
    table = torch.randn(S, n_g, d, d, generator=g).cuda()
    return table, expand(table, n)


DETECT_SHAPES = [(n, d) for n in (6, 1031) for d in (2, 3)]


@pytest.mark.parametrize("n,d", DETECT_SHAPES)
def test_detector_accepts_constant_slabs_with_a_distinct_matrix_each(eng, n, d):
    table, jgx = constant_jacobian(n, d)
    assert len({tuple(m.flatten().tolist()) for m in table.reshape(-1, d, d).cpu()}) == 6
    got, const = eng.jacobian_constant(jgx)
    assert const is True and got.shape == table.shape and torch.equal(got, table)
    got1, const1 = eng.jacobian_constant(jgx[1])                 # one problem: (n_g, N, d, d) -> (n_g, d, d)
    assert const1 is True and torch.equal(got1, table[1])


@pytest.mark.parametrize("n,d", DETECT_SHAPES)
def test_detector_refuses_one_ulp_negative_zero_and_nan(eng, n, d):
    table, jgx0 = constant_jacobian(n, d)
    S, n_g = table.shape[:2]
    # (problem, group element, point, row, column): first point, last point, a point of the last partial chunk,
    # and the very last word of the last problem's last group element
    where = [(0, 0, 0, 0, 0), (0, 1, n - 1, d - 1, 0), (1, 0, n - 2, 0, d - 1), (S - 1, n_g - 1, n - 1, d - 1, d - 1)]
    for s, g, pt, a, b in where:
        jgx = jgx0.clone()
        v = jgx[s, g, pt, a, b]
        jgx[s, g, pt, a, b] = torch.nextafter(v, v + 1.0)
        assert not torch.equal(jgx, jgx0)
        assert eng.jacobian_constant(jgx)[1] is False, (s, g, pt, a, b)
    for pt in (0, n - 1):                                         # +0.0 everywhere but one -0.0 (equal as floats, not as bits)
        jgx = jgx0.clone()
        jgx[S - 1, 0, :, 0, d - 1] = 0.0
        assert eng.jacobian_constant(jgx)[1] is True
        jgx[S - 1, 0, pt, 0, d - 1] = -0.0
        assert eng.jacobian_constant(jgx)[1] is False, pt
    for pt in (0, n // 2, n - 1):                                 # a NaN at one point
        jgx = jgx0.clone()
        jgx[1, 1, pt, d - 1, 0] = float("nan")
        assert eng.jacobian_constant(jgx)[1] is False, pt
    jgx = jgx0.clone()                                            # the same NaN at EVERY point of a slab: still not "constant"
    jgx[2, 0, :, 0, 0] = float("nan")
    assert eng.jacobian_constant(jgx)[1] is False
    assert eng.jacobian_constant(jgx0)[1] is True                 # the flag is rewritten by every call


# ---------------------------------------------------------------------------------------- BatchedClosure
class SpyEngine:
    """The real engine, recording the shape of the Jacobian argument of the two closure entries."""

    def __init__(self, eng):
        self._eng, self.jgx_shapes, self.detections = eng, [], 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def loss_grad_reversed(self, x, dx, gx, jgx, *a, **kw):
        self.jgx_shapes.append(tuple(jgx.shape))
        return self._eng.loss_grad_reversed(x, dx, gx, jgx, *a, **kw)

    def symreg_reversed(self, x, gx, jgx, *a, **kw):
        self.jgx_shapes.append(tuple(jgx.shape))
        return self._eng.symreg_reversed(x, gx, jgx, *a, **kw)

    def jacobian_constant(self, jgx):
        self.detections += 1
        return self._eng.jacobian_constant(jgx)


@pytest.fixture(scope="module")
def closure_case(eng):
    S, n, n_g, d, order = 4, 1030, 2, 2, 3
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, d, order, eng, seed=3)
    return dict(S=S, n=n, n_g=n_g, d=d, order=order, x=x, dx=dx, gx=gx, table=table, xi=xi, mask=mask)


def build(c, spy, jgx, **kw):
    from symode_amd.batched import BatchedClosure
    return BatchedClosure(c["x"], c["dx"], c["order"], engine=spy, reversed_sym=(c["gx"], jgx, 0.1), **kw)


def run(clos, c):
    loss, g, _ = clos.evaluate(c["xi"], None, c["mask"])
    return loss.clone(), g.clone()


@pytest.mark.parametrize("fuse", [True, False])
def test_batched_closure_hands_the_compact_table_to_the_engine(eng, closure_case, fuse):
    c = closure_case
    jgx = expand(c["table"], c["n"])
    spy = SpyEngine(eng)
    clos = build(c, spy, jgx, fuse_sym=fuse)
    assert spy.detections == 1
    got = run(clos, c)
    assert spy.jgx_shapes == [(c["S"], c["n_g"], c["d"], c["d"])] and spy.detections == 1
    assert clos.sym[1].shape == jgx.shape                          # self.sym is kept as it was
    ref_spy = SpyEngine(eng)
    ref = run(build(c, ref_spy, jgx, fuse_sym=fuse, const_jacobian=False), c)
    assert ref_spy.jgx_shapes == [tuple(jgx.shape)] and ref_spy.detections == 0
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # two chunks equal one chunk
    spy2 = SpyEngine(eng)
    two = run(build(c, spy2, jgx, fuse_sym=fuse, n_chunks=2), c)
    assert spy2.jgx_shapes == [(c["S"] // 2, c["n_g"], c["d"], c["d"])] * 2
    assert torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])


def test_batched_closure_keeps_the_materialised_path_for_a_point_dependent_jacobian(eng, closure_case):
    c = closure_case
    jgx = expand(c["table"], c["n"])
    jgx[2, 1, 517, 0, 1] += 0.25
    spy = SpyEngine(eng)
    got = run(build(c, spy, jgx), c)
    assert spy.jgx_shapes == [tuple(jgx.shape)] and spy.detections == 1
    ref = run(build(c, SpyEngine(eng), jgx, const_jacobian=False), c)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_batched_closure_detects_again_after_an_in_place_write(eng, closure_case):
    c = closure_case
    jgx = expand(c["table"], c["n"])
    spy = SpyEngine(eng)
    clos = build(c, spy, jgx)
    before = run(clos, c)
    run(clos, c)
    assert spy.detections == 1 and spy.jgx_shapes == [(c["S"], c["n_g"], c["d"], c["d"])] * 2      # remembered while nothing changes
    jgx[1, 0, 1000:] = jgx[1, 0, 1000:] * 1.5                       # now point dependent
    after = run(clos, c)
    assert spy.detections == 2 and spy.jgx_shapes[-1] == tuple(jgx.shape)
    ref = run(build(c, SpyEngine(eng), jgx, const_jacobian=False), c)
    assert torch.equal(after[0], ref[0]) and torch.equal(after[1], ref[1])
    assert not torch.equal(after[0], before[0])
