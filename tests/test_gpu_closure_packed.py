"""The packed-fp32 body of the constant-Jacobian closure kernels (symreg_reversed_kernel, PK: the point's two library
evaluations as one evaluation on pairs) against the scalar body (SYMODE_CLOSURE_PK=0).

The packed body forms every product and every sum the scalar one forms, in its order, on the same chunk-to-lane
assignment, so the two are held to BIT identity; against the oracle the packed body is held to the tolerances of
test_gpu_constj.py::test_compact_table_against_the_oracle (loss rtol 2e-5, gradient 3e-5 of its scale)."""
import os

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.test_gpu_constj import assert_close_scaled, expand, make_case

pytestmark = pytest.mark.gpu

S, D, W_SYM = 3, 2, 0.37


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


class pk_env:
    """SYMODE_CLOSURE_PK for the duration of a block (the library reads its variables once: engine.reload_env)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        import symode_amd
        self.old = os.environ.get("SYMODE_CLOSURE_PK")
        if self.value is None:
            os.environ.pop("SYMODE_CLOSURE_PK", None)
        else:
            os.environ["SYMODE_CLOSURE_PK"] = self.value
        symode_amd.engine.reload_env()

    def __exit__(self, *exc):
        import symode_amd
        if self.old is None:
            os.environ.pop("SYMODE_CLOSURE_PK", None)
        else:
            os.environ["SYMODE_CLOSURE_PK"] = self.old
        symode_amd.engine.reload_env()


def distinct_tables(table):
    return len({tuple(m.flatten().tolist()) for m in table.reshape(-1, D, D).cpu()}) == table.shape[0] * table.shape[1]


# (order, flags) -> the body the launcher's table gives the compact-table form.  Order 4 plain is one of the issue's cases and
# keeps the scalar body (packed measured 5 % slower there): its rows pin that the knob changes nothing; (4, 2) -- order 4
# with exp columns -- is the order-4 library that IS packed.
LIBS = {(4, 0): "scalar", (4, 2): "packed", (5, 0): "packed"}


def both_closures(eng, c, order, flags, mask):
    """(fused loss pair, fused gradient, regulariser loss, regulariser gradient), and the body each of the two launches took"""
    x, dx, gx, table, xi = c
    batched = x.dim() == 3
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, flags, x.shape[0] if batched else 1, x.shape[-2]))
    fused = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, flags, w_sym=W_SYM, ws=ws)
    bodies = [eng.closure_body(ws)]
    alone = eng.symreg_reversed(x, gx, table, xi, mask, order, flags, ws=ws)
    bodies.append(eng.closure_body(ws))
    return (*fused, *alone), bodies


def lib_case(eng, S_, n, n_g, order, flags, seed=0):
    """make_case of test_gpu_constj.py for a library with sine / exp columns (same distributions)"""
    g = torch.Generator().manual_seed(1000 * S_ + 10 * n + n_g + D + 100 * flags + seed)
    p = eng.lib_size(D, order, flags)
    x = (torch.randn(S_, n, D, generator=g) * 0.5).cuda()
    dx = torch.randn(S_, n, D, generator=g).cuda()
    gx = (torch.randn(S_, n_g, n, D, generator=g) * 0.5).cuda()
    table = (torch.eye(D) + 0.3 * torch.randn(S_, n_g, D, D, generator=g)).cuda()
    xi = (torch.randn(S_, D, p, generator=g) * 0.3).cuda()
    mask = (torch.rand(S_, D, p, generator=g) > 0.25).float().cuda()
    return x, dx, gx, table, xi, mask


def assert_same_bits(eng, c, order, flags, mask):
    with pk_env("0"):
        want, bodies0 = both_closures(eng, c, order, flags, mask)
    with pk_env(None):
        got, bodies1 = both_closures(eng, c, order, flags, mask)
    assert bodies0 == ["scalar"] * 2 and bodies1 == [LIBS[order, flags]] * 2
    assert torch.isfinite(want[0]).all() and want[1].abs().max() > 0 and want[3].abs().max() > 0
    for g, w, what in zip(got, want, ("fused closure: loss pair", "fused closure: gradient", "regulariser alone: loss",
                                      "regulariser alone: gradient")):
        assert torch.equal(g, w), what


# N = 1031: odd, several ring turns of a 256-lane workgroup plus a ragged tail -- with S = 3 problems an odd N leaves the
# slabs of problems 1, 2 off the 16-byte grid, so the launcher takes the per-point path; N = 1032 is its even neighbour, on
# which the vector ring itself runs (4 chunks per workgroup turn, a partial last turn); N = 5: shorter than one ring turn.
@pytest.mark.parametrize("order,flags", sorted(LIBS))
@pytest.mark.parametrize("n_g", [1, 2])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("n", [1031, 1032, 5])
def test_packed_body_is_bit_identical_to_the_scalar_body(eng, order, flags, n_g, masked, n):
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, D, order, eng) if flags == 0 else lib_case(eng, S, n, n_g, order, flags)
    assert distinct_tables(table)
    if masked:
        mask[:, :, 2] = 0.0                                   # besides the random zeros: a whole column gone in every problem
        assert (mask.sum(dim=(0, 1)) == 0).any()
    else:
        mask = None
    assert_same_bits(eng, (x, dx, gx, table, xi), order, flags, mask)


@pytest.mark.parametrize("order,flags", sorted(LIBS))
@pytest.mark.parametrize("masked", [True, False])
def test_ring_turns_and_the_ragged_tail_in_one_launch(eng, order, flags, masked):
    """ONE aligned problem of N = 1031 points, one group element: the vector ring takes the 515 chunks (two turns of the
    256-lane workgroup and a partial third) and the per-point path the leftover point, both adding into the same sums."""
    x, dx, gx, table, xi, mask = lib_case(eng, 1, 1031, 1, order, flags, seed=5)
    x, dx, gx, table, xi, mask = x[0], dx[0], gx[0], table[0], xi[0], mask[0]
    for t in (x, dx, gx):
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    assert_same_bits(eng, (x, dx, gx, table, xi), order, flags, mask if masked else None)


@pytest.mark.parametrize("order,flags", sorted(LIBS))
@pytest.mark.parametrize("n", [1031, 1030, 5])
def test_packed_body_on_pointers_offset_by_one_float(eng, order, flags, n):
    """One problem whose x, dx, g(x) start one float past a 16-byte boundary: the non-vector path of both bodies.  (One
    problem, one group element: further slabs would have to be aligned among themselves.)  N = 1030 / 1031: the offset path
    is per-point whatever the parity; both are here because the aligned form treats them differently."""
    g = torch.Generator().manual_seed(17 * n + order + 100 * flags)
    p = eng.lib_size(D, order, flags)

    def off(t):                                               # the same values, one float into a fresh allocation
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:] = t.reshape(-1).cuda()
        return buf[1:].view(t.shape)
    x, dx, gx = off(torch.randn(n, D, generator=g) * 0.5), off(torch.randn(n, D, generator=g)), off(torch.randn(1, n, D, generator=g) * 0.5)
    for t in (x, dx, gx):
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    table = (torch.eye(D) + 0.3 * torch.randn(1, D, D, generator=g)).cuda()
    xi = (torch.randn(D, p, generator=g) * 0.3).cuda()
    mask = (torch.rand(D, p, generator=g) > 0.25).float().cuda()
    assert_same_bits(eng, (x, dx, gx, table, xi), order, flags, mask)


# the sine / exp libraries the launcher's table gives the packed body (sinf / expf of a pair are the scalar functions on each half)
@pytest.mark.parametrize("order,flags", [(5, 2), (5, 3), (4, 2)])
@pytest.mark.parametrize("n", [1032, 5])
def test_packed_body_with_sine_and_exp_columns(eng, order, flags, n):
    n_g = 2
    g = torch.Generator().manual_seed(31 * n + 7 * order + flags)
    p = eng.lib_size(D, order, flags)
    x = (torch.randn(S, n, D, generator=g) * 0.5).cuda()
    dx = torch.randn(S, n, D, generator=g).cuda()
    gx = (torch.randn(S, n_g, n, D, generator=g) * 0.5).cuda()
    table = (torch.eye(D) + 0.3 * torch.randn(S, n_g, D, D, generator=g)).cuda()
    xi = (torch.randn(S, D, p, generator=g) * 0.3).cuda()
    mask = (torch.rand(S, D, p, generator=g) > 0.25).float().cuda()
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, flags, S, n))

    def run():
        out = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, flags, w_sym=W_SYM, ws=ws)
        body = eng.closure_body(ws)
        return (*out, *eng.symreg_reversed(x, gx, table, xi, mask, order, flags, ws=ws)), body
    with pk_env("0"):
        want, body0 = run()
    with pk_env(None):
        got, body1 = run()
    assert (body0, body1) == ("scalar", "packed")
    assert torch.isfinite(want[0]).all() and want[1].abs().max() > 0
    for g_, w in zip(got, want):
        assert torch.equal(g_, w)


def test_packed_body_against_the_oracle(eng):
    """Order 5, S = 3, n_g = 2, N = 1032 (the vector ring), masked: tolerances of test_compact_table_against_the_oracle."""
    n, n_g, order = 1032, 2, 5
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, D, order, eng)
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, 0, S, n))
    loss2, grad = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws)
    assert eng.closure_body(ws) == "packed"
    l_s, g_s = eng.symreg_reversed(x, gx, table, xi, mask, order, 0, ws=ws)
    assert eng.closure_body(ws) == "packed"
    jgx = expand(table, n).cpu()
    xc, dxc, gxc, xic, mc = x.cpu(), dx.cpu(), gx.cpu(), xi.cpu(), mask.cpu()
    for s in range(S):
        reg = O.OracleRegressor(D, order, False, False, Xi0=xic[s])
        reg.mask = mc[s]
        mse = torch.nn.functional.mse_loss(reg(xc[s]), dxc[s])
        sym = O.symreg_reversed_precomputed(xc[s], list(gxc[s]), list(jgx[s]), reg)
        g_sym, = torch.autograd.grad(sym, reg.Xi, retain_graph=True)
        (mse + W_SYM * sym).backward()
        assert np.isclose(loss2[s, 0].item(), mse.item(), rtol=2e-5) and np.isclose(loss2[s, 1].item(), sym.item(), rtol=2e-5)
        assert_close_scaled(grad[s].cpu(), reg.Xi.grad * mc[s], 3e-5, f"fused closure grad, problem {s}")
        assert np.isclose(l_s[s].item(), sym.item(), rtol=2e-5)
        assert_close_scaled(g_s[s].cpu(), g_sym * mc[s], 3e-5, f"regulariser grad, problem {s}")


def test_the_launcher_takes_the_packed_body_at_order_5_and_the_knob_turns_it_off(eng):
    """The body a launch took, as the kernel itself records it in the workspace header (engine.closure_body): packed for the
    compact table at order 5, scalar under SYMODE_CLOSURE_PK=0, scalar for the materialised Jacobian, at d = 3 and for the
    d = 2 libraries outside the launcher's table."""
    n, order = 1032, 5
    x, dx, gx, table, xi, mask = make_case(S, n, 1, D, order, eng)
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(D, order, 0, S, n))
    assert eng.closure_body(ws) is None

    def fused(jgx):
        eng.loss_grad_reversed(x, dx, gx, jgx, xi, mask, order, 0, w_sym=W_SYM, ws=ws)
        return eng.closure_body(ws)

    def alone(jgx):
        eng.symreg_reversed(x, gx, jgx, xi, mask, order, 0, ws=ws)
        return eng.closure_body(ws)
    with pk_env(None):
        assert fused(table) == "packed" and fused(expand(table, n)) == "scalar" and alone(table) == "packed"
    with pk_env("1"):
        assert fused(table) == "packed" and alone(table) == "packed"
    with pk_env("0"):
        assert fused(table) == "scalar" and alone(table) == "scalar"
    with pk_env(None):
        assert fused(table) == "packed"
        x3, dx3, gx3, t3, xi3, m3 = make_case(2, 516, 1, 3, 2, eng)
        ws3 = eng.new_workspace(x3.device, eng.lib.symode_workspace_bytes(3, 2, 0, 2, 516))
        eng.loss_grad_reversed(x3, dx3, gx3, t3, xi3, m3, 2, 0, w_sym=W_SYM, ws=ws3)
        assert eng.closure_body(ws3) == "scalar"
        # d = 2 libraries the table leaves scalar: order 4 plain, order 4 with sine and exp columns, order 5 with sine columns
        # alone, order 3
        for o, fl in ((4, 0), (4, 3), (5, 1), (3, 0)):
            assert both_closures(eng, lib_case(eng, S, 1032, 1, o, fl)[:5], o, fl, None)[1] == ["scalar"] * 2
