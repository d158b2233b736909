"""The steady state of the streaming schedules at small n, for every chunk layout (d = 1: 4 points per 16 bytes, d = 2: 2,
d = 3: coalesced tiles through the wave's LDS slab, d = 4: 1).

By default a launch is sized so that a lane gets one chunk until the grid reaches 512 workgroups (hundreds of thousands of
points), so below that ``chunk_ring`` never refills a slot and the two-chunk steps of ``for_each_chunk2`` and of the d = 3
loop of ``for_each_chunk_ring`` are never taken.  The grid caps (SYMODE_SMALL_GRID, SYMODE_REDUCE_GRID, SYMODE_MAP_GRID) bring
that regime down to a few thousand points: with 1 and 3 workgroups and 256 * 6 + 77 chunks a lane makes a full ring turn
(or three two-chunk steps and a remainder) and drains ragged, the last round of a wave only partly populated.

Tolerances and fp64 reference expressions are those of the uncapped tests of the same op: test_loss_grad_ragged_sizes_vs_oracle,
test_streaming_maps_and_euler_pair_random, test_forward_and_odeint_chunked_streams_vs_oracle (tests/test_gpu_kernels.py,
tests/test_gpu_property.py), and test_euler_reverse_sweep_state_stack_equals_recompute for ``euler_jvp_vjp``.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.helpers import _env, only_compiled

pytestmark = pytest.mark.gpu

PPT = {1: 4, 2: 2, 3: 4, 4: 1}
REDUCE_N = {1: 6455, 2: 3227, 3: 6455, 4: 1613}                               # 256 * 6 + 77 chunks, and a ragged tail
MAP_N = {d: ppt * (256 * 5 + 77) + (ppt - 1) for d, ppt in PPT.items()}
# one plain and one sine + exp library per d; (2, 5, 0): the four-round slabs of the forward map, the heavy grid rules
LIBS = only_compiled([(1, 3, 0), (1, 2, 3), (2, 3, 0), (2, 2, 3), (2, 5, 0), (3, 3, 0), (3, 2, 3), (4, 2, 0), (4, 2, 3)])
GRIDS = (1, 3)
ids = lambda v: "d%do%df%d" % tuple(v) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def close(got, want, tol, what):
    """Every entry within ``tol`` of the reference's largest magnitude (the criterion of the uncapped tests)."""
    got, want = got.detach().cpu().double(), want.detach().double()
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-6)
    assert err <= tol, f"{what}: max scaled error {err:.3e} > {tol}"


@functools.lru_cache(maxsize=None)
def problem(lib, n):
    """Inputs (float32, CPU) of library ``lib`` at ``n`` points, drawn once."""
    d, order, fl = lib
    gen = torch.Generator().manual_seed(9000 + 100 * d + 10 * order + fl + n)
    p = O.term_count(d, order, bool(fl & 1), bool(fl & 2))
    mk = lambda s: (torch.randn(n, d, generator=gen) * s).clamp(-2.5 * s, 2.5 * s)  # noqa: E731
    return dict(x=mk(0.4), dx=mk(1.0), v=mk(0.4), g1=mk(0.4), g2=mk(0.4), xi=torch.randn(d, p, generator=gen) * 0.2,
                mask=(torch.rand(d, p, generator=gen) > 0.3).float(), p=p)


def f64(lib, pr):
    d, order, fl = lib
    W = (pr["xi"] * pr["mask"]).double().requires_grad_(True)
    return W, lambda a: O.theta(a, order, bool(fl & 1), bool(fl & 2)) @ W.T


@functools.lru_cache(maxsize=None)
def reduce_reference(lib):
    """fp64: loss_grad, vjp and jvp_vjp of the reduction problem of ``lib``, computed once."""
    d, order, fl = lib
    pr = problem(lib, REDUCE_N[d])
    md = pr["mask"].double()
    wl, wg = O.mse_loss_and_grad(pr["x"].double(), pr["dx"].double(), pr["xi"].double(), md, order, bool(fl & 1), bool(fl & 2))
    W, f = f64(lib, pr)
    X = pr["x"].double().requires_grad_(True)
    (f(X) * pr["g1"].double()).sum().backward()
    vjp = (X.grad, W.grad * md)
    W, f = f64(lib, pr)
    X, V = pr["x"].double().requires_grad_(True), pr["v"].double().requires_grad_(True)
    out, jv = torch.autograd.functional.jvp(f, X, V, create_graph=True)
    ((out * pr["g1"].double()).sum() + (jv * pr["g2"].double()).sum()).backward()
    return dict(loss=wl, grad=wg, vjp=vjp, jvp_vjp=(X.grad, V.grad, W.grad * md))


def cuda(pr, *names):
    return [pr[k].cuda() for k in names]


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib,grid,segmented", [(lib, g, s) for lib in LIBS for g in GRIDS for s in (1, 0, 2) if s == 1 or lib[0] == 2], ids=ids)
def test_loss_grad_steady_state(eng, lib, grid, segmented):
    """SYMODE_SEGMENTED (read at d = 2 only, the RING4 form): 1 the default, 0 off, 2 contiguous slabs from two workgroups up."""
    d, order, fl = lib
    pr, ref = problem(lib, REDUCE_N[d]), reduce_reference(lib)
    x, dx, xi, mask = cuda(pr, "x", "dx", "xi", "mask")
    with _env(SYMODE_SMALL_GRID=grid, SYMODE_SEGMENTED=segmented):
        loss, grad = eng.loss_grad(x, dx, xi, mask, order, fl)
    assert np.isclose(loss.item(), ref["loss"].item(), rtol=2e-5), (loss.item(), ref["loss"].item())
    close(grad, ref["grad"], 2e-5, "loss_grad grad")


@pytest.mark.parametrize("need_grad_x", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("lib", LIBS, ids=ids)
def test_vjp_steady_state(eng, lib, grid, need_grad_x):
    d, order, fl = lib
    pr, ref = problem(lib, REDUCE_N[d]), reduce_reference(lib)
    x, g1, xi, mask = cuda(pr, "x", "g1", "xi", "mask")
    with _env(SYMODE_REDUCE_GRID=grid):
        gx, gxi = eng.vjp(x, g1, xi, mask, order, fl, need_grad_x=need_grad_x)
    close(gxi, ref["vjp"][1], 5e-5, "vjp grad_xi")
    if need_grad_x:
        close(gx, ref["vjp"][0], 5e-5, "vjp grad_x (every row)")
    else:
        assert gx is None


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("lib", LIBS, ids=ids)
def test_jvp_vjp_steady_state(eng, lib, grid):
    d, order, fl = lib
    pr, ref = problem(lib, REDUCE_N[d]), reduce_reference(lib)
    x, v, g1, g2, xi, mask = cuda(pr, "x", "v", "g1", "g2", "xi", "mask")
    with _env(SYMODE_REDUCE_GRID=grid):
        got = eng.jvp_vjp(x, v, g1, g2, xi, mask, order, fl)
    for a, b, nm in zip(got, ref["jvp_vjp"], ("grad_x (every row)", "grad_v (every row)", "grad_xi")):
        close(a, b, 5e-5, "jvp_vjp " + nm)


# ---------------------------------------------------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------------------------------------------------
STEPS, DT = 3, 0.02


@functools.lru_cache(maxsize=None)
def map_reference(lib):
    d, order, fl = lib
    pr = problem(lib, MAP_N[d])
    W, f = f64(lib, pr)
    with torch.no_grad():
        X, V = pr["x"].double(), pr["v"].double()
        out, jv = torch.autograd.functional.jvp(f, X, V)
        xs, ts = X, V
        for _ in range(STEPS):
            h, jt = torch.autograd.functional.jvp(f, xs, ts)
            xs, ts = xs + DT * h, ts + DT * jt
        return dict(forward=f(X), rk4=O.odeint(f, X, STEPS * DT + DT / 2, DT, "rk4"), euler=O.odeint(f, X, STEPS * DT + DT / 2, DT, "euler"),
                    forward_jvp=(out, jv), euler_jvp=(xs, ts))


def run_maps(eng, lib, pr):
    d, order, fl = lib
    x, v, xi, mask = cuda(pr, "x", "v", "xi", "mask")
    return dict(forward=eng.forward(x, xi, mask, order, fl), rk4=eng.odeint(x, xi, mask, order, fl, STEPS, DT, "rk4"),
                euler=eng.odeint(x, xi, mask, order, fl, STEPS, DT, "euler"), forward_jvp=eng.forward_jvp(x, v, xi, mask, order, fl),
                euler_jvp=eng.euler_jvp(x, v, xi, mask, order, fl, STEPS, DT))


@pytest.mark.parametrize("cap", GRIDS)
@pytest.mark.parametrize("lib", LIBS, ids=ids)
def test_maps_steady_state(eng, lib, cap):
    """forward, odeint (rk4, euler), forward_jvp, euler_jvp under SYMODE_MAP_GRID: every output row against fp64, and bit for
    bit the uncapped launch on the same inputs (the per-point arithmetic does not depend on the schedule)."""
    d = lib[0]
    pr, ref = problem(lib, MAP_N[d]), map_reference(lib)
    with _env(SYMODE_MAP_GRID=cap):
        got = run_maps(eng, lib, pr)
    free = run_maps(eng, lib, pr)
    close(got["forward"], ref["forward"], 2e-6, "forward")
    for m in ("rk4", "euler"):
        assert np.allclose(got[m].cpu().double().numpy(), ref[m].numpy(), rtol=2e-5, atol=2e-6), "odeint " + m
    for k in range(2):
        close(got["forward_jvp"][k], ref["forward_jvp"][k], 5e-5, f"forward_jvp output {k}")
        close(got["euler_jvp"][k], ref["euler_jvp"][k], 2e-5, f"euler_jvp output {k}")
    tensors = lambda r: (r,) if torch.is_tensor(r) else r  # noqa: E731
    unequal = [k for k in got if not all(torch.equal(a, b) for a, b in zip(tensors(got[k]), tensors(free[k])))]
    assert unequal == [], unequal


# ---------------------------------------------------------------------------------------------------------------------
# euler_jvp_vjp has no grid knob: a launch just large enough for lanes to take a second chunk (grid 512, K = 2)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", only_compiled([(1, 3, 0), (2, 3, 0), (3, 2, 0), (4, 2, 0)]), ids=ids)
def test_euler_jvp_vjp_second_chunk(eng, lib):
    """Above 512 * 256 chunks the grid stays at 512 workgroups: 77 lanes take a second chunk, and a ragged tail follows."""
    d, order, fl = lib
    K, dt = 2, 0.01
    n = PPT[d] * (512 * 256 + 77) + (PPT[d] - 1)
    pr = problem(lib, n)
    x, v, g1, g2, xi, mask = cuda(pr, "x", "v", "g1", "g2", "xi", "mask")
    got = eng.euler_jvp_vjp(x, v, g1, g2, xi, mask, order, fl, K, dt)
    W, f = f64(lib, pr)
    X, V = pr["x"].double().requires_grad_(True), pr["v"].double().requires_grad_(True)
    xs, ts = X, V
    for _ in range(K):
        h, jt = torch.autograd.functional.jvp(f, xs, ts, create_graph=True)
        xs, ts = xs + dt * h, ts + dt * jt
    ((xs * pr["g1"].double()).sum() + (ts * pr["g2"].double()).sum()).backward()
    for a, b, nm in zip(got, (X.grad, V.grad, W.grad * pr["mask"].double()), ("grad_x (every row)", "grad_v (every row)", "grad_xi")):
        close(a, b, 3e-5, "euler_jvp_vjp " + nm)
