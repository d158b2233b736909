"""The two levers on the fold kernel of a linear action (closure_fold.hpp: symreg_fold_kernel<FoldLevers<Lib, PK, SADDR>, ..>;
SYMODE_FOLD_PK): the packed-fp32 body over the two equation rows and the uniform ring that keeps the chunk addressing in SGPRs.

Both perform the scalar body's fmaf on the same operands in the same order on the same chunk-to-lane assignment, so what
the launcher routes to under SYMODE_FOLD_PK=1 is held to torch.equal with the parent's kernel (SYMODE_FOLD_PK=0) in the loss
pair and in the gradient.  Which kernel a launch took is read back from the workspace header (engine.closure_levers) and held
to the launcher's table.  Where the table routes nothing new for an instantiation both runs take the same kernel; the test
says so and compares all the same.

By default a launch of a few thousand points gives every lane at most one chunk, so the ring never refills a slot.  The grid
caps (SYMODE_SMALL_GRID for one problem, SYMODE_MAX_GRID with SYMODE_MIN_GRID_X=1 for a batch, as in
tests/test_gpu_stream_steady_state.py) bring the steady state down to these sizes: every case runs on the launcher's own grid,
on ONE workgroup and on three.  Chunks (n // 2), full rounds and ragged lanes of chunk_ring_uniform, ring depth 2:
  n        chunks   1 workgroup (256 lanes)             3 workgroups (768 lanes)
  1023       511    1 full + 255                        0 full + 511
  1026       513    2 full + 1                          0 full + 513
  2048      1024    4 full, none ragged (loop once)     1 full + 256
  4098/9    2049    8 full + 1 (loop three times)       2 full + 513
  6144      3072    12 full, none ragged                4 full, none ragged (loop once)
  7834      3917    15 full + 77                        5 full + 77 (loop once, four rounds peeled)"""
import contextlib

import pytest
import torch

from tests.test_gpu_closure_fold import linear_case, workspace
from tests.test_gpu_closure_live import PATTERN, env

pytestmark = pytest.mark.gpu

D, W_SYM = 2, 0.37
# the launcher's table (closure_fold.hpp: closure_fold_pk_pays / closure_fold_saddr_pays), (order, odd set?) -> (packed, uniform ring);
# held to what the kernels report (engine.closure_levers)
ROUTED = {(1, False): (False, False), (2, False): (False, False), (3, False): (False, False), (4, False): (False, False),
          (5, False): (True, True), (4, True): (False, False), (5, True): (False, True)}
# n = 1: the ragged tail only; 2: one chunk; 7: chunks plus an odd point; the others: see the table above
SIZES = (1, 2, 7, 1023, 1026, 2048, 4098, 4099, 6144, 7834)
GRIDS = (None, 1, 3)                                  # the launcher's own, one workgroup per problem, three
INSTANCES = [(o, None) for o in (1, 2, 3, 4, 5)] + [(4, PATTERN[4]), (5, PATTERN[5]), (4, PATTERN[4] & ~1), (5, PATTERN[5] & ~(1 | 1 << 7))]


def grid_cap(gx, S):
    """the launcher held to ``gx`` workgroups per problem (None: its own rule)"""
    stack = contextlib.ExitStack()
    if gx is not None and S == 1:
        stack.enter_context(env("SYMODE_SMALL_GRID", str(gx)))
    elif gx is not None:
        stack.enter_context(env("SYMODE_MAX_GRID", str(gx * S)))
        stack.enter_context(env("SYMODE_MIN_GRID_X", "1"))
    return stack


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def both_knobs(eng, x, dx, gx, table, xi, mask, order, live):
    """(loss pair, gradient) of the routed fold kernel and of the parent's; the body and the levers each launch left in the workspace"""
    M, linear = eng.linear_action(x, gx, table, order)
    assert linear
    ws = workspace(eng, x, order)
    kw = {} if live is None else {"live_columns": live}
    out, bodies, levers = [], [], []
    for knob in ("1", "0"):
        with env("SYMODE_FOLD_PK", knob):
            got = eng.loss_grad_reversed(x, dx, gx, table, xi, mask, order, 0, w_sym=W_SYM, ws=ws, linear_m=M, **kw)
            out.append(tuple(t.clone() for t in got))
            bodies.append(eng.closure_body(ws))
            levers.append(eng.closure_levers(ws))
    return out, bodies, levers


def check(eng, case, order, live, masked, what):
    x, dx, gx, table, xi, mask = case
    (new, old), bodies, levers = both_knobs(eng, x, dx, gx, table, xi, mask if masked else None, order, live)
    assert bodies == ["fold" if live is None else "fold-live"] * 2, (what, bodies)
    assert levers == [ROUTED[(order, live is not None)], (False, False)], (what, levers)
    assert torch.isfinite(old[0]).all() and torch.isfinite(old[1]).all() and old[1].abs().max() > 0, what
    assert torch.equal(new[0], old[0]), f"{what}: loss pair"
    assert torch.equal(new[1], old[1]), f"{what}: gradient"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("order,live", INSTANCES)
def test_levers_are_bit_identical_to_the_parent_body(eng, order, live, S, masked):
    """Orders 1-5 on every column, orders 4-5 on the odd set and on a strict subset of it; S = 3 with an odd n takes the
    per-point path (a problem's slab does not start on a 16-byte boundary)."""
    packed, ring = ROUTED[(order, live is not None)]
    if not (packed or ring):
        print(f"order {order}, {'odd set' if live is not None else 'every column'}: the table routes nothing new here; "
              "both runs take the parent's kernel")
    for n in SIZES:
        case = linear_case(S, n, order, eng)
        for gx in GRIDS:
            with grid_cap(gx, S):
                check(eng, case, order, live, masked, f"order={order} live={live} S={S} n={n} masked={masked} grid={gx}")


@pytest.mark.parametrize("order,live", [(5, None), (5, PATTERN[5]), (4, PATTERN[4]), (3, None)])
def test_x_offset_by_one_float(eng, order, live):
    """x starts 4 bytes past a 16-byte boundary: no 16-byte vectors, every point by per-lane loads"""
    for n in (7, 1026):
        x, dx, gx, table, xi, mask = linear_case(1, n, order, eng, seed=3)
        buf = torch.zeros(x.numel() + 1, dtype=torch.float32, device=x.device)
        buf[1:] = x.reshape(-1)
        xo = buf[1:].view(x.shape)
        assert xo.data_ptr() % 16 == 4 and torch.equal(xo, x)
        for grid in (None, 1):
            with grid_cap(grid, 1):
                check(eng, (xo, dx, gx, table, xi, mask), order, live, True, f"offset x, order={order} live={live} n={n} grid={grid}")
