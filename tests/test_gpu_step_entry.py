"""The native entry of the step on the reduced form (csrc/step_entry.cpp, engine.quad_step_plan) on the device, against the
step in Python (engine.ReducedStep, SYMODE_STEP_ENTRY=0): the same kernel with the same arguments, so every comparison is
``torch.equal``.
S = 1 takes the stride rule of a single problem, 5 is a ragged workgroup, 70 is the first size with more than one workgroup's
worth of 16-lane groups in flight beside a ragged last one (256 / 16 = 16 problems per workgroup)."""
import pytest
import torch

from symode_amd import engine as E
from symode_amd.engine import SymodeError
from tests.test_gpu_closure_live import env
from tests.test_gpu_closure_reduced import batched_inputs, clones, make_closure

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 70)
NAMES = ("loss", "d/dbeta", "d/dconst")


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def pair(eng, S, **kw):
    """(inputs, closure on the native plan, closure on the Python step), both with their form built"""
    inputs = batched_inputs(eng, S)
    x, dx, gx, table, Q, use_kron, beta, const = inputs
    const = const if kw.get("allow_constant", True) else None
    new, old = make_closure_kw(eng, inputs, **kw), make_closure_kw(eng, inputs, **kw)
    new.evaluate(beta, const)
    with env("SYMODE_STEP_ENTRY", "0"):                     # read where the plan is made: this closure keeps the Python step
        old.evaluate(beta, const)
    assert eng.step_entry_loaded and E.step_entry_loaded, E.step_entry_error
    assert type(new._reduced_step) is E._step_entry.Plan and type(new._reduced_step.slow) is E.ReducedStep
    assert type(old._reduced_step) is E.ReducedStep
    assert new.reduced_builds == 1 and old.reduced_builds == 1
    return inputs, new, old


def make_closure_kw(eng, inputs, allow_constant=True, **kw):
    x, dx, gx, table, Q, use_kron, beta, const = inputs
    if allow_constant:
        return make_closure(eng, x, dx, gx, table, Q, use_kron, **kw)
    from symode_amd.batched import BatchedClosure
    from tests.test_gpu_constj import expand
    return BatchedClosure(x, dx, 5, Q=Q, use_kron_product=use_kron, allow_constant=False, engine=eng,
                          reversed_sym=(gx, expand(table, x.shape[1]), 0.1), **kw)


def same(got, want, S, r, dc, what):
    shapes = ((S,), (S, r), (S, dc, 1))
    for a, b, shape, name in zip(got, want, shapes, NAMES):
        if name == "d/dconst" and dc == 0:
            assert a is None and b is None, what
            continue
        assert a.shape == shape == b.shape and a.dtype == torch.float32 and a.is_contiguous() and not a.requires_grad, (what, name)
        assert torch.equal(a, b), (what, name)


@pytest.mark.parametrize("S", SIZES)
def test_native_against_the_python_step(eng, S):
    inputs, new, old = pair(eng, S)
    beta, const = inputs[6], inputs[7]
    r = beta.shape[1]
    same(clones(new.evaluate(beta, const)), clones(old.evaluate(beta, const)), S, r, 2, "dense")
    assert eng.closure_reduced(new._ws_kw["ws"]) and eng.closure_reduced(old._ws_kw["ws"])
    # rows of a flat [beta | const] state, as the sweep passes them
    state = new.coef.join(beta * 1.25, const).contiguous()
    b, c = new.coef.split(state)
    assert S == 1 or not b.is_contiguous()
    same(clones(new.evaluate(b, c)), clones(old.evaluate(b, c)), S, r, 2, "rows of a flat state")
    # alias: the same objects every time, the values of the call
    first = new.evaluate(beta, const, alias=True)
    want = clones(old.evaluate(beta, const, alias=True))
    same(first, want, S, r, 2, "alias")
    second = new.evaluate(beta * 1.5, const, alias=True)
    assert all(p is q for p, q in zip(first, second))
    same(second, clones(old.evaluate(beta * 1.5, const)), S, r, 2, "alias, second call")
    out = new.evaluate(beta, const)
    assert len({t.untyped_storage().data_ptr() for t in out}) == 1 and out[0].data_ptr() != first[0].data_ptr()
    assert new.reduced_builds == 1 and old.reduced_builds == 1


@pytest.mark.parametrize("S", SIZES)
def test_without_constants(eng, S):
    inputs, new, old = pair(eng, S, allow_constant=False)
    beta = inputs[6]
    got, want = new.evaluate(beta), old.evaluate(beta)
    same(clones(got[:2]) + (got[2],), clones(want[:2]) + (want[2],), S, beta.shape[1], 0, "no constants")
    assert new.reduced_builds == 1 and old.reduced_builds == 1 and eng.closure_reduced(new._ws_kw["ws"])


def test_every_step_passes_the_one_door(eng):
    inputs, new, _ = pair(eng, 5)
    beta, const = inputs[6], inputs[7]
    orig, passes = eng.loss_grad_reversed, []

    def counting(*args, **kw):
        passes.append(kw.get("reduced"))
        return orig(*args, **kw)
    eng.loss_grad_reversed = counting                       # on the instance, as a timer or a trace would
    try:
        outs = [clones(new.evaluate(beta, const)) for _ in range(3)]
    finally:
        del eng.loss_grad_reversed
    assert eng.loss_grad_reversed == orig
    assert len(passes) == 3 and all(p is not None and p[0] is new._reduced_step for p in passes)
    assert eng.closure_reduced(new._ws_kw["ws"]) and new.reduced_builds == 1
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))


def test_the_keys_still_rebuild(eng):
    inputs, _, _ = pair(eng, 5)
    x, dx, gx, table, Q, use_kron, beta, const = inputs
    xs = x.clone()
    new = make_closure(eng, xs, dx, gx, table, Q, use_kron)
    first = clones(new.evaluate(beta, const))
    new.evaluate(beta, const)
    assert new.reduced_builds == 1
    new.sym = new.sym[:2] + (5.0,)                          # a rebound weight
    second = clones(new.evaluate(beta, const))
    assert new.reduced_builds == 2 and not torch.equal(first[0], second[0]) and type(new._reduced_step) is E._step_entry.Plan
    dx2 = dx.clone()
    other = make_closure(eng, xs, dx2, gx, table, Q, use_kron)
    other.evaluate(beta, const)
    dx2.mul_(1.25)                                          # an in-place write
    other.evaluate(beta, const)
    other.evaluate(beta, const)
    assert other.reduced_builds == 2 and eng.closure_reduced(other._ws_kw["ws"])


def test_the_stream_is_read_per_call(eng):
    inputs, new, old = pair(eng, 5)                         # both plans were made on the default stream
    beta, const = inputs[6], inputs[7]
    want = clones(old.evaluate(beta, const))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    late = torch.zeros_like(beta)
    busy = torch.randn(2048, 2048, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):                                  # work ahead of the operand on the side stream: a launch on
            busy = busy @ busy * 1e-3                       # another stream would read the zeros
        late.copy_(beta)
        got = new.evaluate(late, const)
    side.synchronize()
    same(got, want, 5, beta.shape[1], 2, "side stream")


def test_a_captured_step_follows_its_operand(eng):
    inputs, new, old = pair(eng, 5)                         # B is built: the capture records the step on it
    _, _, _, _, _, _, beta, const = inputs
    b = beta.clone()
    want1 = clones(old.evaluate(b, const))
    want2 = clones(old.evaluate(b * 1.5, const))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = new.evaluate(b, const)
    graph.replay()
    torch.cuda.synchronize()
    same(out, want1, 5, beta.shape[1], 2, "first replay")
    b.mul_(1.5)
    graph.replay()
    torch.cuda.synchronize()
    same(out, want2, 5, beta.shape[1], 2, "second replay")
    assert new.reduced_builds == 1 and eng.closure_reduced(new._ws_kw["ws"])


def test_operands_the_plan_does_not_take(eng):
    inputs, new, old = pair(eng, 5)
    beta, const = inputs[6], inputs[7]
    want = clones(old.evaluate(beta, const))
    wide = torch.zeros(5, 2 * beta.shape[1], device="cuda")[:, ::2]
    wide.copy_(beta)
    assert wide.stride(1) == 2
    same(clones(new.evaluate(wide, const)), want, 5, beta.shape[1], 2, "last axis of stride 2")
    a, b = new.evaluate(wide, const, alias=True), new.evaluate(beta, const, alias=True)
    assert all(p is q for p, q in zip(a, b))                # the slow path writes the plan's own buffers
    same(b, want, 5, beta.shape[1], 2, "alias after the slow path")
    with pytest.raises(SymodeError):
        new.evaluate(beta.double(), const)
    with pytest.raises(SymodeError):
        new.evaluate(beta.cpu(), const)
    with pytest.raises(SymodeError):
        new.evaluate(beta, const.cpu())
    same(clones(new.evaluate(beta, const)), want, 5, beta.shape[1], 2, "after the refusals")
    assert new.reduced_builds == 1
