"""The native entry of the step on the reduced form (csrc/step_entry.cpp -> _symode_step; engine.quad_step_plan) on the host:
the module is driven on CPU tensors with a recording stub in the place of symode_quad_step, so every argument of the call,
every outcome and the key handling are checked without a GPU.  The device rule -- the engine alone passes the library's real
address, and only for device tensors -- is HipEngine.quad_step_plan's and is not exercised here."""
import ctypes
import os
import types

import pytest
import torch

from symode_amd import engine as E

R = 6
SIG = ctypes.CFUNCTYPE(ctypes.c_int, *E._SIGNATURES["symode_quad_step"][1])
NAMES = ("b", "n_problems", "k", "d_c", "order", "live", "beta", "beta_stride", "const", "const_stride", "loss", "g_beta", "g_const",
         "workspace", "workspace_bytes", "stream")


class Stub:
    """a C-callable that records the sixteen arguments of every call and returns ``rc``"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc
        self.c = SIG(self._record)
        self.address = ctypes.cast(self.c, ctypes.c_void_p).value

    def _record(self, *args):
        self.calls.append(dict(zip(NAMES, args)))
        return self.rc


def case(S, dc, rc=0, live=0x3F, weight=0.1):
    """(stub, plan, key operands (x, dx, sym, Q, live), B, ws) on CPU tensors"""
    assert E.step_entry_loaded, E.step_entry_error
    g = torch.Generator().manual_seed(10 * S + dc)
    K = R + dc
    B = torch.randn(S, K + 1, K + 1, generator=g, dtype=torch.float64)
    ws = torch.zeros(24, dtype=torch.float64)
    x, dx, gx, jgx, Q = (torch.randn(4, generator=g) for _ in range(5))
    key = (x, dx, (gx, jgx, weight), Q, live)
    stub = Stub(rc)
    plan = E._step_entry.Plan(stub.address, B, ws, R, dc, 5, live, key, "the slow path")
    return stub, plan, key, B, ws


def operands(S, dc, flat):
    g = torch.Generator().manual_seed(7)
    if flat:                                                          # rows of a flat (S, r + d_c) state
        state = torch.randn(S, R + dc, generator=g)
        return state[:, :R], (state[:, R:].unsqueeze(-1) if dc else None)
    return torch.randn(S, R, generator=g), (torch.randn(S, dc, 1, generator=g) if dc else None)


def call(plan, beta, const, key, alias=False):
    return plan((plan, beta, const, alias) + key)


def test_the_module_is_built_and_loaded():
    assert E.step_entry_loaded and E.step_entry_error is None
    assert E._step_entry.STALE == E.STEP_STALE and E._step_entry.SLOW == E.STEP_SLOW
    # clear of the library's own return codes, which the plan hands back as they are
    assert E.STEP_STALE < -100 and E.STEP_SLOW < -100 and E.STEP_STALE != E.STEP_SLOW


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("dc", [0, 2])
@pytest.mark.parametrize("S", [1, 5])
def test_arguments_of_the_call_and_the_views(S, dc, flat):
    stub, plan, key, B, ws = case(S, dc)
    beta, const = operands(S, dc, flat)
    out = call(plan, beta, const, key)
    assert len(stub.calls) == 1
    a = stub.calls[0]
    base = out[0].data_ptr()
    assert (a["b"], a["n_problems"], a["k"], a["d_c"], a["order"], a["live"]) == (B.data_ptr(), S, R + dc, dc, 5, 0x3F)
    assert a["beta"] == beta.data_ptr() and a["const"] == (const.data_ptr() if dc else None)
    # the row strides as they lie (R + dc for rows of the flat state); with one problem the width, whatever the tensor says
    assert a["beta_stride"] == (beta.stride(0) if S > 1 else R)
    assert a["const_stride"] == ((const.stride(0) if S > 1 else dc) if dc else 0)
    if flat and S > 1:
        assert a["beta_stride"] == R + dc
    assert (a["loss"], a["g_beta"], a["g_const"]) == (base, base + 4 * S, (base + 4 * S * (1 + R)) if dc else None)
    assert a["stream"] is None
    assert (a["workspace"], a["workspace_bytes"]) == (ws.data_ptr(), ws.numel() * 8) == (plan.ws.data_ptr(), plan.ws_bytes)
    assert plan.B.data_ptr() == B.data_ptr() and (plan.S, plan.r, plan.dc, plan.order, plan.live) == (S, R, dc, 5, 0x3F)
    loss, g_beta, g_const = out
    assert loss.shape == (S,) and g_beta.shape == (S, R) and (g_const.shape == (S, dc, 1) if dc else g_const is None)
    live = [t for t in out if t is not None]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.grad_fn is None for t in live)
    assert len({t.untyped_storage().data_ptr() for t in live}) == 1 and live[0].untyped_storage().nbytes() == 4 * S * (1 + R + dc)
    # a fresh storage per call: the first results are still held here
    again = call(plan, beta, const, key)
    assert again[0].untyped_storage().data_ptr() != base and len(stub.calls) == 2


@pytest.mark.parametrize("dc", [0, 2])
def test_alias_returns_the_same_objects(dc):
    stub, plan, key, B, ws = case(5, dc)
    beta, const = operands(5, dc, False)
    first, second = call(plan, beta, const, key, alias=True), call(plan, beta, const, key, alias=True)
    assert len(stub.calls) == 2 and stub.calls[0]["loss"] == stub.calls[1]["loss"] == first[0].data_ptr()
    assert all(p is q for p, q in zip(first, second))
    buf, views = plan.alias_buffers()
    assert all(p is q for p, q in zip(first, views)) and buf.data_ptr() == first[0].data_ptr() and buf.numel() == 5 * (1 + R + dc)
    assert call(plan, beta, const, key)[0].data_ptr() != first[0].data_ptr()


def test_refused_and_error_codes():
    stub, plan, key, _, _ = case(5, 2, rc=-1)
    beta, const = operands(5, 2, False)
    assert call(plan, beta, const, key) is None and len(stub.calls) == 1
    stub, plan, key, _, _ = case(5, 2, rc=3)
    assert call(plan, beta, const, key) == 3 and len(stub.calls) == 1
    stub, plan, key, _, _ = case(5, 2, rc=-3)                         # SYMODE_E_BADSIZE is not taken for an outcome of the plan
    assert call(plan, beta, const, key) == -3 and len(stub.calls) == 1


def test_the_key():
    stub, plan, key, _, _ = case(5, 2)
    beta, const = operands(5, 2, False)
    x, dx, (gx, jgx, w), Q, live = key
    assert type(call(plan, beta, const, key)) is tuple
    for moved in ((x, dx, (gx, jgx, 0.2), Q, live), (x, dx, (gx, jgx, w), Q, None), (x, dx, (gx, jgx, w), Q, live ^ 1),
                  (x.clone(), dx, (gx, jgx, w), Q, live), (x, dx, (gx, jgx.clone(), w), Q, live), (x, dx, (gx, jgx, w), Q.clone(), live)):
        assert call(plan, beta, const, moved) == E.STEP_STALE
    assert type(call(plan, beta, const, key)) is tuple and type(call(plan, beta, const, (x, dx, (gx, jgx, w), Q, live))) is tuple
    assert len(stub.calls) == 3                                       # a stale call launches nothing


@pytest.mark.parametrize("which", ["x", "dx", "gx", "jgx", "Q"])
def test_an_in_place_write_is_stale(which):
    stub, plan, key, _, _ = case(5, 2)
    beta, const = operands(5, 2, False)
    t = dict(x=key[0], dx=key[1], gx=key[2][0], jgx=key[2][1], Q=key[3])[which]
    assert type(call(plan, beta, const, key)) is tuple
    ptr = t.data_ptr()
    t.mul_(1.25)
    assert t.data_ptr() == ptr and call(plan, beta, const, key) == E.STEP_STALE and len(stub.calls) == 1
    # the Python step keeps the same key
    eng = types.SimpleNamespace(lib=types.SimpleNamespace(symode_quad_step=None))
    slow = E.ReducedStep(eng, plan.B, 5, 0x3F, R, 2, plan.ws, key)
    assert slow.key == E.step_key(*key)
    t.mul_(1.25)
    assert slow((slow, beta, const, False) + key) == E.STEP_STALE


def test_operands_for_the_slow_path():
    stub, plan, key, _, _ = case(5, 2)
    beta, const = operands(5, 2, False)
    wide = torch.zeros(5, R + 1)
    strided = torch.zeros(5, 2 * R)[:, ::2]
    assert strided.shape == (5, R) and strided.stride(1) == 2
    for b, c in ((beta.double(), const), (wide, const), (strided, const), (beta, torch.empty(5, 2, 1, device="meta")),
                 (beta, const.double()), (beta[:4], const), (beta.reshape(-1), const)):
        assert call(plan, b, c, key) == E.STEP_SLOW
    assert not stub.calls and plan.slow == "the slow path"
    assert type(call(plan, beta, const, key)) is tuple


def test_what_is_no_tensor_raises():
    stub, plan, key, _, _ = case(5, 2)
    beta, const = operands(5, 2, False)
    x, dx, sym, Q, live = key
    for args in ((plan, [1.0], const, False) + key, (plan, beta, None, False) + key, (plan, beta, const, False, None, dx, sym, Q, live),
                 (plan, beta, const, False, x, dx, (sym[0], 1.0, sym[2]), Q, live), (plan, beta, const, False, x, dx, sym, Q, "all"),
                 (plan, beta, const, False)):
        with pytest.raises(TypeError):
            plan(args)
    with pytest.raises(TypeError):
        plan(plan, beta, const)
    assert not stub.calls
    # without constants the third slot is not read
    stub, plan, key, _, _ = case(5, 0)
    assert type(call(plan, beta, None, key)) is tuple and type(call(plan, beta, "unused", key)) is tuple


def test_a_plan_checks_what_it_is_made_of():
    stub, plan, key, B, ws = case(5, 2)
    make = E._step_entry.Plan
    for args, err in (((0, B, ws, R, 2, 5, 0, key), ValueError), ((stub.address, B.float(), ws, R, 2, 5, 0, key), ValueError),
                      ((stub.address, B, ws, R + 1, 2, 5, 0, key), ValueError), ((stub.address, B, ws.float(), R, 2, 5, 0, key), ValueError),
                      ((stub.address, B, torch.empty(8, dtype=torch.float64, device="meta"), R, 2, 5, 0, key), ValueError),
                      ((stub.address, B, ws, R, 2, 5, 0, key[:4]), TypeError), ((stub.address, "B", ws, R, 2, 5, 0, key), TypeError)):
        with pytest.raises(err):
            make(*args)


def test_the_switch_chooses_the_python_step():
    old = os.environ.get("SYMODE_STEP_ENTRY")
    try:
        os.environ.pop("SYMODE_STEP_ENTRY", None)
        assert E.step_entry_enabled()
        os.environ["SYMODE_STEP_ENTRY"] = "0"
        assert not E.step_entry_enabled()
        os.environ["SYMODE_STEP_ENTRY"] = "1"
        assert E.step_entry_enabled()
    finally:
        if old is None:
            os.environ.pop("SYMODE_STEP_ENTRY", None)
        else:
            os.environ["SYMODE_STEP_ENTRY"] = old
