"""The regulariser operators on the device against the fp64 models of tests/regulariser_model.py, on the decks of
tests/regulariser_cases.py, within the derived tolerances.

S4 (``symreg_reversed_kernel``, plain materialised form): through ``engine.symreg_reversed`` (the batched C entry) and through
the one-problem C entry ``symode_symreg_reversed``, entry by entry; the exact zeros, outputs pre-filled with NaN, repeated
launches, one operand at a time off its 16-byte boundary.

S2 / S3: ``forward_jvp``, ``vjp``, ``jvp_vjp`` (with and without g_out), ``euler_jvp`` and ``euler_jvp_vjp`` on either side of
the K at which the reverse sweep leaves its LDS state column; and ``rollout_error`` against an fp64 integration."""
import pytest
import torch

from tests import regulariser_cases as C
from tests import regulariser_model as M
from tests.helpers import _env

pytestmark = pytest.mark.gpu

LIBS = C.libs()
TOL = C.TOL["symreg_reversed"]
lib_id = lambda l: "d%do%df%d" % tuple(l)  # noqa: E731


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def on_device(t, shift):
    """t as a view of a flat device buffer that starts ``shift`` floats into its allocation."""
    flat = torch.zeros(t.numel() + shift, dtype=torch.float32, device="cuda")
    flat[shift:] = t.reshape(-1).cuda()
    view = flat[shift:].view(t.shape)
    assert view.is_contiguous() and (t.numel() == 0 or (view.data_ptr() % 16 != 0) == (shift % 4 != 0))
    return view


def device_operands(c):
    x, gx, jgx, xi, mask = C.operands(c)
    place = lambda t, name: on_device(t, c.shift[1] if c.shift[0] == name else 0)  # noqa: E731
    return place(x, "x"), place(gx, "gx"), place(jgx, "jgx"), xi.cuda(), None if mask is None else mask.cuda()


def launch(eng, c):
    """One launch through the engine; the outputs were full of NaN before it."""
    x, gx, jgx, xi, mask = device_operands(c)
    S, _, d = c.x.shape
    out = (torch.full((S,), float("nan"), device="cuda"), torch.full((S, d, xi.shape[-1]), float("nan"), device="cuda"))
    with _env(**c.env):
        loss, grad = eng.symreg_reversed(x, gx, jgx, xi, mask, c.lib[1], c.lib[2], out=out, inv_count=c.inv_count)
    assert loss.data_ptr() == out[0].data_ptr() and grad.data_ptr() == out[1].data_ptr()
    return loss.cpu(), grad.cpu()


def launch_one_problem_entry(eng, c):
    """The same through ``symode_symreg_reversed``, the C entry of one problem and the plain mean."""
    assert not c.batched and c.inv_count is None
    x, gx, jgx, xi, mask = device_operands(c)
    n, d = x.shape
    loss = torch.full((1,), float("nan"), device="cuda")
    grad = torch.full(tuple(xi.shape), float("nan"), device="cuda")
    with _env(**c.env):
        ws = eng.workspace(x.device, d, c.lib[1], c.lib[2], 1, n)
        rc = eng.lib.symode_symreg_reversed(eng._ptr(x), eng._ptr(gx) if gx.numel() else None, eng._ptr(jgx) if jgx.numel() else None,
                                            gx.shape[0], n, d, c.lib[1], c.lib[2], eng._ptr(xi), eng._ptr(mask), eng._ptr(loss),
                                            eng._ptr(grad), eng._ptr(ws), ws.numel() * 8, eng._stream(x))
        assert rc == 0, (c.name, rc)
        torch.cuda.synchronize()
    return loss[0].cpu(), grad.cpu()


def judge(c, loss, grad, bad, worst):
    d = c.lib[0]
    ref = C.reference(c.name)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()), f"{c.name}: an output entry was not written"
    dl, dg = M.deviation_s4(loss, grad, ref)
    worst[0], worst[1] = max(worst[0], dl / TOL[d]["loss"]), max(worst[1], dg / TOL[d]["grad"])
    if not (dl <= TOL[d]["loss"] and dg <= TOL[d]["grad"]):
        frac = M.fractions(grad, ref["grad"], ref["grad_yard"])
        bad.append((c.name, dl, dg, "worst grad entry (flat index) %d" % int(frac.argmax())))
    if c.exact_zero:                                                         # a zero yardstick: deviation_s4 demanded the exact 0
        assert not bool(loss.any()) and not bool(grad.any()), c.name
    if c.mask is not None:                                                   # a masked entry gets exactly zero gradient
        assert not bool(grad.reshape(-1)[(c.mask == 0).reshape(-1)].any()), c.name


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_s4_deck_vs_fp64_model(eng, lib):
    bad, worst = [], [0.0, 0.0]
    for c in C.s4_cases(tuple(lib)):
        judge(c, *launch(eng, c), bad, worst)
    print(f"symreg_reversed {lib_id(lib)}: worst deviation in units of the tolerance: loss {worst[0]:.3f}, grad {worst[1]:.3f}")
    assert bad == [], bad


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_s4_one_problem_entry_vs_fp64_model(eng, lib):
    bad, worst, seen = [], [0.0, 0.0], 0
    for c in C.s4_cases(tuple(lib)):
        if not c.batched and c.inv_count is None:
            seen += 1
            judge(c, *launch_one_problem_entry(eng, c), bad, worst)
    print(f"symode_symreg_reversed {lib_id(lib)}: worst deviation in units of the tolerance: loss {worst[0]:.3f}, grad {worst[1]:.3f}")
    assert seen >= 10 and bad == [], bad


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_s4_two_launches_on_one_workspace_give_equal_bits(eng, lib):
    for c in C.s4_cases(tuple(lib)):
        a, b = launch(eng, c), launch(eng, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), c.name


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_s4_misaligned_operand_against_the_aligned_copy(eng, lib):
    """Each of x, g(x), J_g off its 16-byte boundary in turn: the per-point loads give what the 16-byte loads give, to the
    tolerance (the two forms add the same terms in another order)."""
    d = lib[0]
    operands = set()
    for c in C.s4_cases(tuple(lib)):
        if c.shift[1]:
            operands.add(c.shift[0])
            (l0, g0), (l1, g1) = launch(eng, c._replace(shift=(None, 0))), launch(eng, c)
            ref = C.reference(c.name)
            dl = float(M.fractions(l1, l0.double(), ref["loss_yard"]).max())
            dg = float(M.fractions(g1, g0.double(), ref["grad_yard"]).max())
            assert dl <= TOL[d]["loss"] and dg <= TOL[d]["grad"], (c.name, dl, dg)
    assert operands == {"x", "gx", "jgx"}


# ---------------------------------------------------------------------------------------------------------------------
# S2 / S3: forward_jvp, vjp, jvp_vjp, euler_jvp, euler_jvp_vjp
# ---------------------------------------------------------------------------------------------------------------------
class nan_outputs:
    """Every float tensor the engine allocates inside the block starts full of NaN: an output entry a launch leaves
    unwritten shows (the engine hands its outputs out of ``torch.empty`` / ``torch.empty_like``)."""

    def __enter__(self):
        self.saved = torch.empty, torch.empty_like
        fill = lambda t: t.fill_(float("nan")) if t.is_floating_point() else t  # noqa: E731
        torch.empty = lambda *a, **k: fill(self.saved[0](*a, **k))
        torch.empty_like = lambda *a, **k: fill(self.saved[1](*a, **k))

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self.saved


def play(eng, c, name, **kw):
    """One play of an S2 / S3 case on the device: the operator's outputs in the order of ``regulariser_model.OPS``, on the host."""
    place = lambda t, operand: on_device(t, c.shift[1] if c.shift[0] == operand else 0)  # noqa: E731
    x, v, ga, gb = place(c.x, "x"), place(c.v, "v"), place(c.ga, "ga"), place(c.gb, "gb")
    xi, mask, (_, order, flags) = c.xi.cuda(), None if c.mask is None else c.mask.cuda(), c.lib
    with _env(**c.env), nan_outputs():
        if name == "forward_jvp":
            got = eng.forward_jvp(x, v, xi, mask, order, flags, **kw)
        elif name == "vjp":
            got = eng.vjp(x, ga, xi, mask, order, flags, **kw)
        elif name in ("jvp_vjp", "jvp_vjp_null"):
            got = eng.jvp_vjp(x, v, None if name == "jvp_vjp_null" else ga, gb, xi, mask, order, flags)
        elif name == "euler_jvp":
            got = eng.euler_jvp(x, v, xi, mask, order, flags, c.K, c.dt)
        elif name == "odeint":
            got = (eng.odeint(x, xi, mask, order, flags, c.K, c.dt, "euler"),)
        else:
            got = eng.euler_jvp_vjp(x, v, ga, gb, xi, mask, order, flags, c.K, c.dt)
    return tuple(None if t is None else t.cpu() for t in got)


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_ops_deck_vs_fp64_model(eng, lib):
    """Every play of every case within the derived tolerance of the fp64 model, every output entry written, exact zeros
    where the yardstick is zero (a mask of zeros, a masked entry of grad_xi), no step = the inputs bit for bit."""
    d = lib[0]
    bad, worst = [], {}
    for c in C.ops_cases(tuple(lib)):
        for name, op in C.PLAYS[c.kind]:
            got = play(eng, c, name)
            ref = C.ops_reference(c.name, name)
            assert all(bool(torch.isfinite(t).all()) for t in got), f"{c.name} {name}: an output entry was not written"
            for field, dev in M.deviation_op(op, got, ref).items():
                tol = C.OPS_TOL[op][d][field]
                worst[op, field] = max(worst.get((op, field), 0.0), dev / tol)
                if not dev <= tol:
                    bad.append((c.name, name, field, dev, tol))
            fields = dict(zip(M.OPS[op], got))
            if "grad_xi" in fields and c.mask is not None:
                assert not bool(fields["grad_xi"][c.mask == 0].any()), (c.name, name)
            if c.exact_zero and c.kind == "step":
                assert not any(bool(t.any()) for t in got), (c.name, name)
            if c.kind == "euler" and c.K == 0:
                first, second = (c.x, c.v) if op == "euler_jvp" else (c.ga, c.gb)
                assert torch.equal(got[0], first) and torch.equal(got[1], second), (c.name, name)
                assert op == "euler_jvp" or not bool(got[2].any()), (c.name, name)
    for (op, field), w in sorted(worst.items()):
        print(f"{op} {lib_id(lib)} {field}: worst deviation {w:.3f} of the tolerance")
    assert bad == [], bad


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_ops_optional_outputs_and_the_plain_flow_give_equal_bits(eng, lib):
    """``need_out=False`` and ``need_grad_x=False`` leave the other output as it was, bit for bit; ``odeint(..., "euler")``
    is x_K of ``euler_jvp`` bit for bit: both claim the same step."""
    for c in C.ops_cases(tuple(lib)):
        if c.kind == "step":
            (out, jv), (none, jv_alone) = play(eng, c, "forward_jvp"), play(eng, c, "forward_jvp", need_out=False)
            assert none is None and torch.equal(jv, jv_alone), c.name
            (_, gxi), (none, gxi_alone) = play(eng, c, "vjp"), play(eng, c, "vjp", need_grad_x=False)
            assert none is None and torch.equal(gxi, gxi_alone), c.name
        elif c.K >= 1:
            assert torch.equal(play(eng, c, "odeint")[0], play(eng, c, "euler_jvp")[0]), c.name


@pytest.mark.parametrize("lib", LIBS, ids=lib_id)
def test_ops_two_launches_on_one_workspace_give_equal_bits(eng, lib):
    for c in C.ops_cases(tuple(lib)):
        for name, _ in C.PLAYS[c.kind]:
            a, b = play(eng, c, name), play(eng, c, name)
            assert all(torch.equal(s, t) for s, t in zip(a, b)), (c.name, name)


@pytest.mark.parametrize("lib", C.rollout_libs(), ids=lib_id)
@pytest.mark.parametrize("method", ["rk4", "euler"])
def test_rollout_error_vs_fp64_integration(eng, lib, method):
    """``rollout_error``'s err against the squared error of an fp64 integration of the same float32 inputs
    (``regulariser_model.rollout_error``): a judge of ``integrate_steps`` that shares no code with it."""
    c = C.rollout_case(tuple(lib))
    ref, yard = C.rollout_reference(tuple(lib), method)
    err, mean_err, horizon = eng.rollout_error(c.x_true.cuda(), c.xi.cuda(), c.mask.cuda(), lib[1], lib[2], c.dt, method=method)
    assert tuple(err.shape) == (C.ROLLOUT_MODELS, C.ROLLOUT_ICS, C.ROLLOUT_STEPS)
    dev = float(M.fractions(err.cpu(), ref, yard).max())
    tol = C.ROLLOUT_TOL[lib[0]][method]
    print(f"rollout_error {lib_id(lib)} {method}: worst deviation {dev:.3e} of the yardstick, {dev / tol:.3f} of the tolerance {tol:.1e}")
    assert dev <= tol
    assert torch.allclose(mean_err.cpu(), err.cpu().double().mean(-1), rtol=1e-14, atol=0.0)      # the fp32 values added in fp64
    assert bool((horizon.cpu() == C.ROLLOUT_STEPS).all())
