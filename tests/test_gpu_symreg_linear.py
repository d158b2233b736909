"""S1 (``symreg_linear_kernel``) on the device against the fp64 model of tests/symreg_linear_model.py: the deck of
tests/symreg_linear_cases.py through ``engine.symreg_linear`` within the derived tolerances, the exact zeros, repeated
launches, misaligned bases, the raw C entry without generators, and the autograd wrapper ``model_utils.symmreg_linear``."""
import pytest
import torch

from oracle import sindy_oracle as O
from tests import symreg_linear_cases as C
from tests import symreg_linear_model as M
from tests.helpers import _env, compiled

pytestmark = pytest.mark.gpu

LIBS = C.libs()


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def on_device(z, shift):
    """z (n, d) as a view of a flat device buffer that starts ``shift`` floats into its allocation."""
    n, d = z.shape
    flat = torch.zeros(n * d + shift, dtype=torch.float32, device="cuda")
    flat[shift:] = z.reshape(-1).cuda()
    view = flat[shift:].view(n, d)
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == (shift % 4 != 0)
    return view


def launch(eng, c, shift=None):
    mask = None if c.mask is None else c.mask.cuda()
    with _env(**c.env):
        loss, grad = eng.symreg_linear(on_device(c.z, c.shift if shift is None else shift), c.xi.cuda(), mask, c.L.cuda(), c.lib[1], c.lib[2])
    return loss.cpu(), grad.cpu()


def run_deck(eng, lib):
    """Every case of ``lib``: (failures, worst (loss, grad) deviation as fractions of the yardsticks)."""
    d = lib[0]
    bad, wl, wg = [], 0.0, 0.0
    for c in C.lib_cases(tuple(lib)):
        loss, grad = launch(eng, c)
        ref = C.reference(c.name)
        dl, dg = M.deviation(loss, grad, ref)
        wl, wg = max(wl, dl), max(wg, dg)
        if not (dl <= C.TOL[d]["loss"] and dg <= C.TOL[d]["grad"]):
            bad.append((c.name, dl, dg))
        if c.exact_zero or c.L.shape[0] == 0:                                # a zero yardstick: deviation() demanded the exact 0
            assert float(loss) == 0.0 and not bool(grad.any()) and bool(torch.isfinite(grad).all()), c.name
        if c.mask is not None:                                               # a masked entry gets exactly zero gradient
            assert not bool(grad[c.mask == 0].any()), c.name
    return bad, (wl, wg)


@pytest.mark.parametrize("lib", LIBS, ids=lambda l: "d%do%df%d" % tuple(l))
def test_deck_vs_fp64_model(eng, lib):
    bad, (wl, wg) = run_deck(eng, lib)
    tol = C.TOL[lib[0]]
    print(f"{lib}: worst deviation loss {wl:.3e} (tolerance {tol['loss']:.1e}), grad {wg:.3e} (tolerance {tol['grad']:.1e})")
    assert bad == [], bad


@pytest.mark.parametrize("lib", LIBS, ids=lambda l: "d%do%df%d" % tuple(l))
def test_two_launches_on_one_workspace_give_equal_bits(eng, lib):
    for c in C.lib_cases(tuple(lib)):
        a, b = launch(eng, c), launch(eng, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), c.name


@pytest.mark.parametrize("lib", LIBS, ids=lambda l: "d%do%df%d" % tuple(l))
def test_misaligned_base_against_the_aligned_copy(eng, lib):
    d = lib[0]
    seen = 0
    for c in C.lib_cases(tuple(lib)):
        if c.shift:
            seen += 1
            (l0, g0), (l1, g1) = launch(eng, c, shift=0), launch(eng, c)
            ref = C.reference(c.name)
            dl = abs(float(l1) - float(l0)) / float(ref["loss_yard"]) if float(ref["loss_yard"]) else abs(float(l1) - float(l0))
            dg = float((g1.double() - g0.double()).abs().max()) / max(float(ref["grad_yard"].max()), 1e-300)
            assert dl <= C.TOL[d]["loss"] and dg <= C.TOL[d]["grad"], (c.name, dl, dg)
    assert seen >= 3


@pytest.mark.parametrize("d,order,flags", [lib for lib in [(1, 3, 0), (2, 3, 0), (3, 2, 1), (3, 3, 0), (4, 2, 0)] if compiled(*lib)])
def test_no_generator_through_the_raw_c_entry(eng, d, order, flags):
    """n_gen = 0 with L == NULL, which the C ABI allows: return code 0, loss and gradient finite and exactly 0 (outputs
    pre-filled with NaN: they must be written)."""
    p = eng.lib_size(d, order, flags)
    gen = torch.Generator().manual_seed(5 + d)
    z = (0.5 * torch.randn(1031, d, generator=gen)).cuda()
    xi = (0.4 * torch.randn(d, p, generator=gen)).cuda()
    loss = torch.full((1,), float("nan"), device="cuda")
    grad = torch.full((d, p), float("nan"), device="cuda")
    ws = eng.workspace(z.device, d, order, flags, 1, z.shape[0])
    rc = eng.lib.symode_symreg_linear(eng._ptr(z), z.shape[0], d, order, flags, eng._ptr(xi), None, None, 0, eng._ptr(loss), eng._ptr(grad),
                                      eng._ptr(ws), ws.numel() * 8, eng._stream(z))
    assert rc == 0
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and bool((grad == 0).all())
    l2, g2 = eng.symreg_linear(z, xi, None, torch.empty(0, d, d, device="cuda"), order, flags)
    assert float(l2) == 0.0 and bool((g2 == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the autograd wrapper
# ---------------------------------------------------------------------------------------------------------------------
UPSTREAM = 0.37
EPS = 2.0 ** -24


@pytest.mark.parametrize("d,order,sine,constrained", [c for c in [(2, 3, False, False), (2, 3, False, True), (3, 2, True, False), (1, 4, False, False),
                                                                  (4, 2, False, False)] if compiled(c[0], c[1])])
def test_wrapper_gradients_reach_every_trainable_parameter(eng, d, order, sine, constrained):
    """``model_utils.symmreg_linear`` on an unconstrained and a constrained SINDyRegression: a basis list of (d+1) x (d+1)
    matrices whose leading d x d block is the generator, z shaped (a, b, d) with requires_grad (z.grad stays None, as the
    docstring says), the loss multiplied by 0.37 before backward(); the gradient of every trainable parameter against fp64
    autograd through the oracle and the coefficient map.

    Tolerances.  The kernel's (loss, d/dXi) deviate by at most TOL of their yardsticks.  On top of that float32 autograd
    rounds 0.37 itself and the product 0.37 * grad (3 * 2^-24 in all), and under the constraint
      * the dot products Q^T g of length d p: forward error at most d p * 2^-24 of |Q|^T |g| <= |Q|^T yardstick;
      * the kernel is handed Xi = Q beta + const rounded in float32, each entry off by at most (r + 1) * 2^-24 <= (d p + 1) *
        2^-24 of |Q| |beta| + |const|, where the fp64 reference maps the float32 beta exactly: the loss moves by at most
        sum |dloss/dXi| |dXi| and the gradient by the same sum over its own derivative, both at most that fraction of the
        yardsticks, which carry |Xi| |dth| and |Xi| |th| in every term.
    So (d p + 4) * 2^-24 on the loss and (2 d p + 4) * 2^-24 on the gradients, of the yardstick carried through the same map
    with |Q| in place of Q."""
    from symode_amd import model_utils
    from symode_amd.sindy import SINDyRegression
    torch.manual_seed(40 + 10 * d + order)
    L_list = [torch.tensor([[0.0, 1.0], [-1.0, 0.0]])] if constrained else []
    reg = SINDyRegression(d, order, sine, False, L_list=L_list, threshold=0.1, device="cuda:0", constrain_constant=False)
    flags = reg.flags
    p = reg.get_term_num()
    with torch.no_grad():
        for q in reg.parameters():
            q.mul_(0.4)
    reg.mask = (torch.rand(d, p) >= 0.25).float().cuda()
    basis = [(0.5 + 0.5 * torch.rand(d + 1, d + 1)) * torch.where(torch.rand(d + 1, d + 1) < 0.5, -1.0, 1.0) for _ in range(2)]
    z = (0.5 * torch.randn(7, 33, d)).clamp(-1.2, 1.2).cuda().requires_grad_(True)
    loss = model_utils.symmreg_linear(z, reg, [b.cuda() for b in basis])
    (UPSTREAM * loss).backward()
    assert z.grad is None
    params = [q for q in reg.parameters() if q.requires_grad]
    assert len(params) == (2 if constrained else 1) and all(q.grad is not None for q in params)

    # fp64: the same float32 numbers through the oracle and the coefficient map
    mask = reg.mask.cpu().double()
    p64 = [q.detach().cpu().double().requires_grad_(True) for q in params]

    def xi_of(ps, Q):
        if not constrained:
            return ps[0]
        beta, const = (ps[0], ps[1]) if ps[0].dim() == 1 else (ps[1], ps[0])
        return O.xi_from_beta(Q, beta, const, d, reg.use_kron_product, reg.allow_constant)
    Q = reg.Q.cpu().double() if constrained else None
    xi64 = xi_of(p64, Q)
    h = lambda a: O.theta(a, order, sine, False) @ (xi64 * mask).T  # noqa: E731
    Ls = [b[:d, :d].double() for b in basis]
    z64 = z.detach().cpu().double().reshape(-1, d)
    want = O.symreg_linear_latent(z64, Ls, h)
    want_grads = torch.autograd.grad(UPSTREAM * want, p64)
    ref = M.evaluate(z64.float(), xi64.detach().float(), mask.float(), torch.stack(Ls).float(), order, flags)
    # (the model at the float32 Xi the kernel was handed only supplies the yardsticks)
    tol_l = C.TOL[d]["loss"] + ((d * p + 4) if constrained else 3) * EPS
    tol_g = C.TOL[d]["grad"] + ((2 * d * p + 4) if constrained else 3) * EPS
    got_loss, want_loss = float(loss.detach()), float(want.detach())
    assert abs(got_loss - want_loss) <= tol_l * float(ref["loss_yard"]), (got_loss, want_loss)
    ones = [torch.ones_like(q).requires_grad_(True) for q in p64]
    yard = torch.autograd.grad((xi_of(ones, None if Q is None else Q.abs()) * ref["grad_yard"]).sum(), ones)
    for q, g64, y in zip(params, want_grads, yard):
        dev = float((q.grad.cpu().double() - g64).abs().max()) / (UPSTREAM * float(y.max()))
        print(f"d={d} order={order} constrained={constrained} {tuple(q.shape)}: deviation {dev:.3e} of the yardstick, tolerance {tol_g:.2e}")
        assert dev <= tol_g, (tuple(q.shape), dev, tol_g)
