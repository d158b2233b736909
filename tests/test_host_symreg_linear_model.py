"""CPU witness of the S1 tests: the model is the oracle's formula, the tolerances of tests/symreg_linear_cases.py are what
the float32 replay gives, and the deck notices every mutant of tests/symreg_linear_model.py.  Runs on the whole deck (all
libraries, compiled or not): nothing here touches the device library."""
import pytest
import torch

from oracle import sindy_oracle as O
from tests import symreg_linear_cases as C
from tests import symreg_linear_model as M

NOISE = 1e-12          # model = oracle to this fraction of the yardstick; a mutant's change below it is fp64 rounding, no change


@pytest.fixture(scope="module")
def cases():
    return C.deck(C.all_libs())


def test_model_is_the_oracle_formula_by_fp64_autograd(cases):
    worst = (0.0, 0.0)
    for c in cases:
        d, order, flags = c.lib
        ref = C.reference(c.name)
        xi = c.xi.double().requires_grad_(True)
        mk = torch.ones_like(xi) if c.mask is None else c.mask.double()
        h = lambda a: O.theta(a, order, bool(flags & 1), bool(flags & 2)) @ (xi * mk).T  # noqa: E731
        loss = O.symreg_linear_latent(c.z.double(), list(c.L.double()), h)
        if torch.is_tensor(loss) and loss.requires_grad:
            grad, = torch.autograd.grad(loss, xi)
        else:                                                                # no generator: the oracle's sum is the float 0.0
            assert c.L.shape[0] == 0 and float(loss) == 0.0
            grad = torch.zeros_like(xi)
        dev = M.deviation(float(loss.detach()) if torch.is_tensor(loss) else loss, grad, ref)
        assert dev[0] <= NOISE and dev[1] <= NOISE, (c.name, dev)
        worst = (max(worst[0], dev[0]), max(worst[1], dev[1]))
    print("model vs oracle, worst fraction of the yardstick (loss, grad):", worst)


def replay_figures(cases):
    """Per d and field: the worst deviation of the float32 sequential model from the fp64 model, as a fraction of the yardstick."""
    worst = {}
    for c in cases:
        got = M.evaluate(c.z, c.xi, c.mask, c.L, c.lib[1], c.lib[2], dt=torch.float32, sequential=True)
        dl, dg = M.deviation(got["loss"], got["grad"], C.reference(c.name))
        w = worst.setdefault(c.lib[0], {"loss": (0.0, None), "grad": (0.0, None)})
        if dl > w["loss"][0]:
            w["loss"] = (dl, c.name)
        if dg > w["grad"][0]:
            w["grad"] = (dg, c.name)
    return worst


def test_tolerances_are_four_times_the_float32_replay(cases):
    worst = replay_figures(cases)
    for d in sorted(worst):
        for field in ("loss", "grad"):
            fig, where = worst[d][field]
            print(f"d = {d} {field}: replay {fig:.3e} at {where}, 4 x rounded up {C.round_up_2(4 * fig):.1e}, deck {C.TOL[d][field]:.1e}")
    for d in sorted(worst):
        for field in ("loss", "grad"):
            assert C.TOL[d][field] == C.round_up_2(4 * worst[d][field][0]), (d, field, worst[d][field])


def test_exact_zero_cases(cases):
    """A mask of zeros and no generator: the model's result AND yardsticks are exactly 0, in fp64 and in the float32 replay."""
    seen = 0
    for c in cases:
        if c.exact_zero or c.L.shape[0] == 0:
            seen += 1
            for dt, seq in ((torch.float64, False), (torch.float32, True)):
                r = M.evaluate(c.z, c.xi, c.mask, c.L, c.lib[1], c.lib[2], dt=dt, sequential=seq)
                assert float(r["loss"]) == 0.0 and not bool(r["grad"].any()) and float(r["grad_yard"].max()) == 0.0, c.name
    assert seen >= 2 * len(C.all_libs())


def test_equivariant_case_is_exactly_zero_in_fp64(cases):
    for c in cases:
        if "-equivariant-" in c.name:
            ref = C.reference(c.name)
            assert float(ref["loss"]) == 0.0 and not bool(ref["grad"].any()) and float(ref["loss_yard"]) > 0.0, c.name


def test_every_mutant_is_caught_and_every_case_decides(cases):
    """Each mutant moves at least one case by more than that case's tolerance; and no case is moved by a mutant by an amount
    the tolerance could hide: a change is either fp64 rounding (<= NOISE of the yardstick: the mutant does not apply to the
    case, e.g. a transposed generator at d = 1) or larger than the tolerance."""
    caught = {m: 0 for m in M.MUTANTS}
    undecided = []
    for c in cases:
        d, order, flags = c.lib
        ref = C.reference(c.name)
        tol = C.TOL[d]
        for m in M.MUTANTS:
            if m.startswith("sine") and not flags & 1 or m.startswith("exp") and not flags & 2:
                continue
            if m.startswith("further") and c.L.shape[0] < 2 or m.startswith("mask") and c.mask is None:
                continue
            got = M.evaluate(c.z, c.xi, c.mask, c.L, order, flags, mutant=m)
            dl, dg = M.deviation(got["loss"], got["grad"], ref)
            hit = dl > tol["loss"] or dg > tol["grad"]
            caught[m] += int(hit)
            if not hit and max(dl, dg) > NOISE:
                undecided.append((c.name, m, dl, dg))
    assert undecided == [], undecided[:10]
    assert all(caught.values()), caught
    print("cases that catch each mutant:", caught)
