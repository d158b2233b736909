"""CPU witness of the regulariser tests (S4, the S2 / S3 operators and the roll-out check): the hand-written gradients and
adjoint sweeps of tests/regulariser_model.py are what fp64 autograd gives through the model's own forward side, the model is
the oracle's formula, the tolerances of tests/regulariser_cases.py are what the float32 replay gives, and the deck of EVERY
library rejects every mutant that applies to it.  Runs on the whole deck (all libraries, compiled or not): nothing here
touches the device library."""
import pytest
import torch

from oracle import sindy_oracle as O
from tests import regulariser_cases as C
from tests import regulariser_model as M

NOISE = 1e-12          # model = autograd = oracle to this fraction of the yardsticks
MARGIN = 4.0           # a mutant has to move a case of every library by more than MARGIN x the tolerance


@pytest.fixture(scope="module")
def cases():
    return C.s4_deck(C.all_libs())


def test_s4_gradient_is_fp64_autograd_through_the_model_forward(cases):
    worst = 0.0
    for c in cases:
        x, gx, jgx, xi, mask = C.operands(c)
        ref = C.reference(c.name)
        xi = xi.double().requires_grad_(True)
        r = M.evaluate_s4(x, gx, jgx, xi, mask, c.lib[1], c.lib[2], inv_count=c.inv_count)
        assert torch.equal(r["loss"].detach(), ref["loss"]) and torch.equal(r["grad"].detach(), ref["grad"]), c.name
        if r["loss"].requires_grad:
            auto, = torch.autograd.grad(r["loss"].sum(), xi)
        else:
            assert c.gx.shape[1] == 0
            auto = torch.zeros_like(xi)
        dev = float(M.fractions(auto, ref["grad"], ref["grad_yard"]).max())
        assert dev <= NOISE, (c.name, dev)
        worst = max(worst, dev)
    print("S4 hand-written gradient vs fp64 autograd, worst fraction of the yardstick:", worst)


def oracle_libs():
    """Three libraries per d: the lowest and the highest order, and the highest with sine and exp."""
    return [lib for d, orders in C.ORDERS.items() for lib in ((d, orders[0], 0), (d, orders[-1], 0), (d, orders[-1], 3))]


def test_s4_model_is_the_oracle_formula():
    worst = (0.0, 0.0)
    for c in C.s4_deck(oracle_libs()):
        d, order, flags = c.lib
        S, n, _ = c.x.shape
        ref = C.evaluate(c, round_inv=False)             # the oracle's mean divides by n d exactly
        scale = 1.0 if c.inv_count is None else c.inv_count * n * d
        for s in range(S):
            xi = c.xi[s].double().requires_grad_(True)
            mk = torch.ones_like(xi) if c.mask is None else c.mask[s].double()
            h = lambda a: O.theta(a, order, bool(flags & 1), bool(flags & 2)) @ (xi * mk).T  # noqa: E731
            loss = scale * O.symreg_reversed_precomputed(c.x[s].double(), list(c.gx[s].double()), list(c.jgx[s].double()), h)
            if torch.is_tensor(loss) and loss.requires_grad:
                grad, = torch.autograd.grad(loss, xi)
            else:                                        # no group element: the oracle's sum is the float 0.0
                assert c.gx.shape[1] == 0 and float(loss) == 0.0
                grad = torch.zeros_like(xi)
            one = {k: (v[s] if c.batched and v.dim() else v) for k, v in ref.items()}
            dev = M.deviation_s4(float(loss.detach()) if torch.is_tensor(loss) else loss, grad, one)
            assert dev[0] <= NOISE and dev[1] <= NOISE, (c.name, s, dev)
            worst = (max(worst[0], dev[0]), max(worst[1], dev[1]))
    print("S4 model vs oracle, worst fraction of the yardstick (loss, grad):", worst)


def replay_figures(cases):
    """Per d and field: the worst deviation of the float32 sequential model from the fp64 model, as a fraction of the yardstick."""
    worst = {}
    for c in cases:
        got = C.evaluate(c, dt=torch.float32, sequential=True)
        dl, dg = M.deviation_s4(got["loss"], got["grad"], C.reference(c.name))
        w = worst.setdefault(c.lib[0], {"loss": (0.0, None), "grad": (0.0, None)})
        if dl > w["loss"][0]:
            w["loss"] = (dl, c.name)
        if dg > w["grad"][0]:
            w["grad"] = (dg, c.name)
    return worst


def test_s4_tolerances_are_four_times_the_float32_replay(cases):
    worst = replay_figures(cases)
    tol = C.TOL["symreg_reversed"]
    for d in sorted(worst):
        for field in ("loss", "grad"):
            fig, where = worst[d][field]
            print(f"symreg_reversed d = {d} {field}: replay {fig:.3e} at {where}, 4 x rounded up {C.round_up_2(4 * fig):.1e}, deck {tol[d][field]:.1e}")
    for d in sorted(worst):
        for field in ("loss", "grad"):
            assert tol[d][field] == C.round_up_2(4 * worst[d][field][0]), (d, field, worst[d][field])


def test_s4_exact_zero_cases(cases):
    """A mask of zeros and no group element: the model's result AND yardsticks are exactly 0, in fp64 and in the float32
    replay.  J_g = I with g x = x: the fp64 result is exactly 0 under a yardstick that is not."""
    seen = identity = 0
    for c in cases:
        if c.exact_zero:
            seen += 1
            for dt, seq in ((torch.float64, False), (torch.float32, True)):
                r = C.evaluate(c, dt=dt, sequential=seq)
                assert not bool(r["loss"].any()) and not bool(r["grad"].any()), c.name
                assert not bool(r["loss_yard"].any()) and not bool(r["grad_yard"].any()), c.name
        if "-identity-" in c.name:
            identity += 1
            ref = C.reference(c.name)
            assert float(ref["loss"]) == 0.0 and not bool(ref["grad"].any()) and float(ref["loss_yard"]) > 0.0, c.name
            assert bool((ref["grad_yard"] > 0).any()), c.name
    assert seen >= 3 * len(C.all_libs()) and identity == len(C.all_libs())


def test_s4_every_mutant_is_rejected_by_the_deck_of_every_library():
    """Each mutant moves at least one case of EVERY library it applies to by more than 4 x that library's tolerance."""
    tol = C.TOL["symreg_reversed"]
    missed, caught = [], {m: 0 for m in M.S4_MUTANTS}
    for lib in C.all_libs():
        d = lib[0]
        deck = C.s4_cases(tuple(lib))
        for m in M.S4_MUTANTS:
            # a library is outside a mutant's reach only where the mistake changes nothing at ANY shape: a transpose, a
            # stride of n d for n d d and a divisor n for n d at d = 1, a ragged point where a chunk holds one point (d = 4)
            beyond = d == 1 and m in ("jg_transposed", "grad_jg_for_jg_t", "jgx_group_stride_n_d", "divisor_n") or \
                M.PPT[d] == 1 and m == "last_ragged_point_dropped"
            assert any(C.applies(m, c) for c in deck) != beyond, (lib, m)
            if beyond:
                continue
            hit = False
            for c in deck:                               # (the first case that rejects it settles the library)
                if C.applies(m, c):
                    got = C.evaluate(c, mutant=m)
                    dl, dg = M.deviation_s4(got["loss"], got["grad"], C.reference(c.name))
                    if dl > MARGIN * tol[d]["loss"] or dg > MARGIN * tol[d]["grad"]:
                        hit = True
                        break
            caught[m] += int(hit)
            if not hit:
                missed.append((lib, m))
    print("libraries whose deck rejects each S4 mutant:", caught)
    assert missed == [], missed


# ---------------------------------------------------------------------------------------------------------------------
# S2 / S3: forward_jvp, vjp, jvp_vjp, euler_jvp, euler_jvp_vjp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    return C.ops_deck(C.all_libs())


def against_fp64_autograd(c, forward):
    """Every play of case ``c`` of the model against fp64 autograd through ``forward(x, v, xi) -> (out, jv)`` [the flow:
    (x_K, t_K)]: {(operator, field): worst fraction of the yardstick}."""
    x, v, xi = (t.double().requires_grad_(True) for t in (c.x, c.v, c.xi))
    ga, gb = c.ga.double(), c.gb.double()
    first, second = forward(x, v, xi)
    worst = {}
    for play, op in C.PLAYS[c.kind]:
        if op in ("forward_jvp", "euler_jvp"):
            got = (first.detach(), second.detach())
        else:
            target = 0.0
            if play != "jvp_vjp_null":
                target = target + (first * ga).sum()
            if op != "vjp":
                target = target + (second * gb).sum()
            grads = torch.autograd.grad(target, (x, v, xi), retain_graph=True, allow_unused=True)
            gx, gv, gxi = (torch.zeros_like(t) if g is None else g for g, t in zip(grads, (x, v, xi)))
            got = dict(grad_x=gx, grad_v=gv, grad_xi=gxi)
        for field, dev in M.deviation_op(op, got, C.ops_reference(c.name, play)).items():
            worst[op, field] = max(worst.get((op, field), 0.0), dev)
    return worst


def model_forward(c):
    op = "forward_jvp" if c.kind == "step" else "euler_jvp"
    def forward(x, v, xi):
        r = M.evaluate_op(op, x, v, None, None, xi, c.mask, c.lib[1], c.lib[2], K=c.K, dt=c.dt, yardsticks=False)
        return tuple(r[f] for f in M.OPS[op])
    return forward


def oracle_forward(c):
    d, order, flags = c.lib
    mk = torch.ones(c.xi.shape, dtype=torch.float64) if c.mask is None else c.mask.double()
    def forward(x, v, xi):
        f = lambda a: O.forward(a, xi, mk, order, bool(flags & 1), bool(flags & 2))  # noqa: E731
        flow = f if c.kind == "step" else (lambda a: O.odeint(f, a, (c.K + 0.5) * c.dt, c.dt, "euler"))
        return torch.autograd.functional.jvp(flow, x, v, create_graph=True)
    return forward


def merge(into, new, name):
    for key, dev in new.items():
        assert dev <= NOISE, (name, key, dev)
        into[key] = max(into.get(key, 0.0), dev)


def test_ops_adjoints_are_fp64_autograd_through_the_model_forward(ops):
    """The hand-written reverse modes (one step and the sweep of the flow) against autograd through the model's own forward
    side, on every case; the forward fields are compared too (they are the same computation: 0)."""
    worst = {}
    for c in ops:
        merge(worst, against_fp64_autograd(c, model_forward(c)), c.name)
    print("hand-written adjoints vs fp64 autograd through the model forward, worst fraction of the yardstick:", worst)


def test_ops_model_is_the_oracle_formula():
    """``oracle.sindy_oracle.forward`` and ``odeint`` under autograd (the jvp by the double-backward trick)."""
    worst = {}
    for c in C.ops_deck(oracle_libs()):
        merge(worst, against_fp64_autograd(c, oracle_forward(c)), c.name)
    print("model vs oracle forward / odeint under fp64 autograd, worst fraction of the yardstick:", worst)


@pytest.fixture(scope="module")
def replays(ops):
    """{(case, play): the float32 sequential model}, computed once for the tests below"""
    return {(c.name, play): C.evaluate_play(c, play, dtype=torch.float32, sequential=True, yardsticks=False) for c in ops for play, _ in C.PLAYS[c.kind]}


def ops_replay_figures(cases, replays):
    """{operator: {d: {field: (worst deviation of the float32 sequential model from the fp64 model, case)}}}"""
    worst = {}
    for c in cases:
        for play, op in C.PLAYS[c.kind]:
            got = replays[c.name, play]
            for field, dev in M.deviation_op(op, got, C.ops_reference(c.name, play)).items():
                w = worst.setdefault(op, {}).setdefault(c.lib[0], {})
                if dev >= w.get(field, (0.0, None))[0]:
                    w[field] = (dev, c.name)
    return worst


def test_ops_tolerances_are_four_times_the_float32_replay(ops, replays):
    worst = ops_replay_figures(ops, replays)
    derived = {op: {d: {f: C.round_up_2(4 * fig) for f, (fig, _) in fields.items()} for d, fields in per_d.items()} for op, per_d in worst.items()}
    for op in M.OPS:
        for d in sorted(worst[op]):
            for field in M.OPS[op]:
                fig, where = worst[op][d][field]
                print(f"{op} d = {d} {field}: replay {fig:.3e} at {where}, 4 x rounded up {derived[op][d][field]:.1e}, deck {C.OPS_TOL[op][d][field]:.1e}")
    print("OPS_TOL =", derived)
    assert C.OPS_TOL == derived


def test_ops_zero_yardsticks_and_the_cases_without_a_step(ops, replays):
    """Where a yardstick is zero the model is exactly zero, in fp64 and in the float32 replay; a mask of zeros zeroes every
    field of the one-step operators and grad_xi of the flow; no step returns the inputs bit for bit."""
    zero_mask = no_step = 0
    for c in ops:
        for play, op in C.PLAYS[c.kind]:
            ref = C.ops_reference(c.name, play)
            replay = replays[c.name, play]
            for field in M.OPS[op]:
                dead = ref[field + "_yard"] == 0
                assert not bool(ref[field][dead].any()) and not bool(replay[field][dead].any()), (c.name, play, field)
                if c.exact_zero and (c.kind == "step" or field == "grad_xi"):
                    assert bool(dead.all()), (c.name, play, field)
            if c.kind == "euler" and c.K == 0:
                first, second = (c.x, c.v) if op == "euler_jvp" else (c.ga, c.gb)
                assert torch.equal(replay[M.OPS[op][0]], first) and torch.equal(replay[M.OPS[op][1]], second), (c.name, play)
                assert op == "euler_jvp" or not bool(ref["grad_xi_yard"].any()), c.name
        zero_mask += int(c.exact_zero)
        no_step += int(c.kind == "euler" and c.K == 0)
    assert zero_mask == 2 * len(C.all_libs()) and no_step == len(C.all_libs())


def test_ops_stack_boundary_cases_are_in_every_deck():
    """K = 1 and 2, the last K of the LDS state column and the first K that recomputes, at the ragged size; the column's own
    sizes again with the column switched off."""
    for lib in C.all_libs():
        deck = C.ops_cases(tuple(lib))
        last = C.STACK_LAST[lib[0]]
        assert last * 2 * lib[0] * 256 * 4 <= 65536 < (last + 1) * 2 * lib[0] * 256 * 4
        plain = {c.K for c in deck if c.kind == "euler" and c.x.shape[0] == 1031 and not c.env}
        off = {c.K for c in deck if c.env.get("SYMODE_EULER_STACK") == 0}
        assert {0, 1, 2, last, last + 1} <= plain and off == {2, last}, lib
        assert all(c.K * c.dt <= C.FLOW_TIME and float(torch.tensor(c.dt, dtype=torch.float32)) == c.dt for c in deck)


def test_ops_every_mutant_is_rejected_by_the_deck_of_every_library():
    """Each mutant moves at least one play of one case of EVERY library it applies to by more than 4 x the tolerance."""
    missed, caught = [], {m: 0 for m in M.OPS_MUTANTS}
    for lib in C.all_libs():
        d, order, flags = lib
        deck = C.ops_cases(tuple(lib))
        flat = order == 1 and flags == 0                 # a library without a second derivative
        for m in M.OPS_MUTANTS:
            beyond = {"tangent_step_uses_updated_x": flat, "second_order_term_missing": flat, "second_order_roles_swapped": flat or d == 1, "sine_second_derivative_sign": not flags & 1,
                      "exp_second_derivative_zero": not flags & 2, "last_ragged_point_dropped": M.PPT[d] == 1}.get(m, False)
            plays = [(c, play, op) for c in deck for play, op in C.PLAYS[c.kind] if C.ops_applies(m, c, play)]
            assert bool(plays) != beyond, (lib, m)
            hit = False
            for c, play, op in plays:                    # (the first play that rejects it settles the library)
                got = C.evaluate_play(c, play, mutant=m, yardsticks=False)
                dev = M.deviation_op(op, got, C.ops_reference(c.name, play))
                if any(dev[f] > MARGIN * C.OPS_TOL[op][d][f] for f in dev):
                    hit = True
                    break
            caught[m] += int(hit)
            if plays and not hit:
                missed.append((lib, m))
    print("libraries whose deck rejects each S2 / S3 mutant:", caught)
    assert missed == [], missed


def test_rollout_tolerances_are_four_times_the_float32_replay():
    derived = {}
    for d, lib in C.ROLLOUT_LIBS.items():
        c = C.rollout_case(lib)
        for method in ("rk4", "euler"):
            ref, yard = C.rollout_reference(lib, method)
            got, _ = M.rollout_error(c.x_true, c.xi, c.mask, lib[1], lib[2], c.dt, method, dtype=torch.float32, sequential=True)
            fig = float(M.fractions(got, ref, yard).max())
            derived.setdefault(d, {})[method] = C.round_up_2(4 * fig)
            print(f"rollout_error d = {d} {method}: replay {fig:.3e}, 4 x rounded up {derived[d][method]:.1e}, deck {C.ROLLOUT_TOL[d][method]:.1e}")
            # the model's integrator is the oracle's, step for step
            f = lambda a: O.forward(a, c.xi[0].double(), c.mask[0].double(), lib[1], bool(lib[2] & 1), bool(lib[2] & 2))  # noqa: E731
            traj = O.odeint(f, c.x_true[:, 0].double(), (C.ROLLOUT_STEPS + 0.5) * c.dt, c.dt, method, full_traj=True)
            want = ((c.x_true[:, 1:].double() - traj.transpose(0, 1)) ** 2).mean(-1)
            assert float(M.fractions(ref[0], want, yard[0]).max()) <= NOISE
    print("ROLLOUT_TOL =", derived)
    assert C.ROLLOUT_TOL == derived
