"""The cases of the regulariser tests, with their tolerances: S4 (the materialised reversed symmetry regulariser) first, then
the S2 / S3 operators (forward_jvp, vjp, jvp_vjp, euler_jvp, euler_jvp_vjp), then the roll-out check.

``tests/test_gpu_regulariser_ops.py`` plays them through the engine on the device,
``tests/test_host_regulariser_model.py`` replays them on the CPU with the float32 model standing where the device stands.
Either is compared with the fp64 model (tests/regulariser_model.py) on the same float32 inputs, the deviation taken as a
fraction of the model's yardsticks: entry by entry for reduced outputs, point by point for per-point outputs
(``regulariser_model.deviation_s4``, ``deviation_op``).

Everything is seeded; the deck of a library does not depend on which other libraries are compiled.  The libraries, the sizes
and the point, mask and shift draws are those of tests/symreg_linear_cases.py.

S4: the plain materialised entry only: no ``live_columns``, no compact J table, no ``dx`` -- those have their own tests.
"""
import functools
from collections import namedtuple

import torch

from tests import regulariser_model as M
from tests.helpers import only_compiled
from tests.symreg_linear_cases import ORDERS, STEADY_GRIDS, STEADY_N, _deck, _mask, _z, all_libs, equivariant_xi, round_up_2, sizes  # noqa: F401
from tests.symreg_linear_model import terms

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances, per operator, output field and state dimension (the d = 4 libraries are an optional part of the build).
# Derived, not chosen: tests/test_host_regulariser_model.py replays every case below with the model in float32, every sum
# taken one term after the other, against the model in fp64 from the same float32 inputs, takes per field the worst
# entry-by-entry deviation as a fraction of the yardstick, and asserts that each constant here is 4 x that figure (rounded up
# to two digits; x 4 for the reason tests/adam_cases.py states: the device adds per-thread partial sums, a wave butterfly and
# wave partials where the replay adds sequentially).  The replay figures and the worst the MI355X run showed are in
# profiles/regulariser_cases.txt.
# ---------------------------------------------------------------------------------------------------------------------
TOL = {"symreg_reversed": {1: {"loss": 3.7e-8, "grad": 6.0e-8}, 2: {"loss": 5.5e-8, "grad": 1.2e-7}, 3: {"loss": 2.2e-8, "grad": 1.7e-7},
                           4: {"loss": 2.7e-8, "grad": 7.6e-8}}}

MAJORANT_BOUND = 1e3                                     # on a, the majorant of u at a point (the loss is a mean of its squares)

# shift: (operand, floats) -- the base pointer of ONE operand moved off its 16-byte boundary; batched: the (S, ...) layout
S4Case = namedtuple("S4Case", "name lib x gx jgx xi mask inv_count shift env exact_zero batched")


def libs():
    return only_compiled(all_libs())


def _near_rotation(n_g, d, gen):
    """Dense near-rotations: exp of 0.3 x an antisymmetric plus 0.1 x a dense draw (d = 1: a scale near 1)."""
    a = torch.randn(n_g, d, d, generator=gen)
    return torch.linalg.matrix_exp(0.3 * (a - a.transpose(1, 2)) + 0.1 * torch.randn(n_g, d, d, generator=gen))


def quarter_turn(d):
    """The exact rotation by 90 degrees in the (0, 1) plane (entries 0, +-1: products with it are exact); d = 1: [[1]]."""
    R = torch.eye(d)
    if d > 1:
        R[0, 0], R[1, 1], R[0, 1], R[1, 0] = 0.0, 0.0, 1.0, -1.0
    return R


def _masks(kind, S, d, p, gen):
    """One mask per problem, no two alike; ``none`` is no mask at all and ``zero`` the zero mask for every problem."""
    if kind == "none":
        return None
    kinds = ["zero"] * S if kind == "zero" else [kind, "random", "row_off"][:S]          # every draw is a fresh one
    return torch.stack([_mask(k, d, p, gen) for k in kinds])


@functools.lru_cache(maxsize=None)
def s4_cases(lib):
    d, order, flags = lib
    p = terms(d, order, flags)
    gen = torch.Generator().manual_seed(47000 + 1000 * d + 10 * order + flags)
    near = 1031                                          # ragged for every chunk width above 1; slabs off the 16-byte grid
    even = 1028                                          # every slab (problem, group element) starts on a 16-byte boundary
    tag = f"d{d}o{order}f{flags}"
    out = []

    def add(name, n, n_g, S, mask, shift=(None, 0), env=None, inv_count=None, xi=None, action=None, exact_zero=False):
        x = torch.stack([_z(n, d, gen) for _ in range(S)])
        if action == "identity":                         # J_g = I and g x = x bit for bit: u = 0 in exact arithmetic
            gx, jgx = x[:, None].repeat(1, n_g, 1, 1), torch.eye(d).expand(S, n_g, n, d, d).contiguous()
        elif action == "quarter_turn":
            R = quarter_turn(d)
            gx, jgx = (x @ R.T)[:, None].repeat(1, n_g, 1, 1), R.expand(S, n_g, n, d, d).contiguous()
        else:                                            # g x a near-rotation of x, J_g a dense near-rotation at every point
            R = _near_rotation(S * n_g, d, gen).reshape(S, n_g, d, d)
            gx = torch.einsum("sgij,snj->sgni", R, x) + 0.05 * torch.randn(S, n_g, n, d, generator=gen)
            jgx = R[:, :, None] + 0.05 * torch.randn(S, n_g, n, d, d, generator=gen)
        xi = 0.4 * torch.randn(S, d, p, generator=gen) if xi is None else xi[None].repeat(S, 1, 1)
        mk = _masks(mask, S, d, p, gen)
        inv = None if inv_count is None else inv_count / (n * d)
        c = S4Case(f"{tag}-{name}-n{n}-g{n_g}-S{S}-{mask}-{shift[0] or 'x'}{shift[1]}", lib, x.contiguous(), gx.contiguous(), jgx.contiguous(),
                   xi.contiguous(), mk, inv, shift, env or {}, exact_zero or n_g == 0, S > 1)
        ref = evaluate(c)
        assert float(ref["majorant"]) < MAJORANT_BOUND, c.name
        _REFERENCE[c.name] = ref
        out.append(c)

    ns = sizes(d)
    gens, probs, masks = _deck([0, 1, 2, 3], len(ns), gen), _deck([1, 1, 3], len(ns), gen), _deck(["none", "random", "row_off"], len(ns), gen)
    for k, n in enumerate(ns):
        add("size", n, gens[k], probs[k], masks[k])
    for n_g, mask in zip((0, 1, 2, 3), ("random", "row_off", "none", "random")):
        for S in (1, 3):
            add("gen", near, n_g, S, mask)
    add("vec", even, 2, 3, "random")
    for operand, floats in (("x", 1), ("gx", 2), ("jgx", 3)):        # one operand off the boundary at a time, all else vector-ready
        add("shift", even, 2, 1, "none", shift=(operand, floats))
    add("shift", even, 1, 3, "random", shift=("gx", 1))
    add("maskzero", near, 2, 1, "zero", exact_zero=True)
    add("sharded", near, 2, 3, "random", inv_count=0.5)                      # a rank holding half the points: 1 / (2 n d)
    add("identity", near, 1, 1, "random", action="identity")
    add("equivariant", near, 1, 1, "none", action="quarter_turn", xi=equivariant_xi(d, p, gen))
    for k, grid in enumerate(STEADY_GRIDS):              # SYMODE_SMALL_GRID is the cap this launch reads for one problem
        add(f"steady{grid}", STEADY_N[d], 1 + k, 1, ("random", "none")[k], env={"SYMODE_REDUCE_GRID": grid, "SYMODE_SMALL_GRID": grid})
    return tuple(out)


def operands(c):
    """The operands of a case in the form the entry takes: without the problem axis for one problem."""
    if c.batched:
        return c.x, c.gx, c.jgx, c.xi, c.mask
    return c.x[0], c.gx[0], c.jgx[0], c.xi[0], None if c.mask is None else c.mask[0]


def evaluate(c, **kw):
    """The S4 model of a case."""
    x, gx, jgx, xi, mask = operands(c)
    return M.evaluate_s4(x, gx, jgx, xi, mask, c.lib[1], c.lib[2], inv_count=c.inv_count, **kw)


_REFERENCE = {}


def s4_deck(which=None):
    return [c for lib in (libs() if which is None else which) for c in s4_cases(tuple(lib))]


def reference(name):
    """The fp64 model of a case: computed once, when the case was built, and shared."""
    if name not in _REFERENCE:
        for lib in all_libs():
            if name.startswith("d%do%df%d-" % tuple(lib)):
                s4_cases(tuple(lib))
    return _REFERENCE[name]


def applies(mutant, c):
    S, n, d = c.x.shape
    return M.s4_mutant_applies(mutant, d, c.gx.shape[1], S, n, c.mask is not None, c.inv_count is None)


# ---------------------------------------------------------------------------------------------------------------------
# S2 / S3: forward_jvp, vjp, jvp_vjp on the "step" cases, euler_jvp and euler_jvp_vjp on the "euler" cases
# ---------------------------------------------------------------------------------------------------------------------
# Tolerances per operator, output field and state dimension, derived like TOL above (jvp_vjp: over the plays with and
# without g_out).
OPS_TOL = {
    "forward_jvp": {1: {"out": 8.5e-07, "jv": 8.4e-07},
                   2: {"out": 2.3e-06, "jv": 1.9e-06},
                   3: {"out": 2.7e-06, "jv": 1.5e-06},
                   4: {"out": 1.8e-06, "jv": 1.3e-06}},
    "vjp": {1: {"grad_x": 9.5e-07, "grad_xi": 2.4e-07},
           2: {"grad_x": 1.3e-06, "grad_xi": 5.3e-07},
           3: {"grad_x": 1.6e-06, "grad_xi": 5.0e-07},
           4: {"grad_x": 8.8e-07, "grad_xi": 5.1e-07}},
    "jvp_vjp": {1: {"grad_x": 9.4e-07, "grad_v": 8.2e-07, "grad_xi": 6.1e-07},
               2: {"grad_x": 1.2e-06, "grad_v": 1.5e-06, "grad_xi": 4.8e-07},
               3: {"grad_x": 1.5e-06, "grad_v": 1.4e-06, "grad_xi": 5.8e-07},
               4: {"grad_x": 8.3e-07, "grad_v": 1.1e-06, "grad_xi": 5.7e-07}},
    "euler_jvp": {1: {"x_out": 4.5e-06, "t_out": 5.5e-06},
                 2: {"x_out": 2.9e-06, "t_out": 3.5e-06},
                 3: {"x_out": 1.9e-06, "t_out": 1.7e-06},
                 4: {"x_out": 1.1e-06, "t_out": 1.2e-06}},
    "euler_jvp_vjp": {1: {"grad_x": 6.5e-06, "grad_v": 6.0e-06, "grad_xi": 7.9e-07},
                     2: {"grad_x": 3.2e-06, "grad_v": 2.8e-06, "grad_xi": 7.0e-07},
                     3: {"grad_x": 1.7e-06, "grad_v": 1.8e-06, "grad_xi": 4.7e-07},
                     4: {"grad_x": 1.2e-06, "grad_v": 1.2e-06, "grad_xi": 4.8e-07}},
}

# The reverse sweep of the flow keeps its states in an LDS column while n_steps * 2 d * 256 floats fit 64 KiB, and needs
# n_steps > 1 for it: the last K that takes the column (the next one recomputes the states, as K = 1 does)
STACK_LAST = {1: 32, 2: 16, 3: 10, 4: 8}
FLOW_TIME = 0.35                                         # K dt <= this

# kind: "step" or "euler"; ga, gb: the cotangents (g of vjp / g_out / g_x, and g_jv / g_t); shift: (operand, floats)
OpsCase = namedtuple("OpsCase", "name lib kind x v ga gb xi mask K dt shift env exact_zero")
PLAYS = {"step": (("forward_jvp", "forward_jvp"), ("vjp", "vjp"), ("jvp_vjp", "jvp_vjp"), ("jvp_vjp_null", "jvp_vjp")),
         "euler": (("euler_jvp", "euler_jvp"), ("euler_jvp_vjp", "euler_jvp_vjp"))}


def evaluate_play(c, play, **kw):
    """The model of one play of a case (``jvp_vjp_null``: jvp_vjp with g_out = None)."""
    op = dict(PLAYS[c.kind])[play]
    return M.evaluate_op(op, c.x, c.v, None if play == "jvp_vjp_null" else c.ga, c.gb, c.xi, c.mask, c.lib[1], c.lib[2], K=c.K, dt=c.dt, **kw)


def _float32_step(total, K):
    """The largest float32 dt with K dt <= total, as a Python float."""
    dt = torch.tensor(total / K, dtype=torch.float32)
    if float(dt) * K > total:
        dt = torch.nextafter(dt, torch.zeros(()))
    return float(dt)


@functools.lru_cache(maxsize=None)
def ops_cases(lib):
    d, order, flags = lib
    p = terms(d, order, flags)
    gen = torch.Generator().manual_seed(53000 + 1000 * d + 10 * order + flags)
    near, even = 1031, 1028
    tag = f"d{d}o{order}f{flags}"
    out = []

    def add(kind, name, n, mask, K=0, shift=(None, 0), env=None, exact_zero=False):
        x, v, ga, gb = (_z(n, d, gen) for _ in range(4))                       # tangents and cotangents like the points
        xi = (0.4 if kind == "step" else 0.2) * torch.randn(d, p, generator=gen)
        mk = _mask(mask, d, p, gen)
        total = FLOW_TIME
        while True:                                      # a flow whose majorant leaves the bound gets a shorter time
            dt = _float32_step(total, K) if K else 0.125
            c = OpsCase(f"{tag}-{kind}-{name}-n{n}-K{K}-{mask}-{shift[0] or 'x'}{shift[1]}", lib, kind, x, v, ga, gb, xi, mk, K, dt, shift,
                        env or {}, exact_zero)
            refs = {play: evaluate_play(c, play) for play, _ in PLAYS[kind]}
            if all(r["majorant"] < MAJORANT_BOUND for r in refs.values()):
                break
            assert kind == "euler" and total > 0.01, c.name
            total /= 2
        for play, r in refs.items():
            _OPS_REFERENCE[c.name, play] = r
        out.append(c)

    ns = sizes(d)
    masks = _deck(["none", "random", "row_off"], len(ns), gen)
    for k, n in enumerate(ns):
        add("step", "size", n, masks[k])
    for operand, floats in (("x", 1), ("v", 2), ("ga", 3), ("gb", 1)):       # one operand off its boundary at a time
        add("step", "shift", even, "none", shift=(operand, floats))
    for mask in ("random", "row_off"):
        add("step", "mask", near, mask)
    add("step", "maskzero", near, "zero", exact_zero=True)
    for k, grid in enumerate(STEADY_GRIDS):
        add("step", f"steady{grid}", STEADY_N[d], ("random", "none")[k], env={"SYMODE_REDUCE_GRID": grid, "SYMODE_MAP_GRID": grid})

    last = STACK_LAST[d]
    steps, masks = _deck([1, 2, last, last + 1], len(ns), gen), _deck(["none", "random", "row_off"], len(ns), gen)
    for k, n in enumerate(ns):
        add("euler", "size", n, masks[k], steps[k])
    for K, mask in zip((1, 2, last, last + 1), ("random", "none", "row_off", "random")):
        add("euler", "steps", near, mask, K)
    for K in (2, last):                                  # the sizes the column would take, recomputed instead
        add("euler", "recompute", near, "random", K, env={"SYMODE_EULER_STACK": 0})
    add("euler", "nostep", near, "random", 0)
    for operand, floats in (("x", 1), ("v", 2), ("ga", 3), ("gb", 1)):
        add("euler", "shift", even, "none", 2, shift=(operand, floats))
    add("euler", "maskzero", near, "zero", 2, exact_zero=True)
    for k, grid in enumerate(STEADY_GRIDS):
        add("euler", f"steady{grid}", STEADY_N[d], ("random", "none")[k], 2, env={"SYMODE_REDUCE_GRID": grid, "SYMODE_MAP_GRID": grid})
    return tuple(out)


_OPS_REFERENCE = {}


def ops_deck(which=None):
    return [c for lib in (libs() if which is None else which) for c in ops_cases(tuple(lib))]


def ops_reference(name, play):
    """The fp64 model of a play of a case: computed once, when the case was built, and shared."""
    if (name, play) not in _OPS_REFERENCE:
        for lib in all_libs():
            if name.startswith("d%do%df%d-" % tuple(lib)):
                ops_cases(tuple(lib))
    return _OPS_REFERENCE[name, play]


def ops_applies(mutant, c, play):
    op = dict(PLAYS[c.kind])[play]
    return M.ops_mutant_applies(mutant, op, c.lib[0], c.lib[1], c.lib[2], c.x.shape[0], c.K, c.mask is not None, play != "jvp_vjp_null")


# ---------------------------------------------------------------------------------------------------------------------
# The roll-out check: 5 trajectories x 3 models, 12 steps, one library per state dimension, RK4 and Euler
# ---------------------------------------------------------------------------------------------------------------------
ROLLOUT_LIBS = {1: (1, 3, 0), 2: (2, 3, 0), 3: (3, 2, 1), 4: (4, 2, 0)}
ROLLOUT_STEPS, ROLLOUT_ICS, ROLLOUT_MODELS, ROLLOUT_DT = 12, 5, 3, 0.015625
# derived like TOL above: 4 x the float32 replay of ``regulariser_model.rollout_error`` against its fp64 run, per d and method
ROLLOUT_TOL = {1: {"rk4": 5.3e-9, "euler": 6.2e-9}, 2: {"rk4": 8.0e-9, "euler": 9.9e-9}, 3: {"rk4": 4.6e-9, "euler": 1.1e-8}, 4: {"rk4": 1.8e-8, "euler": 8.3e-9}}

RolloutCase = namedtuple("RolloutCase", "lib x_true xi mask dt")


def rollout_libs():
    return only_compiled(list(ROLLOUT_LIBS.values()))


@functools.lru_cache(maxsize=None)
def rollout_case(lib):
    """Truth: an fp64 RK4 orbit of a drawn system, rounded to float32 and perturbed; the models: that system's coefficients
    perturbed, one of them under a mask."""
    d, order, flags = lib
    p = terms(d, order, flags)
    gen = torch.Generator().manual_seed(59000 + 1000 * d + 10 * order + flags)
    truth = 0.2 * torch.randn(1, d, p, generator=gen)
    x = [_z(ROLLOUT_ICS, d, gen).double()]
    from oracle import sindy_oracle as O
    f = lambda a: O.forward(a, truth[0].double(), torch.ones(d, p, dtype=torch.float64), order, bool(flags & 1), bool(flags & 2))  # noqa: E731
    x += list(O.odeint(f, x[0], (ROLLOUT_STEPS + 0.5) * ROLLOUT_DT, ROLLOUT_DT, "rk4", full_traj=True))
    x_true = (torch.stack(x, dim=1) + 0.01 * torch.randn(ROLLOUT_ICS, ROLLOUT_STEPS + 1, d, generator=gen).double()).float().contiguous()
    xi = (truth + 0.05 * torch.randn(ROLLOUT_MODELS, d, p, generator=gen)).contiguous()
    mask = torch.stack([torch.ones(d, p), _mask("random", d, p, gen), torch.ones(d, p)])
    return RolloutCase(lib, x_true, xi, mask, ROLLOUT_DT)


@functools.lru_cache(maxsize=None)
def rollout_reference(lib, method):
    c = rollout_case(lib)
    err, yard = M.rollout_error(c.x_true, c.xi, c.mask, lib[1], lib[2], c.dt, method)
    assert float(yard.max()) < MAJORANT_BOUND
    return err, yard
