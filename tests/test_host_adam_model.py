"""The witness of tests/adam_model.py (the fp64 model the GPU step tests compare the device Adam trainer with), on the CPU:
the model chained against torch.optim.Adam driven by autograd, every GPU case of tests/test_gpu_adam_steps.py replayed with
the float32 model where the device will stand -- which shows that the committed inputs are decidable and yields the
tolerances of tests/adam_cases.py -- and each of sixteen deliberate mistakes played in the device's place, which the cases
must notice."""
import math

import pytest
import torch

from oracle import sindy_oracle as O
from tests import adam_cases as C
from tests import adam_model as M


# ---------------------------------------------------------------------------------------------------------------------
# the anchor: five chained steps of the model equal torch.optim.Adam on the loss of include/symode.h, by autograd
# ---------------------------------------------------------------------------------------------------------------------
def _scaled(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


ANCHORS = [((2, 2, 2), "xi", "weighted", "rev3", "half", 9), ((2, 5, 0), "xi", "default", "plain", "row_off", 0),
           ((3, 3, 1), "q5c", "w_x4", "rev3", "half", 999), ((2, 5, 0), "q1c", "weighted", "rev1", "ones", 0),
           ((3, 3, 0), "qm", "weighted", "rev3", "half", 1), ((2, 2, 2), "q5", "w_x4", "plain", "row_off", 9),
           ((1, 3, 0), "xi", "beta1_0", "rev3", "ones", 0), ((2, 5, 0), "xi", "no_l1", "rev0", "half", 100000)]


@pytest.mark.parametrize("lib, form, hyper, entry, mask_kind, t0", ANCHORS)
def test_chained_model_equals_torch_adam_by_autograd(lib, form, hyper, entry, mask_kind, t0):
    d, order, flags = lib
    p, dp = C.lib_dims(lib)
    cfg = C._cfg(lib, hyper, entry, form)
    n = dp if cfg["q"] is None else cfg["q"].shape[1] + d
    gen = torch.Generator().manual_seed(3 + dp + t0)
    st32 = C._state(1, n, d, p, [t0], [mask_kind], cfg["l1"], gen)
    st = {k: st32[k][0].double() for k in ("params", "m", "v", "mask")}
    st["step"] = t0
    data = C.data_of(cfg)
    x, dx = data["x"].double(), data["dx"].double()
    gxs = [] if data["gx"] is None else [g.double() for g in data["gx"]]
    jgs = [] if data["jgx"] is None else [j.double() for j in data["jgx"]]
    mask = st["mask"].view(d, p)
    # torch's side: fp64 leaves; the oracle regressor where it can express the form (Xi, or Q beta + const), else plain torch
    oracle_form = cfg["q"] is None or cfg["allow_const"]
    reg = O.OracleRegressor(d, order, bool(flags & 1), bool(flags & 2), Xi0=torch.zeros(d, p))
    reg.mask = mask.clone()
    if cfg["q"] is None:
        reg.Xi = st["params"].view(d, p).clone().requires_grad_(True)
        leaves = [reg.Xi]
    else:
        r = cfg["q"].shape[1]
        beta = st["params"][:r].clone().requires_grad_(True)
        const = st["params"][r:].reshape(d, 1).clone().requires_grad_(True)
        leaves = [beta, const]
        if oracle_form:
            reg.constraint, reg.Q, reg.use_kron_product, reg.allow_constant, reg.Xi = True, cfg["q"].double(), True, True, None
            reg.beta, reg.const = beta, const
    if oracle_form:
        h = reg
    else:                                                    # a dense Q_eff whose constants are not read
        h = lambda y: O.theta(y, order, bool(flags & 1), bool(flags & 2)) @ ((cfg["q"].double() @ beta).view(d, p) * mask).T  # noqa: E731
    opt = torch.optim.Adam(leaves, lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    if t0 > 0:
        at = 0
        for q in leaves:
            k = q.numel()
            opt.state[q] = dict(step=torch.tensor(float(t0)), exp_avg=st["m"][at:at + k].reshape(q.shape).clone(),
                                exp_avg_sq=st["v"][at:at + k].reshape(q.shape).clone())
            at += k
    for k in range(5):
        rows = C._rows(65, "scattered", gen)
        valid = M.valid_rows(rows, C.N_SRC)
        mse = torch.nn.functional.mse_loss(h(x[valid]), dx[valid])
        sym = O.symreg_reversed_precomputed(x[valid], [g[valid] for g in gxs], [j[valid] for j in jgs], h) if gxs else torch.zeros((), dtype=torch.float64)
        l1 = sum(q.abs().sum() for q in leaves)
        loss = cfg["w_x"] * mse + cfg["w_sym"] * sym + (cfg["w_reg"] * l1 if cfg["l1"] else 0.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        st, rec = M.step(st, rows, data, cfg)
        flat = lambda key: torch.cat([opt.state[q][key].reshape(-1) for q in leaves])  # noqa: E731
        errs = dict(params=_scaled(st["params"], torch.cat([q.detach().reshape(-1) for q in leaves])), m=_scaled(st["m"], flat("exp_avg")),
                    v=_scaled(st["v"], flat("exp_avg_sq")), mse=_scaled(rec["mse"], mse.detach()), l1=_scaled(rec["l1"], l1.detach()),
                    sym=_scaled(rec["sym"], sym.detach()))
        assert max(errs.values()) <= 1e-12, (k, errs)
        assert st["step"] == t0 + k + 1 == int(opt.state[leaves[0]]["step"])


# ---------------------------------------------------------------------------------------------------------------------
# the replay: float32 model with sequential sums as the device, fp64 model as the reference, over every GPU case
# ---------------------------------------------------------------------------------------------------------------------
def _round_up(v):
    """v to two significant digits, upwards."""
    if v == 0.0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


@pytest.fixture(scope="module")
def replay():
    rep, dev = C.Report(), C.ModelDevice()
    for case in C.grid_cases():
        C.check_launch(rep, case, dev)
    for case in C.freeze_cases():
        C.check_freeze(rep, case, dev)
    for case in C.epoch_cases():
        C.check_epoch(rep, case, dev)
    for case in C.structure_cases():
        C.check_structure(case, dev)
    return rep


def test_replay_every_gpu_case_is_decided_by_the_reference_alone(replay):
    """Float32 and fp64 agree on every discrete outcome and no margin of a thresholding event is closer than the tolerance
    of xi; the near counts of the epoch cases (asserted against the construction inside check_epoch) are not zero."""
    assert replay.mismatch == [] and replay.unsettled == []
    assert 150 <= len(C.grid_cases()) + len(C.freeze_cases()) + len(C.epoch_cases()) <= 300
    assert all(sum(c.expect["near"]) > 0 for c in C.epoch_cases() if c.expect["event"])


def test_the_grid_covers_what_it_claims():
    cases = C.grid_cases()
    seen = lambda f: {f(c) for c in cases}  # noqa: E731
    assert seen(lambda c: c.tables.shape[3]) == set(C.BATCHES)
    assert seen(lambda c: (c.cfg["entry"], c.cfg["n_g"], c.cfg["w_x"])) >= {("reversed", g, M.f32(w)) for g in (1, 3) for w in (0.37, 1.0, 4.0)} | {("reversed", 0, 1.0)}
    assert seen(lambda c: (c.cfg["q"] is None, c.cfg["allow_const"])) == {(True, True), (False, True), (False, False)}
    assert seen(lambda c: c.cfg["beta1"]) >= {0.0} and seen(lambda c: c.cfg["l1"]) == {True, False}
    assert {int(t) for c in cases for t in c.state["step"]} == set(C.STARTS)
    assert C.libs_of(cases) == sorted(C.LIBS)
    for lib in C.LIBS:                                       # every library meets every value of the padding, mask and form axes
        mine = [c for c in cases if (c.cfg["d"], c.cfg["order"], c.cfg["flags"]) == lib]
        assert {c.name.split("-")[3] for c in mine} == set(C.PADS) and {c.name.split("-")[4] for c in mine} == set(C.FORMS)
        assert any((c.state["mask"] == 0).all() for c in mine) and any(c.tables.shape[1] == 3 for c in mine)


def test_tolerances_are_four_times_the_replay_deviation(replay):
    for k in sorted(C.TOL):
        worst, where = replay.worst.get(k, (0.0, None))
        print(f"adam steps, {k}: float32 against fp64 {worst:.3e} at {where}; x 4 -> {_round_up(4 * worst):.1e} (committed {C.TOL[k]:.1e})")
    assert set(replay.worst) == set(C.TOL)
    for k, (worst, where) in replay.worst.items():
        # the committed figure is 4 x the replay deviation on the machine that derived it; another CPU's own arithmetic
        # (vector width of cumsum, fused multiply-add) moves the replay figure by a few per cent: 3 x .. 5 x
        assert 3.0 * worst <= C.TOL[k] <= 5.0 * worst, (k, worst, C.TOL[k])


# ---------------------------------------------------------------------------------------------------------------------
# teeth: every mutant of the model, played in the device's place, is noticed
# ---------------------------------------------------------------------------------------------------------------------
DISCRETE = {"threshold_not_strict": "mask", "near_ignores_mask": "log column 3 (near)"}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_a_mutant_in_the_devices_place_is_caught(mutant):
    """At least one case shows a deviation of 10 x the field's tolerance or more (the two mutants of the thresholding
    event change no float: they must show as a wrong mask / a wrong near count)."""
    dev = C.ModelDevice(torch.float64, False, mutant)
    caught = None
    for case in C.epoch_cases() + C.grid_cases():
        rep = C.Report()
        C.check_launch(rep, case, dev)
        if mutant in DISCRETE:
            hits = [m for m in rep.mismatch if m[2] == DISCRETE[mutant]]
            if hits:
                caught = (case.name, hits[0][2:])
        else:
            over = {k: v[0] / C.TOL[k] for k, v in rep.worst.items() if C.TOL[k] > 0 and v[0] >= 10.0 * C.TOL[k]}
            if over:
                caught = (case.name, over)
        if caught:
            break
    print(f"mutant {mutant}: caught by {caught}")
    assert caught is not None, f"no case notices the mutant {mutant}"
