"""The witness of tests/adam_latent_model.py (the fp64 model the GPU step tests compare symode_adam_epochs_latent with), on
the CPU: the model chained against torch.optim.Adam driven by autograd on the loss of include/symode.h (mse_x detached, as
compute_dx leaves it), every GPU case of tests/test_gpu_adam_latent_steps.py replayed with the float32 model where the
device will stand -- which shows that the committed inputs are decidable and yields the tolerances of
tests/adam_latent_cases.py -- and each of eight deliberate mistakes played in the device's place, which the cases must
notice."""
import pytest
import torch

from oracle import sindy_oracle as O
from tests import adam_latent_cases as C
from tests import adam_latent_model as M
from tests.test_host_adam_model import _round_up, _scaled

ANCHORS = [((2, 2, 2), "xi", "weighted", 3, 2, "half", 9), ((2, 5, 0), "xi", "default", 1, 0, "row_off", 0),
           ((3, 3, 1), "q5c", "w_z4", 3, 2, "half", 999), ((1, 3, 0), "xi", "beta1_0", 3, 0, "ones", 0),
           ((3, 3, 0), "qm", "weighted", 1, 2, "half", 1), ((2, 5, 0), "xi", "no_l1", 0, 2, "half", 100000)]


@pytest.mark.parametrize("lib, form, hyper, n_gen, d_extra, mask_kind, t0", ANCHORS)
def test_chained_model_equals_torch_adam_by_autograd(lib, form, hyper, n_gen, d_extra, mask_kind, t0):
    d, order, flags = lib
    p, dp = C.lib_dims(lib)
    cfg = C._cfg(lib, hyper, form, n_gen, d_extra)
    n = dp if cfg["q"] is None else cfg["q"].shape[1] + d
    gen = torch.Generator().manual_seed(5 + dp + t0)
    st32 = C._state(1, n, d, p, [t0], [mask_kind], cfg["l1"], gen)
    st = {k: st32[k][0].double() for k in ("params", "m", "v", "mask")}
    st["step"] = t0
    data = C.data_of(cfg)
    mask = st["mask"].view(d, p)
    leaf = st["params"].clone().requires_grad_(True)
    theta = lambda y: O.theta(y, order, bool(flags & 1), bool(flags & 2))  # noqa: E731

    def h(y):                                                 # the regressor: Theta(y) (Xi * mask)^T
        if cfg["q"] is None:
            xi = leaf.view(d, p)
        else:
            r = cfg["q"].shape[1]
            xi = (cfg["q"].double() @ leaf[:r]).view(d, p)
            if cfg["allow_const"]:
                xi = xi + torch.cat([leaf[r:].view(d, 1), torch.zeros(d, p - 1, dtype=torch.float64)], dim=1)
        return theta(y) @ (xi * mask).T

    opt = torch.optim.Adam([leaf], lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    if t0 > 0:
        opt.state[leaf] = dict(step=torch.tensor(float(t0)), exp_avg=st["m"].clone(), exp_avg_sq=st["v"].clone())
    for k in range(4):
        rows = C._rows(65, "scattered", gen)
        valid = M.valid_rows(rows, C.N_SRC)
        z, dz, B, y = (data[key].double()[valid] for key in ("z", "dz", "B", "y"))
        hz = h(z)
        mse_z = torch.nn.functional.mse_loss(hz, dz)
        # decoder Jacobian A = Q B with orthonormal Q: |A h - dx|^2 = |B h - y|^2 + e; the term is cut from the graph
        x_sq = (torch.einsum("bij,bj->bi", B, hz.detach()) - y).square().sum()
        if data["e"] is not None:
            x_sq = x_sq + data["e"].double()[valid].sum()
        mse_x = x_sq / (len(valid) * cfg["D_obs"])
        sym = torch.zeros((), dtype=torch.float64)
        if data["L"] is not None:
            sym = O.symreg_linear_latent(z, list(data["L"].double()), h)
        l1 = leaf.abs().sum()
        loss = cfg["w_z"] * mse_z + cfg["w_x"] * mse_x + cfg["w_sym"] * sym + (cfg["w_reg"] * l1 if cfg["l1"] else 0.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        st, rec = M.step(st, rows, data, cfg)
        errs = dict(params=_scaled(st["params"], leaf.detach()), m=_scaled(st["m"], opt.state[leaf]["exp_avg"]),
                    v=_scaled(st["v"], opt.state[leaf]["exp_avg_sq"]), mse_z=_scaled(rec["mse_z"], mse_z.detach()),
                    mse_x=_scaled(rec["mse_x"], mse_x.detach()), l1=_scaled(rec["l1"], l1.detach()), sym=_scaled(rec["sym"], sym.detach()))
        assert max(errs.values()) <= 1e-11, (k, errs)
        assert st["step"] == t0 + k + 1 == int(opt.state[leaf]["step"])


# ---------------------------------------------------------------------------------------------------------------------
# the replay: float32 model with sequential sums as the device, fp64 model as the reference, over every GPU case
# ---------------------------------------------------------------------------------------------------------------------
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
    assert replay.mismatch == [] and replay.unsettled == []
    assert all(sum(c.expect["near"]) > 0 for c in C.epoch_cases() if c.expect["event"])


def test_the_grid_covers_what_it_claims():
    cases = C.grid_cases()
    seen = lambda f: {f(c) for c in cases}  # noqa: E731
    assert seen(lambda c: c.tables.shape[3]) == set(C.BATCHES)
    assert seen(lambda c: c.cfg["n_gen"]) == set(C.N_GENS) and seen(lambda c: c.cfg["D_obs"] - c.cfg["d"]) == set(C.D_EXTRA)
    assert seen(lambda c: (c.cfg["w_z"], c.cfg["w_x"])) >= {(M.f32(0.37), M.f32(0.6)), (1.0, 1.0), (4.0, 0.0)}
    assert seen(lambda c: (c.cfg["q"] is None, c.cfg["allow_const"])) == {(True, True), (False, True), (False, False)}
    assert seen(lambda c: c.cfg["beta1"]) >= {0.0} and seen(lambda c: c.cfg["l1"]) == {True, False}
    assert {int(t) for c in cases for t in c.state["step"]} == set(C.STARTS)
    assert C.libs_of(cases) == sorted(C.LIBS)
    for lib in C.LIBS:                                       # every library meets every value of the padding, form, n_gen and D axes
        mine = [c for c in cases if (c.cfg["d"], c.cfg["order"], c.cfg["flags"]) == lib]
        assert {c.name.split("-")[3] for c in mine} == set(C.PADS) and {c.name.split("-")[4] for c in mine} == set(C.FORMS)
        assert {(c.cfg["n_gen"] > 0, c.cfg["D_obs"] > c.cfg["d"]) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}
        assert any(c.tables.shape[1] == 3 for c in mine) and any(c.tables.shape[2] == 2 for c in mine)


def test_tolerances_are_four_times_the_replay_deviation(replay):
    for k in sorted(C.TOL):
        worst, where = replay.worst.get(k, (0.0, None))
        print(f"adam latent steps, {k}: float32 against fp64 {worst:.3e} at {where}; x 4 -> {_round_up(4 * worst):.1e} (committed {C.TOL[k]:.1e})")
    assert set(replay.worst) == set(C.TOL)
    for k, (worst, where) in replay.worst.items():
        # the committed figure is 4 x the replay deviation on the machine that derived it; another CPU's own arithmetic
        # (vector width of cumsum, fused multiply-add) moves the replay figure by a few per cent: 3 x .. 5 x
        assert 3.0 * worst <= C.TOL[k] <= 5.0 * worst, (k, worst, C.TOL[k])


# ---------------------------------------------------------------------------------------------------------------------
# teeth: every mutant of the model, played in the device's place, is noticed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_a_mutant_in_the_devices_place_is_caught(mutant):
    """At least one case shows a deviation of 10 x the field's tolerance or more."""
    dev = C.ModelDevice(torch.float64, False, mutant)
    caught = None
    for case in C.grid_cases():
        rep = C.Report()
        C.check_launch(rep, case, dev)
        over = {k: v[0] / C.TOL[k] for k, v in rep.worst.items() if C.TOL[k] > 0 and v[0] >= 10.0 * C.TOL[k]}
        if over:
            caught = (case.name, over)
            break
    print(f"mutant {mutant}: caught by {caught}")
    assert caught is not None, f"no case notices the mutant {mutant}"
