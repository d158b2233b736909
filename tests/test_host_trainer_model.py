"""The witness of tests/trainer_model.py (the fp64 model the GPU step tests compare the trainer's launches with), on the CPU:
the model chained against torch.optim.LBFGS and against oracle.lbfgs_fit, and every GPU case of
tests/test_gpu_trainer_steps.py replayed with the model in float32 where the device will stand -- which shows that the
committed inputs are decidable (same discrete outcomes, no unsettled margin) and yields the tolerances of
tests/trainer_cases.py."""
import math

import pytest
import torch

from oracle import sindy_oracle as O
from tests import trainer_cases as C
from tests import trainer_model as M


def _fresh(params, mask, cfg):
    dt = params.dtype
    z = lambda: torch.zeros((), dtype=dt)  # noqa: E731
    return dict(params=params.clone(), xi=M.xi_of(params, cfg), mask=mask.clone(), g=torch.zeros_like(params), d=torch.zeros_like(params),
                prev_g=torch.zeros_like(params), prev=params.clone(), pprev=params.clone(), loss=z(), t=z(), h_diag=z() + 1.0,
                prev_loss=z(), l1_last=z(), act=0, n_iter=0, head=0, done=0, n_iters=0, nan=0, finished=0, epochs=0, near=0, pairs=[])


@pytest.mark.parametrize("kind, l1, pair", [("none", False, False), ("q5c", False, False), ("q5", False, False), ("q5c", True, True)])
def test_chained_model_equals_torch_lbfgs_on_convex_quadratics(kind, l1, pair):
    """Three epochs of max_iter = 4 over a memory of 3 pairs (it wraps), everything in fp64: the model's launches chained
    (BEGIN, ACCEPT x 3 per epoch, the closure evaluated at the model's Xi) against torch.optim.LBFGS stepped three times."""
    d, p, S = 2, 10, 1
    dp = d * p
    Q = None if kind == "none" else C.householder_q(dp, 5).double()
    n = dp if Q is None else 5 + d
    cfg = M.make_cfg(lr=0.5, history=3, w_x=2.0 if l1 else 1.0, w_reg=1e-3 if l1 else 0.0, l1=l1, pair=pair, w_pair=0.37 if pair else 0.0,
                     map=None if Q is None else (Q, 5, p, kind != "q5"), d=d)
    quad = C.Quadratic(S, dp, 3, pair, cfg["w_pair"])
    P0 = 0.5 * torch.randn(n, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    mask = torch.ones(dp, dtype=torch.float64)
    st = _fresh(P0, mask, cfg)
    # torch's side: the same objective by autograd on the same parameters
    w = P0.clone().requires_grad_(True)
    opt = torch.optim.LBFGS([w], lr=cfg["lr"], max_iter=4, history_size=3)

    def closure():
        opt.zero_grad()
        xi = w if Q is None else Q @ w[:5] + (torch.zeros(d, p, dtype=torch.float64).index_put((torch.arange(d), torch.zeros(d, dtype=torch.long)), w[5:]).reshape(-1)
                                              if kind != "q5" else 0.0)
        z = xi * mask
        f0, _ = quad.half(0, z[None])
        f1, _ = quad.half(1, z[None])
        data = f0[0] + cfg["w_pair"] * f1[0] if pair else f0[0]
        loss = cfg["w_x"] * data + cfg["w_reg"] * w.abs().sum()
        loss.backward()
        return loss

    for epoch in range(3):
        for it in range(4):
            l2, gr = quad(st["xi"][None], mask[None])
            st, _ = M.update(st, l2[0], gr[0], cfg, M.BEGIN if it == 0 else M.ACCEPT)
        opt.step(closure)
        err = float((st["params"] - w.detach()).abs().max() / w.detach().abs().max())
        assert err <= 1e-12, (epoch, err)
        assert st["n_iter"] == opt.state[w]["n_iter"] == 4 * (epoch + 1) and len(st["pairs"]) == 3


def _oracle_problem(n_points=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = 0.8 * torch.randn(n_points, 2, generator=g, dtype=torch.float64)
    truth = torch.tensor(O.SINDY_TRUTH["dosc"])[:, :6]
    dx = O.theta(x, 2) @ truth.T + 0.02 * torch.randn(n_points, 2, generator=g, dtype=torch.float64)
    Xi0 = 0.3 * torch.randn(2, 6, generator=g, dtype=torch.float64)
    return x, dx, Xi0


def test_chained_epoch_logic_equals_the_oracle_fit():
    """oracle.lbfgs_fit in fp64 (damped oscillator, 64 points, order 2) against the model chained over the same epochs with
    the closure from oracle.mse_loss_and_grad: the same events at the same epochs -- 'conv', 'freq' and 'final' all occur
    -- and the same mask after every epoch."""
    x, dx, Xi0 = _oracle_problem()
    lr, st_freq, tol, thr, epochs = 0.1, 3, 2e-2, 0.05, 40
    reg = O.OracleRegressor(2, 2, threshold=thr, Xi0=Xi0)
    reg.Xi = Xi0.clone().requires_grad_(True)
    reg.mask = reg.mask.double()
    hist = O.lbfgs_fit(reg, x, dx, epochs, lr, sindy_reg_type="none", st_freq=st_freq, threshold=thr, tol=tol)
    cfg = M.make_cfg(lr=lr, l1=False, threshold=thr, tol_update=tol, st_freq=st_freq, d=2)
    cfg.update(threshold=thr, tol_update=tol, lr=lr)          # fp64 against fp64: the settings unrounded
    st = _fresh(Xi0.reshape(-1), torch.ones(12, dtype=torch.float64), cfg)
    names = {M.EVENT_CONV: "conv", M.EVENT_FREQ: "freq", M.EVENT_FINAL: "final", M.EVENT_NAN: "nan"}
    events, masks, xis = [], [], []
    for epoch in range(epochs):
        for it in range(20):
            loss, grad = O.mse_loss_and_grad(x, dx, st["xi"].view(2, 6), st["mask"].view(2, 6), 2)
            st, _ = M.update(st, torch.stack([loss.detach(), torch.zeros((), dtype=torch.float64)]), grad.reshape(-1), cfg,
                             M.BEGIN if it == 0 else M.ACCEPT)
        st, rec, _ = M.epoch_end(st, torch.zeros(2), cfg, epoch)
        if rec["code"] in names:
            events.append((epoch, names[rec["code"]]))
        if st["done"]:
            break
        masks.append(st["mask"].view(2, 6).clone())
        xis.append(st["xi"].view(2, 6).clone())
    print("oracle events", hist["events"], "\nmodel events ", events)
    assert events == hist["events"]
    assert {"conv", "freq", "final"} <= {e for _, e in events}
    assert len(masks) == len(hist["mask"]) and all(torch.equal(a.bool(), b.bool()) for a, b in zip(masks, hist["mask"]))
    devs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(xis, hist["Xi"])]
    print("model against oracle, Xi per epoch:", ["%.1e" % v for v in devs])
    # (autograd against the closed-form gradient, through 20 iterations an epoch over a memory of nearly parallel pairs: the
    # last bit grows by about six orders per epoch, so only the first epoch is held to round-off; events and masks decide)
    assert devs[0] <= 1e-12
    assert int(hist["mask"][-1].sum()) < 12                  # thresholding did remove coefficients


# ---------------------------------------------------------------------------------------------------------------------
# the replay: float32 model as the device, fp64 model as the reference, over every case of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _round_up(v):
    """v to two significant digits, upwards."""
    if v == 0.0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


@pytest.fixture(scope="module")
def replay():
    rep_u, rep_e, outcomes = C.Report(), C.Report(), {}
    for case in C.update_cases():
        su = C.case_setup(case)
        cfg = su.cfg
        dev = C.ModelDevice(C.S_UPDATE, su.n, su.dp, cfg["history"], cfg, cfg["pair"])
        dev.load(C.start_state(cfg, su.n, su.dp, cfg["history"], su.P0, su.mask0))
        C.drive_update_case(case, dev, rep_u, su)
    for crafted in C.crafted_cases():
        cfg, hs = crafted.cfg, crafted.hs
        S, n = hs["params"].shape
        dev = C.ModelDevice(S, n, hs["mask"].shape[1], cfg["history"], cfg, crafted.pair)
        outcomes[crafted.name] = (C.drive_crafted(crafted, dev, rep_u), crafted.expect)
    for case in C.epoch_cases():
        cfg, Q, n, dp, hs, cl = C.epoch_setup(case)
        dev = C.ModelDevice(C.S_EPOCH, n, dp, cfg["history"], cfg, case[4])
        C.drive_epoch_case(case, dev, rep_e)
    return rep_u, rep_e, outcomes


def test_replay_every_gpu_case_is_decidable(replay):
    """Float32 and fp64 take every branch alike, no margin is closer than the float tolerance, and no randomised update
    launch is skipped (every one goes into its iteration and moves)."""
    rep_u, rep_e, outcomes = replay
    assert rep_u.mismatch == [] and rep_e.mismatch == []
    assert rep_u.unsettled == [] and rep_e.unsettled == []
    n_random = len(C.update_cases()) * 2 * C.MAX_ITER * C.S_UPDATE
    assert rep_u.launches >= n_random
    for name, (got, want) in outcomes.items():
        assert got == want, (name, got, want)
    for where, codes in rep_e.events:
        assert codes == C.WANT_CODES, (where, codes)


def test_randomised_update_launches_all_move():
    """The cap of the randomised cases as a condition: in the float32 replay every launch of every problem comes out active
    (no stop, no skipped iteration), in both epochs."""
    for case in C.update_cases():
        su = C.case_setup(case)
        cfg = su.cfg
        dev = C.ModelDevice(C.S_UPDATE, su.n, su.dp, cfg["history"], cfg, cfg["pair"])
        dev.load(C.start_state(cfg, su.n, su.dp, cfg["history"], su.P0, su.mask0))
        seen = []
        real = dev.update
        dev.update = lambda mode: (real(mode), seen.append((dev.hs["act"].tolist(), dev.hs["n_iter"].tolist())))
        C.drive_update_case(case, dev, C.Report(), su)
        assert all(a == [1, 1, 1] for a, _ in seen), (C.case_id(case), seen)
        assert seen[-1][1] == [4, 4, 8], (C.case_id(case), seen[-1])       # problems 0 and 1 were reset, problem 2 carried on
        assert int(dev.hs["count"].min()) == min(3, cfg["history"])          # history 3: the ring wrapped


def test_tolerances_are_four_times_the_replay_deviation(replay):
    rep_u, rep_e, _ = replay
    for title, rep, tol in (("update", rep_u, C.STEP_TOL), ("epoch", rep_e, C.EPOCH_TOL)):
        for k in sorted(tol):
            worst, where = rep.worst.get(k, (0.0, None))
            print(f"trainer steps, {title} launch, {k}: float32 against fp64 {worst:.3e} at {where}; x 4 -> {_round_up(4 * worst):.1e} (committed {tol[k]:.1e})")
    for rep, tol in ((rep_u, C.STEP_TOL), (rep_e, C.EPOCH_TOL)):
        assert set(rep.worst) == set(tol)
        for k, (worst, where) in rep.worst.items():
            # the committed figure is 4 x the replay deviation on the machine that derived it; a CPU's own summation order
            # moves the replay figure by a few per cent, so 3 x .. 5 x is as close as another machine can hold it
            assert 3.0 * worst <= tol[k] <= 5.0 * worst, (k, worst, tol[k])


# ---------------------------------------------------------------------------------------------------------------------
# the free-running check's data and tolerance
# ---------------------------------------------------------------------------------------------------------------------
def test_free_running_tolerance_is_four_times_the_float32_oracle_deviation():
    worst = 0.0
    for case in C.FREE_RUN_CASES:
        h64 = C.free_run_oracle(case, torch.float64)
        h32 = C.free_run_oracle(case, torch.float32)
        assert h64["events"] == [] and h32["events"] == [] and len(h64["Xi"]) == C.FREE_RUN_EPOCHS
        for e, (a, b) in enumerate(zip(h32["Xi"], h64["Xi"])):
            dev = float((a.double() - b).abs().max() / b.abs().max())
            worst = max(worst, dev)
            print(f"free-running {case} epoch {e}: float32 oracle against fp64 {dev:.3e}")
    print(f"free-running: worst {worst:.3e}; x 4 -> {_round_up(4 * worst):.1e} (committed {C.FREE_RUN_TOL:.1e})")
    assert 3.0 * worst <= C.FREE_RUN_TOL <= 5.0 * worst      # as above: 4 x, to what another CPU's summation order allows
