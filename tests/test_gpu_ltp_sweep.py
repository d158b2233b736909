"""symode_rollout_error on the GPU: the roll-out error of S models in one launch against the per-model path
(evaluation.eval_ltp_accuracy on a SINDyRegression per model -- symode_odeint_traj plus torch ops), against the CPU
oracle, on a diverging model, its summaries (mean_err, horizon) against the host restatement, val_mse_sweep against
regressor.mse_loss, and ``main_sweep --eval_ltp`` end to end."""
import os

import numpy as np
import pytest
import torch

import symode_amd
from oracle import sindy_oracle as O
from symode_amd import evaluation
from symode_amd.sindy import SINDyRegression

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    return symode_amd.get_engine()


def _fl(flags):
    return bool(flags & 1), bool(flags & 2)


def _pad(table, p):
    out = np.zeros((table.shape[0], p))
    out[:, :table.shape[1]] = table
    return out


def _base(name, d, order, flags):
    """The generating model of a case: a truth table of evaluation.sindy_truth (padded to the library), or a contracting
    stand-in for the state dimensions no task of the reference has."""
    p = O.term_count(d, order, *_fl(flags))
    if name in evaluation.sindy_truth:
        return _pad(evaluation.sindy_truth[name], p)
    xi = np.zeros((d, p))
    for j in range(d):
        xi[j, 1 + j] = -1.0                               # linear damping
    if d == 1:
        xi[0, 3] = -0.5                                   # x' = -x - 0.5 x^3
    else:
        xi[0, 2], xi[1, 1] = -0.7, 0.7                    # a rotation in the first two coordinates
        if flags & 1:
            xi[2, p - d] = 0.2                            # + 0.2 sin(x_0) (the sine columns close the library)
        else:
            xi[2, p - 1] = -0.2                           # - 0.2 x the last monomial: |x| <= 1, the damping dominates
    return xi


def _truth_trajectories(base, d, order, flags, x0, dt, n_points, sub=10):
    """(n_ics, n_points, d) fp32: the base model integrated in fp64 with RK4 at dt / sub."""
    Xi, mask = torch.from_numpy(base), torch.ones(base.shape, dtype=torch.float64)
    f = lambda a: O.forward(a, Xi, mask, order, *_fl(flags))  # noqa: E731
    fine = O.odeint(f, torch.from_numpy(x0), (n_points - 1) * dt + 0.25 * dt / sub, dt / sub, "rk4", full_traj=True)
    fine = torch.cat([torch.from_numpy(x0)[None], fine])[::sub]
    assert fine.shape[0] == n_points
    return fine.transpose(0, 1).float().contiguous()


def _models(base, S, seed):
    """S models: the base table with per-model relative perturbations of 1e-2; the entries outside its support carry junk
    that the mask (zeros there) removes."""
    g = torch.Generator().manual_seed(seed)
    b = torch.from_numpy(base).float()
    Xi = b[None] * (1 + 1e-2 * torch.randn(S, *b.shape, generator=g)) + 0.3 * torch.randn(S, *b.shape, generator=g) * (b[None] == 0)
    mask = (b != 0).float()[None].expand(S, -1, -1).contiguous()
    assert (mask == 0).any()
    return Xi.contiguous(), mask


def _x0(name, d, n_ics, seed):
    rng = np.random.RandomState(seed)
    if name == "dosc":
        return O.ics_dosc(n_ics, rng)
    if name == "growth":
        return O.ics_growth(n_ics, rng)
    if name == "lv":
        return O.ics_lv(n_ics, rng)
    return rng.uniform(-1.0, 1.0, (n_ics, d))


def _per_model(x, Xi, mask, order, flags, dt):
    """The yardstick: evaluation.eval_ltp_accuracy of a SINDyRegression carrying Xi[s], mask[s], one model at a time."""
    d = x.shape[-1]
    out = []
    for s in range(Xi.shape[0]):
        reg = SINDyRegression(d, order, *_fl(flags), threshold=0.05, device="cuda:0")
        with torch.no_grad():
            reg.Xi.copy_(Xi[s])
        reg.mask = mask[s].clone().cuda()
        out.append(evaluation.eval_ltp_accuracy(reg, None, x, dt)["error"])
    return np.stack(out)


# name, d, order, flags, n_ics, n_steps, dt, method, offset_rows
CASES = [
    ("dosc", 2, 2, 0, 10, 100, 0.2, "rk4", 0),            # the dosc validation recipe: 10 x 100 steps, dt 0.2
    ("dosc", 2, 2, 0, 10, 100, 0.2, "euler", 0),
    ("growth", 2, 2, 0, 20, 100, 0.02, "rk4", 0),         # growth: 20 x 100
    ("decay1", 1, 3, 0, 10, 100, 0.1, "rk4", 0),          # a d = 1 library
    ("spiral3", 3, 2, 1, 10, 100, 0.1, "rk4", 0),         # a d = 3 library (with sine columns)
    ("dosc", 2, 5, 0, 10, 100, 0.2, "rk4", 0),            # d = 2 order 5 (p = 21)
    ("lv", 2, 2, 2, 10, 200, 0.002, "rk4", 0),            # order 2 + exp (the lv library) on 200 steps
    ("dosc", 2, 2, 0, 10, 103, 0.2, "rk4", 0),            # an odd n_steps: the ragged tail of the truth and err groups
    ("dosc", 2, 2, 0, 10, 103, 0.2, "rk4", 1),            # ... and the truth one row past a 16-byte boundary: the scalar path
    ("dosc", 2, 2, 0, 10, 99, 0.2, "rk4", 0),             # 100 time points, as the validation files hold them
    ("spiral3", 3, 2, 1, 10, 101, 0.1, "rk4", 1),
    # d = 3 order 3: d p = 60 coefficients per lane, past the 48 up to which load_xi's default keeps them in VGPRs -- its
    # default form above that holds ONE model's coefficients per wave, and these waves straddle models
    ("spiral3", 3, 3, 0, 10, 100, 0.1, "rk4", 0),
]


@pytest.mark.parametrize("name,d,order,flags,n_ics,n_steps,dt,method,offset_rows", CASES)
def test_rollout_error_against_the_per_model_path(eng, name, d, order, flags, n_ics, n_steps, dt, method, offset_rows):
    """err[s] of ONE launch over S = 7 models x n_ics trajectories (waves straddle models) against eval_ltp_accuracy per
    model.  Both kernels instantiate the same step, so bit-equality is expected (the count of differing words is
    printed); asserted: rtol 1e-5 with atol 1e-5 max|err| -- these systems contract, a last-bit difference cannot grow.
    ``offset_rows`` = 1 places the truth tensor one row (d floats) past a 16-byte boundary: the scalar path.
    Measured on MI355X (the lines this test prints): 0 differing words in every d = 1 and d = 2 case; at d = 3, 1274 of
    7000 (order 2 + sine), 1287 of 7070 (offset row) and 1331 of 7000 (order 3) words differ in the last place (max |diff|
    1.8e-12 at errors of 2e-5): torch's reduction adds the three squares of a row in its own order, the kernel adds them
    in index order."""
    S = 7
    base = _base(name, d, order, flags)
    x = _truth_trajectories(base, d, order, flags, _x0(name, d, n_ics, 11), dt, n_steps + 1)
    Xi, mask = _models(base, S, 5)
    if offset_rows:
        buf = torch.zeros(x.numel() + 4 * d, device="cuda")
        assert buf.data_ptr() % 16 == 0
        xg = buf[offset_rows * d: offset_rows * d + x.numel()].view(x.shape)
        xg.copy_(x)
        assert xg.data_ptr() % 16 != 0
    else:
        xg = x.cuda()
    err, mean_err, horizon = eng.rollout_error(xg, Xi.cuda(), mask.cuda(), order, flags, dt, method, float("inf"), True)
    assert err.shape == (S, n_ics, n_steps) and mean_err.shape == (S, n_ics) and horizon.shape == (S, n_ics)
    got = err.cpu().numpy()
    if method == "rk4":
        want = _per_model(xg, Xi.cuda(), mask.cuda(), order, flags, dt)
    else:                                                  # eval_ltp_accuracy is RK4 only: its two steps, with Euler
        traj = torch.stack([eng.odeint_traj(xg[:, 0].contiguous(), Xi[s].cuda(), mask[s].cuda(), order, flags, n_steps, dt, "euler")
                            for s in range(S)]).transpose(1, 2)
        want = torch.mean((xg[None, :, 1:] - traj) ** 2, dim=-1).cpu().numpy()
    differing = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{name} d={d} order={order} flags={flags} {method} n_steps={n_steps} offset={offset_rows}: "
          f"{differing} of {got.size} words differ, max |diff| {np.abs(got - want).max():.3e}, max err {np.abs(want).max():.3e}")
    assert np.isfinite(want).all()
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # summaries of the same launch
    assert np.array_equal(horizon.cpu().numpy(), np.full((S, n_ics), n_steps))
    assert np.allclose(mean_err.cpu().numpy(), np.cumsum(got.astype(np.float64), -1)[..., -1] / n_steps, rtol=1e-12, atol=0)


def test_rollout_error_against_the_cpu_oracle(eng):
    """The dosc case against oracle.sindy_oracle.odeint(..., "rk4", full_traj=True) through an OracleRegressor, at the
    tolerance of the existing full-trajectory parity test (tests/test_gpu_kernels.py): rtol 3e-4, atol 2e-5."""
    S, n_ics, n_steps, dt = 7, 10, 100, 0.2
    base = _base("dosc", 2, 2, 0)
    x = _truth_trajectories(base, 2, 2, 0, _x0("dosc", 2, n_ics, 11), dt, n_steps + 1)
    Xi, mask = _models(base, S, 5)
    err, _, _ = eng.rollout_error(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt)
    got = err.cpu().numpy()
    for s in range(S):
        reg = O.OracleRegressor(2, 2, Xi0=Xi[s])
        reg.mask = mask[s]
        with torch.no_grad():
            pred = O.odeint(reg, x[:, 0], n_steps * dt + 0.5 * dt, dt, "rk4", full_traj=True).transpose(0, 1)
        want = torch.mean((x[:, 1:] - pred) ** 2, dim=-1).numpy()
        print(f"model {s}: max |diff| {np.abs(got[s] - want).max():.3e}, max err {want.max():.3e}")
        assert np.allclose(got[s], want, rtol=3e-4, atol=2e-5)


def test_a_diverging_model_is_ordinary_inf_nan_arithmetic(eng):
    """One model with x0' = x0^2 on dosc data: the state runs to inf, then NaN.  The isfinite mask of err equals the
    per-model path's, and horizon with bound = inf is the count of leading finite steps; the other models are untouched."""
    S, n_ics, n_steps, dt = 3, 10, 100, 0.2
    base = _base("dosc", 2, 2, 0)
    x = _truth_trajectories(base, 2, 2, 0, _x0("dosc", 2, n_ics, 11), dt, n_steps + 1)
    Xi, mask = _models(base, S, 5)
    Xi[1], mask[1] = 0.0, 0.0
    Xi[1, 0, 3], mask[1, 0, 3] = 1.0, 1.0                  # columns of d = 2 order 2: 1, x0, x1, x0^2, x0 x1, x1^2
    err, mean_err, horizon = eng.rollout_error(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt)
    got = err.cpu().numpy()
    want = _per_model(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    assert not np.isfinite(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    fin = np.isfinite(got)
    assert np.allclose(got[fin], want[fin], rtol=1e-5, atol=1e-5 * np.abs(want[[0, 2]]).max())
    leading = np.cumprod(fin, axis=-1).sum(-1)
    assert np.array_equal(horizon.cpu().numpy(), leading)
    assert (leading[1] < n_steps).any() and (leading[[0, 2]] == n_steps).all()
    m = mean_err.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.cumsum(got.astype(np.float64), -1)[..., -1] / n_steps
    assert np.array_equal(np.isnan(m), np.isnan(ref)) and np.array_equal(np.isinf(m), np.isinf(ref))


@pytest.mark.parametrize("n_steps", [100, 103, 2])
def test_summaries_equal_the_host_restatement_and_need_no_err(eng, n_steps):
    """horizon = the host count of leading steps with err <= bound, exactly; mean_err = the fp64 running sum of the fp32
    errors over n_steps to 1e-12; with err = NULL both are bit-identical to the run that returned err."""
    S, n_ics, dt = 7, 10, 0.2
    base = _base("dosc", 2, 2, 0)
    x = _truth_trajectories(base, 2, 2, 0, _x0("dosc", 2, n_ics, 11), dt, n_steps + 1)
    Xi, mask = _models(base, S, 5)
    Xi[3, 0, 2] = -0.6                                     # one model visibly off: it leaves the bound early
    free = eng.rollout_error(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt)[0].cpu().numpy()
    bound = float(np.median(free[:, :, -1]))               # a bound that separates lanes and cuts inside trajectories
    err, mean_err, horizon = eng.rollout_error(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt, "rk4", bound, True)
    got = err.cpu().numpy()
    assert np.array_equal(got, free)                       # the bound does not touch the errors
    want_h = np.cumprod(got <= np.float32(bound), axis=-1).sum(-1)
    assert np.array_equal(horizon.cpu().numpy(), want_h)
    if n_steps > 2:
        assert len(np.unique(want_h)) > 1                  # the bound cuts at different steps in different lanes
    want_m = np.cumsum(got.astype(np.float64), -1)[..., -1] / n_steps
    assert np.allclose(mean_err.cpu().numpy(), want_m, rtol=1e-12, atol=0)
    none, mean2, hor2 = eng.rollout_error(x.cuda(), Xi.cuda(), mask.cuda(), 2, 0, dt, "rk4", bound, False)
    assert none is None
    assert torch.equal(mean2.view(torch.int64), mean_err.view(torch.int64)) and torch.equal(hor2, horizon)
    # a single (d, p) model and no mask
    e1, m1, h1 = eng.rollout_error(x.cuda(), (Xi[0] * mask[0]).cuda(), None, 2, 0, dt, "rk4", bound, True)
    assert torch.equal(e1[0], err[0]) and torch.equal(m1[0], mean_err[0]) and torch.equal(h1[0], horizon[0])


def test_eval_ltp_sweep_on_the_gpu_is_eval_ltp_accuracy_per_model(eng):
    S, n_ics, n_steps, dt = 5, 10, 100, 0.2
    base = _base("dosc", 2, 2, 0)
    x = _truth_trajectories(base, 2, 2, 0, _x0("dosc", 2, n_ics, 11), dt, n_steps + 1).cuda()
    Xi, mask = _models(base, S, 5)
    out = evaluation.eval_ltp_sweep(Xi.cuda(), mask.cuda(), x, task="dosc", poly_order=2, include_sine=False, include_exp=False,
                                    bound_rel=0.05)
    want = _per_model(x, Xi.cuda(), mask.cuda(), 2, 0, dt)
    assert np.allclose(out["error"], want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert np.allclose(out["mse_step"], want.mean(1), rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert np.allclose(out["t"], dt * np.arange(1, n_steps + 1))
    bound = 0.05 * ((x - x.mean(dim=(0, 1))) ** 2).mean().item()
    assert np.array_equal(out["horizon"], np.cumprod(out["error"] <= np.float32(bound), axis=-1).sum(-1))


def test_val_mse_sweep_against_mse_loss_per_model(eng):
    S, n_ics, n_points, dt = 7, 10, 100, 0.2
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(n_ics, np.random.RandomState(2)), dt, n_points)
    x, dx = torch.from_numpy(xs.reshape(-1, 2)).float().cuda(), torch.from_numpy(dxs.reshape(-1, 2)).float().cuda()
    dx = dx + 0.05 * torch.randn(dx.shape, generator=torch.Generator().manual_seed(1)).cuda()
    Xi, mask = _models(_base("dosc", 2, 2, 0), S, 5)
    got = evaluation.val_mse_sweep(Xi.cuda(), mask.cuda(), x, dx, poly_order=2, include_sine=False, include_exp=False)
    assert got.shape == (S,)
    for s in range(S):
        reg = SINDyRegression(2, 2, False, False, threshold=0.05, device="cuda:0")
        with torch.no_grad():
            reg.Xi.copy_(Xi[s])
        reg.mask = mask[s].clone().cuda()
        with torch.no_grad():
            want = torch.nn.functional.mse_loss(reg(x), dx).item()
        print(f"model {s}: val_mse {got[s]:.8e}, mse_loss {want:.8e}")
        assert np.isclose(got[s], want, rtol=1e-5, atol=0)


def test_engine_rollout_error_refuses_bad_shapes(eng):
    """x_true that is not (n_ics, n_steps + 1, d), and xi / mask whose size is not S x d x p of the library, are refused
    before any launch."""
    x = torch.zeros(3, 11, 2, device="cuda")
    xi = torch.zeros(4, 2, 6, device="cuda")
    with pytest.raises(symode_amd.SymodeError, match="x_true must be"):
        eng.rollout_error(x.reshape(33, 2), xi, None, 2, 0, 0.1)
    with pytest.raises(symode_amd.SymodeError, match="x_true must be"):
        eng.rollout_error(x[None], xi, None, 2, 0, 0.1)
    with pytest.raises(symode_amd.SymodeError, match="xi has 40 elements, expected 4x2x6"):
        eng.rollout_error(x, torch.zeros(4, 2, 5, device="cuda"), None, 2, 0, 0.1)
    with pytest.raises(symode_amd.SymodeError, match="xi has 48 elements, expected 4x2x10"):
        eng.rollout_error(x, xi, None, 3, 0, 0.1)          # the order-3 library has 10 columns
    with pytest.raises(symode_amd.SymodeError, match="mask has 12 elements, expected 4x2x6"):
        eng.rollout_error(x, xi, torch.ones(2, 6, device="cuda"), 2, 0, 0.1)
    with pytest.raises(ValueError):
        eng.rollout_error(x, xi, None, 2, 0, 0.1, "midpoint")
    err, mean_err, horizon = eng.rollout_error(x, xi, torch.ones(4, 2, 6, device="cuda"), 2, 0, 0.1)
    assert err.shape == (4, 3, 10) and (err == 0).all() and (horizon == 10).all()   # zero model on zero data


CURRENT_KEYS = {"coefficients", "correct_form", "mse", "correct_form_all", "mse_all"}


def test_main_sweep_eval_ltp_on_the_dosc_config(tmp_path, monkeypatch, capsys):
    """dosc/noise20_sindy.cfg with a few seeds: the new npz keys with their shapes; a second run without the flag writes
    the current key set and the same coefficients; aggregate_results runs on both."""
    import shutil
    from symode_amd import main_sweep
    monkeypatch.chdir(tmp_path)
    shutil.copytree(os.path.join(os.path.dirname(os.path.abspath(main_sweep.__file__)), "run_configs"), tmp_path / "run_configs")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--config", "dosc/noise20_sindy.cfg", "--n_seeds", "3", "--seed", "0"]
    res = main_sweep.main(argv + ["--save_dir", "scored", "--eval_ltp", "--ltp_bound_rel", "0.1"])
    scored_out = capsys.readouterr().out
    assert res["n_runs"] == 3 and "roll-out error" in scored_out and "correct form among the best 1" in scored_out
    res = main_sweep.main(argv + ["--save_dir", "plain"])
    plain_out = capsys.readouterr().out
    assert res["n_runs"] == 3 and "roll-out error" not in plain_out
    for s in range(3):
        a = np.load(tmp_path / "eval_results" / "plain" / f"seed{s}.npz")
        b = np.load(tmp_path / "eval_results" / "scored" / f"seed{s}.npz")
        assert set(a.files) == CURRENT_KEYS and set(b.files) == CURRENT_KEYS | {"ltp_mean_error", "ltp_horizon", "val_mse"}
        for k in CURRENT_KEYS:
            assert np.array_equal(a[k], b[k]), k
        assert b["ltp_mean_error"].shape == (10,) and b["ltp_mean_error"].dtype == np.float64      # 10 validation trajectories
        assert b["ltp_horizon"].shape == (10,) and b["ltp_horizon"].dtype == np.int32 and b["val_mse"].shape == ()
        assert (b["ltp_horizon"] >= 0).all() and (b["ltp_horizon"] <= 99).all() and np.isfinite(b["val_mse"])
    assert evaluation.aggregate_results("scored", 0, 3)["n_runs"] == 3
    assert os.path.exists("eval_results/plain/seed0.npz")
