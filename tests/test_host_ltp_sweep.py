"""Host logic of the sweep's roll-out scoring, without a GPU: evaluation.eval_ltp_sweep / val_mse_sweep and
``main_sweep --eval_ltp`` driven through a test double whose rollout_error is the oracle integrator (the product's only
engine is the HIP one; the double lives here, as tests/oracle_engine.py does for the other entries)."""
import os

import numpy as np
import pytest
import torch

import symode_amd  # noqa: F401
from oracle import sindy_oracle as O
from symode_amd import evaluation
from tests.oracle_engine import OracleEngine, _fl

torch.set_num_threads(4)
FLT_MAX = float(np.finfo(np.float32).max)


class LtpOracleEngine(OracleEngine):
    """OracleEngine + the two entries the roll-out scoring uses, restated with the oracle / plain torch."""

    def rollout_error(self, x_true, xi, mask, order, flags, dt, method="rk4", bound=float("inf"), want_error=True):
        XI = xi.reshape(-1, xi.shape[-2], xi.shape[-1])
        M = torch.ones_like(XI) if mask is None else mask.reshape(XI.shape)
        n_steps = x_true.shape[1] - 1
        errs = []
        for s in range(XI.shape[0]):
            f = lambda a: O.forward(a, XI[s], M[s], order, *_fl(flags))  # noqa: E731
            pred = O.odeint(f, x_true[:, 0], n_steps * dt + 0.5 * dt, dt, method, full_traj=True).transpose(0, 1)
            errs.append(((x_true[:, 1:] - pred) ** 2).mean(-1))
        err = torch.stack(errs)
        mean_err = err.double().cumsum(-1)[..., -1] / n_steps
        ok = (err <= min(bound, FLT_MAX)).int()
        horizon = ok.cumprod(-1).sum(-1).int()
        return (err if want_error else None), mean_err, horizon

    def quad_closure(self, G, R, xi, mask, inv_count, w_sym=1.0):
        assert R is None
        S, d, p = xi.shape
        W = (xi if mask is None else xi * mask).double()
        A = torch.cat([W, -torch.eye(d, dtype=torch.float64).expand(S, d, d)], dim=2)          # r = [Theta | dx] A^T
        AG = A @ G
        loss = inv_count * (AG * A).sum((1, 2))
        grad = 2.0 * inv_count * AG[:, :, :p]
        return loss.float(), (grad if mask is None else grad * mask).float()


def _dosc_validation(n_ics=5, n_points=41, dt=0.05, seed=3):
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(n_ics, np.random.RandomState(seed)), dt, n_points)
    return torch.from_numpy(xs).float(), torch.from_numpy(dxs).float()


def _models(S, seed=0):
    """The dosc truth table with per-model relative perturbations of 1e-2, a mask with zeros; the last model is wrong."""
    g = torch.Generator().manual_seed(seed)
    truth = torch.from_numpy(O.SINDY_TRUTH["dosc"]).float()
    Xi = truth[None] * (1 + 1e-2 * torch.randn(S, *truth.shape, generator=g)) + 0.3 * (truth[None] == 0)
    mask = (truth != 0).float()[None].expand(S, -1, -1).clone()
    Xi[-1, 0, 2] = -0.5
    return Xi, mask


def test_eval_ltp_sweep_is_the_per_model_evaluation_for_every_model():
    """The plumbing of eval_ltp_sweep: shapes, dtypes, t, the bound from ``bound_rel``, mse_step, and that model s of the
    result is model s of the input.  The double's rollout_error IS the oracle integrator, so the comparison with
    O.odeint below cannot detect a wrong integrator: that is what tests/test_gpu_ltp_sweep.py checks on the kernel."""
    x, _ = _dosc_validation()
    Xi, mask = _models(4)
    eng = LtpOracleEngine()
    out = evaluation.eval_ltp_sweep(Xi, mask, x, 0.05, poly_order=2, include_sine=False, include_exp=False, bound_rel=0.01, engine=eng)
    S, n_ics, n_steps = 4, x.shape[0], x.shape[1] - 1
    assert out["error"].shape == (S, n_ics, n_steps) and out["mean_error"].shape == (S, n_ics)
    assert out["horizon"].shape == (S, n_ics) and out["mse_step"].shape == (S, n_steps) and out["t"].shape == (n_steps,)
    assert out["mean_error"].dtype == np.float64 and out["horizon"].dtype == np.int32
    assert np.allclose(out["t"], 0.05 * np.arange(1, n_steps + 1))
    for s in range(S):
        f = lambda a: O.forward(a, Xi[s], mask[s], 2)  # noqa: E731
        pred = O.odeint(f, x[:, 0], n_steps * 0.05 + 0.025, 0.05, "rk4", full_traj=True).transpose(0, 1)
        want = ((x[:, 1:] - pred) ** 2).mean(-1).numpy()
        assert np.array_equal(out["error"][s], want)
    assert np.allclose(out["mse_step"], out["error"].mean(1), rtol=1e-6)
    assert np.allclose(out["mean_error"], out["error"].astype(np.float64).mean(-1), rtol=1e-12)
    # the bound: 0.01 x the mean squared deviation from each dimension's mean
    bound = 0.01 * ((x - x.mean(dim=(0, 1))) ** 2).mean().item()
    want_h = np.cumprod(out["error"] <= bound, axis=-1).sum(-1)
    assert np.array_equal(out["horizon"], want_h)
    assert (out["horizon"][:3] == n_steps).all() and (out["horizon"][3] < n_steps).all()     # the wrong model leaves the bound
    assert np.median(out["mean_error"][3]) > 100 * np.median(out["mean_error"][:3])
    # no bound: every finite step counts
    free = evaluation.eval_ltp_sweep(Xi, mask, x, 0.05, poly_order=2, include_sine=False, include_exp=False, engine=eng)
    assert (free["horizon"] == n_steps).all()


def test_eval_ltp_sweep_looks_dt_up_by_task_like_eval_ltp_accuracy():
    x, _ = _dosc_validation(dt=0.2)
    Xi, mask = _models(2)
    eng = LtpOracleEngine()
    kw = dict(poly_order=2, include_sine=False, include_exp=False, engine=eng)
    a = evaluation.eval_ltp_sweep(Xi, mask, x, task="dosc", **kw)
    b = evaluation.eval_ltp_sweep(Xi, mask, x, 0.2, **kw)
    assert np.array_equal(a["error"], b["error"]) and np.allclose(a["t"][:2], [0.2, 0.4])
    c = evaluation.eval_ltp_sweep(Xi, mask, x, 0.1, **kw)
    assert np.median(c["mean_error"]) > 10 * np.median(a["mean_error"])        # the data's own step is the one that fits it


def test_latent_or_autoencoder_roll_outs_are_refused_by_name():
    x, _ = _dosc_validation()
    Xi, mask = _models(2)
    kw = dict(poly_order=2, include_sine=False, include_exp=False, engine=LtpOracleEngine())
    with pytest.raises(NotImplementedError, match="eval_ltp_accuracy"):
        evaluation.eval_ltp_sweep(Xi, mask, x, 0.05, autoencoder=object(), **kw)
    with pytest.raises(NotImplementedError, match="eval_ltp_accuracy"):
        evaluation.eval_ltp_sweep(Xi, mask, x[:, :, None, :].expand(-1, -1, 2, -1), 0.05, **kw)


def test_val_mse_sweep_is_the_mse_of_every_model():
    x, dx = _dosc_validation()
    Xi, mask = _models(3)
    got = evaluation.val_mse_sweep(Xi, mask, x.reshape(-1, 2), dx.reshape(-1, 2), poly_order=2, include_sine=False, include_exp=False,
                                   engine=LtpOracleEngine())
    assert got.shape == (3,)
    for s in range(3):
        want = torch.nn.functional.mse_loss(O.forward(x.reshape(-1, 2), Xi[s], mask[s], 2), dx.reshape(-1, 2)).item()
        assert np.isclose(got[s], want, rtol=1e-5, atol=1e-9)


CURRENT_KEYS = {"coefficients", "correct_form", "mse", "correct_form_all", "mse_all"}


@pytest.mark.parametrize("method", ["lbfgs", "stlsq"])
def test_main_sweep_eval_ltp_adds_its_keys_and_nothing_else_changes(method, tmp_path, monkeypatch, capsys):
    from symode_amd import dataset as D, main_sweep
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples, noise-free
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)
    argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--lbfgs_subsample", "0.5",
            "--lr_sindy", "0.1", "--w_sindy_x", "1.0", "--w_sindy_z", "0.0", "--w_sindy_reg", "0.0", "--w_sym_reg", "0.0",
            "--poly_order", "2", "--st_freq", "50", "--threshold", "5e-2", "--num_epochs", "60", "--gpu", "-1",
            "--n_seeds", "4", "--method", method, "--seed", "0"]
    eng = LtpOracleEngine()
    main_sweep.main(argv + ["--save_dir", "plain"], engine=eng)
    plain_out = capsys.readouterr().out
    res = main_sweep.main(argv + ["--save_dir", "scored", "--eval_ltp", "--ltp_bound_rel", "0.01"], engine=eng)
    scored_out = capsys.readouterr().out
    assert res["n_runs"] == 4                                                  # aggregate_results reads its own keys only
    assert "roll-out error" not in plain_out and "roll-out error" in scored_out
    assert "correct form among the best 1 by roll-out error: 1/1" in scored_out
    for s in range(4):
        a = np.load(tmp_path / "eval_results" / "plain" / f"seed{s}.npz")
        b = np.load(tmp_path / "eval_results" / "scored" / f"seed{s}.npz")
        assert set(a.files) == CURRENT_KEYS
        assert set(b.files) == CURRENT_KEYS | {"ltp_mean_error", "ltp_horizon", "val_mse"}
        for k in CURRENT_KEYS:
            assert np.array_equal(a[k], b[k]), k
        assert b["ltp_mean_error"].shape == (3,) and b["ltp_mean_error"].dtype == np.float64
        assert b["ltp_horizon"].shape == (3,) and b["val_mse"].shape == ()
        assert bool(b["correct_form_all"])
        assert (b["ltp_horizon"] == 199).all() and b["ltp_mean_error"].max() < 1e-4 and float(b["val_mse"]) < 1e-4
    assert evaluation.aggregate_results("plain", 0, 4)["n_runs"] == 4 and os.path.isdir("eval_results/scored")
