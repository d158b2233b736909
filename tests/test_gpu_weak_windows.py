"""The weak-SINDy seed sweep on the device: symode_weak_normal_windows (window contraction + normal matrices),
engine.weak_normal_windows, sweep.SeedSweepWSINDy and main_sweep --wsindy / --wsindy_grid.

  Z      window s of z_out is, bit for bit, what symode_weak_gram writes for the copied window;
  N      aug_out against Z^T (M Z) in numpy fp64 on the device's own Z.  Both sides are two nested length-K fp64 sums;
         each errs by at most (2 g + g^2) B elementwise, B = |Z|^T |M| |Z|, g = K u / (1 - K u), u = 2^-53, whatever the
         summation order, with or without FMA; so |aug_out - Z^T (M Z)| <= 4 (K + 1) u B;
  guard  rows outside the data set read nothing, give zeros and a flag; the others are untouched by them;
  fit    SeedSweepWSINDy against WSINDyWrapper + train_WSINDy per copied window (driver gels): equal masks and passes,
         coefficients within 1e-5 of the row's largest (the tolerance the weak path is held to against f7), and the
         reference's f7 fixture as a one-window sweep;
  grid, driver: bit for bit the scalar runs; seed n of the sweep is main_wsindy --seed n."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import stlsq_cases as C
from tests import weak_sweep_model as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
N_ICS, TAIL = 3, 11                                          # n_steps = n_t + 11


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


@functools.lru_cache(maxsize=None)
def _tests(n_t, K, dt=0.02):
    """(V, V_drv fp32, M fp64) on the device, by the expressions every weak fit uses."""
    from symode_amd.sindy import weak_test_functions
    _, _, V, V_drv, M = weak_test_functions(torch.arange(n_t) * dt, n_t * dt, K, "trig", DEV)
    return V, V_drv, torch.from_numpy(np.ascontiguousarray(M)).to(DEV)


@functools.lru_cache(maxsize=None)
def _data(d, n_t):
    rng = np.random.RandomState(100 * d + n_t)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, (N_ICS, n_t + TAIL, d)).astype(np.float32)).to(DEV)


def _windows(n_t, seed):
    """S = 7: the first row of the data set, an odd start, the window that ends on the data set's last row, a duplicate
    pair, the rest random."""
    rng = np.random.RandomState(seed)
    rows = [[0, 0], [1, 7], [N_ICS - 1, TAIL], [1, 4], [1, 4]]
    rows += [[int(rng.randint(0, N_ICS)), int(rng.randint(0, TAIL + 1))] for _ in range(2)]
    return np.array(rows, dtype=np.int64)


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "d%d-o%d-f%d" % s)
@pytest.mark.parametrize("K", [5, 50, 128])
@pytest.mark.parametrize("n_t", [37, 160, 700])
def test_z_is_the_single_trajectory_entry_and_n_is_fp64(eng, n_t, K, shape):
    d, order, flags = shape
    p = eng.lib_size(d, order, flags)
    F = p + d
    x3, (V, V_drv, M) = _data(d, n_t), _tests(n_t, K)
    win = _windows(n_t, 1000 * n_t + K)
    aug, z, bad = eng.weak_normal_windows(x3, win, n_t, V, V_drv, M, order, flags, want_z=True)
    R, Cc = 16 * ((2 * K + 15) // 16), 16 * ((F + 15) // 16)
    assert aug.shape == (7, F, F) and z.shape == (7, R, Cc) and bad.cpu().tolist() == [0] * 7
    zh, Mh = z.cpu().numpy(), M.cpu().numpy()
    for s, (tr, st) in enumerate(win.tolist()):
        G, b = eng.weak_gram(x3[tr, st:st + n_t].contiguous(), V, V_drv, order, flags)
        assert _bytes(z[s, :K, :p]) == _bytes(G) and _bytes(z[s, K:2 * K, p:F]) == _bytes(b), (s, tr, st)
    assert _bytes(z[3]) == _bytes(z[4]) and _bytes(aug[3]) == _bytes(aug[4])            # the duplicate pair
    assert _bytes(z[0]) != _bytes(z[1])
    # N against fp64 on the device's own Z
    augh = aug.cpu().numpy()
    worst = 0.0
    for s in range(7):
        Z = np.concatenate([zh[s, :K, :p], zh[s, K:2 * K, p:F]], axis=1)
        want, B = Z.T @ (Mh @ Z), np.abs(Z).T @ (np.abs(Mh) @ np.abs(Z))
        err = np.abs(augh[s] - want)
        worst = max(worst, float((err / (4 * (K + 1) * U * B + 1e-300)).max()))
        assert (err <= 4 * (K + 1) * U * B).all(), (s, worst)
        assert augh[s].tobytes() == np.ascontiguousarray(augh[s].T).tobytes(), s            # exactly symmetric
    print("n_t", n_t, "K", K, shape, "max |dN| / bound %.3g" % worst)
    # a second launch gives the same bytes; without z_out the matrices are the same
    aug2, z2, _ = eng.weak_normal_windows(x3, win, n_t, V, V_drv, M, order, flags, want_z=True)
    assert _bytes(aug2) == _bytes(aug) and _bytes(z2) == _bytes(z)
    assert _bytes(eng.weak_normal_windows(x3, win, n_t, V, V_drv, M, order, flags)[0]) == _bytes(aug)
    # S = 1
    one, z1, bad1 = eng.weak_normal_windows(x3, win[2:3], n_t, V, V_drv, M, order, flags, want_z=True)
    assert _bytes(one[0]) == _bytes(aug[2]) and _bytes(z1[0]) == _bytes(z[2]) and bad1.cpu().tolist() == [0]


def test_the_guard_reads_nothing_for_rows_outside_the_data_set(eng):
    """Straight to the entry, behind the engine's host check: a trajectory == n_ics and a start one past the last valid one."""
    import symode_amd
    d, order, flags, n_t, K = 2, 3, 0, 160, 50
    x3, (V, V_drv, M) = _data(d, n_t), _tests(n_t, K)
    good = _windows(n_t, 5)
    table = np.concatenate([good[:2], [[N_ICS, 0]], good[2:5], [[0, TAIL + 1]], good[5:]]).astype(np.int32)
    is_bad = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0], dtype=bool)
    with pytest.raises(symode_amd.SymodeError, match=r"windows\[2\] = \[3, 0\] is out of range"):
        eng.weak_normal_windows(x3, table, n_t, V, V_drv, M, order, flags)
    aug, z, bad = eng._weak_normal_windows(x3, np.ascontiguousarray(table), n_t, V, V_drv, M, order, flags, True)
    want_aug, want_z, want_bad = eng.weak_normal_windows(x3, good, n_t, V, V_drv, M, order, flags, want_z=True)
    torch.cuda.synchronize()
    assert bad.cpu().numpy().tolist() == is_bad.astype(int).tolist() and want_bad.cpu().tolist() == [0] * 7
    aug, z = aug.cpu().numpy(), z.cpu().numpy()
    assert not aug[is_bad].any() and not z[is_bad].any()
    assert aug[is_bad].tobytes() == np.zeros_like(aug[is_bad]).tobytes()                     # +0.0, not -0.0
    assert aug[~is_bad].tobytes() == _bytes(want_aug) and z[~is_bad].tobytes() == _bytes(want_z)


# ---- the fit ------------------------------------------------------------------------------------------------------------------
SEEDS = range(8)


@functools.lru_cache(maxsize=None)
def _sweep():
    from symode_amd.sweep import SeedSweepWSINDy
    return SeedSweepWSINDy(W.dosc_data().to(DEV), W.ORDER, dt=W.DT, seeds=SEEDS, num_test_funcs=W.K)


@pytest.mark.parametrize("w_sindy_reg, threshold", W.FIT_POINTS)
def test_the_sweep_is_the_per_seed_route(eng, w_sindy_reg, threshold):
    from symode_amd.sweep import weak_windows
    sw = _sweep()
    assert sw.n_t == W.N_T == 160 and np.array_equal(sw.windows, weak_windows(SEEDS, W.N_ICS, W.N_STEPS, W.N_T))
    xi, mask, passes, near = W.per_seed(W.dosc_data(), sw.windows, W.N_T, W.DT, W.ORDER, w_sindy_reg, threshold, device=DEV)
    size = mask.reshape(8, -1).sum(axis=1)
    print((w_sindy_reg, threshold), "per-seed passes", passes.tolist(), "support", size.tolist(), "near", near.tolist())
    assert W.conditions(mask, passes, near) == (True, True, True)          # the conditions the comparison rests on
    Xi, m, ps = sw.solve(w_sindy_reg, threshold, max_iter=W.MAX_ITER)
    Xi, m = Xi.numpy(), m.numpy() > 0
    assert sw.near_threshold == [] and sw.bad.tolist() == [0] * 8
    assert np.array_equal(m, mask) and np.array_equal(ps, passes)
    err = np.abs(Xi.astype(np.float64) - xi.astype(np.float64)) / np.abs(xi).max(axis=-1, keepdims=True)
    print("max |dXi| / largest of the row %.3g" % err.max())
    assert (err <= 1e-5).all()
    # and the fp64 restatement of the sweep (tests/weak_sweep_model.py) on the device's own matrices
    mxi, mmask, mpasses, _ = W.sweep(sw.normals(), 2, W.N_T, w_sindy_reg, threshold)
    assert np.array_equal(m, mmask) and np.array_equal(ps, mpasses)
    assert (np.abs(Xi.astype(np.float64) - mxi) <= 1e-5 * np.abs(mxi).max(axis=-1, keepdims=True)).all()


def test_the_reference_fixture_as_a_one_window_sweep(eng, golden):
    from symode_amd.sweep import SeedSweepWSINDy
    w = golden("f7_wsindy")
    x = torch.from_numpy(w["x"]).float().to(DEV)
    n = x.shape[0]
    assert abs(float(w["tmax"]) - n * 0.02) <= 1e-6 * n * 0.02
    sw = SeedSweepWSINDy(x[None], 3, dt=0.02, windows=np.array([[0, 0]]), n_t=n)
    assert np.allclose(sw.V[:, :48].cpu().numpy(), w["V_head"], rtol=1e-5, atol=1e-7)
    Xi, mask, passes = sw.solve(0.0, 0.05, max_iter=len(w["masks"]))
    wx = w["xis"][-1]
    assert np.array_equal(mask[0].numpy(), w["masks"][-1]) and int(passes[0]) == len(w["masks"]) and bool(w["conv"][-1])
    assert np.allclose(Xi[0].numpy(), wx, rtol=1e-5, atol=1e-5 * np.abs(wx).max())


def test_a_grid_is_the_scalar_solves(eng):
    sw = _sweep()
    points = [(w, t) for w in (1e-4, 1e-3) for t in (0.2, 0.3)]
    hyper = {"w_reg": [w for w, _ in points for _ in SEEDS], "threshold": [t for _, t in points for _ in SEEDS]}
    Xi, mask, passes = sw.solve(7.0, 7.0, max_iter=W.MAX_ITER, hyper=hyper)
    assert Xi.shape == (32, 2, 10) and passes.shape == (32,)
    for g, (w, t) in enumerate(points):
        at = slice(8 * g, 8 * g + 8)
        one = sw.solve(w, t, max_iter=W.MAX_ITER)
        assert Xi[at].numpy().tobytes() == one[0].numpy().tobytes() and np.array_equal(mask[at].numpy(), one[1].numpy()), g
        assert np.array_equal(passes[at], one[2]), g
    assert not np.array_equal(mask[:8].numpy(), mask[24:].numpy())                          # the values decide


# ---- main_sweep --wsindy and --wsindy_grid ------------------------------------------------------------------------------------
# (order 2, the weak configs' own: main_wsindy scores against the task's six-column truth table as it stands)
BASE = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--poly_order", "2", "--threshold", "0.05", "--w_sindy_reg", "1e-4",
        "--num_epochs", "10", "--lstsq_driver", "gels"]


def _in(tmp, fn, argv):
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        return fn(list(argv))
    finally:
        os.chdir(cwd)


def _sweep_main(tmp, save_dir, extra):
    from symode_amd import main_sweep
    return _in(tmp, main_sweep.main, BASE + ["--seed", "4", "--n_seeds", "4", "--wsindy", "--save_dir", save_dir] + extra)


@pytest.fixture()
def small_dosc(monkeypatch):
    from symode_amd import dataset as D
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)


def test_main_sweep_wsindy_is_main_wsindy_per_seed(eng, tmp_path, small_dosc, capsys):
    from symode_amd import main_wsindy
    res = _sweep_main(tmp_path, "sweep", [])                                       # (writes the data files the per-seed runs read)
    out = capsys.readouterr().out
    assert res["n_runs"] == 4
    assert "4 seeds x 160 time points of one trajectory each, 50 test functions, STLSQ passes " in out
    assert "near-threshold coefficients (| |coef| - thr | < 1e-4): none" in out        # near == 0: no decision on a rounding
    root = tmp_path / "eval_results"
    for s in (4, 5, 6, 7):
        _in(tmp_path, main_wsindy.main, BASE + ["--seed", str(s), "--save_dir", "per_seed"])
        want, got = np.load(root / "per_seed" / f"seed{s}.npz"), np.load(root / "sweep" / f"seed{s}.npz")
        assert set(got.files) == set(want.files) == {"coefficients", "correct_form", "mse", "correct_form_all", "mse_all"}
        a, b = want["coefficients"].astype(np.float64), got["coefficients"].astype(np.float64)
        assert np.array_equal(a != 0, b != 0), s
        assert (np.abs(a - b) <= 1e-5 * np.abs(a).max(axis=-1, keepdims=True)).all(), s
        assert np.array_equal(want["correct_form"], got["correct_form"]) and bool(want["correct_form_all"]) == bool(got["correct_form_all"])
    capsys.readouterr()
    # --eval_ltp: the same fit, scored by the one roll-out launch
    _sweep_main(tmp_path, "scored", ["--eval_ltp", "--ltp_bound_rel", "0.1"])
    out = capsys.readouterr().out
    assert "seeds by median roll-out error on the validation trajectories" in out
    for s in (4, 5, 6, 7):
        plain, scored = np.load(root / "sweep" / f"seed{s}.npz"), np.load(root / "scored" / f"seed{s}.npz")
        assert set(scored.files) == set(plain.files) | {"ltp_mean_error", "ltp_horizon", "val_mse"}
        assert scored["coefficients"].tobytes() == plain["coefficients"].tobytes()


def test_main_sweep_wsindy_grid_is_main_sweep_at_every_point(eng, tmp_path, small_dosc, capsys):
    T = ("0.05", "0.3")
    res = _sweep_main(tmp_path, "grid", ["--wsindy_grid", "threshold=" + ",".join(T)])
    out = capsys.readouterr().out
    assert sorted(res) == [0, 1] and all(r["n_runs"] == 4 for r in res.values())
    assert "grid of 2 points x 4 seeds" in out and "grid 1: STLSQ passes" in out and "2 grid points on their normal matrices" in out
    root = tmp_path / "eval_results"
    listed = json.loads((root / "grid" / "grid.json").read_text())
    assert listed["axes"] == [["threshold", [0.05, 0.3]]] and listed["n_seeds"] == 4 and listed["seed0"] == 4
    assert [p["threshold"] for p in listed["points"]] == [0.05, 0.3]
    assert sorted(p.name for p in (root / "grid").iterdir()) == ["grid.json", "grid0", "grid1"]
    coefs = []
    for g, thr in enumerate(T):
        scalar = _sweep_main(tmp_path, f"point{g}", ["--threshold", thr])
        assert repr(res[g]) == repr(scalar), g
        for s in (4, 5, 6, 7):
            want, got = np.load(root / f"point{g}" / f"seed{s}.npz"), np.load(root / "grid" / f"grid{g}" / f"seed{s}.npz")
            assert set(got.files) == set(want.files) | {"threshold", "w_sindy_reg"}
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            assert float(got["threshold"]) == float(thr) and float(got["w_sindy_reg"]) == 1e-4
            coefs.append(got["coefficients"])
    assert not np.array_equal(coefs[0], coefs[4])                                          # the threshold decides
