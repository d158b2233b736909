"""The rank-revealing mode of the constrained device sweep (symode_stlsq_sweep_minnorm, engine.stlsq_sweep_minnorm,
SeedSweepSTLSQ.solve(device=True, coef=..., min_norm=True), main_sweep --min_norm_stlsq) against
tests/stlsq_minnorm_model.py, the kernel's algorithm in numpy, on the cases of tests/stlsq_minnorm_cases.py; against the
existing entry where every pass has full rank; and against the flag-and-host route it replaces.

Bounds are derived, not measured: a full-rank pass has tests/stlsq_constrained_model.py's (cond(Gq)), a truncated pass
``M.var_bound`` / ``M.xi_bound`` with cond(R11)^2 cond(Wm Wm^T) in its place.  Model and kernel perform the same operations
in the same order, so equal bytes are expected and printed; the bound is what is asserted.  The conditions on the inputs
(margins of the rank decision, condition number <= 1e6) are asserted by tests/test_host_stlsq_minnorm_model.py."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_constrained_cases as C
from tests import stlsq_constrained_model as M0
from tests import stlsq_minnorm_cases as K
from tests import stlsq_minnorm_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("xi", "mask", "passes", "near", "fell", "var", "trunc", "rank")
WORDS = "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead"


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _device(eng, G, coef, gamma, threshold, max_iter, entry="minnorm", **kw):
    qs, qx = (torch.from_numpy(q).to(DEV) for q in C.matrices(coef))
    G = torch.as_tensor(G).to(DEV)
    G = G if G.dim() == 3 else G[None]
    if entry == "minnorm":
        out = eng.stlsq_sweep_minnorm(G, K.N_POINTS, gamma, threshold, max_iter, qs, qx, coef.allow_constant, d=coef.d, rcond=M.RCOND,
                                      near_band=K.BAND, **kw)
    else:
        out = eng.stlsq_sweep_constrained(G, K.N_POINTS, gamma, threshold, max_iter, qs, qx, coef.allow_constant, d=coef.d,
                                          pivot_floor=M0.PIVOT_FLOOR, near_band=K.BAND, **kw)
    out = [t.cpu().numpy() for t in out]
    out[1] = out[1].astype(bool)
    return out


@functools.lru_cache(maxsize=None)
def _model(key, gamma, max_iter, threshold=K.THRESHOLD):
    G, coef = K.inputs(key)
    qs, qx = C.matrices(coef)
    trace = []
    out = M.sweep(G, coef.d, gamma, threshold, max_iter, qs, qx, coef.allow_constant, band=K.BAND, trace=trace)
    return out, trace


def _bounds(out, trace, coef):
    """(bound on Xi, bound on var) of the model's last pass."""
    info, Gq = trace[-1][5], trace[-1][2]
    cond, n = M.pass_cond(info, Gq), info["n"]
    which = M if info["rank"] < n else M0
    return (which.xi_bound(coef.xi_matrix(), out["var"], cond, n, coef.d, coef.p, coef.allow_constant), which.var_bound(out["var"], cond, n),
            cond)


# ---- 1. the raw entry against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.ALL)
def test_raw_entry_equals_the_model(eng, key):
    G, coef = K.inputs(key)
    for gamma in K.GAMMAS:
        for max_iter in K.MAX_ITERS:
            out, trace = _model(key, gamma, max_iter)
            dev = dict(zip(NAMES, _device(eng, G, coef, gamma, K.THRESHOLD, max_iter)))
            assert dev["xi"].shape == (1, coef.d, coef.p) and dev["var"].shape == (1, C.matrices(coef)[0].shape[1])
            for name in ("passes", "near", "fell", "trunc", "rank"):
                assert dev[name].tolist() == [out[name]], (key, gamma, max_iter, name, dev[name], out[name])
            assert out["fell"] == 0 and np.array_equal(dev["mask"][0], out["mask"]), (key, gamma, max_iter)
            bx, bv, cond = _bounds(out, trace, coef)
            ex = np.abs(dev["xi"][0].astype(np.float64) - out["xi"])
            ev = np.abs(dev["var"][0].astype(np.float64) - out["var"])
            print(key, gamma, max_iter, "passes", out["passes"], "trunc", out["trunc"], "rank", out["rank"], "cond %.3g" % cond,
                  "max |dXi| / bound %.3g" % (ex / bx).max(),
                  "bit-equal", dev["xi"][0].tobytes() == out["xi"].tobytes() and dev["var"][0].tobytes() == out["var"].tobytes())
            assert (ex <= bx).all() and (ev <= bv).all(), (key, gamma, max_iter, ex.max(), ev.max())
    if key in K.TRUNCATED:
        assert _model(key, 0.0, 10)[0]["trunc"] >= 1


# ---- 2. full rank: the existing entry, byte for byte ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.FULL)
def test_a_full_rank_problem_is_the_existing_entrys_byte_for_byte(eng, key):
    G, coef = K.inputs(key)
    for gamma in K.GAMMAS:
        for max_iter in K.MAX_ITERS:
            new = dict(zip(NAMES, _device(eng, G, coef, gamma, K.THRESHOLD, max_iter)))
            old = dict(zip(NAMES, _device(eng, G, coef, gamma, K.THRESHOLD, max_iter, entry="constrained")))
            assert old["fell"].tolist() == [0] and new["fell"].tolist() == [0] and new["trunc"].tolist() == [0]
            for name in ("xi", "var", "mask", "passes", "near"):
                assert new[name].tobytes() == old[name].tobytes(), (key, gamma, max_iter, name)


# ---- 3. tables -----------------------------------------------------------------------------------------------------------------
def test_a_table_problem_is_the_scalar_launch_on_its_set(eng):
    coef = C.coef_map("so2_o3_cc1")
    G = np.stack([C.rankdef_gram(), C.gram("so2_o3_cc1")[0]])
    W, T = (0.0, float(np.float32(0.1))), (float(np.float32(0.05)), K.THRESHOLD)
    table = torch.tensor([[w, t] for w in W for t in T for _ in range(2)], dtype=torch.float32)         # 8 problems on 2 sets
    grid = _device(eng, G, coef, -1.0, -1.0, 10, hyper=table.to(DEV))
    assert grid[0].shape == (8, 2, 10) and grid[5].shape == (8, 4) and grid[6].shape == (8,)
    again = _device(eng, G, coef, -1.0, -1.0, 10, hyper=table.to(DEV))
    for name, a, b in zip(NAMES, grid, again):
        assert a.tobytes() == b.tobytes(), name
    for g in range(4):                                                  # four scalar launches over the two sets
        one = _device(eng, G, coef, float(table[2 * g, 0]), float(table[2 * g, 1]), 10)
        assert not one[4].any()
        for name, a, b in zip(NAMES, grid, one):
            assert a[2 * g:2 * g + 2].tobytes() == b.tobytes(), (g, name)
    assert grid[6][0] > 0 and grid[6][1] == 0                           # the rank-deficient set is truncated, the other is not


# ---- 4. solve(min_norm=True) against the flag-and-host route -------------------------------------------------------------------
def _sweep_on(eng, G, d, order):
    """A SeedSweepSTLSQ whose matrices are handed in on the host (the device route uploads exactly these)."""
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d, device=DEV), torch.zeros(8, d, device=DEV), order, n_seeds=S, engine=eng,
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.ascontiguousarray(G), K.N_POINTS
    replays = []
    inner = sw._replay
    sw._replay = lambda s, *a: (replays.append(s), inner(s, *a))[1]
    return sw, replays


def _solve(sw, *a, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, passes = sw.solve(*a, **kw)
    return Xi.numpy(), mask.numpy() > 0, np.asarray(passes), [str(w.message) for w in rec if w.category is RuntimeWarning]


@pytest.mark.parametrize("keys, order", [(("rankdef", "so2_o3_cc1"), 3), (("negdet_o2_cc1",), 2), (("so3a_o2",), 2)])
def test_solve_with_min_norm_equals_the_flag_and_host_route(eng, keys, order):
    coef = K.inputs(keys[0])[1]
    G = np.stack([K.inputs(k)[0] for k in keys])
    sw_old, replays_old = _sweep_on(eng, G, coef.d, order)
    old = _solve(sw_old, 0.0, K.THRESHOLD, max_iter=10, device=True, coef=coef)
    sw_new, replays_new = _sweep_on(eng, G, coef.d, order)
    new = _solve(sw_new, 0.0, K.THRESHOLD, max_iter=10, device=True, coef=coef, min_norm=True)
    assert old[3] == [WORDS] and new[3] == [WORDS]                      # exactly one warning, the existing words
    assert sw_new.near_threshold == [] and replays_new == [] and len(replays_old) >= 1
    assert sw_new.rank_truncated.tolist() == [k in K.TRUNCATED for k in keys]
    assert np.array_equal(new[1], old[1]) and np.array_equal(new[2], old[2])
    for k, key in enumerate(keys):
        out, trace = _model(key, 0.0, 10)
        bound = 2 * _bounds(out, trace, coef)[0]                        # two summation orders: twice the bound
        err = np.abs(new[0][k].astype(np.float64) - old[0][k])
        print(key, "max |dXi| / bound %.3g" % (err / bound).max())
        assert (err <= bound).all(), (key, err.max())


def test_hyper_tables_work_with_min_norm(eng):
    coef = C.coef_map("so2_o3_cc1")
    G = np.stack([C.rankdef_gram(), C.gram("so2_o3_cc1")[0]])
    plain = _solve(_sweep_on(eng, G, 2, 3)[0], 0.0, K.THRESHOLD, max_iter=10, device=True, coef=coef, min_norm=True)
    hyper = {"threshold": [K.THRESHOLD] * 2 + [0.5] * 2}
    grid = _solve(_sweep_on(eng, G, 2, 3)[0], 0.0, 7.0, max_iter=10, device=True, hyper=hyper, coef=coef, min_norm=True)
    assert grid[0].shape == (4, 2, 10) and grid[0][:2].tobytes() == plain[0].tobytes() and grid[1][:2].tobytes() == plain[1].tobytes()


# ---- 5. main_sweep --min_norm_stlsq ------------------------------------------------------------------------------------------------
def _main(tmp, argv):
    from symode_amd import main_sweep
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        return main_sweep.main(list(argv))
    finally:
        os.chdir(cwd)


# dosc is linear and so(2)-equivariant: at order 3 the first thresholding leaves the linear terms, on which Q's columns span two
# directions only (tests/stlsq_constrained_cases.rankdef on real data) -- the run without the flag flags its seeds
ARGV = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--w_sym_reg", "0.0",
        "--lbfgs_subsample", "0.5", "--repr", "(1,so2)", "--group_idx", "0", "--latent_dim", "2", "--n_comps", "1",
        "--poly_order", "3", "--threshold", "0.05", "--w_sindy_reg", "0.25", "--num_epochs", "10", "--seed", "4", "--n_seeds", "4",
        "--device_stlsq", "--equiv_stlsq", "--eq_constraint"]
LINE = "rank-truncated passes (minimum-norm solution inside the launch): "


@pytest.fixture()
def small_dosc(monkeypatch):
    from symode_amd import dataset as D
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)


def test_main_sweep_min_norm_stlsq_is_the_run_without_the_flag(eng, tmp_path, small_dosc, capsys, monkeypatch):
    seen = {}
    launch = eng.stlsq_sweep_constrained

    def spy(G, *a, **kw):
        out = launch(G, *a, **kw)
        seen.update(G=G.cpu().numpy(), fell=np.array(out[4]), n_points=a[0], gamma=a[1], thr=a[2], max_iter=a[3],
                    q=(a[4].cpu().numpy(), a[5].cpu().numpy()), allow_constant=a[6], d=kw["d"])
        return out

    monkeypatch.setattr(eng, "stlsq_sweep_constrained", spy)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        old = _main(tmp_path, ARGV + ["--save_dir", "flagged"])
        out_old = capsys.readouterr().out
        monkeypatch.setattr(eng, "stlsq_sweep_constrained", launch)
        new = _main(tmp_path, ARGV + ["--save_dir", "minnorm", "--min_norm_stlsq"])
        out_new = capsys.readouterr().out
    assert old["n_runs"] == new["n_runs"] == 4
    # the run without the flag flags at least one seed: through the raw entry on one seed's matrix
    assert seen["fell"].any(), seen["fell"]
    s = int(np.nonzero(seen["fell"])[0][0])
    qs, qx = seen["q"]
    gamma, thr, d, p = seen["gamma"], seen["thr"], seen["d"], 10
    assert (gamma, thr, seen["max_iter"], d) == (float(np.float32(0.25)), float(np.float32(0.05)), 10, 2)
    one = eng.stlsq_sweep_constrained(torch.from_numpy(seen["G"][s:s + 1]).to(DEV), seen["n_points"], gamma, thr, 10,
                                      torch.from_numpy(qs).to(DEV), torch.from_numpy(qx).to(DEV), seen["allow_constant"], d=d,
                                      pivot_floor=M0.PIVOT_FLOOR, near_band=K.BAND)
    assert one[4].cpu().tolist() == [1]
    # the summary line
    assert LINE not in out_old and LINE in out_new
    count = int(out_new.split(LINE)[1].split(" of ")[0])
    assert count >= int(seen["fell"].sum()) >= 1 and f"{LINE}{count} of 4 problems" in out_new
    # masks equal, coefficients within twice the bound of the model's last pass
    for k, seed in enumerate((4, 5, 6, 7)):
        want = np.load(tmp_path / "eval_results" / "flagged" / f"seed{seed}.npz")["coefficients"]
        got = np.load(tmp_path / "eval_results" / "minnorm" / f"seed{seed}.npz")["coefficients"]
        assert np.array_equal(got != 0, want != 0), seed
        trace = []
        out = M.sweep(seen["G"][k], d, gamma, thr, 10, qs, qx, seen["allow_constant"], band=K.BAND, trace=trace)
        info, Gq = trace[-1][5], trace[-1][2]
        cond, n = M.pass_cond(info, Gq), info["n"]
        assert cond <= K.COND_BOUND
        which = M if info["rank"] < n else M0
        bound = 2 * which.xi_bound(qx, out["var"], cond, n, d, p, seen["allow_constant"])
        err = np.abs(got.astype(np.float64) - want)
        print("seed", seed, "fell", seen["fell"][k], "trunc", out["trunc"], "rank", out["rank"], "cond %.3g" % cond,
              "max |dXi| / bound %.3g" % (err / bound).max())
        assert (err <= bound).all(), (seed, err.max())
