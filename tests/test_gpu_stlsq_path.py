"""The sparsity path on the device (symode_stlsq_path, engine.stlsq_path, SeedSweepSTLSQ.solve_path, main_sweep --stlsq_path)
against the numpy model of the kernel (tests/stlsq_path_model.py) on the deck of tests/stlsq_path_cases.py.

Integer outputs and masks must be EQUAL; the floats are held to the derived bounds of tests/test_host_stlsq_path_model.py (the
coefficients against the dense fp64 reference, 4 n^2 cond(A) 2^-53 |x|_max + 2^-24 |x| per step; the errors against the
np.longdouble quadratic form of the launch's own coefficients, (n + 2)^2 2^-53 (Hyy + 2 |w|^T |c| + |w|^T |H| |w|)).  That test
asserts, without a GPU, the conditions under which equal decisions are a fair demand: every elimination and every comparison
behind ``best`` is decided by at least 100 such bounds.  Whether the bytes were in fact equal is printed (profiles/stlsq_path.txt).
Launches against launches (geometry, repeats, step 0 against symode_stlsq_sweep) are bit for bit."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import stlsq_path_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("Xi", "mask", "order", "rss_train", "rss_val", "best", "near", "fell", "path_xi")
IDS = [f"{name}-g{gamma}-tol{tol}" for name, gamma, tol in P.RUNS]


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _launch(eng, G, V, d, gamma, tol, n_problems=None):
    """engine.stlsq_path on host matrices: every output as a numpy array."""
    o = eng.stlsq_path(torch.from_numpy(np.ascontiguousarray(G)).to(DEV), torch.from_numpy(np.ascontiguousarray(V)).to(DEV), 200, gamma, tol,
                       P.FLOOR_REL, n_problems, d=d, near_band=P.BAND)
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same_bytes(a, b, keys=KEYS):
    return [k for k in keys if a[k].tobytes() != b[k].tobytes()]


# ---- 1. the raw entry against the model, the whole deck ---------------------------------------------------------------------------
@pytest.mark.parametrize("name, gamma, tol", P.RUNS, ids=IDS)
def test_raw_entry_against_the_model(eng, name, gamma, tol):
    d, G, V, _, _ = P.case(name)
    m, r = P.model(name, gamma, tol), P.reference(name, gamma, tol)
    o = _launch(eng, G, V, d, gamma, tol)
    S, p = G.shape[0], G.shape[1] - d
    assert o["path_xi"].shape == (S, d, p + 1, p) and o["rss_val"].shape == (S, d, p + 1) and o["order"].shape == (S, d, p)
    assert not o["fell"].any() and not m["fell"].any()
    print(name, gamma, tol, "p", p, "d", d, "outputs that differ from the model in a byte:", _same_bytes(o, {**m, "mask": m["mask"].astype(np.uint8)}) or "none")
    for key in ("order", "best", "near"):
        assert np.array_equal(o[key], m[key]), key
    assert np.array_equal(o["mask"].astype(bool), m["mask"])
    assert (np.abs(o["path_xi"].astype(np.float64) - r["x"]) <= r["coef_bound"]).all()
    for s in range(S):
        for j in range(d):
            for t in range(p + 1):
                v = o["path_xi"][s, j, t].astype(np.float64)
                for key, H in (("rss_train", G[s]), ("rss_val", V[s % V.shape[0]])):
                    assert abs(o[key][s, j, t] - P._quad(H, p, j, v)) <= P.err_bound(H, p, j, v), (key, s, j, t)
            assert o["Xi"][s, j].tobytes() == o["path_xi"][s, j, o["best"][s, j]].tobytes()             # the chosen step, bit for bit
            assert np.array_equal(np.sort(o["order"][s, j, o["best"][s, j]:]), np.nonzero(o["mask"][s, j])[0])


# ---- 2. step 0 is one pass of the threshold-loop kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.DECK))
def test_step_0_is_one_pass_of_the_threshold_loop_launch(eng, name):
    d, G, V, _, _ = P.case(name)
    for gamma in P.DECK[name][2]:
        o = _launch(eng, G, V, d, gamma, P.DECK[name][3][0])
        xi = eng.stlsq_sweep(torch.from_numpy(G).to(DEV), 200, gamma, 0.0, 1, d=d, near_band=P.BAND)[0].cpu().numpy()
        assert o["path_xi"][:, :, 0, :].tobytes() == xi.tobytes(), (name, gamma)


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------------
def test_sets_validation_sets_and_problems(eng):
    d, G, V, _, _ = P.case("o3")
    assert G.shape[0] == V.shape[0] == 3
    each = _launch(eng, G, V, d, 0.1, P.TOL_DEFAULT)                                     # n_sets = n_val_sets = n_problems = 3
    again = _launch(eng, G, V, d, 0.1, P.TOL_DEFAULT)
    assert not _same_bytes(each, again)                                                  # a second launch: equal bytes
    shared = _launch(eng, G, V[1:2], d, 0.1, P.TOL_DEFAULT)                              # n_val_sets = 1: every problem on V[1]
    for k in range(3):
        one = _launch(eng, G[k:k + 1], V[1:2], d, 0.1, P.TOL_DEFAULT)
        assert not _same_bytes({key: v[k:k + 1] for key, v in shared.items()}, one), k
    assert not _same_bytes({key: v[1:2] for key, v in shared.items()}, {key: v[1:2] for key, v in each.items()})
    assert shared["rss_val"][0].tobytes() != each["rss_val"][0].tobytes()                # ... and V[1] is not V[0]
    assert shared["rss_train"].tobytes() == each["rss_train"].tobytes() and shared["order"].tobytes() == each["order"].tobytes()
    many = _launch(eng, G, V, d, 0.1, P.TOL_DEFAULT, n_problems=27)                      # 27 problems on 3 + 3 sets
    assert many["Xi"].shape == (27, 2, 10) and not many["fell"].any()
    for s in range(27):
        one = _launch(eng, G[s % 3:s % 3 + 1], V[s % 3:s % 3 + 1], d, 0.1, P.TOL_DEFAULT)
        assert not _same_bytes({key: v[s:s + 1] for key, v in many.items()}, one), s
    two_val = _launch(eng, G, V[:2], d, 0.1, P.TOL_DEFAULT)                              # n_val_sets = 2: problem 2 on V[0]
    assert two_val["rss_val"][2].tobytes() == _launch(eng, G[2:], V[:1], d, 0.1, P.TOL_DEFAULT)["rss_val"][0].tobytes()


def test_the_largest_and_the_smallest_system(eng):
    """p = 64, d = 4: 131 KiB of LDS, the attribute path of the launcher, every lane a column; p = 1: one step and the empty model."""
    from symode_amd import SymodeError
    d, G, V, _, _ = P.case("pd_p64_d4")
    o = _launch(eng, G, V, d, 0.1, P.TOL_DEFAULT)
    m = P.model("pd_p64_d4", 0.1, P.TOL_DEFAULT)
    assert o["path_xi"].shape == (1, 4, 65, 64) and np.array_equal(o["order"], m["order"]) and np.array_equal(o["best"], m["best"])
    assert sorted(o["order"][0, 0].tolist()) == list(range(64)) and (o["path_xi"][0, :, 64] == 0).all()
    d, G, V, _, _ = P.case("p1")
    o = _launch(eng, G, V, d, 0.0, 0.0)
    assert o["path_xi"].shape == (3, 2, 2, 1) and (o["order"] == 0).all() and (o["path_xi"][:, :, 1] == 0).all()
    assert np.array_equal(o["rss_val"][:, :, 1], V[:, [1, 2], [1, 2]])                   # the empty model's error is Vyy itself
    with pytest.raises(SymodeError):
        eng.stlsq_path(torch.zeros(1, 69, 69, dtype=torch.float64, device=DEV), torch.zeros(1, 69, 69, dtype=torch.float64, device=DEV),
                       10, 0.0, 0.0, 0.0, d=4)                                           # p = 65
    with pytest.raises(SymodeError):
        eng.stlsq_path(torch.from_numpy(G).to(DEV), torch.from_numpy(V[:, :2, :2].copy()).to(DEV), 10, 0.0, 0.0, 0.0, d=d)


# ---- 4. a singular support --------------------------------------------------------------------------------------------------------
def _sweep_on(eng, G, d, n_points=200):
    """A SeedSweepSTLSQ whose matrices are handed in on the host (the device route uploads exactly these)."""
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d, device=DEV), torch.zeros(8, d, device=DEV), 1, n_seeds=S, engine=eng,
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    sw.p, sw._gram, sw.n_points = G.shape[1] - d, np.ascontiguousarray(G), n_points
    return sw


def _duplicate_columns():
    """2 sets, p = 3, d = 1, small integers (exact in fp64).  Set 1: column 1 repeats column 0 (norm^2 16, a square: the first
    pivot leaves its twin's diagonal at exactly 0), column 2 is orthogonal to both.  Set 0 is regular."""
    c0, c2 = np.array([2.0, 2.0, 2.0, 2.0]), np.array([1.0, -1.0, 1.0, -1.0])
    regular = np.stack([c0, np.array([1.0, 0.0, -1.0, 2.0]), c2, 1.0 * c0 + 2.0 * c2 + np.array([0.0, 1.0, 0.0, 0.0])], axis=1)
    twin = np.stack([c0, c0, c2, 1.0 * c0 + 2.0 * c2], axis=1)
    G = np.stack([regular.T @ regular, twin.T @ twin])
    val = np.stack([c2 + c0, c0, c2, 2.0 * c0 + 3.0 * c2 + np.array([1.0, 0.0, 0.0, 0.0])], axis=1)
    return G, (val.T @ val)[None]


def test_a_singular_support_falls_to_the_host_twin(eng):
    G, V = _duplicate_columns()
    o = _launch(eng, G, V, 1, 0.0, 0.0)
    assert o["fell"].tolist() == [0, 1]
    assert not _launch(eng, G, V, 1, 0.5, 0.0)["fell"].any()                             # a ridge makes it regular
    alone = _launch(eng, G[:1], V, 1, 0.0, 0.0)
    assert not _same_bytes({k: v[:1] for k, v in o.items()}, alone)                      # the neighbour is solved as it is alone
    runs = {}
    for device in (True, False):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            Xi, mask, record = _sweep_on(eng, G, 1, 4).solve_path(0.0, V, 0.0, device=device, keep_path=True)
        runs[device] = (Xi.numpy(), mask.numpy(), record, [str(w.message) for w in rec if w.category is RuntimeWarning])
    dev, host = runs[True], runs[False]
    assert "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead" in dev[3]
    assert dev[0][1].tobytes() == host[0][1].tobytes() and np.array_equal(dev[1][1], host[1][1])        # the twin's own answer
    for k in ("order", "rss_train", "rss_val", "best", "near", "path_xi"):
        assert dev[2][k][1].tobytes() == host[2][k][1].tobytes(), k
    assert np.isfinite(dev[0]).all() and abs(dev[2]["path_xi"][1, 0, 0, 0] - dev[2]["path_xi"][1, 0, 0, 1]) < 1e-6   # minimum norm
    assert np.array_equal(dev[1][0], host[1][0]) and np.array_equal(dev[2]["order"][0], host[2]["order"][0])


# ---- 5. solve_path(device=True) against device=False ------------------------------------------------------------------------------
@pytest.mark.parametrize("name, gamma, tol", [("o5", 0.0, P.TOL_DEFAULT), ("d3_o2_exp", 0.1, 0.0), ("zero_rhs", 0.1, P.TOL_DEFAULT)])
def test_solve_path_on_the_device_equals_the_host_twin(eng, name, gamma, tol):
    d, G, V, _, _ = P.case(name)
    r = P.reference(name, gamma, tol)
    sw = _sweep_on(eng, G, d)
    on_dev = sw.solve_path(gamma * gamma, torch.from_numpy(V).to(DEV), tol, keep_path=True)
    on_host = sw.solve_path(gamma * gamma, V, tol, device=False, keep_path=True)
    assert sw.grams(device=True).is_cuda and on_dev[0].dtype == on_host[0].dtype == torch.float32
    assert torch.equal(on_dev[1], on_host[1]) and sorted(on_dev[2]) == sorted(on_host[2])
    for k in ("order", "best", "near"):
        assert np.array_equal(on_dev[2][k], on_host[2][k]), k
    for fit in (on_dev, on_host):                                                        # both within the bound of the reference
        assert (np.abs(fit[2]["path_xi"].astype(np.float64) - r["x"]) <= r["coef_bound"]).all()
    at = on_dev[2]["best"][:, :, None, None].astype(np.int64)
    assert np.array_equal(on_dev[0].numpy(), np.take_along_axis(on_dev[2]["path_xi"], at, 2)[:, :, 0])
    assert "path_xi" not in sw.solve_path(gamma * gamma, V[:1], tol)[2]                  # fetched on request only


# ---- 6. main_sweep --stlsq_path ---------------------------------------------------------------------------------------------------
N_SEEDS = 8
ARGV = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--w_sym_reg", "0.0", "--lbfgs_subsample", "0.5",
        "--poly_order", "3", "--threshold", "0.05", "--w_sindy_reg", "0.01", "--num_epochs", "10", "--seed", "4"]
FLAGS = ["--method", "stlsq", "--device_stlsq", "--stlsq_path", "--n_seeds", str(N_SEEDS)]


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


@pytest.fixture(scope="module")
def small_dosc(tmp_path_factory):
    """6 + 3 trajectories x 200 samples of the damped oscillator, in the data files the drivers (and their ranks) load."""
    from symode_amd import dataset as D
    from symode_amd.parser_utils import get_args
    tmp = tmp_path_factory.mktemp("stlsq-path-dosc")
    cwd, old, old_dt = os.getcwd(), D._RECIPES["dosc"], D.ode_dt_dict["dosc"]
    os.chdir(tmp)
    D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = (6, 3, 600, 3, 0.01), 0.03
    try:
        D.get_dataset(vars(get_args(argv=list(ARGV))))
        yield tmp
    finally:
        D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = old, old_dt
        os.chdir(cwd)


def _files(tmp, save_dir):
    d = tmp / "eval_results" / save_dir
    return d, np.stack([np.load(d / f"seed{s}.npz")["coefficients"] for s in range(4, 4 + N_SEEDS)]), np.load(d / "path.npz")


def test_main_sweep_stlsq_path_is_solve_path(eng, small_dosc, capsys, monkeypatch):
    from symode_amd import main_sweep
    from symode_amd.sweep import SeedSweepSTLSQ
    seen = {}
    solve_path = SeedSweepSTLSQ.solve_path

    def recorded(self, *a, **kw):
        seen.update(sw=self, a=a, kw=kw)
        return solve_path(self, *a, **kw)

    monkeypatch.setattr(SeedSweepSTLSQ, "solve_path", recorded)
    monkeypatch.setattr(SeedSweepSTLSQ, "solve", lambda *a, **k: pytest.fail("the threshold loop ran"))
    res = _main(small_dosc, ARGV + FLAGS + ["--save_dir", "path"])
    out = capsys.readouterr().out
    monkeypatch.undo()
    sw, (w_reg, V, tol) = seen["sw"], seen["a"]
    assert (w_reg, tol, seen["kw"]) == (0.01, main_sweep.PATH_TOL, {}) and tuple(V.shape) == (1, 12, 12) and V.is_cuda
    assert res["n_runs"] == N_SEEDS and (sw.S, sw.d, sw.p) == (N_SEEDS, 2, 10)
    d, coefs, path = _files(small_dosc, "path")
    assert sorted(f.name for f in d.iterdir()) == sorted([f"seed{s}.npz" for s in range(4, 4 + N_SEEDS)] + ["path.npz"])
    assert sorted(np.load(d / "seed4.npz").files) == ["coefficients", "correct_form", "correct_form_all", "mse", "mse_all"]
    Xi, mask, record = sw.solve_path(w_reg, V, tol)                                      # called directly, on the same matrices
    assert coefs.tobytes() == (Xi.numpy() * mask.numpy()).astype(coefs.dtype).tobytes()
    assert sorted(path.files) == ["best", "order", "path_tol", "rss_train", "rss_val", "seeds"]
    for k in ("order", "rss_train", "rss_val", "best"):
        assert path[k].tobytes() == record[k].tobytes() and path[k].shape[0] == N_SEEDS, k
    assert path["seeds"].tolist() == list(range(4, 4 + N_SEEDS)) and float(path["path_tol"]) == main_sweep.PATH_TOL
    assert np.array_equal(coefs != 0, (mask.numpy() > 0) & (Xi.numpy() != 0))
    size = 10 - record["best"]
    lines = out.splitlines()
    assert (f"{N_SEEDS} seeds x 600 points (over 1 rank(s)), sparsity path of 11 models per row, scored on 600 validation points, "
            f"path_tol {main_sweep.PATH_TOL:g}") in lines
    assert ("chosen support size per row: " + ", ".join(f"row {j}: {size[:, j].min()}-{size[:, j].max()}" for j in range(2))) in lines
    assert f"near-tie eliminations: {int((record['near'] > 0).sum())} of {N_SEEDS} problems" in lines
    assert "--threshold (0.05) is not used by the path" in lines
    # the host twin takes the same decisions on these matrices, and the tolerance is the flag's
    host = sw.solve_path(w_reg, V, tol, device=False)
    assert torch.equal(host[1], mask) and np.array_equal(host[2]["best"], record["best"]) and np.array_equal(host[2]["order"], record["order"])
    _main(small_dosc, ARGV + FLAGS + ["--save_dir", "path-tol", "--path_tol", "0.5"])
    capsys.readouterr()
    loose = _files(small_dosc, "path-tol")[2]
    assert float(loose["path_tol"]) == 0.5 and loose["rss_val"].tobytes() == path["rss_val"].tobytes()
    assert (loose["best"] >= path["best"]).all() and (loose["best"] > path["best"]).any()


def test_main_sweep_stlsq_path_with_eval_ltp(eng, small_dosc, capsys):
    res = _main(small_dosc, ARGV + FLAGS + ["--save_dir", "path-ltp", "--eval_ltp"])
    out = capsys.readouterr().out
    d, coefs, path = _files(small_dosc, "path-ltp")
    assert res["n_runs"] == N_SEEDS and "seeds by median roll-out error on the validation trajectories" in out
    got = np.load(d / "seed4.npz")
    assert {"ltp_mean_error", "ltp_horizon", "val_mse"} <= set(got.files) and np.isfinite(got["val_mse"])
    _main(small_dosc, ARGV + FLAGS + ["--save_dir", "path-plain"])                       # the fit does not depend on the scoring
    capsys.readouterr()
    plain = _files(small_dosc, "path-plain")
    assert coefs.tobytes() == plain[1].tobytes() and path["best"].tobytes() == plain[2]["best"].tobytes()


def test_two_ranks_equal_one_rank(eng, small_dosc):
    from tests.test_gpu_sym_sweep import _free_port, _rank
    _main(small_dosc, ARGV + FLAGS + ["--save_dir", "one-rank"])
    mp.spawn(_rank, args=(2, _free_port(), str(small_dosc), ARGV + FLAGS + ["--save_dir", "two-ranks"], str(small_dosc / "allreduce-path")),
             nprocs=2, join=True)
    (_, one, p1), (_, two, p2) = _files(small_dosc, "one-rank"), _files(small_dosc, "two-ranks")
    assert np.array_equal(one != 0, two != 0) and np.array_equal(p1["best"], p2["best"]) and np.array_equal(p1["order"], p2["order"])
    assert np.allclose(one, two, rtol=1e-5, atol=1e-5 * np.abs(one).max())               # fp64 Gram sums differ in the last bits only
    assert [int(open(small_dosc / f"allreduce-path.{r}").read()) for r in range(2)] == [2, 2]     # matrices and count: nothing for V
