"""The sparsity path with the reversed symmetry regulariser on the device (symode_stlsq_path_symreg, engine.stlsq_path_symreg,
SeedSweepSTLSQ.solve_path(rev=...), main_sweep --symreg_path) against the numpy model of the kernel (tests/stlsq_path_symreg_model.py) on the deck of
tests/stlsq_path_symreg_cases.py; against symode_stlsq_sweep_symreg at step 0; against symode_stlsq_path at w_sym = 0; and
against the host twin.

Integer outputs and masks must be EQUAL.  The floats are held to derived bounds, not measured ones:
  path_xi, xi_out   against the dense fp64 solve of the step's system: 4 n^2 cond(A) 2^-53 |v|_max + 2^-24 |v| per coefficient
                    (the bound tests/test_gpu_stlsq_symreg.py derives: the backward-stable Cholesky solve, then the rounding
                    to fp32);
  mse_train, mse_val against the np.longdouble form of the launch's OWN coefficients: per row (n_j + 2)^2 2^-53 (Hyy +
                    2 |w|^T |c| + |w|^T |H| |w|) -- n_j + 2 terms per sum, two nested sums, the bound of
                    tests/test_gpu_stlsq_path.py -- summed over the rows, plus d 2^-53 of the same magnitudes for the d
                    additions of the rows' terms (``P.mse_bound``);
  reg_train         likewise (n + 2)^2 2^-53 |v|^T |R| |v| (``P.reg_bound``).
tests/test_host_stlsq_path_symreg_model.py asserts, without a GPU, the conditions under which equal decisions are a fair
demand: cond(A) <= 1e6, every elimination and every comparison behind ``best`` decided by at least 100 such bounds (the tie
and the zero right-hand side are decided by index).  Model and kernel perform the same operations in the same order, so equal
bytes are expected and printed.  Launches against launches (step 0, tables, repeats) are bit for bit."""
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import stlsq_path_symreg_cases as P
from tests import stlsq_path_symreg_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("Xi", "mask", "order", "mse_train", "reg_train", "mse_val", "best", "near", "fell", "path_xi")


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[None])).to(DEV)


def _launch(eng, G, R, V, d, gamma, w_sym, tol, **kw):
    """engine.stlsq_path_symreg on host matrices: every output as a numpy array."""
    o = eng.stlsq_path_symreg(_dev(G), _dev(R), _dev(V), P.N_POINTS, gamma, w_sym, tol, P.FLOOR_REL, d=d, pivot_floor=M.PIVOT_FLOOR,
                              near_band=P.BAND, **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}


def _differ(a, b, keys=KEYS):
    return [k for k in keys if a[k].tobytes() != b[k].tobytes()]


def _one(o, s):
    return {k: v[s:s + 1] for k, v in o.items()}


# ---- 1. the raw entry against the model, the whole deck ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.DECK)
def test_raw_entry_against_the_model(eng, name):
    G, R, V, d = P.case(name)
    p = G.shape[0] - d
    n0 = d * p
    equal = 0
    for gamma, w_sym in P.CONFIGS:
        x, bound = P.reference(name, gamma, w_sym)
        for tol in P.TOLS:
            m = P.modelled(name, gamma, w_sym, tol)
            o = _launch(eng, G, R, V, d, gamma, w_sym, tol)
            assert o["path_xi"].shape == (1, n0 + 1, d, p) and o["order"].shape == (1, n0) and o["Xi"].shape == (1, d, p)
            for key in ("mse_train", "reg_train", "mse_val"):
                assert o[key].shape == (1, n0 + 1) and o[key].dtype == np.float64
            assert o["fell"].tolist() == [0] and m["fell"] == 0
            assert np.array_equal(o["order"][0], m["order"]) and o["best"][0] == m["best"] and o["near"][0] == m["near"], (name, gamma, w_sym, tol)
            assert np.array_equal(o["mask"][0].astype(bool), m["mask"])
            err = np.abs(o["path_xi"][0].astype(np.float64) - x)
            assert (err <= bound).all(), (name, gamma, w_sym, (err / np.where(bound > 0, bound, 1)).max())
            for t in range(n0 + 1):
                xi = o["path_xi"][0, t]
                assert abs(o["mse_train"][0, t] - P.quad(G, d, p, xi)) <= P.mse_bound(G, d, p, xi), (name, gamma, w_sym, t)
                assert abs(o["mse_val"][0, t] - P.quad(V, d, p, xi)) <= P.mse_bound(V, d, p, xi), (name, gamma, w_sym, t)
                vl = xi.reshape(-1).astype(np.longdouble)
                assert abs(o["reg_train"][0, t] - vl @ R.astype(np.longdouble) @ vl) <= P.reg_bound(R, xi), (name, gamma, w_sym, t)
            best = o["best"][0]
            assert o["Xi"][0].tobytes() == o["path_xi"][0, best].tobytes()                       # the chosen step, bit for bit
            assert np.array_equal(np.sort(o["order"][0, best:]), np.nonzero(o["mask"][0].reshape(-1))[0])
            assert not o["path_xi"][0, n0].any()
            want = {"Xi": m["Xi"], "mask": m["mask"].astype(np.uint8), "order": m["order"], "mse_train": m["mse_train"],
                    "reg_train": m["reg_train"], "mse_val": m["mse_val"], "path_xi": m["path_xi"]}
            off = [k for k in want if o[k][0].tobytes() != want[k].tobytes()]
            equal += not off
            print(name, "gamma", gamma, "w_sym", w_sym, "tol", tol, "n", n0, "best", best, "max |dXi| / bound %.3g" % (err / np.where(bound > 0, bound, 1)).max(),
                  "outputs that differ from the model in a byte:", off or "none")
    print(name, "bit-equal launches", equal, "of", len(P.CONFIGS) * len(P.TOLS))


# ---- 2. step 0 is one pass of the threshold-loop launch ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.DECK)
def test_step_0_is_one_pass_of_the_threshold_loop_launch(eng, name):
    G, R, V, d = P.case(name)
    for gamma, w_sym in P.CONFIGS:
        o = _launch(eng, G, R, V, d, gamma, w_sym, P.TOL_DEFAULT)
        xi = eng.stlsq_sweep_symreg(_dev(G), _dev(R), P.N_POINTS, gamma, 0.0, w_sym, 1, d=d, pivot_floor=M.PIVOT_FLOOR, near_band=P.BAND)[0]
        assert o["path_xi"][:, 0].tobytes() == xi.cpu().numpy().tobytes(), (name, gamma, w_sym)


# ---- 3. w_sym = 0 uncouples the rows: symode_stlsq_path ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.DECK)
def test_without_weight_the_rows_follow_the_plain_path(eng, name):
    G, R, V, d = P.case(name)
    p = G.shape[0] - d
    n0 = d * p
    for gamma in P.GAMMAS:
        g32 = M.f32(gamma)                                                               # what the regularised launch holds
        for R_any in (R, 3.0 * R + 1.0):                                                 # any finite R
            o = _launch(eng, G, R_any, V, d, g32, 0.0, P.TOL_DEFAULT)
            plain = eng.stlsq_path(_dev(G), _dev(V), P.N_POINTS, g32, P.TOL_DEFAULT, P.FLOOR_REL, d=d, near_band=P.BAND)
            plain = {k: v.cpu().numpy() for k, v in plain.items()}
            assert not o["fell"].any() and not plain["fell"].any()
            order = o["order"][0]
            _, bound = P.reference(name, gamma, 0.0)
            same = True
            for j in range(d):
                mine = [int(b) % p for b in order if int(b) // p == j]
                assert mine == plain["order"][0, j].tolist(), (name, gamma, j)            # row j's eliminations in the joint chain
                gone = 0
                for t in range(n0 + 1):
                    a, b = o["path_xi"][0, t, j], plain["path_xi"][0, j, gone]
                    assert (np.abs(a.astype(np.float64) - b) <= bound[t, j]).all(), (name, gamma, j, t)
                    same &= a.tobytes() == b.tobytes()
                    gone += t < n0 and int(order[t]) // p == j
            print(name, gamma, "coefficients bit-equal to symode_stlsq_path at matching supports:", same)


# ---- 4. tables, sets and repeats --------------------------------------------------------------------------------------------------
def test_a_table_problem_is_the_scalar_launch_on_its_set(eng):
    name, d = "osc_o3", 2
    pairs = [P.C.pair(name, v) for v in range(3)]
    G3, R3 = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
    V3 = np.stack([P.C.pair(name, v + 3)[0] for v in range(3)])
    rows = [[g, w] for g in (0.0, 0.1) for w in (0.0, 10.0) for _ in range(3)]            # 4 points x 3 sets = 12 problems
    table = torch.tensor(rows, dtype=torch.float32)
    grid = _launch(eng, G3, R3, V3, d, 7.0, 7.0, P.TOL_DEFAULT, hyper=table.to(DEV))
    assert grid["Xi"].shape == (12, 2, 10) and grid["order"].shape == (12, 20) and not grid["fell"].any()
    for s, (g, w) in enumerate(table.tolist()):
        k = s % 3
        one = _launch(eng, G3[k], R3[k], V3[k], d, g, w, P.TOL_DEFAULT)
        assert not _differ(_one(grid, s), one), (s, _differ(_one(grid, s), one))
    assert len({grid["order"][s].tobytes() for s in range(12)}) > 3                       # the points and the sets decide
    again = _launch(eng, G3, R3, V3, d, 7.0, 7.0, P.TOL_DEFAULT, hyper=table.to(DEV))
    assert not _differ(grid, again)                                                       # a second launch: equal bytes
    # without a table: problem s on set s % 3 and validation set s % n_val_sets
    many = _launch(eng, G3, R3, V3[:2], d, 0.1, 1.0, 0.0, n_problems=6)
    for s in range(6):
        one = _launch(eng, G3[s % 3], R3[s % 3], V3[s % 2], d, 0.1, 1.0, 0.0)
        assert not _differ(_one(many, s), one), s


def test_the_largest_and_the_smallest_system(eng):
    """n = 64: 130 KiB of LDS, the attribute path of the launcher, every lane an entry, 65 steps; n = 1: one step and the empty model."""
    from symode_amd import SymodeError
    for name in ("spd_d1_p64", "spd_d4_p16"):
        G, R, V, d = P.case(name)
        o = _launch(eng, G, R, V, d, 0.1, 1.0, P.TOL_DEFAULT)
        assert o["path_xi"].shape[:2] == (1, 65) and sorted(o["order"][0].tolist()) == list(range(64)) and not o["path_xi"][0, 64].any()
        again = _launch(eng, G, R, V, d, 0.1, 1.0, P.TOL_DEFAULT)
        assert not _differ(o, again)
    G, R, V, d = P.case("n1")
    o = _launch(eng, G, R, V, d, 0.0, 1.0, 0.0)
    assert o["path_xi"].shape == (1, 2, 1, 1) and o["order"].tolist() == [[0]] and o["mse_val"][0, 1] == V[1, 1]    # the empty model's error is Vyy itself
    with pytest.raises(SymodeError):
        eng.stlsq_path_symreg(torch.zeros(1, 35, 35, dtype=torch.float64, device=DEV), torch.zeros(1, 66, 66, dtype=torch.float64, device=DEV),
                              torch.zeros(1, 35, 35, dtype=torch.float64, device=DEV), 10, 0.0, 1.0, 0.0, 0.0, d=2, pivot_floor=M.PIVOT_FLOOR)   # d p = 66
    with pytest.raises(SymodeError):
        eng.stlsq_path_symreg(_dev(G), _dev(np.zeros((1, 2, 2))), _dev(V), 10, 0.0, 1.0, 0.0, 0.0, d=d, pivot_floor=M.PIVOT_FLOOR)


# ---- 5. the exactly singular pair -------------------------------------------------------------------------------------------------
def _sweep_on(eng, G, n_points, d, order):
    """A SeedSweepSTLSQ whose matrices are handed in on the host (the device route uploads exactly these)."""
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d, device=DEV), torch.zeros(8, d, device=DEV), order, n_seeds=S, engine=eng,
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.ascontiguousarray(G), n_points
    return sw


def _solve_path(sw, *a, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, record = sw.solve_path(*a, **kw)
    return Xi.numpy(), mask.numpy() > 0, record, [w for w in rec if w.category is RuntimeWarning]


def test_an_exactly_singular_pair_is_flagged_and_solved_on_the_host(eng, monkeypatch):
    from symode_amd import lstsq
    from symode_amd.sindy import stlsq_path_symreg_from_gram
    G0, R0, V, d = P.case("singular")
    assert _launch(eng, G0, R0, V, d, 0.0, 1.0, P.TOL_DEFAULT)["fell"].tolist() == [1]
    G1, R1, _, _ = P.case("osc_o2")
    both_G, both_R = np.stack([G0, G1]), np.stack([R0, R1])                               # ... next to a problem the device solves
    monkeypatch.setattr(lstsq, "_warned_singular", True)                                  # (the fallback's own warning: once per process)
    Xi, mask, rec, warned = _solve_path(_sweep_on(eng, both_G, P.N_POINTS, d, 2), 0.0, V[None], P.TOL_DEFAULT, keep_path=True, rev=(both_R, 1.0))
    assert len(warned) == 1
    assert "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead" == str(warned[0].message)
    xi, m, r = stlsq_path_symreg_from_gram(G0, R0, V, 0.0, 1.0, P.TOL_DEFAULT, P.FLOOR_REL, P.BAND, d, P.N_POINTS)
    assert Xi[0].tobytes() == xi.tobytes() and np.array_equal(mask[0], m) and not xi.any() and not m.any()
    for key in ("order", "mse_train", "reg_train", "mse_val", "best", "near", "path_xi"):
        assert np.asarray(rec[key][0]).tobytes() == np.asarray(r[key], dtype=rec[key].dtype).tobytes(), key
    one = _launch(eng, G1, R1, V, d, 0.0, 1.0, P.TOL_DEFAULT)
    assert Xi[1].tobytes() == one["Xi"][0].tobytes() and np.array_equal(rec["order"][1], one["order"][0]) and rec["best"][1] == one["best"][0]


# ---- 6. solve_path(device=True, rev=) against solve_path(device=False, rev=) ----------------------------------------------------
def test_solve_path_on_the_device_equals_solve_path_on_the_host(eng):
    name, d, S = "osc_o3", 2, 5
    pairs = [P.C.pair(name, v) for v in range(S)]
    G, R = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
    V = P.C.pair(name, 9)[0][None]
    w_reg, w_sym = 0.01, 10.0
    on_host = _solve_path(_sweep_on(eng, G, P.N_POINTS, d, 3), w_reg, V, P.TOL_DEFAULT, device=False, keep_path=True, rev=(R, w_sym))
    on_dev = _solve_path(_sweep_on(eng, G, P.N_POINTS, d, 3), w_reg, torch.from_numpy(V).to(DEV), P.TOL_DEFAULT, keep_path=True,
                         rev=(torch.from_numpy(R).to(DEV), w_sym))
    assert not on_host[3] and not on_dev[3]
    assert sorted(on_dev[2]) == sorted(on_host[2]) == ["best", "mse_train", "mse_val", "near", "order", "path_xi", "reg_train"]
    assert np.array_equal(on_dev[2]["order"], on_host[2]["order"]) and np.array_equal(on_dev[2]["best"], on_host[2]["best"])
    assert np.array_equal(on_dev[1], on_host[1]) and np.array_equal(on_dev[2]["near"], on_host[2]["near"])
    gamma = M.f32(np.sqrt(w_reg))
    for k in range(S):
        trace = []
        o = M.chain(G[k], R[k], V[0], d, gamma, w_sym, P.BAND, trace=trace)
        assert np.array_equal(on_dev[2]["order"][k], o["order"])
        for t, (active, A, b, sel) in enumerate(trace):
            cond = np.linalg.cond(A)
            assert cond <= P.COND_BOUND
            bound = M.xi_bound(o["path_xi"][t][active], cond, len(sel))
            dense = np.linalg.solve(A, b)
            dev_t, host_t = (side[2]["path_xi"][k, t][active].astype(np.float64) for side in (on_dev, on_host))
            assert (np.abs(dev_t - dense) <= bound).all() and (np.abs(host_t - dense) <= bound).all(), (k, t)   # each against the dense solve
            err = np.abs(dev_t - host_t)
            assert (err <= bound).all(), (k, t, (err / bound).max())                       # ... and device against host: the same bound
        assert on_dev[0][k].tobytes() == on_dev[2]["path_xi"][k, on_dev[2]["best"][k]].tobytes()
    # a table over the same seeds
    hyper = {"w_reg": [w_reg] * S + [0.0] * S, "w_sym": [w_sym] * S + [0.0] * S}
    grid = _solve_path(_sweep_on(eng, G, P.N_POINTS, d, 3), 5.0, V, P.TOL_DEFAULT, hyper=hyper, rev=(R, 99.0))
    assert grid[0].shape == (2 * S, d, 10) and grid[0][:S].tobytes() == on_dev[0].tobytes()
    assert np.array_equal(grid[2]["order"][:S], on_dev[2]["order"]) and not np.array_equal(grid[2]["order"][S:], grid[2]["order"][:S])
    # without rev the method is what it was
    plain = _solve_path(_sweep_on(eng, G, P.N_POINTS, d, 3), w_reg, V, P.TOL_DEFAULT)
    assert plain[2]["order"].shape == (S, d, 10) and sorted(plain[2]) == ["best", "near", "order", "rss_train", "rss_val"]


# ---- 7. main_sweep --symreg_path ---------------------------------------------------------------------------------------------------
N_SEEDS = 8
FLAGS = ["--method", "stlsq", "--device_stlsq", "--symreg_path", "--n_seeds", str(N_SEEDS)]


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
def small_lv(tmp_path_factory):
    """The small LV set of tests/test_gpu_sym_sweep.py with its frozen random LaLiGAN, in the files main.py writes."""
    from tests.test_gpu_sym_sweep import CASES, _prepare
    tmp = tmp_path_factory.mktemp("symreg-path-lv")
    _prepare(tmp, "lv")
    return tmp, list(CASES["lv"][0])


def _files(tmp, save_dir):
    d = tmp / "eval_results" / save_dir
    return d, np.stack([np.load(d / f"seed{s}.npz")["coefficients"] for s in range(N_SEEDS)]), np.load(d / "path.npz")


def test_main_sweep_symreg_path_is_solve_path_with_rev(eng, small_lv, capsys, monkeypatch):
    from symode_amd import main_sweep
    from symode_amd.sweep import SeedSweepSTLSQ
    tmp, argv = small_lv
    seen = {}
    solve_path = SeedSweepSTLSQ.solve_path

    def recorded(self, *a, **kw):
        seen.update(sw=self, a=a, kw=kw)
        return solve_path(self, *a, **kw)

    monkeypatch.setattr(SeedSweepSTLSQ, "solve_path", recorded)
    monkeypatch.setattr(SeedSweepSTLSQ, "solve", lambda *a, **k: pytest.fail("the threshold loop ran"))
    res = _main(tmp, argv + FLAGS + ["--save_dir", "path"])
    out = capsys.readouterr().out
    monkeypatch.undo()
    sw, (w_reg, V, tol), kw = seen["sw"], seen["a"], seen["kw"]
    assert tol == main_sweep.PATH_TOL and tuple(V.shape) == (1, 10, 10) and V.is_cuda and sorted(kw) == ["hyper", "rev"] and kw["hyper"] is None
    assert kw["rev"][1] == 0.1 / 1.0 and tuple(kw["rev"][0].shape) == (N_SEEDS, 16, 16)      # w_sym_reg / w_sindy_x
    assert res["n_runs"] == N_SEEDS and (sw.S, sw.d, sw.p) == (N_SEEDS, 2, 8)
    d, coefs, path = _files(tmp, "path")
    assert sorted(f.name for f in d.iterdir()) == sorted([f"seed{s}.npz" for s in range(N_SEEDS)] + ["path.npz"])
    assert sorted(np.load(d / "seed0.npz").files) == ["coefficients", "correct_form", "correct_form_all", "mse", "mse_all"]
    Xi, mask, record = sw.solve_path(w_reg, V, tol, rev=kw["rev"])                         # called directly, on the same matrices
    assert coefs.tobytes() == (Xi.numpy() * mask.numpy()).astype(coefs.dtype).tobytes()
    assert sorted(path.files) == ["best", "mse_train", "mse_val", "near", "order", "path_tol", "reg_train", "seeds"]
    for k in ("order", "mse_train", "reg_train", "mse_val", "best", "near"):
        assert path[k].tobytes() == record[k].tobytes() and path[k].shape[0] == N_SEEDS, k
    assert path["order"].shape == (N_SEEDS, 16) and path["mse_val"].shape == (N_SEEDS, 17)
    assert path["seeds"].tolist() == list(range(N_SEEDS)) and float(path["path_tol"]) == main_sweep.PATH_TOL
    size = 16 - record["best"]
    lines = out.splitlines()
    n_val = [ln for ln in lines if ln.startswith(f"{N_SEEDS} seeds x ")]
    assert len(n_val) == 1 and "regularised sparsity path of 17 models per problem (one chain over the 2 rows), scored on " in n_val[0]
    assert n_val[0].endswith(f"validation points, path_tol {main_sweep.PATH_TOL:g}") and "(over 1 rank(s))" in n_val[0]
    assert f"chosen support size: {size.min()}-{size.max()} of 16" in lines
    assert f"near-tie eliminations: {int((record['near'] > 0).sum())} of {N_SEEDS} problems" in lines
    assert "--threshold (0.15) is not used by the path" in lines
    # the host twin takes the same decisions on these matrices
    host = sw.solve_path(w_reg, V, tol, device=False, rev=kw["rev"])
    assert torch.equal(host[1], mask) and np.array_equal(host[2]["best"], record["best"]) and np.array_equal(host[2]["order"], record["order"])
    # the tolerance is the flag's, --eval_ltp goes through the unchanged tail and does not touch the fit
    _main(tmp, argv + FLAGS + ["--save_dir", "path-tol", "--path_tol", "0.5", "--eval_ltp"])
    assert "seeds by median roll-out error on the validation trajectories" in capsys.readouterr().out
    loose = _files(tmp, "path-tol")[2]
    assert float(loose["path_tol"]) == 0.5 and loose["mse_val"].tobytes() == path["mse_val"].tobytes()
    assert (loose["best"] >= path["best"]).all()
    assert {"ltp_mean_error", "ltp_horizon", "val_mse"} <= set(np.load(tmp / "eval_results" / "path-tol" / "seed0.npz").files)


def test_main_sweep_symreg_path_grid_is_the_scalar_run_at_every_point(eng, small_lv, capsys):
    tmp, argv = small_lv
    W, G_ = ("0.1", "5"), ("0", "0.01")
    res = _main(tmp, argv + FLAGS + ["--save_dir", "grid", "--stlsq_grid", "w_sym_reg=" + ",".join(W), "--stlsq_grid", "w_sindy_reg=" + ",".join(G_)])
    assert sorted(res) == [0, 1, 2, 3]
    listed = json.loads((tmp / "eval_results" / "grid" / "grid.json").read_text())
    assert listed["axes"] == [["w_sym_reg", [0.1, 5.0]], ["w_sindy_reg", [0.0, 0.01]]] and listed["n_seeds"] == N_SEEDS
    whole = np.load(tmp / "eval_results" / "grid" / "path.npz")
    assert whole["order"].shape == (4 * N_SEEDS, 16) and whole["best"].shape == (4 * N_SEEDS,)
    coefs = []
    for g, (w, r) in enumerate([(w, r) for w in W for r in G_]):                        # the first axis slowest
        point = list(argv)
        point[point.index("--w_sym_reg") + 1] = w
        scalar = _main(tmp, point + ["--w_sindy_reg", r] + FLAGS + ["--save_dir", f"point{g}"])
        assert repr(res[g]) == repr(scalar), g
        for s in range(N_SEEDS):
            want = np.load(tmp / "eval_results" / f"point{g}" / f"seed{s}.npz")
            got = np.load(tmp / "eval_results" / "grid" / f"grid{g}" / f"seed{s}.npz")
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            assert (float(got["w_sym_reg"]), float(got["w_sindy_reg"])) == (float(w), float(r)) and "threshold" not in got.files
        one = _files(tmp, f"point{g}")
        for key in ("order", "mse_train", "reg_train", "mse_val", "best", "near"):
            assert whole[key][g * N_SEEDS:(g + 1) * N_SEEDS].tobytes() == one[2][key].tobytes(), (g, key)
        coefs.append(one[1])
    out = capsys.readouterr().out
    assert "4 grid points on their Gram matrices" in out and "grid 3: chosen support size: " in out
    assert not np.array_equal(coefs[0], coefs[2])                                         # the points decide


def test_two_ranks_equal_one_rank_with_one_all_reduce(small_lv):
    from tests.test_gpu_sym_sweep import _free_port, _rank
    tmp, argv = small_lv
    _main(tmp, argv + FLAGS + ["--save_dir", "one-rank"])
    cnt = str(tmp / "allreduce-symreg-path")
    mp.spawn(_rank, args=(2, _free_port(), str(tmp), argv + FLAGS + ["--save_dir", "two-ranks"], cnt), nprocs=2, join=True)
    (_, one, p1), (_, two, p2) = _files(tmp, "one-rank"), _files(tmp, "two-ranks")
    assert np.array_equal(one != 0, two != 0) and np.array_equal(p1["best"], p2["best"]) and np.array_equal(p1["order"], p2["order"])
    assert np.allclose(one, two, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(one).max()))
    assert [int(open(f"{cnt}.{r}").read()) for r in range(2)] == [1, 1]                  # ONE collective of [G | R | count] per rank: nothing for V
