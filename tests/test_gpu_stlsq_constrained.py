"""The device STLSQ sweep under the equivariance constraint (symode_stlsq_sweep_constrained, engine.stlsq_sweep_constrained,
SeedSweepSTLSQ.solve(device=True, coef=...), main_sweep --equiv_stlsq) against tests/stlsq_constrained_model.py, the kernel's
algorithm in numpy, on the deck of tests/stlsq_constrained_cases.py; against the host loop; and against the reference's
recorded passes (tests/golden/f5_constraint.npz).

Bounds are derived, not measured (``M.xi_bound`` / ``M.var_bound``): the fp64 solve of Gq contributes 4 n^2 cond(Gq) 2^-53
max|beta| per variable, mapped through |q_xi|, the fp32 steps (rounding of the variables, r products and r + 1 additions per
entry of Xi) (r' + 2) 2^-24 (|q_xi| |beta32| + |const32|).  Model and kernel perform the same operations in the same order, so
equal bytes are expected and printed; the bound is what is asserted.  cond(Gq) <= 1e6, near == 0 and fell == 0 on the deck
are asserted by the CPU test (tests/test_host_stlsq_constrained_model.py) on the same inputs."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_cases as U
from tests import stlsq_constrained_cases as C
from tests import stlsq_constrained_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("xi", "mask", "passes", "near", "fell", "var")


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _device(eng, G, coef, gamma, threshold, max_iter, n_points=C.N_POINTS, **kw):
    qs, qx = (torch.from_numpy(q).to(DEV) for q in C.matrices(coef))
    G = torch.as_tensor(G).to(DEV)
    out = eng.stlsq_sweep_constrained(G if G.dim() == 3 else G[None], n_points, gamma, threshold, max_iter, qs, qx,
                                      coef.allow_constant, d=coef.d, pivot_floor=M.PIVOT_FLOOR, near_band=C.BAND, **kw)
    xi, mask, passes, near, fell, var = (t.cpu().numpy() for t in out)
    return xi, mask.astype(bool), passes, near, fell, var


@functools.lru_cache(maxsize=None)
def _model(key, gamma, max_iter):
    G, coef = _inputs(key)
    qs, qx = C.matrices(coef)
    trace = []
    out = M.sweep(G, coef.d, gamma, C.THRESHOLD, max_iter, qs, qx, coef.allow_constant, band=C.BAND, trace=trace)
    return out, trace


def _inputs(key):
    if key == "r64":
        return C.orthonormal_case()
    if key == "ortho_d3":
        return C.orthonormal_case(d=3, p=10, r=8, allow_constant=True, seed=6)
    return C.gram(key)[0], C.coef_map(key)


def _assert_as_the_model(dev, k, out, trace, coef, what):
    """Problem k of the launch ``dev`` against the model's ``out``."""
    assert dev[4][k] == out["fell"] and dev[2][k] == out["passes"], (what, dev[2][k], dev[4][k], out["passes"], out["fell"])
    if out["fell"]:
        return                                     # flagged: the other outputs are unspecified
    assert np.array_equal(dev[1][k], out["mask"]) and dev[3][k] == out["near"], what
    qx = coef.xi_matrix()
    cond = np.linalg.cond(trace[-1][2]) if len(trace[-1][4]) else 1.0
    n = len(trace[-1][4])
    bx, bv = M.xi_bound(qx, out["var"], cond, n, coef.d, coef.p, coef.allow_constant), M.var_bound(out["var"], cond, n)
    ex = np.abs(dev[0][k].astype(np.float64) - out["xi"])
    ev = np.abs(dev[5][k].astype(np.float64) - out["var"])
    print(what, "passes", out["passes"], "n", n, "cond %.3g" % cond, "max |dXi| / bound %.3g" % (ex / bx).max(),
          "bit-equal", dev[0][k].tobytes() == out["xi"].tobytes() and dev[5][k].tobytes() == out["var"].tobytes())
    assert (ex <= bx).all() and (ev <= bv).all(), (what, ex.max(), ev.max())


# ---- 1. the raw entry against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(C.DECK) + ["ortho_d3", "r64"])
def test_raw_entry_equals_the_model(eng, key):
    G, coef = _inputs(key)
    assert key != "r64" or (coef.r == 64 and coef.p == 41 and coef.d == 2)                # the lane limit at the largest compiled p
    for gamma in C.GAMMAS:
        for max_iter in C.MAX_ITERS:
            out, trace = _model(key, gamma, max_iter)
            dev = _device(eng, G, coef, gamma, C.THRESHOLD, max_iter)
            assert dev[0].shape == (1, coef.d, coef.p) and dev[5].shape == (1, C.matrices(coef)[0].shape[1])
            _assert_as_the_model(dev, 0, out, trace, coef, (key, gamma, max_iter))
            assert out["fell"] == (1 if key in C.FLAGGED and max_iter > 1 else 0)


def test_the_shapes_the_deck_is_meant_to_cover(eng):
    shapes = {(C.coef_map(k).d, C.coef_map(k).p) for k in C.DECK}
    assert {(2, 6), (2, 10), (3, 10)} <= shapes
    # r64: the largest p of the default build, with d = 2 (two rows of 41 columns hold the 64 orthonormal columns of Q; the
    # d = 2 libraries themselves end at p = 25, where d p < 64)
    assert max(eng.lib.symode_lib_size(d, o, f) for d in (1, 2, 3) for o in (1, 2, 3, 4, 5) for f in (0, 1, 2, 3)) == 41
    assert {C.coef_map(k).use_kron for k in C.SOLVED} == {True, False}
    assert {C.coef_map(k).allow_constant for k in C.SOLVED} == {True, False}
    assert max(_model(k, 0.0, 10)[0]["passes"] for k in C.SOLVED) >= 3


# ---- 2. the flagged case -------------------------------------------------------------------------------------------------------
def _sweep_on(eng, G, n_points, d, order):
    """A SeedSweepSTLSQ whose matrices are handed in on the host (the device route uploads exactly these)."""
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d, device=DEV), torch.zeros(8, d, device=DEV), order, n_seeds=S, engine=eng,
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.ascontiguousarray(G), n_points
    return sw


def _solve(sw, *a, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, passes = sw.solve(*a, **kw)
    return Xi.numpy(), mask.numpy() > 0, np.asarray(passes), list(sw.near_threshold), [w for w in rec if w.category is RuntimeWarning]


def test_the_rank_deficient_case_is_flagged_and_solved_on_the_host(eng):
    G, coef = C.rankdef_gram(), C.coef_map("so2_o3_cc1")
    dev = _device(eng, G, coef, 0.0, C.THRESHOLD, 10)
    assert dev[4].tolist() == [1] and dev[2].tolist() == [2]            # so(2), order 3: the first thresholding leaves the linear terms
    both = np.stack([G, C.gram("so2_o3_cc1")[0]])                       # ... next to a problem the device solves to the end
    on_device = _solve(_sweep_on(eng, both, C.N_POINTS, 2, 3), 0.0, C.THRESHOLD, max_iter=10, device=True, coef=coef)
    assert len(on_device[4]) == 1
    assert "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead" == str(on_device[4][0].message)
    sw = _sweep_on(eng, both, C.N_POINTS, 2, 3)
    Xi, mask, passes = np.zeros((2, 2, 10), dtype=np.float32), np.ones((2, 2, 10), dtype=bool), np.zeros(2, dtype=np.int64)
    sw.near_threshold = []
    sw._replay(0, G, 0.0, C.THRESHOLD, 10, "min_norm", Xi, mask, passes, coef)           # the host loop's minimum-norm answer
    assert on_device[0][0].tobytes() == Xi[0].tobytes() and np.array_equal(on_device[1][0], mask[0]) and on_device[2][0] == passes[0]
    assert mask[0].sum() > 0 and np.isfinite(Xi[0]).all()
    out, trace = _model("so2_o3_cc1", 0.0, 10)
    assert np.array_equal(on_device[1][1], out["mask"]) and on_device[2][1] == out["passes"]
    assert on_device[0][1].tobytes() == _device(eng, both[1], coef, 0.0, C.THRESHOLD, 10)[0][0].tobytes()


# ---- 3. tables -----------------------------------------------------------------------------------------------------------------
def test_a_table_problem_is_the_scalar_launch_on_its_set(eng):
    name = "negdet_o3_cc0"
    coef = C.coef_map(name)
    G = np.stack([C.gram(name, v)[0] for v in range(3)])
    W, T = (0.0, 0.1, 3.0), (0.05, 0.1, 0.7)
    table = torch.tensor([[w, t] for w in W for t in T for _ in range(3)], dtype=torch.float32)        # 27 problems on 3 sets
    grid = _device(eng, G, coef, -1.0, -1.0, 10, hyper=table.to(DEV))
    assert grid[0].shape == (27, 2, 10) and grid[5].shape == (27, 6)
    again = _device(eng, G, coef, -1.0, -1.0, 10, hyper=table.to(DEV))
    for name_, a, b in zip(NAMES, grid, again):
        assert a.tobytes() == b.tobytes(), name_
    for g in range(9):                                                  # nine scalar launches over the three sets
        one = _device(eng, G, coef, float(table[3 * g, 0]), float(table[3 * g, 1]), 10)
        for name_, a, b in zip(NAMES, grid, one):
            if name_ in ("xi", "var"):
                keep = one[4] == 0                                      # a flagged problem's other outputs are unspecified
                assert a[3 * g:3 * g + 3][keep].tobytes() == b[keep].tobytes(), (g, name_)
            else:
                assert a[3 * g:3 * g + 3].tobytes() == b.tobytes(), (g, name_)
    assert len({grid[1][s].tobytes() for s in range(0, 27, 3)}) > 1     # the points decide


# ---- 4. solve(device=True, coef=) against solve(device=False, coef=) ------------------------------------------------------------
@pytest.mark.parametrize("name", ["negdet_o3_cc1", "scaling2_o2_cc0", "so2_o3_cc1"])
def test_solve_on_the_device_equals_solve_on_the_host(eng, name):
    coef = C.coef_map(name)
    order = C.DECK[name][2]
    G = np.stack([C.gram(name, v)[0] for v in range(3)])
    gamma = float(np.float32(0.1))
    on_host = _solve(_sweep_on(eng, G, C.N_POINTS, coef.d, order), gamma, C.THRESHOLD, max_iter=10, lstsq_driver="gels", coef=coef)
    on_device = _solve(_sweep_on(eng, G, C.N_POINTS, coef.d, order), gamma, C.THRESHOLD, max_iter=10, device=True, coef=coef)
    assert not on_host[3] and not on_host[4] and not on_device[3] and not on_device[4]        # near == 0, fell == 0
    assert np.array_equal(on_device[1], on_host[1]) and np.array_equal(on_device[2], on_host[2])
    qs, qx = C.matrices(coef)
    for k in range(3):
        trace = []
        out = M.sweep(G[k], coef.d, gamma, C.THRESHOLD, 10, qs, qx, coef.allow_constant, band=C.BAND, trace=trace)
        cond, n = np.linalg.cond(trace[-1][2]), len(trace[-1][4])
        assert cond <= C.COND_BOUND
        # two fp64 solves of the same system (the host's LAPACK-order sums, the kernel's) and two fp32 products: twice the bound
        bound = 2 * M.xi_bound(qx, out["var"], cond, n, coef.d, coef.p, coef.allow_constant)
        err = np.abs(on_device[0][k].astype(np.float64) - on_host[0][k])
        print(name, k, "max |dXi| / bound %.3g" % (err / bound).max())
        assert (err <= bound).all()
    # a table over the same seeds
    hyper = {"threshold": [C.THRESHOLD] * 3 + [0.5] * 3}
    grid = _solve(_sweep_on(eng, G, C.N_POINTS, coef.d, order), gamma, 7.0, max_iter=10, device=True, hyper=hyper, coef=coef)
    assert grid[0].shape == (6, coef.d, coef.p) and grid[0][:3].tobytes() == on_device[0].tobytes()


# ---- 5. the reference's recorded passes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", C.SOLVE_TAGS)
def test_the_reference_fixture(eng, tag):
    g = C.golden()
    d, order, cc = [int(v) for v in g[f"{tag}_cfg"]]
    gamma, thr = [float(v) for v in g[f"{tag}_hp"]]
    coef = C.fixture_coef(tag)
    x, dx = torch.from_numpy(g[f"{tag}_x"]).to(DEV), torch.from_numpy(g[f"{tag}_dx"]).to(DEV)
    G = eng.aug_gram(x, dx, order)[None]
    for max_iter in (1, 2):
        dev = _device(eng, G, coef, gamma, thr, max_iter, n_points=x.shape[0])
        conv = g[f"{tag}_conv"]
        recorded = 1 + int(np.argmax(conv)) if conv.any() else len(conv)
        assert dev[4].tolist() == [0] and dev[2].tolist() == [min(max_iter, recorded)]
        k = dev[2][0] - 1
        assert np.array_equal(dev[1][0], g[f"{tag}_masks"][k] > 0), (tag, max_iter)
        assert np.allclose(dev[0][0], g[f"{tag}_xis"][k], rtol=1e-5, atol=1e-6), (tag, max_iter)      # test_oracle_golden's tolerance


# ---- 6. main_sweep --equiv_stlsq -----------------------------------------------------------------------------------------------
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


ARGV = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--w_sym_reg", "0.0",
        "--lbfgs_subsample", "0.5", "--repr", "(1,so2)", "--group_idx", "0", "--latent_dim", "2", "--n_comps", "1",
        "--poly_order", "2", "--threshold", "0.05", "--w_sindy_reg", "0.25", "--num_epochs", "10", "--seed", "4", "--n_seeds", "4",
        "--device_stlsq", "--equiv_stlsq", "--eq_constraint"]


@pytest.fixture()
def small_dosc(monkeypatch):
    from symode_amd import dataset as D
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)


def test_main_sweep_equiv_stlsq_is_solve_sindy_per_seed(eng, tmp_path, small_dosc, capsys, monkeypatch):
    from symode_amd import main_sweep
    from symode_amd.sindy import solve_SINDy
    from symode_amd.sweep import seeded_subsamples
    seen = {}
    fit = main_sweep._fit_stlsq
    monkeypatch.setattr(main_sweep, "_fit_stlsq", lambda ctx: seen.setdefault("ctx", ctx) and fit(ctx))
    res = _main(tmp_path, ARGV + ["--save_dir", "equiv"])
    out = capsys.readouterr().out
    assert res["n_runs"] == 4 and "STLSQ passes" in out
    assert "near-threshold coefficients (| |coef| - thr | < 1e-4): none" in out
    ctx = seen["ctx"]
    rows = seeded_subsamples(ctx.x_all.shape[0], ctx.m, ctx.seeds, ctx.dev)
    gamma, thr = float(np.float32(0.25)), float(np.float32(0.05))
    for k, s in enumerate(ctx.seeds):
        reg = main_sweep._template(ctx)[0]
        x, dx = ctx.x_all[rows[k].long()].contiguous(), ctx.dx_all[rows[k].long()].contiguous()
        solve_SINDy(reg, x, dx, gamma, thr, max_iter=10, lstsq_driver="gels")
        mask = reg.mask.cpu().numpy() > 0
        want = reg.get_Xi().detach().cpu().numpy() * mask
        got = np.load(tmp_path / "eval_results" / "equiv" / f"seed{s}.npz")["coefficients"]
        assert np.array_equal(got != 0, mask), s
        coef = reg.coef
        var = np.concatenate([reg.beta.detach().cpu().numpy().reshape(-1), reg.const.detach().cpu().numpy().reshape(-1)])
        var = var[:coef.r + (coef.d if coef.allow_constant else 0)]
        n = int(np.count_nonzero(var))
        # cond(Gq) <= 1e6 is generous here (an orthonormal Q on a well-conditioned order-2 library); two solves: twice the bound
        bound = 2 * M.xi_bound(coef.xi_matrix(), var, 1e6, max(n, 1), coef.d, coef.p, coef.allow_constant)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), s


def test_main_sweep_equiv_stlsq_grid_is_the_scalar_run_at_every_point(eng, tmp_path, small_dosc, capsys):
    T = ("0.05", "0.6")
    res = _main(tmp_path, ARGV + ["--save_dir", "grid", "--stlsq_grid", "threshold=" + ",".join(T)])
    assert sorted(res) == [0, 1]
    listed = json.loads((tmp_path / "eval_results" / "grid" / "grid.json").read_text())
    assert listed["axes"] == [["threshold", [0.05, 0.6]]] and listed["n_seeds"] == 4
    coefs = []
    for g, t in enumerate(T):
        argv = [a for a in ARGV]
        argv[argv.index("--threshold") + 1] = t
        scalar = _main(tmp_path, argv + ["--save_dir", f"point{g}"])
        assert repr(res[g]) == repr(scalar), g
        for s in (4, 5, 6, 7):
            want = np.load(tmp_path / "eval_results" / f"point{g}" / f"seed{s}.npz")
            got = np.load(tmp_path / "eval_results" / "grid" / f"grid{g}" / f"seed{s}.npz")
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            coefs.append(got["coefficients"])
    capsys.readouterr()
    assert not np.array_equal(coefs[0], coefs[4])                       # the threshold decides


# ---- 7. the unconstrained entry computes what it computed -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.SHAPES[:3], ids=lambda s: "d%d_o%d_f%d" % s)
def test_the_unconstrained_entry_is_unchanged(eng, shape):
    import symode_amd
    d, order, flags = shape
    x, dx, _ = U.points(shape)
    G = symode_amd.get_engine().aug_gram(x.to(DEV), dx.to(DEV), order, flags)
    host = U.host_sweep(G.cpu().numpy(), d, 0.1, U.THRESHOLD, 10)
    xi, mask, passes, near, fell = (t.cpu().numpy() for t in eng.stlsq_sweep(G, U.N_POINTS, 0.1, U.THRESHOLD, 10, d=d, near_band=U.BAND))
    assert not fell.any() and np.array_equal(mask.astype(bool), host[1]) and np.array_equal(passes, host[2]) and np.array_equal(near, host[3])
    bound = np.spacing(np.abs(host[0]).max(axis=-1, keepdims=True).astype(np.float32)).astype(np.float64)
    assert (np.abs(xi.astype(np.float64) - host[0]) <= bound).all()
