"""symode_stlsq_bag (engine.stlsq_bag) against the numpy model tests/stlsq_bag_model.py, and SeedSweepSTLSQ.solve_bagged
(device=True) against its numpy route.

Integer outputs (mask, fell, count, valid) are equal: the inclusion rule is integer arithmetic on both sides.  mean and std lie
within the bound ``stlsq_bag_model.statistic_bounds`` derives from the arithmetic (whether the bytes were equal is printed).
The refit's coefficients lie within the bound tests/test_gpu_stlsq_device.py derives for an fp64 solve rounded once to fp32,
|Xi_dev - Xi_model| <= spacing(fp32(max |Xi_model| over the row)), which rests on n <= 64 unknowns and cond <= 1e6: the
condition number of every seed's ridge system is asserted here on the host (a principal submatrix of a positive definite
matrix is no worse conditioned than the matrix).  A launch against another launch is bit for bit."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_bag_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("xi", "mask", "fell", "count", "valid", "mean", "std")


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _bag(eng, G, rxi, rmask, rfell, B, gamma, d, **kw):
    out = eng.stlsq_bag(torch.from_numpy(np.ascontiguousarray(G)).to(DEV), torch.from_numpy(np.ascontiguousarray(rxi)).to(DEV),
                        torch.from_numpy(np.ascontiguousarray(rmask)).to(DEV), torch.from_numpy(np.ascontiguousarray(rfell)).to(DEV),
                        B, gamma, d=d, to_host=True, **kw)
    return dict(zip(NAMES, (np.array(a) for a in out)))


def _cond(G, d, gamma):
    p = G.shape[1] - d
    return max(np.linalg.cond(G[k, :p, :p] + gamma * gamma * np.eye(p)) for k in range(G.shape[0]))


def _assert_as_the_model(dev, want, rxi, rmask, B, what):
    for name in ("mask", "fell", "count", "valid"):
        assert np.array_equal(dev[name], want[name]), (what, name)
        assert dev[name].dtype == want[name].dtype, (what, name)
    mean_bound, std_bound = M.statistic_bounds(rxi, rmask, B, want["std"])
    e_mean, e_std = np.abs(dev["mean"] - want["mean"]), np.abs(dev["std"] - want["std"])
    err = np.abs(dev["xi"].astype(np.float64) - want["xi"])
    print(what, "mean bytes equal", dev["mean"].tobytes() == want["mean"].tobytes(), "std bytes equal",
          dev["std"].tobytes() == want["std"].tobytes(), "max mean err %.3g std err %.3g" % (e_mean.max(), e_std.max()),
          "max |dXi| / bound %.3g" % (err / M.row_bound(want["xi"])).max())
    assert (e_mean <= mean_bound).all() and (e_std <= std_bound).all(), what
    assert (err <= M.row_bound(want["xi"])).all(), (what, err.max())
    assert not dev["xi"][dev["mask"] == 0].any()


# ---- 1. the raw entry against the model, every size --------------------------------------------------------------------------
# (S, d, p, B, flagged replicas per seed): p = 1; the flagship's library; d = 1 with p = 64 lanes; d = 4 with p = 64 (131 KiB
# of LDS: the attribute call); an odd p with B = 33
SIZES = ((3, 2, 1, 5, 0), (3, 2, 10, 5, 1), (2, 1, 64, 4, 0), (2, 4, 64, 3, 1), (3, 3, 23, 33, 2))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "S%d_d%d_p%d_B%d_f%d" % s)
def test_raw_entry_equals_the_model(eng, size):
    S, d, p, B, n_fell = size
    gamma = 0.1
    G, _ = M.random_grams(S, d, p, seed=p)
    cond = _cond(G, d, gamma)
    print(size, "cond %.3g" % cond)
    assert cond <= M.COND_BOUND
    rxi, rmask, rfell = M.random_replicas(S, B, d, p, seed=p, n_fell=n_fell)
    tau = [t for t in (0, 500, 600, 1000) for _ in range(S)]
    dev = _bag(eng, G, rxi, rmask, rfell, B, gamma, d, tau_table=tau)
    want = M.bag(G, rxi, rmask, rfell, tau, gamma)
    assert dev["xi"].shape == (4 * S, d, p) and dev["count"].shape == (S, d, p) and dev["valid"].tolist() == [B - n_fell] * S
    assert not want["fell"].any()
    _assert_as_the_model(dev, want, rxi, rmask, B, size)
    if p > 1:
        supports = {dev["mask"][g * S:(g + 1) * S].tobytes() for g in range(4)}
        assert len(supports) >= 3                                              # the levels decide
    assert dev["mask"][:S].all()                                               # level 0 keeps everything


# ---- 2. what the entry is bit for bit ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_grams():
    G, _ = M.random_grams(3, 2, 10, seed=3)
    return G


def test_level_zero_is_one_pass_of_the_sweep(eng):
    G, gamma = _fit_grams(), 0.1
    Gd = torch.from_numpy(G).to(DEV)
    xi, mask, passes, near, fell = (t.cpu().numpy() for t in eng.stlsq_sweep(Gd, 400, gamma, 0.0, 1, d=2))
    rxi, rmask, rfell = M.random_replicas(3, 2, 2, 10, seed=1)
    dev = _bag(eng, G, rxi, rmask, rfell, 2, gamma, 2, tau_milli=0)
    assert dev["xi"].tobytes() == xi.tobytes() and dev["mask"].all() and not dev["fell"].any() and not fell.any()
    assert dev["xi"].any()


def test_one_converged_replica_at_level_one_is_that_fit(eng):
    G, gamma, thr = _fit_grams(), 0.1, 0.2
    Gd = torch.from_numpy(G).to(DEV)
    xi, mask, passes, near, fell = eng.stlsq_sweep(Gd, 400, gamma, thr, 10, d=2)
    assert (passes.cpu().numpy() < 10).all() and not fell.any().item()         # converged: the last pass solved ON the final support
    out = eng.stlsq_bag(Gd, xi, mask, fell, 1, gamma, tau_milli=1000, d=2)
    assert out[0].cpu().numpy().tobytes() == xi.cpu().numpy().tobytes()
    assert out[1].cpu().numpy().tobytes() == mask.cpu().numpy().tobytes()
    assert 0 < mask.sum().item() < mask.numel()                                # a sparse support, not the full one
    assert np.array_equal(out[3].cpu().numpy(), mask.cpu().numpy().astype(np.int32)) and out[4].tolist() == [1, 1, 1]
    assert out[5].cpu().numpy().tobytes() == (xi.cpu().numpy().astype(np.float64) * mask.cpu().numpy()).tobytes()
    assert not out[6].any().item()


def test_flagged_replicas_are_left_out(eng):
    S, d, p, B = 3, 2, 10, 7
    G = _fit_grams()
    rxi, rmask, rfell = M.random_replicas(S, B, d, p, seed=5, n_fell=2)
    assert rfell.reshape(S, B).sum(axis=1).tolist() == [2, 2, 2]
    tau = [600] * S
    dev = _bag(eng, G, rxi, rmask, rfell, B, 0.0, d, tau_table=tau)
    assert dev["valid"].tolist() == [5, 5, 5]
    keep = rfell == 0                                                          # the same launch without them, B = 5
    less = _bag(eng, G, rxi[keep], rmask[keep], rfell[keep], B - 2, 0.0, d, tau_table=tau)
    for name in NAMES:
        assert dev[name].tobytes() == less[name].tobytes(), name
    # poisoning what a flagged replica holds changes nothing
    rxi2, rmask2 = rxi.copy(), rmask.copy()
    rxi2[~keep], rmask2[~keep] = np.float32(np.nan), 1
    again = _bag(eng, G, rxi2, rmask2, rfell, B, 0.0, d, tau_table=tau)
    for name in NAMES:
        assert dev[name].tobytes() == again[name].tobytes(), name


def test_no_valid_replica_gives_the_empty_model(eng):
    S, d, p, B = 3, 2, 10, 4
    rxi, rmask, _ = M.random_replicas(S, B, d, p, seed=6)
    rfell = np.ones(S * B, dtype=np.int32)
    rfell[B:2 * B] = 0                                                         # seed 1 keeps its replicas
    for tau in (0, 1000):
        dev = _bag(eng, _fit_grams(), rxi, rmask, rfell, B, 0.1, d, tau_milli=tau)
        assert dev["valid"].tolist() == [0, B, 0]
        for k in (0, 2):
            assert not dev["xi"][k].any() and not dev["mask"][k].any() and not dev["count"][k].any()
            assert not dev["mean"][k].any() and not dev["std"][k].any()
        assert dev["mask"][1].any() and not dev["fell"].any()


def test_a_table_problem_is_the_scalar_launch(eng):
    S, d, p, B = 3, 2, 10, 5
    G = _fit_grams()
    rxi, rmask, rfell = M.random_replicas(S, B, d, p, seed=8, n_fell=1)
    levels = (400, 750, 1000)
    grid = _bag(eng, G, rxi, rmask, rfell, B, 0.1, d, tau_table=[t for t in levels for _ in range(S)])
    assert grid["xi"].shape == (9, d, p)
    for g, t in enumerate(levels):
        one = _bag(eng, G, rxi, rmask, rfell, B, 0.1, d, tau_milli=t)
        for name in ("xi", "mask", "fell"):
            assert grid[name][g * S:(g + 1) * S].tobytes() == one[name].tobytes(), (t, name)
        for name in ("count", "valid", "mean", "std"):
            assert grid[name].tobytes() == one[name].tobytes(), (t, name)
    assert len({grid["mask"][g * S:(g + 1) * S].tobytes() for g in range(3)}) == 3


def test_the_wrapper_refuses_a_level_outside_the_range(eng):
    from symode_amd.engine import SymodeError
    rxi, rmask, rfell = M.random_replicas(3, 2, 2, 10)
    for bad in ([0, 1001, 5], [-1, 0, 0]):
        with pytest.raises(SymodeError, match="0 .. 1000"):
            _bag(eng, _fit_grams(), rxi, rmask, rfell, 2, 0.1, 2, tau_table=bad)
    with pytest.raises(SymodeError, match="symode_stlsq_bag failed"):
        _bag(eng, _fit_grams(), rxi, rmask, rfell, 2, 0.1, 2, tau_milli=1001)
    with pytest.raises(SymodeError, match="n_seeds \\* n_replicas"):
        _bag(eng, _fit_grams(), rxi[:5], rmask[:5], rfell[:5], 2, 0.1, 2)


# ---- 3. an exactly singular support ------------------------------------------------------------------------------------------------
def _integer_grams():
    """3 sets for p = 6, d = 2 from integer data (exact in fp64 whatever the summation order); set 1 has an all-zero library
    column 2, so row and column 2 of its Gtt are exactly zero."""
    rng = np.random.RandomState(5)
    A = rng.randint(-3, 4, size=(3, 40, 8)).astype(np.float64)
    A[:, :, 0] = 1.0
    A[1, :, 2] = 0.0
    return np.einsum("sna,snb->sab", A, A)


def test_a_singular_support_is_flagged(eng):
    G = _integer_grams()
    rxi = np.ones((3, 2, 6), dtype=np.float32)
    full, rfell = np.ones((3, 2, 6), dtype=np.uint8), np.zeros(3, dtype=np.int32)
    dev = _bag(eng, G, rxi, full, rfell, 1, 0.0, 2, tau_milli=1000)
    assert dev["fell"].tolist() == [0, 1, 0]
    want = M.bag(G, rxi, full, rfell, [1000] * 3, 0.0)
    assert want["fell"].tolist() == [0, 1, 0]
    for k in (0, 2):                                                           # the neighbours are solved
        assert (np.abs(dev["xi"][k].astype(np.float64) - want["xi"][k]) <= M.row_bound(want["xi"][k])).all()
    without = full.copy()
    without[1, :, 2] = 0                                                       # the same seed with the empty column left out: solved
    dev = _bag(eng, G, rxi, without, rfell, 1, 0.0, 2, tau_milli=1000)
    assert dev["fell"].tolist() == [0, 0, 0] and dev["xi"][1].any() and not dev["xi"][1, :, 2].any()


# ---- 4. solve_bagged: the device route against the numpy route ---------------------------------------------------------------------
def _sweep(order, eng):
    """3 seeds x 400 rows of a damped oscillator on [-1, 1]^2 with 2 % noise"""
    from symode_amd.sweep import SeedSweepSTLSQ
    rng = np.random.RandomState(11)
    x = rng.uniform(-1.0, 1.0, size=(1200, 2))
    dx = np.stack([-0.1 * x[:, 0] + 2.0 * x[:, 1], -2.0 * x[:, 0] - 0.1 * x[:, 1]], axis=1) + 0.02 * rng.randn(1200, 2)
    to = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)              # noqa: E731
    return SeedSweepSTLSQ(to(x), to(dx), order, n_seeds=3, subsample=1.0 / 3.0, seed0=3, engine=eng)


def _bagged(sw, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, record = sw.solve_bagged(0.0, 0.05, 5, n_chunks=8, inclusion=[0.5, 1.0], **kw)
    return Xi.numpy(), mask.numpy() > 0, record, [w for w in rec if w.category is RuntimeWarning]


@pytest.mark.parametrize("order", (2, 3))
def test_solve_bagged_device_equals_the_numpy_route(eng, order):
    from symode_amd.sweep import resample_grams
    from tests.stlsq_cases import host_sweep
    sw = _sweep(order, eng)
    assert sw.m_local == 400
    chunk = sw.chunk_grams(8)
    p = sw.p
    assert tuple(chunk.shape) == (3, 8, p + 2, p + 2)
    # the chunk matrices add up to the Gram of the first C L rows, which here are all rows: the seed's own matrix
    G = sw.grams()
    total = chunk.cpu().numpy().sum(axis=1)
    assert np.abs(total - G).max() <= 400 * 2.0 ** -52 * np.abs(G).max()
    # the conditions the comparison rests on, on the host: no replica decision hangs on a last bit, nothing is singular
    rep, _ = resample_grams(chunk.cpu().numpy(), sw.seeds, 5)
    ref = host_sweep(rep, 2, 0.0, 0.05, 10, n_points=400)
    assert not ref[3].any() and not ref[4].any() and (ref[2] < 10).all()
    assert max(_cond(rep, 2, 0.0), _cond(G, 2, 0.0)) <= M.COND_BOUND
    dev, host = _bagged(sw, device=True), _bagged(sw, device=False)
    assert dev[0].shape == (6, 2, p) and not dev[3] and not host[3] and not dev[2]["fell"].any()
    assert np.array_equal(dev[1], host[1])
    assert np.array_equal(dev[2]["count"], host[2]["count"]) and np.array_equal(dev[2]["valid"], host[2]["valid"])
    assert dev[2]["valid"].tolist() == [5, 5, 5] and dev[2]["count"].dtype == np.int32
    # a replica coefficient is the host's within eps = its row bound (one fp32 bit), so the mean moves by at most eps and the
    # std by at most 2 eps (the shift of the values and the shift of the mean, triangle inequality)
    eps = M.row_bound(ref[0]).reshape(3, 5, 2, 1).max(axis=1)
    assert (np.abs(dev[2]["mean"] - host[2]["mean"]) <= eps).all() and (np.abs(dev[2]["std"] - host[2]["std"]) <= 2 * eps).all()
    assert (np.abs(dev[0].astype(np.float64) - host[0]) <= M.row_bound(host[0])).all()
    truth = np.zeros((2, p), dtype=bool)
    truth[:, 1:3] = True                                                       # columns x0, x1 of the polynomial library
    assert all(np.array_equal(dev[1][s], truth) for s in range(3, 6))          # at inclusion 1.0 every seed ends on the truth
    print("order", order, "bit-equal Xi", dev[0].tobytes() == host[0].tobytes(), "supports at 0.5",
          dev[1][:3].sum(axis=(1, 2)).tolist())


def test_a_singular_refit_goes_to_the_host_twin(eng):
    sw = _sweep(2, eng)
    G = sw.grams().copy()
    G[1, 2, :] = 0.0
    G[1, :, 2] = 0.0                                                           # seed 1's own matrix loses column x1: exactly singular
    sw.set_grams(torch.from_numpy(G).to(DEV), 400)
    dev, host = _bagged(sw, device=True), _bagged(sw, device=False)
    assert dev[2]["fell"].tolist() == [False, True, False, False, True, False]
    assert len(dev[3]) >= 1 and "singular normal equations under the full-rank (gels) driver" in str(dev[3][0].message)
    for s in (1, 4):                                                           # the host's own answer, bit for bit
        assert dev[0][s].tobytes() == host[0][s].tobytes() and np.array_equal(dev[1][s], host[1][s])
        assert not dev[0][s][:, 2].any() and dev[1][s][:, 2].all()            # kept by the vote, zero by the minimum-norm rule
    assert np.array_equal(dev[1], host[1])
    assert (np.abs(dev[0].astype(np.float64) - host[0]) <= M.row_bound(host[0])).all()


# ---- 5. main_sweep --bagging ----------------------------------------------------------------------------------------------------------
N_SEEDS = 4
ARGV = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--w_sym_reg", "0.0", "--lbfgs_subsample", "0.5",
        "--poly_order", "3", "--threshold", "0.05", "--w_sindy_reg", "0.01", "--num_epochs", "10", "--seed", "4"]
FLAGS = ["--method", "stlsq", "--device_stlsq", "--bagging", "4", "--bag_chunks", "8", "--n_seeds", str(N_SEEDS)]


def _main(tmp, argv):
    import os
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
    """6 + 3 trajectories x 200 samples of the damped oscillator, in the data files the driver loads"""
    import os
    from symode_amd import dataset as D
    from symode_amd.parser_utils import get_args
    tmp = tmp_path_factory.mktemp("stlsq-bag-dosc")
    cwd, old, old_dt = os.getcwd(), D._RECIPES["dosc"], D.ode_dt_dict["dosc"]
    os.chdir(tmp)
    D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = (6, 3, 600, 3, 0.01), 0.03
    try:
        D.get_dataset(vars(get_args(argv=list(ARGV))))
        yield tmp
    finally:
        D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = old, old_dt
        os.chdir(cwd)


def test_main_sweep_bagging_is_solve_bagged(eng, small_dosc, capsys, monkeypatch):
    import json
    from symode_amd.sweep import SeedSweepSTLSQ
    seen = {}
    solve_bagged = SeedSweepSTLSQ.solve_bagged

    def recorded(self, *a, **kw):
        seen.update(sw=self, a=a, kw=kw)
        return solve_bagged(self, *a, **kw)

    monkeypatch.setattr(SeedSweepSTLSQ, "solve_bagged", recorded)
    monkeypatch.setattr(SeedSweepSTLSQ, "solve", lambda *a, **k: pytest.fail("the plain threshold fit ran"))
    res = _main(small_dosc, ARGV + FLAGS + ["--bag_inclusion", "0.5,1", "--save_dir", "bag"])
    out = capsys.readouterr().out
    monkeypatch.undo()
    sw = seen["sw"]
    assert seen["a"] == (0.01, 0.05, 4) and seen["kw"] == dict(n_chunks=8, inclusion=[0.5, 1.0], max_iter=10)
    assert (sw.S, sw.d, sw.p, sw.m_local) == (N_SEEDS, 2, 10, 600) and sw.seeds == [1_000_003 * s for s in range(4, 4 + N_SEEDS)]
    assert sorted(res) == [0, 1] and all(res[g]["n_runs"] == N_SEEDS for g in res)
    d = small_dosc / "eval_results" / "bag"
    assert sorted(f.name for f in d.iterdir()) == ["bag.npz", "grid.json", "grid0", "grid1"]
    Xi, mask, record = sw.solve_bagged(0.01, 0.05, 4, n_chunks=8, inclusion=[0.5, 1.0], max_iter=10)      # directly, the same matrices
    for g in (0, 1):
        files = sorted(f.name for f in (d / f"grid{g}").iterdir())
        assert files == sorted(f"seed{s}.npz" for s in range(4, 4 + N_SEEDS))
        one = np.load(d / f"grid{g}" / "seed4.npz")
        assert sorted(one.files) == ["bag_inclusion", "coefficients", "correct_form", "correct_form_all", "mse", "mse_all"]
        assert float(one["bag_inclusion"]) == (0.5, 1.0)[g]
        coefs = np.stack([np.load(d / f"grid{g}" / f"seed{s}.npz")["coefficients"] for s in range(4, 4 + N_SEEDS)])
        at = slice(g * N_SEEDS, (g + 1) * N_SEEDS)
        assert coefs.tobytes() == (Xi.numpy() * mask.numpy())[at].astype(coefs.dtype).tobytes()
    bag = np.load(d / "bag.npz")
    assert sorted(bag.files) == ["count", "fell", "inclusion", "mean", "n_chunks", "n_replicas", "seeds", "std", "valid"]
    for k in ("count", "valid", "mean", "std", "fell"):
        assert bag[k].tobytes() == record[k].tobytes(), k
    assert bag["count"].shape == (N_SEEDS, 2, 10) and bag["fell"].shape == (2 * N_SEEDS,) and bag["seeds"].tolist() == list(range(4, 8))
    assert (int(bag["n_replicas"]), int(bag["n_chunks"]), bag["inclusion"].tolist()) == (4, 8, [0.5, 1.0])
    table = json.load(open(d / "grid.json"))
    assert table["axes"] == [["bag_inclusion", [0.5, 1.0]]] and [p["bag_inclusion"] for p in table["points"]] == [0.5, 1.0]
    size = (mask.numpy() > 0).sum(axis=(1, 2)).reshape(2, N_SEEDS)
    assert (f"{N_SEEDS} seeds x 600 points (over 1 rank(s)), bagged: 4 replicas of 8 chunks x 75 rows per seed, valid replicas "
            f"{record['valid'].min()}-{record['valid'].max()} of 4, support size {size[0].min()}-{size[0].max()} at inclusion 0.5, "
            f"{size[1].min()}-{size[1].max()} at inclusion 1, refits solved on the host: 0") in out.splitlines()
    assert (size[1] <= size[0]).all()                                           # a higher level keeps no more
    # one level: no grid, the plain result files, the default level
    res = _main(small_dosc, ARGV + FLAGS + ["--save_dir", "bag-one"])
    capsys.readouterr()
    d1 = small_dosc / "eval_results" / "bag-one"
    assert res["n_runs"] == N_SEEDS
    assert sorted(f.name for f in d1.iterdir()) == sorted([f"seed{s}.npz" for s in range(4, 4 + N_SEEDS)] + ["bag.npz"])
    coefs = np.stack([np.load(d1 / f"seed{s}.npz")["coefficients"] for s in range(4, 4 + N_SEEDS)])
    assert coefs.tobytes() == (Xi.numpy() * mask.numpy())[N_SEEDS:].astype(coefs.dtype).tobytes()       # the default is inclusion 1.0
    assert np.load(d1 / "bag.npz")["inclusion"].tolist() == [1.0]
