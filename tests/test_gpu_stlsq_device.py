"""The device STLSQ sweep (symode_stlsq_sweep, engine.stlsq_sweep, SeedSweepSTLSQ.solve(device=True, hyper=), main_sweep
--device_stlsq / --stlsq_grid) against the host loop it restates, symode_host_stlsq_sweep with driver 1 (gels), on the same
matrices.

The bound on the coefficients is derived, not measured: both sides solve in fp64 and round once to fp32; the normwise error
of the fp64 solve is <= c n 2^-53 cond ~ 2e-9 relative for n <= 64 and cond <= 1e6, far below fp32 rounding, so only the
last fp32 bit of a coefficient can differ: |Xi_dev - Xi_host| <= spacing(fp32(max |Xi_host| over the row)).  The conditions
that derivation rests on are asserted on the inputs: the host reports near == 0 and fell == 0 for every problem at band 1e-4
(so no decision hangs on the last bit) and cond(Gtt) <= 1e6 (tests/stlsq_cases.py says where that cannot hold and why).
Grid launches against scalar launches are bit for bit: a problem is one workgroup that shares no arithmetic with another."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


@functools.lru_cache(maxsize=None)
def _grams(shape):
    """The shape's 3 augmented Gram matrices from symode_aug_gram, on the device and on the host: computed once."""
    import symode_amd
    d, order, flags = shape
    x, dx, _ = C.points(shape)
    G = symode_amd.get_engine().aug_gram(x.to(DEV), dx.to(DEV), order, flags)
    return G, G.cpu().numpy()


def _device(eng, G, d, gamma, threshold, max_iter, **kw):
    xi, mask, passes, near, fell = (t.cpu().numpy() for t in eng.stlsq_sweep(G, C.N_POINTS, gamma, threshold, max_iter, d=d,
                                                                             near_band=C.BAND, **kw))
    return xi, mask.astype(bool), passes, near, fell


def _row_bound(xi_host):
    """spacing(fp32(max |Xi_host| over the row)), per (problem, row), broadcastable against Xi."""
    return np.spacing(np.abs(xi_host).max(axis=-1, keepdims=True).astype(np.float32)).astype(np.float64)


def _assert_as_the_host(dev, host, what):
    xi_d, mask_d, passes_d, near_d = dev[:4]
    xi_h, mask_h, passes_h, near_h = host[:4]
    err = np.abs(xi_d.astype(np.float64) - xi_h.astype(np.float64))
    print(what, "passes", np.asarray(passes_h).tolist(), "max |dXi| / bound %.3g" % (err / _row_bound(xi_h)).max(),
          "bit-equal", bool(np.array_equal(xi_d.view(np.int32), xi_h.view(np.int32))))
    assert np.array_equal(mask_d, mask_h), what
    assert np.array_equal(passes_d, passes_h), what
    assert np.array_equal(near_d, near_h), what
    assert (err <= _row_bound(xi_h)).all(), (what, err.max())


# ---- 1. the raw entry against the host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", C.GAMMAS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "d%d_o%d_f%d" % s)
def test_raw_entry_equals_the_host_loop(eng, shape, gamma):
    d, order, flags = shape
    G, Gh = _grams(shape)
    p = eng.lib_size(d, order, flags)
    assert Gh.shape == (C.N_SETS, p + d, p + d)
    cond, ref = C.conditions(Gh, d, gamma)
    print(shape, "p", p, "gamma", gamma, "cond(Gtt) %.3g" % cond)
    if (shape, gamma) in C.COND_UNATTAINABLE:
        assert cond > C.COND_BOUND                       # stated, not skipped: see tests/stlsq_cases.py
    else:
        assert cond <= C.COND_BOUND
    for max_iter in C.MAX_ITERS:
        host = ref[max_iter]
        assert not host[3].any() and not host[4].any(), (shape, gamma, max_iter, host[3], host[4])      # near == 0, fell == 0
        dev = _device(eng, G, d, gamma, C.THRESHOLD, max_iter)
        assert not dev[4].any()
        _assert_as_the_host(dev, host, (shape, gamma, max_iter))
    full, capped = ref[C.MAX_ITERS[-1]], ref[1]
    assert (full[2] < C.MAX_ITERS[-1]).all() and (capped[2] == 1).all()
    if p > 2:
        assert (full[2] >= 2).any() and (capped[0] != full[0]).any()    # the loop ran on, and the cap of 1 pass cut it
    if gamma > 0 or shape[2] == 0:
        assert (~full[1].any(axis=2)).any()                             # an equation row ended with empty support


def test_the_cases_cover_what_they_are_meant_to(eng):
    sizes = [eng.lib_size(*s) for s in C.SHAPES]
    assert sizes[:3] == [2, 10, 21] and C.SHAPES[3][0] == 3 and C.SHAPES[3][2] != 0
    compiled = [eng.lib.symode_lib_size(d, o, f) for d in (1, 2, 3) for o in (1, 2, 3, 4, 5) for f in (0, 1, 2, 3)]
    assert sizes[4] == max(compiled)                                    # the largest p of the default build
    some = [C.conditions(_grams(s)[1], s[0], g)[1][C.MAX_ITERS[-1]] for s in C.SHAPES for g in C.GAMMAS]
    assert max(int(r[2].max()) for r in some) >= 3                      # a support that shrinks over more than one pass


# ---- 2. an exactly singular system -------------------------------------------------------------------------------------------------
def _integer_grams():
    """3 sets for the (2, 2, 0) library (p = 6, d = 2) from integer data: exact in fp64 whatever the summation order.  Set 1
    has an all-zero library column 2, so row and column 2 of its Gtt are exactly zero."""
    rng = np.random.RandomState(5)
    A = rng.randint(-3, 4, size=(3, 40, 8)).astype(np.float64)
    A[:, :, 0] = 1.0
    A[1, :, 2] = 0.0
    return np.einsum("sna,snb->sab", A, A)


def _sweep_on(eng, G, n_points, d=2, order=2):
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


def test_a_singular_system_falls_to_the_host(eng):
    G = _integer_grams()
    assert not G[1, 2, :6].any() and not G[1, :6, 2].any() and np.array_equal(G, np.round(G))
    dev = _device(eng, torch.from_numpy(G).to(DEV), 2, 0.0, 0.5, 10)
    assert dev[4].tolist() == [0, 1, 0]
    host = C.host_sweep(G, 2, 0.0, 0.5, 10, n_points=40)
    assert host[4][1] >= 1 and host[4][0] == host[4][2] == 0
    for k in (0, 2):                                                 # the neighbours are solved, as the host solves them
        assert np.array_equal(dev[1][k], host[1][k]) and dev[2][k] == host[2][k] and dev[3][k] == host[3][k]
        assert (np.abs(dev[0][k].astype(np.float64) - host[0][k]) <= _row_bound(host[0][k])).all()
    on_host = _solve(_sweep_on(eng, G, 40), 0.0, 0.5, max_iter=10, lstsq_driver="gels")
    on_device = _solve(_sweep_on(eng, G, 40), 0.0, 0.5, max_iter=10, device=True)
    assert len(on_host[4]) >= 1 and len(on_device[4]) >= 1
    assert "singular normal equations under the full-rank (gels) driver" in str(on_device[4][0].message)
    assert str(on_device[4][0].message) == str(on_host[4][0].message)
    assert np.array_equal(on_device[0][1].view(np.int32), on_host[0][1].view(np.int32))      # the host's own answer, bit for bit
    assert np.array_equal(on_device[1], on_host[1]) and np.array_equal(on_device[2], on_host[2]) and on_device[3] == on_host[3]
    assert (np.abs(on_device[0].astype(np.float64) - on_host[0]) <= _row_bound(on_host[0])).all()


# ---- 3. the grid -------------------------------------------------------------------------------------------------------------------
def test_a_grid_problem_is_the_scalar_launch_on_its_set(eng):
    shape = (2, 3, 0)
    G, _ = _grams(shape)
    W, T = (0.0, 0.1, 0.3), (0.05, 0.1, 0.2)
    table = torch.tensor([[w, t] for w in W for t in T for _ in range(C.N_SETS)], dtype=torch.float32)      # 27 problems on 3 sets
    grid = _device(eng, G, 2, -1.0, -1.0, 10, hyper=table.to(DEV))
    assert grid[0].shape == (27, 2, 10) and not grid[4].any()
    for s in range(27):
        k = s % C.N_SETS
        one = _device(eng, G[k:k + 1].contiguous(), 2, float(table[s, 0]), float(table[s, 1]), 10)
        for name, a, b in zip(("xi", "mask", "passes", "near", "fell"), grid, one):
            assert a[s].tobytes() == b[0].tobytes(), (s, name)
    # the points decide: set 1 holds a true coefficient of 0.13, which the threshold 0.2 cuts; the ridge weight moves every fit
    assert len({grid[1][s].tobytes() for s in range(1, 27, 3)}) > 1 and len({grid[0][s].tobytes() for s in range(0, 27, 9)}) == 3
    # a uniform table is the launch without a table
    uniform = _device(eng, G, 2, -1.0, -1.0, 10, hyper=torch.tensor([[0.1, 0.1]] * 3, dtype=torch.float32).to(DEV))
    scalar = _device(eng, G, 2, float(np.float32(0.1)), float(np.float32(0.1)), 10)
    for name, a, b in zip(("xi", "mask", "passes", "near", "fell"), uniform, scalar):
        assert a.tobytes() == b.tobytes(), name
    # ... and what the engine refuses
    import symode_amd
    with pytest.raises(symode_amd.SymodeError):
        eng.stlsq_sweep(G, C.N_POINTS, 0.0, 0.1, 10, d=2, n_problems=6)                 # more problems than sets needs the table
    with pytest.raises(symode_amd.SymodeError):
        eng.stlsq_sweep(G, C.N_POINTS, 0.0, 0.1, 10, d=2, hyper=table[:2].to(DEV))      # fewer problems than sets


def test_the_largest_system_the_entry_takes(eng):
    """p = 64, d = 4 (no compiled library: a synthetic matrix): the 131 KiB of LDS of the largest workgroup, every lane a column."""
    rng = np.random.RandomState(11)
    A = rng.randn(2, 400, 68)
    A[:, :, 64:] = np.einsum("snp,sjp->snj", A[:, :, :64], rng.randn(2, 4, 64) * (rng.rand(2, 4, 64) < 0.1)) + 0.05 * rng.randn(2, 400, 4)
    G = np.einsum("sna,snb->sab", A, A)
    host = C.host_sweep(G, 4, 0.1, 0.1, 10, n_points=400)
    assert not host[3].any() and not host[4].any() and np.linalg.cond(G[0, :64, :64]) <= C.COND_BOUND
    dev = _device(eng, torch.from_numpy(G).to(DEV), 4, 0.1, 0.1, 10)
    assert not dev[4].any()
    _assert_as_the_host(dev, host, "p 64 d 4")


# ---- 4. the near-threshold replay ---------------------------------------------------------------------------------------------
def test_a_threshold_on_a_coefficient_is_replayed_for_the_record(eng):
    shape = (2, 3, 0)
    _, Gh = _grams(shape)
    first = C.host_sweep(Gh, 2, 0.0, C.THRESHOLD, 1)[0]                 # the coefficients of the first pass (full support)
    k = int(np.argmax(np.abs(first[0, 0])))                            # the largest of set 0, row 0
    thr = float(np.float32(abs(float(first[0, 0, k])) + 2e-5))         # 2e-5 above it: inside the band, and the coefficient is cut
    on_host = _solve(_sweep_on(eng, Gh, C.N_POINTS, order=3), 0.0, thr, max_iter=10, lstsq_driver="gels")
    on_device = _solve(_sweep_on(eng, Gh, C.N_POINTS, order=3), 0.0, thr, max_iter=10, device=True)
    assert any(s == 0 and (i, j) == (0, k) for s, _, i, j, _ in on_host[3]), on_host[3]
    assert on_device[3] == on_host[3]
    assert np.array_equal(on_device[1], on_host[1]) and np.array_equal(on_device[2], on_host[2])
    assert (np.abs(on_device[0].astype(np.float64) - on_host[0]) <= _row_bound(on_host[0])).all()


# ---- 5. SeedSweepSTLSQ.solve(device=True) against device=False ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dosc_points():
    from oracle import sindy_oracle as O
    rng = np.random.RandomState(3)
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(6, rng), 0.02, 150)
    x = torch.from_numpy(xs.reshape(-1, 2)).float()
    dx = torch.from_numpy(dxs.reshape(-1, 2)).float() + 0.05 * torch.from_numpy(rng.randn(900, 2)).float()
    return x, dx


@pytest.mark.parametrize("w_reg", [0.0, 0.25])          # exact in fp32: the device route takes its two values in fp32
def test_solve_on_the_device_equals_solve_on_the_host(eng, w_reg):
    from symode_amd.sweep import SeedSweepSTLSQ
    x, dx = _dosc_points()
    thr = float(np.float32(0.05))
    sw = SeedSweepSTLSQ(x.to(DEV), dx.to(DEV), 3, n_seeds=5, subsample=0.5, seed0=2, engine=eng)
    on_host = _solve(sw, w_reg, thr, max_iter=10, lstsq_driver="gels")
    assert not on_host[3] and not on_host[4]                          # near == 0 and fell == 0 ...
    G = sw.grams()
    assert max(np.linalg.cond(G[s, :10, :10] + w_reg * w_reg * np.eye(10)) for s in range(5)) <= C.COND_BOUND     # ... and cond
    assert sw.grams(device=True).is_cuda and np.array_equal(sw.grams(device=True).cpu().numpy(), G)
    on_device = _solve(sw, w_reg, thr, max_iter=10, device=True)
    assert on_device[0].shape == (5, 2, 10) and not on_device[3] and not on_device[4]
    assert np.array_equal(on_device[1], on_host[1]) and np.array_equal(on_device[2], on_host[2])
    assert (np.abs(on_device[0].astype(np.float64) - on_host[0]) <= _row_bound(on_host[0])).all()
    assert (on_host[2] >= 2).any()
    # a table over the same seeds: (G S, d, p) arrays, problem g * S + k = point g on seed k
    points = [(w_reg, thr), (w_reg, float(np.float32(0.2)))]
    hyper = {"w_reg": [w for w, _ in points for _ in range(5)], "threshold": [t for _, t in points for _ in range(5)]}
    grid = _solve(sw, 7.0, 7.0, max_iter=10, device=True, hyper=hyper)
    assert grid[0].shape == (10, 2, 10) and grid[2].shape == (10,)
    assert grid[0][:5].tobytes() == on_device[0].tobytes() and np.array_equal(grid[1][:5], on_device[1])
    second = _solve(sw, w_reg, points[1][1], max_iter=10, device=True)
    assert grid[0][5:].tobytes() == second[0].tobytes() and np.array_equal(grid[2][5:], second[2])


# ---- 6. main_sweep --device_stlsq and --stlsq_grid -----------------------------------------------------------------------------
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


def _dosc(tmp, save_dir, extra):
    argv = ["--task", "dosc", "--noise", "0.02", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--w_sym_reg", "0.0",
            "--lbfgs_subsample", "0.5",
            "--poly_order", "3", "--threshold", "0.05", "--w_sindy_reg", "0.25", "--num_epochs", "10", "--seed", "4", "--n_seeds", "4",
            "--save_dir", save_dir]
    return _main(tmp, argv + extra)


@pytest.fixture()
def small_dosc(monkeypatch):
    from symode_amd import dataset as D
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)


def test_main_sweep_device_stlsq_is_main_sweep_stlsq(eng, tmp_path, small_dosc, capsys):
    host = _dosc(tmp_path, "host", ["--lstsq_driver", "gels"])
    out_host = capsys.readouterr().out
    device = _dosc(tmp_path, "device", ["--device_stlsq"])
    out_device = capsys.readouterr().out
    assert "near-threshold coefficients (| |coef| - thr | < 1e-4): none" in out_host      # near == 0: no decision on a last bit
    summary = [line for line in out_host.splitlines() if "STLSQ passes" in line or "near-threshold" in line]
    assert len(summary) == 2 and all(line in out_device.splitlines() for line in summary)
    assert repr(host) == repr(device)
    root = tmp_path / "eval_results"
    for s in (4, 5, 6, 7):
        want, got = np.load(root / "host" / f"seed{s}.npz"), np.load(root / "device" / f"seed{s}.npz")
        assert set(got.files) == set(want.files)
        a, b = want["coefficients"], got["coefficients"]
        assert np.array_equal(a != 0, b != 0), s                                            # the same masks
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= _row_bound(a)).all(), s
        assert np.array_equal(want["correct_form"], got["correct_form"]) and bool(want["correct_form_all"]) == bool(got["correct_form_all"])


def test_main_sweep_stlsq_grid_is_main_sweep_at_every_point(eng, tmp_path, small_dosc, capsys):
    T, W = ("0.05", "0.3"), ("0", "0.1")
    res = _dosc(tmp_path, "grid", ["--device_stlsq", "--stlsq_grid", "threshold=" + ",".join(T), "--stlsq_grid", "w_sindy_reg=" + ",".join(W)])
    out = capsys.readouterr().out
    assert sorted(res) == [0, 1, 2, 3] and all(r["n_runs"] == 4 for r in res.values())
    assert "grid of 4 points x 4 seeds" in out and "grid 3: STLSQ passes" in out and "4 grid points on their Gram matrices" in out
    root = tmp_path / "eval_results"
    listed = json.loads((root / "grid" / "grid.json").read_text())
    points = [dict(threshold=float(t), w_sindy_reg=float(w)) for t in T for w in W]      # the first axis given is the slowest
    assert [(p["threshold"], p["w_sindy_reg"]) for p in listed["points"]] == [(p["threshold"], p["w_sindy_reg"]) for p in points]
    assert listed["axes"] == [["threshold", [0.05, 0.3]], ["w_sindy_reg", [0.0, 0.1]]] and listed["n_seeds"] == 4
    assert sorted(p.name for p in (root / "grid").iterdir()) == ["grid.json", "grid0", "grid1", "grid2", "grid3"]
    coefs = []
    for g, point in enumerate(points):
        scalar = _dosc(tmp_path, f"point{g}", ["--device_stlsq", "--threshold", T[g // 2], "--w_sindy_reg", W[g % 2]])
        assert repr(res[g]) == repr(scalar), g
        for s in (4, 5, 6, 7):
            want, got = np.load(root / f"point{g}" / f"seed{s}.npz"), np.load(root / "grid" / f"grid{g}" / f"seed{s}.npz")
            assert set(got.files) == set(want.files) | {"threshold", "w_sindy_reg"}
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            assert float(got["threshold"]) == point["threshold"] and float(got["w_sindy_reg"]) == point["w_sindy_reg"]
            coefs.append(got["coefficients"])
    capsys.readouterr()
    assert not np.array_equal(coefs[0], coefs[4]) and not np.array_equal(coefs[0], coefs[8])     # the weight and the threshold decide
    # --eval_ltp: all G x S models through the one roll-out launch, a best point by name
    _dosc(tmp_path, "scored", ["--device_stlsq", "--eval_ltp", "--ltp_bound_rel", "0.1", "--stlsq_grid", "threshold=" + ",".join(T)])
    out = capsys.readouterr().out
    scored = json.loads((root / "scored" / "grid.json").read_text())["points"]
    assert len(scored) == 2 and all("val_mse" in p and "ltp_median_error" in p for p in scored)
    assert "best by validation roll-out error: grid " in out
