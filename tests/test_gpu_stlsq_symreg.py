"""The device STLSQ sweep with the reversed symmetry regulariser (symode_stlsq_sweep_symreg, engine.stlsq_sweep_symreg,
SeedSweepSTLSQ.solve(device=True, rev=...), main_sweep --symreg_stlsq) against tests/stlsq_symreg_model.py, the kernel's
algorithm in numpy, on the deck of tests/stlsq_symreg_cases.py; against symode_stlsq_sweep at w_sym = 0; against
symode_quad_closure (the solution is a stationary point of the closure); and against the host loop.

Bounds are derived, not measured (``M.xi_bound``): the fp64 Cholesky solve of A contributes 4 n^2 cond(A) 2^-53 max|v| per
coefficient, its rounding to fp32 2^-24 |v|.  Model and kernel perform the same operations in the same order, so equal bytes
are expected and printed; the bound is what is asserted.  cond(A) <= 1e6 and the distance of every deciding coefficient from
the threshold are asserted by the CPU test (tests/test_host_stlsq_symreg_model.py) on the same inputs."""
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import stlsq_symreg_cases as C
from tests import stlsq_symreg_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("xi", "mask", "passes", "near", "fell")
THR = M.f32(C.THRESHOLD)


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _device(eng, G, R, d, gamma, threshold, w_sym, max_iter, n_points=C.N_POINTS, **kw):
    G, R = torch.as_tensor(G).to(DEV), torch.as_tensor(R).to(DEV)
    out = eng.stlsq_sweep_symreg(G if G.dim() == 3 else G[None], R if R.dim() == 3 else R[None], n_points, gamma, threshold, w_sym,
                                 max_iter, d=d, pivot_floor=M.PIVOT_FLOOR, near_band=C.BAND, **kw)
    xi, mask, passes, near, fell = (t.cpu().numpy() for t in out)
    return xi, mask.astype(bool), passes, near, fell


def _bound_of(out, trace):
    """The bound on the last solve's Xi (d, p): cond and n of the last pass's system."""
    last = trace[-1]
    n = len(last[4])
    cond = np.linalg.cond(last[2]) if n else 1.0
    return M.xi_bound(out["xi"], cond, n), cond, n


def _assert_as_the_model(dev, k, out, trace, what):
    """Problem k of the launch ``dev`` against the model's ``out``.  Returns whether the bytes were equal."""
    assert dev[4][k] == out["fell"] == 0 and dev[2][k] == out["passes"], (what, dev[2][k], dev[4][k], out["passes"], out["fell"])
    assert np.array_equal(dev[1][k], out["mask"]) and dev[3][k] == out["near"], what
    bound, cond, n = _bound_of(out, trace)
    err = np.abs(dev[0][k].astype(np.float64) - out["xi"])
    same = dev[0][k].tobytes() == out["xi"].tobytes()
    print(what, "passes", out["passes"], "n", n, "cond %.3g" % cond, "max |dXi| / bound %.3g" % (err / bound).max(), "bit-equal", same)
    assert (err <= bound).all(), (what, err.max())
    return same


# ---- 1. the raw entry against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DECK)
def test_raw_entry_equals_the_model(eng, name):
    G, R, d = C.pair(name)
    same = []
    for gamma in C.GAMMAS:
        for w_sym in C.W_SYMS:
            for max_iter in C.MAX_ITERS:
                out, trace = C.modelled(name, gamma, w_sym, max_iter)
                dev = _device(eng, G, R, d, gamma, C.THRESHOLD, w_sym, max_iter)
                assert dev[0].shape == (1, d, G.shape[0] - d)
                same.append(_assert_as_the_model(dev, 0, out, trace, (name, gamma, w_sym, max_iter)))
    print(name, "bit-equal launches", sum(same), "of", len(same))


# ---- 2. w_sym = 0 is symode_stlsq_sweep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DECK)
def test_without_weight_it_is_the_plain_device_sweep(eng, name):
    G, R, d = C.pair(name)
    Gd = torch.from_numpy(G)[None].to(DEV)
    for gamma in (0.0, M.f32(0.1)):
        for max_iter in C.MAX_ITERS:
            plain = [t.cpu().numpy() for t in eng.stlsq_sweep(Gd, C.N_POINTS, gamma, THR, max_iter, d=d, near_band=C.BAND)]
            for R_any in (R, 3.0 * R + 1.0):                                   # any finite R
                dev = _device(eng, G, R_any, d, gamma, THR, 0.0, max_iter)
                assert not plain[4].any() and not dev[4].any()
                assert np.array_equal(dev[1], plain[1].astype(bool)) and np.array_equal(dev[2], plain[2]) and np.array_equal(dev[3], plain[3])
                spacing = np.spacing(np.abs(plain[0]).max(axis=-1, keepdims=True).astype(np.float32)).astype(np.float64)
                assert (np.abs(dev[0].astype(np.float64) - plain[0]) <= spacing).all(), (name, gamma, max_iter)
                print(name, gamma, max_iter, "bit-equal to symode_stlsq_sweep", dev[0].tobytes() == plain[0].tobytes())


# ---- 3. the solution is a stationary point of the closure ------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DECK)
def test_the_first_solve_is_stationary_for_the_quadratic_closure(eng, name):
    G, R, d = C.pair(name)
    p = G.shape[0] - d
    inv = 1.0 / (C.N_POINTS * d)
    Gd, Rd = torch.from_numpy(G)[None].to(DEV), torch.from_numpy(R)[None].to(DEV)
    Gb = np.zeros((d * p, d * p))
    for j in range(d):
        Gb[j * p:(j + 1) * p, j * p:(j + 1) * p] = G[:p, :p]
    for w_sym in C.W_SYMS:
        w32 = M.f32(w_sym)
        xi, mask, passes, near, fell = eng.stlsq_sweep_symreg(Gd, Rd, C.N_POINTS, 0.0, 0.0, w32, 1, d=d, pivot_floor=M.PIVOT_FLOOR)
        assert passes.tolist() == [1] and fell.tolist() == [0]
        _, grad = eng.quad_closure(Gd, Rd, xi, None, inv, w32)
        v = xi.cpu().numpy().astype(np.float64).reshape(-1)
        # the fp32 rounding of Xi through A (2^-24 |A| |v|, times the 2 inv of the gradient), with a factor 2 for the solve's residual
        bound = 2 * 2 * inv * M.U32 * (np.abs(Gb + w32 * R) @ np.abs(v))
        got = np.abs(grad.cpu().numpy().astype(np.float64).reshape(-1))
        print(name, w_sym, "max |grad| / bound %.3g" % (got / bound).max())
        assert (got <= bound).all(), (name, w_sym, (got / bound).max())


# ---- 4. the exactly singular pair ------------------------------------------------------------------------------------------------
def _sweep_on(eng, G, n_points, d, order, include_exp=False):
    """A SeedSweepSTLSQ whose matrices are handed in on the host (the device route uploads exactly these)."""
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d, device=DEV), torch.zeros(8, d, device=DEV), order, include_exp=include_exp, n_seeds=S,
                        engine=eng, idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.ascontiguousarray(G), n_points
    return sw


def _solve(sw, *a, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, passes = sw.solve(*a, **kw)
    return Xi.numpy(), mask.numpy() > 0, np.asarray(passes), list(sw.near_threshold), [w for w in rec if w.category is RuntimeWarning]


def test_an_exactly_singular_pair_is_flagged_and_solved_on_the_host(eng):
    G1, R1, d = C.pair("osc_o2")
    dev = _device(eng, np.zeros_like(G1), np.zeros_like(R1), d, 0.0, THR, 1.0, 10)
    assert dev[4].tolist() == [1] and dev[2].tolist() == [1]
    both_G, both_R = np.stack([np.zeros_like(G1), G1]), np.stack([np.zeros_like(R1), R1])     # ... next to a problem the device solves
    on_device = _solve(_sweep_on(eng, both_G, C.N_POINTS, d, 2), 0.0, THR, max_iter=10, device=True, rev=(both_R, 1.0))
    assert len(on_device[4]) == 1
    assert "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead" == str(on_device[4][0].message)
    sw = _sweep_on(eng, both_G, C.N_POINTS, d, 2)
    Xi, mask, passes = np.ones((2, d, 6), dtype=np.float32), np.ones((2, d, 6), dtype=bool), np.zeros(2, dtype=np.int64)
    sw.near_threshold = []
    sw._replay(0, both_G[0], 0.0, THR, 10, "min_norm", Xi, mask, passes, rev=(both_R[0], 1.0))     # the host loop's minimum-norm answer
    assert on_device[0][0].tobytes() == Xi[0].tobytes() and np.array_equal(on_device[1][0], mask[0]) and on_device[2][0] == passes[0]
    assert not Xi[0].any() and not mask[0].any()                               # nothing to fit: the zero solution, every entry dropped
    out, trace = C.modelled("osc_o2", 0.0, 1.0, 10)
    assert np.array_equal(on_device[1][1], out["mask"]) and on_device[2][1] == out["passes"]
    assert on_device[0][1].tobytes() == _device(eng, G1, R1, d, 0.0, THR, 1.0, 10)[0][0].tobytes()


# ---- 5. tables -------------------------------------------------------------------------------------------------------------------
def test_a_table_problem_is_the_scalar_launch_on_its_set(eng):
    name = "osc_o3"
    d = 2
    # 3 x 3 x 3 = 27 problems on one set
    G, R, _ = C.pair(name)
    rows = [[g, t, w] for g in (0.0, 0.1, 3.0) for t in (0.05, 0.1, 0.7) for w in (0.0, 1.0, 10.0)]
    table = torch.tensor(rows, dtype=torch.float32)
    grid = _device(eng, G, R, d, 0.0, 0.0, 0.0, 10, hyper=table.to(DEV))
    assert grid[0].shape == (27, 2, 10) and not grid[4].any()
    for s, (g, t, w) in enumerate(table.tolist()):
        one = _device(eng, G, R, d, g, t, w, 10)
        for name_, a, b in zip(NAMES, grid, one):
            assert a[s:s + 1].tobytes() == b.tobytes(), (s, name_)
    assert len({grid[1][s].tobytes() for s in range(27)}) > 2                  # the points decide
    # 2 points x 7 sets
    pairs = [C.pair(name, v) for v in range(7)]
    G7, R7 = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
    points = [(0.0, 0.05, 1.0), (0.1, 0.1, 0.1)]
    table = torch.tensor([list(pt) for pt in points for _ in range(7)], dtype=torch.float32)
    grid = _device(eng, G7, R7, d, 0.0, 0.0, 0.0, 10, hyper=table.to(DEV))
    assert grid[0].shape == (14, 2, 10) and not grid[4].any()
    for s, (g, t, w) in enumerate(table.tolist()):
        one = _device(eng, G7[s % 7], R7[s % 7], d, g, t, w, 10)
        for name_, a, b in zip(NAMES, grid, one):
            assert a[s:s + 1].tobytes() == b.tobytes(), (s, name_)
    whole = _device(eng, G7, R7, d, *points[1], 10)                             # ... and the scalar launch over the seven sets
    for name_, a, b in zip(NAMES, grid, whole):
        assert a[7:].tobytes() == b.tobytes(), name_


# ---- 6. solve(device=True, rev=) against solve(device=False, rev=) -------------------------------------------------------------
def test_solve_on_the_device_equals_solve_on_the_host(eng):
    from symode_amd.sweep import SeedSweepSTLSQ
    from tests.test_gpu_sym_sweep import _operands, _table
    d, order, n_g, n_src, S, m = 2, 3, 2, 900, 7, 203
    x, gx, jgx = _operands(d, n_g, n_src, seed=21)
    gen = torch.Generator().manual_seed(22)
    A = torch.tensor([[-0.1, -1.0], [1.0, -0.1]])
    dx = (x.cpu() @ A.T + 0.2 * torch.randn(n_src, d, generator=gen)).to(DEV)
    idx = _table(S, m, n_src, seed=23)
    gamma, w_sym = M.f32(0.1), 1.0

    def sweep():
        sw = SeedSweepSTLSQ(x, dx, order, n_seeds=S, engine=eng, idx=idx)
        return sw, eng.symreg_reversed_gram_gather(x, gx, jgx, sw.idx, order, 0)

    sw, R = sweep()
    assert tuple(R.shape) == (S, 20, 20) and R.is_cuda
    on_host = _solve(sw, gamma, THR, max_iter=10, rev=(R, w_sym))
    sw, R = sweep()
    on_device = _solve(sw, gamma, THR, max_iter=10, device=True, rev=(R, w_sym))
    assert not on_host[4] and not on_device[4]
    assert np.array_equal(on_device[1], on_host[1]) and np.array_equal(on_device[2], on_host[2])
    Gh, Rh = sw.grams(), R.cpu().numpy()
    assert sw.n_points == m
    for k in range(S):
        trace = []
        out = M.sweep(Gh[k], Rh[k], d, gamma, THR, w_sym, 10, band=C.BAND, trace=trace)
        bound, cond, n = _bound_of(out, trace)
        assert cond <= C.COND_BOUND and np.array_equal(on_device[1][k], out["mask"]) and on_device[2][k] == out["passes"]
        err = np.abs(on_device[0][k].astype(np.float64) - on_host[0][k])
        print("seed", k, "passes", out["passes"], "n", n, "cond %.3g" % cond, "max |dXi| / bound %.3g" % (err / bound).max())
        assert (err <= bound).all(), (k, err.max())
    # a table over the same seeds, with a w_sym column
    hyper = {"threshold": [THR] * S + [0.5] * S, "w_sym": [w_sym] * S + [10.0] * S}
    sw, R = sweep()
    grid = _solve(sw, gamma, 7.0, max_iter=10, device=True, hyper=hyper, rev=(R, 99.0))
    assert grid[0].shape == (2 * S, d, 10) and grid[0][:S].tobytes() == on_device[0].tobytes()
    assert not np.array_equal(grid[1][S:], grid[1][:S])


# ---- 7. main_sweep --symreg_stlsq ------------------------------------------------------------------------------------------------
N_SEEDS = 8
FLAGS = ["--method", "stlsq", "--device_stlsq", "--symreg_stlsq", "--n_seeds", str(N_SEEDS)]


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
    tmp = tmp_path_factory.mktemp("symreg-stlsq-lv")
    _prepare(tmp, "lv")
    return tmp, list(CASES["lv"][0])


def _coefs(tmp, save_dir):
    return np.stack([np.load(tmp / "eval_results" / save_dir / f"seed{s}.npz")["coefficients"] for s in range(N_SEEDS)])


def test_main_sweep_symreg_stlsq_writes_the_result_files(eng, small_lv, capsys, monkeypatch):
    from symode_amd import main_sweep
    from symode_amd.sweep import SeedSweepSTLSQ
    tmp, argv = small_lv
    seen = {}
    solve = SeedSweepSTLSQ.solve

    def recorded(self, *a, **kw):
        out = solve(self, *a, **kw)
        seen.update(sw=self, kw=kw, a=a, out=out)
        return out

    monkeypatch.setattr(SeedSweepSTLSQ, "solve", recorded)
    res = _main(tmp, argv + FLAGS + ["--save_dir", "symreg"])
    out = capsys.readouterr().out
    assert res["n_runs"] == N_SEEDS and "STLSQ passes" in out and f"{N_SEEDS} seeds x " in out
    d = tmp / "eval_results" / "symreg"
    assert sorted(f.name for f in d.iterdir()) == sorted(f"seed{s}.npz" for s in range(N_SEEDS))
    for s in range(N_SEEDS):
        assert sorted(np.load(d / f"seed{s}.npz").files) == ["coefficients", "correct_form", "correct_form_all", "mse", "mse_all"]
    sw, kw = seen["sw"], seen["kw"]
    assert kw["device"] is True and kw["rev"][1] == 0.1 / 1.0 and tuple(kw["rev"][0].shape) == (N_SEEDS, 16, 16)       # w_sym_reg / w_sindy_x
    assert (sw.d, sw.p) == (2, 8) and main_sweep.SYMREG_STLSQ_MAX_COEFS == 64
    Xi, mask, passes = seen["out"]
    assert np.array_equal(_coefs(tmp, "symreg") != 0, (mask.numpy() > 0) & (Xi.numpy() != 0))
    # the files hold the host loop's fit of the same matrices
    host = sw.solve(seen["a"][0], seen["a"][1], max_iter=kw["max_iter"], rev=kw["rev"])
    assert torch.equal(host[1], mask) and np.array_equal(host[2], passes)


def test_main_sweep_symreg_stlsq_grid_is_the_scalar_run_at_every_point(eng, small_lv, capsys):
    tmp, argv = small_lv
    W, T = ("0.1", "5"), ("0.15", "0.4")
    res = _main(tmp, argv + FLAGS + ["--save_dir", "grid", "--stlsq_grid", "w_sym_reg=" + ",".join(W), "--stlsq_grid", "threshold=" + ",".join(T)])
    assert sorted(res) == [0, 1, 2, 3]
    listed = json.loads((tmp / "eval_results" / "grid" / "grid.json").read_text())
    assert listed["axes"] == [["w_sym_reg", [0.1, 5.0]], ["threshold", [0.15, 0.4]]] and listed["n_seeds"] == N_SEEDS
    coefs = []
    for g, (w, t) in enumerate([(w, t) for w in W for t in T]):                  # the first axis slowest
        point = list(argv)
        point[point.index("--threshold") + 1] = t
        point[point.index("--w_sym_reg") + 1] = w
        scalar = _main(tmp, point + FLAGS + ["--save_dir", f"point{g}"])
        assert repr(res[g]) == repr(scalar), g
        for s in range(N_SEEDS):
            want = np.load(tmp / "eval_results" / f"point{g}" / f"seed{s}.npz")
            got = np.load(tmp / "eval_results" / "grid" / f"grid{g}" / f"seed{s}.npz")
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            assert (float(got["w_sym_reg"]), float(got["threshold"]), float(got["w_sindy_reg"])) == (float(w), float(t), 0.0)
        coefs.append(_coefs(tmp, f"point{g}"))
    capsys.readouterr()
    assert not np.array_equal(coefs[0] != 0, coefs[1] != 0) or not np.array_equal(coefs[0], coefs[2])      # the points decide


def test_two_ranks_equal_one_rank_with_one_all_reduce(small_lv):
    from tests.test_gpu_sym_sweep import _free_port, _rank
    tmp, argv = small_lv
    _main(tmp, argv + FLAGS + ["--save_dir", "one-rank"])
    cnt = str(tmp / "allreduce-symreg")
    mp.spawn(_rank, args=(2, _free_port(), str(tmp), argv + FLAGS + ["--save_dir", "two-ranks"], cnt), nprocs=2, join=True)
    one, two = _coefs(tmp, "one-rank"), _coefs(tmp, "two-ranks")
    assert np.array_equal(one != 0, two != 0)
    assert np.allclose(one, two, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(one).max()))
    assert [int(open(f"{cnt}.{r}").read()) for r in range(2)] == [1, 1]         # ONE collective of [G | R | count] per rank
