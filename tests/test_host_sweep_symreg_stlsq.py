"""main_sweep --symreg_stlsq and SeedSweepSTLSQ.solve(rev=...) (the device STLSQ sweep with the reversed symmetry
regulariser) on the CPU: the flag is popped before the parser, every refusal it adds is written out below word for word, the
grid under the flag takes w_sym_reg, and without the flag every argument combination keeps its answer -- the combinations of
the existing host sweep tests are enumerated (``combinations``) and compared with the strings ``_refusal`` gave before the
flag existed, recorded in tests/golden/sweep_refusals_before_symreg_stlsq.json."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_refusals_before_symreg_stlsq.json")
NEW = {
    "wsindy": ("--symreg_stlsq is the regularised fit of --method stlsq: the weak-SINDy sweep (--wsindy) has no symmetry "
               "regulariser (drop one of them)"),
    "method": ("--symreg_stlsq is the sequential-threshold least-squares sweep with the reversed symmetry regulariser: it "
               "needs --method stlsq"),
    "device": ("--symreg_stlsq needs --device_stlsq: the regularised fit of the sweep runs on the device (the host route of "
               "--method stlsq sweeps the plain least-squares fit)"),
    "constraint": ("--symreg_stlsq does not go with --eq_constraint / --equiv_stlsq: the regularised fit under the equivariance "
                   "constraint is not covered (use --method lbfgs)"),
    "min_norm": ("--symreg_stlsq does not go with --min_norm_stlsq: the rank-revealing mode belongs to the constrained launch "
                 "(--equiv_stlsq)"),
    "weight": ("--symreg_stlsq needs --w_sym_reg > 0: it is the fit with the symmetry regulariser (drop --symreg_stlsq for the "
               "plain least-squares fit)"),
    "not_r": ("--symreg_stlsq covers the reversed symmetry regulariser only (--sym_reg_type r), not 'f': the other regularisers "
              "are not quadratic in the coefficients"),
    "not_loaded": "--symreg_stlsq needs --load_laligan: the regulariser's matrices are built from the group action of a saved LaLiGAN",
    "not_frozen": "--symreg_stlsq needs --fix_laligan: g(x), J_g(x) are computed once, from a frozen LaLiGAN",
    "gelsy": ("--symreg_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy has no "
              "regularised form"),
    "latent": "--symreg_stlsq does not cover latent fits (--use_latent)",
    "grid_sym": ("--stlsq_grid w_sym_reg=0,0.1: every value must be > 0 (a sweep without the regulariser is another run, without "
                 "--symreg_stlsq)"),
}


# ---- without the flag ------------------------------------------------------------------------------------------------------------
EXTRAS = [dict(zip(("device_stlsq", "stlsq_grid", "equiv_stlsq", "min_norm_stlsq", "wsindy", "lbfgs_grid"), v)) for v in itertools.product(
    (False, True), (None, ["threshold=0.05,0.1"], ["w_sym_reg=0.1,1"], ["threshold=-1"]), (False, True), (False, True), (False, True),
    (None, ["w_sym_reg=0.1,1"]))]
MORE = [dict(lstsq_driver="gelsy"), dict(R, lstsq_driver="gelsy"), dict(gram_closure=True), dict(R, gram_closure=True),
        dict(device_shuffle=True), dict(eq_constraint=True, constrain_constant=True)]


def combinations():
    """(key, args, positional, keywords) of every call: the rows of tests/test_host_sweep_plan.TABLE (and the overrides the
    grid, equiv and min-norm host tests add to them) under every combination of the other flags of the STLSQ sweep."""
    rows = list(TABLE) + [(m, "lbfgs", over, 1, "cuda:0", None, None) for m in ("lbfgs", "stlsq") for over in MORE]
    for i, (method, optimiser, over, world, device, engine, _) in enumerate(rows):
        for j, extra in enumerate(EXTRAS):
            yield f"{i}.{j}", _args(optimiser, device, **over), (method, world, engine), dict(extra, n_seeds=4)


def test_without_the_flag_every_combination_keeps_its_answer():
    from symode_amd.main_sweep import _refusal
    before = json.load(open(GOLDEN))
    seen = 0
    for key, args, pos, kw in combinations():
        want = before["answers"][key]
        want = None if want is None else before["texts"][want]
        assert _refusal(args, *pos, **kw) == want, (key, args, pos, kw)
        assert _refusal(args, *pos, symreg_stlsq=False, **kw) == want, (key, args, pos, kw)
        seen += 1
    assert seen == len(before["answers"]) == (len(TABLE) + 2 * len(MORE)) * len(EXTRAS)
    # the refusal the flag lifts is among them, word for word
    assert TEXT["stlsq_sym"] in before["texts"] and before["texts"].count(TEXT["stlsq_sym"]) == 1


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_without_the_flag_every_row_of_the_plan_keeps_its_answer(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    args = _args(optimiser, device, **over)
    assert _refusal(args, method, world, engine) == _refusal(args, method, world, engine, symreg_stlsq=False) == (
        None if want is None else TEXT[want])


# ---- with the flag ---------------------------------------------------------------------------------------------------------------
# (method, overrides, keywords) -> the refusal with --symreg_stlsq, None = the sweep runs
DEV = dict(device_stlsq=True)
WITH_FLAG = [
    ("stlsq", R, DEV, None),
    ("stlsq", dict(R, lstsq_driver="gels"), DEV, None),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0.1,1", "threshold=0.05,0.1"]), None),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sindy_reg=0,0.1"]), None),
    ("lbfgs", R, DEV, "method"),
    ("stlsq", R, {}, "device"),
    ("stlsq", {}, DEV, "weight"),
    ("stlsq", dict(R, w_sym_reg=0.0), DEV, "weight"),
    ("stlsq", dict(R, sym_reg_type="f"), DEV, "not_r"),
    ("stlsq", dict(R, load_laligan=None), DEV, "not_loaded"),
    ("stlsq", dict(R, fix_laligan=False), DEV, "not_frozen"),
    ("stlsq", dict(R, eq_constraint=True), DEV, "constraint"),
    ("stlsq", R, dict(DEV, equiv_stlsq=True), "constraint"),
    ("stlsq", dict(R, eq_constraint=True), dict(DEV, equiv_stlsq=True, min_norm_stlsq=True), "constraint"),
    ("stlsq", R, dict(DEV, min_norm_stlsq=True), "min_norm"),
    ("stlsq", dict(R, lstsq_driver="gelsy"), DEV, "gelsy"),
    ("stlsq", dict(R, use_latent=True), DEV, "latent"),
    ("lbfgs", R, dict(wsindy=True), "wsindy"),
    ("stlsq", R, dict(DEV, wsindy=True), "wsindy"),
    ("stlsq", R, dict(DEV, wsindy_grid=["threshold=0.1"]), "wsindy"),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0,0.1"]), "grid_sym"),
    # two apply: the order of the list in the module's docstring
    ("lbfgs", {}, {}, "method"),
    ("stlsq", {}, {}, "device"),
    ("stlsq", dict(sym_reg_type="f"), DEV, "weight"),
    ("stlsq", dict(R, sym_reg_type="f", load_laligan=None), DEV, "not_r"),
    ("stlsq", dict(R, load_laligan=None, fix_laligan=False, lstsq_driver="gelsy"), DEV, "not_loaded"),
    ("stlsq", dict(R, lstsq_driver="gelsy", use_latent=True), DEV, "gelsy"),
]


@pytest.mark.parametrize("row", WITH_FLAG)
def test_refusals_with_the_flag(row):
    from symode_amd.main_sweep import _refusal
    method, over, kw, want = row
    args = _args("lbfgs", "cuda:0", **over)
    before = dict(args)
    got = _refusal(args, method, 1, None, n_seeds=4, symreg_stlsq=True, **kw)
    assert got == (None if want is None else NEW[want])
    assert args == before


def test_the_other_rules_still_apply_with_the_flag():
    from symode_amd.main_sweep import _refusal
    ok = dict(device_stlsq=True, symreg_stlsq=True)
    assert _refusal(_args("adam", "cuda:0", **R), "stlsq", **ok) == TEXT["stlsq_opt"]
    assert _refusal(_args("lbfgs", "cpu", **R), "stlsq", **ok) == TEXT["cpu"]
    assert _refusal(_args("lbfgs", "cpu", **R), "stlsq", 2, ENGINE, **ok) is None               # ranks: [G | R | count] is all-reduced
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", grid=["threshold=0.1"], **ok).startswith("--grid gives every problem")
    assert "--stlsq_grid nope=1" in _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", stlsq_grid=["nope=1"], **ok)
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", stlsq_grid=["threshold=-1"], **ok) == "--stlsq_grid threshold=-1: every value must be >= 0"
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", stlsq_grid=["w_sym_reg=1"] * 2, **ok) == "--stlsq_grid w_sym_reg is given twice: one value list per name"
    assert "one launch takes at most 65535" in _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", n_seeds=40000, stlsq_grid=["w_sym_reg=1,2"], **ok)
    # and the refusal the flag lifts is lifted by nothing else; without the flag the grid does not know the axis
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", device_stlsq=True) == TEXT["stlsq_sym"]
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", device_stlsq=True, stlsq_grid=["w_sym_reg=1"]) == (
        "--stlsq_grid w_sym_reg=1: unknown name 'w_sym_reg', the grid axes are threshold, w_sindy_reg (name=v1,v2,...)")


def test_the_grid_under_the_flag_parses_and_orders_as_the_other_grids():
    from symode_amd import main_sweep as MS
    assert MS.STLSQ_GRID_NAMES == {"threshold": "threshold", "w_sindy_reg": "w_reg"}              # unchanged
    assert MS.SYMREG_STLSQ_GRID_NAMES == {"threshold": "threshold", "w_sindy_reg": "w_reg", "w_sym_reg": "w_sym"}
    axes, why = MS._parse_grid(["w_sym_reg=0.1,1,10", "threshold=0.05,0.1"], MS.SYMREG_STLSQ_GRID_NAMES, "--stlsq_grid")
    assert why is None and axes == [("w_sym_reg", [0.1, 1.0, 10.0]), ("threshold", [0.05, 0.1])]
    points = MS._grid_points(axes)                                                              # the first axis slowest
    assert points == [dict(w_sym_reg=w, threshold=t) for w in (0.1, 1.0, 10.0) for t in (0.05, 0.1)]
    assert [MS._grid_problem(s, 4) for s in (0, 3, 4, 23)] == [(0, 0), (0, 3), (1, 0), (5, 3)]
    assert MS._parse_grid(["w_sym_reg=a"], MS.SYMREG_STLSQ_GRID_NAMES, "--stlsq_grid")[1] == (
        "--stlsq_grid w_sym_reg=a: the values of w_sym_reg must be a non-empty comma-separated list of numbers")


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]
SYM = ["--w_sym_reg", "0.1", "--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan"]


@pytest.mark.parametrize("extra, text", [
    (["--symreg_stlsq"] + SYM, NEW["device"]),
    (["--symreg_stlsq", "--device_stlsq"], NEW["weight"]),
    (["--symreg_stlsq", "--device_stlsq"] + SYM[:4], NEW["not_loaded"]),
    (["--symreg_stlsq", "--device_stlsq", "--lstsq_driver", "gelsy"] + SYM, NEW["gelsy"]),
    (["--symreg_stlsq", "--device_stlsq", "--eq_constraint"] + SYM, NEW["constraint"]),
    (["--symreg_stlsq", "--device_stlsq", "--min_norm_stlsq"] + SYM, NEW["min_norm"]),
    (["--symreg_stlsq", "--device_stlsq", "--wsindy"] + SYM, NEW["wsindy"]),
    (["--symreg_stlsq", "--device_stlsq", "--stlsq_grid", "w_sym_reg=0,0.1"] + SYM, NEW["grid_sym"]),
    (["--device_stlsq"] + SYM, TEXT["stlsq_sym"]),                                              # without the flag: as before
    (SYM, TEXT["stlsq_sym"]),
])
def test_the_flag_is_popped_and_refusals_come_before_data_set_and_process_group(extra, text, monkeypatch):
    import torch.distributed as dist
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    monkeypatch.setattr(dist, "init_process_group", _untouchable("init_process_group"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(STLSQ + extra, engine=ENGINE)
    assert str(e.value.code) == text


def test_an_accepted_run_reaches_the_data_set_with_the_flag_gone_from_argv(monkeypatch):
    """The parser never sees --symreg_stlsq (it would reject an unknown flag): main gets as far as the data set."""
    from symode_amd import main_sweep

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "init_ranks", lambda *a, **k: None)
    monkeypatch.setattr(main_sweep, "get_dataset", stop)
    with pytest.raises(Reached):
        main_sweep.main(STLSQ + ["--device_stlsq", "--symreg_stlsq", "--stlsq_grid", "w_sym_reg=0.1,1"] + SYM, engine=ENGINE)


def test_more_than_64_coefficients_are_refused_by_name(monkeypatch):
    """d p is known once the library is: _fit_stlsq raises the SystemExit that names it, before any data is touched."""
    import types

    from symode_amd import main_sweep
    from symode_amd.coef_map import CoefMap
    template = types.SimpleNamespace(coef=CoefMap(2, 41, None, True, True), latent_dim=2, poly_order=5, include_sine=False,
                                     include_exp=True, flags=2)
    monkeypatch.setattr(main_sweep, "_template", lambda ctx: (template, None, (None, None)))
    monkeypatch.setattr(main_sweep, "SeedSweepSTLSQ", _untouchable("SeedSweepSTLSQ"))
    monkeypatch.setattr(main_sweep, "_rows", _untouchable("_rows"))
    ctx = types.SimpleNamespace(args={"poly_order": 5, "include_sine": False, "include_exp": True}, symreg_stlsq=True)
    with pytest.raises(SystemExit) as e:
        main_sweep._fit_stlsq(ctx)
    assert str(e.value.code) == ("--symreg_stlsq: the library has d p = 2 x 41 = 82 coefficients, the device fit takes at most 64; "
                                 "use --method lbfgs")


# ---- SeedSweepSTLSQ.solve(rev=...) -----------------------------------------------------------------------------------------------
def _sweep(d=2, order=2, S=3):
    from symode_amd.sweep import SeedSweepSTLSQ
    from tests.oracle_engine import OracleEngine
    sw = SeedSweepSTLSQ(torch.zeros(8, d), torch.zeros(8, d), order, n_seeds=S, engine=OracleEngine(),
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    p = sw.p
    sw._gram, sw.n_points = np.stack([np.eye(p + d)] * S), 10
    return sw, np.stack([np.eye(d * p)] * S)


def test_solve_refuses_by_name():
    from symode_amd.coef_map import CoefMap
    sw, R_ = _sweep()
    rev = (R_, 1.0)
    coef = CoefMap(2, sw.p, torch.eye(2 * sw.p)[:, :4].contiguous(), True, True)
    with pytest.raises(ValueError, match=r"rev \(the reversed symmetry regulariser\) does not go with coef"):
        sw.solve(0.0, 0.05, rev=rev, coef=coef)
    with pytest.raises(ValueError, match=r"rev \(the reversed symmetry regulariser\) does not go with min_norm=True"):
        sw.solve(0.0, 0.05, rev=rev, device=True, min_norm=True)
    with pytest.raises(ValueError, match=r"rev \(the reversed symmetry regulariser\) does not go with lstsq_driver='gelsy'"):
        sw.solve(0.0, 0.05, rev=rev, lstsq_driver="gelsy")
    with pytest.raises(ValueError, match=r"hyper: a w_sym column needs rev=\(R, w_sym\)"):
        sw.solve(0.0, 0.05, device=True, lstsq_driver="gels", hyper={"w_sym": [1.0] * 3})
    with pytest.raises(ValueError, match=r"rev must be \(R, w_sym\) with R \(S, d p, d p\) = \(3, 12, 12\)"):
        sw.solve(0.0, 0.05, rev=(R_[:2], 1.0))
    for bad in (dict(rev=(R_, -1.0)), dict(rev=(R_, float("nan"))), dict(rev=(R_, float("inf")))):
        with pytest.raises(ValueError, match="w_sym, the ridge weight and the threshold must be finite and >= 0"):
            sw.solve(0.0, 0.05, **bad)
    for w, t in ((-0.1, 0.05), (0.0, -1.0), (float("nan"), 0.05), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="w_sym, the ridge weight and the threshold must be finite and >= 0"):
            sw.solve(w, t, rev=rev)
    big, R_big = _sweep(d=2, order=5, S=1)[0], np.zeros((1, 82, 82))
    big.p = 41                                                              # (order 5 plus sine and exp: 2 x 41 unknowns)
    with pytest.raises(ValueError, match=r"d p = 2 x 41 = 82 unknowns, the joint system of a pass takes at most 64"):
        big.solve(0.0, 0.05, rev=(R_big, 1.0))
    # with rev=None every path is what it was: the identity problem thresholds nothing on the host route
    Xi, mask, passes = sw.solve(0.0, 0.05, lstsq_driver="gels")
    assert tuple(Xi.shape) == (3, 2, sw.p) and passes.tolist() == [2, 2, 2]


def test_the_device_route_refuses_values_and_columns_by_name(monkeypatch):
    """``_solve_device`` decides on the table before it touches the device (grams is never reached)."""
    sw, R_ = _sweep()
    monkeypatch.setattr(type(sw), "grams", _untouchable("grams"))
    with pytest.raises(ValueError, match="are w_reg, threshold and w_sym, got"):
        sw.solve(0.0, 0.05, rev=(R_, 1.0), device=True, hyper={"lr": [1.0] * 3})
    with pytest.raises(ValueError, match="the ridge weight and the threshold of every problem must be finite and >= 0"):
        sw.solve(0.0, 0.05, rev=(R_, 1.0), device=True, hyper={"threshold": [0.1, -0.1, 0.1]})
    with pytest.raises(ValueError, match="hyper: the per-problem columns of the STLSQ sweep are w_reg and threshold, got"):
        sw.solve(0.0, 0.05, device=True, lstsq_driver="gels", hyper={"lr": [1.0] * 3})        # without rev: the words it had


def test_the_words_of_the_device_routes_are_whole(monkeypatch):
    """The refusals of ``_solve_device``, ``solve_path`` and ``_solve_path_symreg`` that read a ``hyper`` table, character for
    character as they stood before the table got one parser."""
    import re
    sw, R_ = _sweep()
    monkeypatch.setattr(type(sw), "grams", _untouchable("grams"))
    V, rev = np.zeros((1, sw.p + 2, sw.p + 2)), (R_, 1.0)
    solve = lambda **kw: sw.solve(0.0, 0.05, rev=rev, device=True, **kw)                       # noqa: E731
    path = lambda *a, **kw: sw.solve_path(0.0, V, *(a or (0.02,)), **kw)                       # noqa: E731
    for call, words in [
        (lambda: solve(hyper={"lr": [1.0] * 3}),
         "hyper: the per-problem columns of the STLSQ sweep with the reversed regulariser are w_reg, threshold and w_sym, got ['lr']"),
        (lambda: solve(hyper={}), "hyper: the per-problem columns of the STLSQ sweep are w_reg and threshold, got []"),
        (lambda: solve(hyper={"w_sym": [1.0, float("nan"), 1.0]}),
         "the weight w_sym of the reversed regulariser must be finite and >= 0 for every problem"),
        (lambda: solve(hyper={"w_sym": [1.0] * 4}),
         "hyper: every column needs one value per problem, a multiple of the 3 seeds (problem s on seed s % 3); got lengths [4]"),
        (lambda: solve(hyper={"w_sym": [1.0] * 3, "w_reg": [0.0] * 6}),
         "hyper: every column needs one value per problem, a multiple of the 3 seeds (problem s on seed s % 3); got lengths [3, 6]"),
        (lambda: solve(hyper={"w_sym": [-1.0] * 3, "threshold": [float("inf")] * 3}),               # the threshold is read first
         "the ridge weight and the threshold of every problem must be finite and >= 0"),
        (lambda: path(hyper={"w_sym": [1.0] * 3}),
         "solve_path: hyper (a per-problem table of w_reg / w_sym) needs rev=(R, w_sym): the table is the regularised path's"),
        (lambda: path(device=False, rev=rev, hyper={"lr": [1.0]}),                                  # the route before the columns
         "solve_path: hyper (a per-problem table of w_reg / w_sym) needs device=True: the host route takes one value each"),
        (lambda: path(rev=rev, hyper={}), "solve_path: hyper: the per-problem columns of the regularised path are w_reg and w_sym, got []"),
        (lambda: path(rev=rev, hyper={"w_sym": [1.0] * 4}),
         "solve_path: hyper: every column needs one value per problem, a multiple of the 3 seeds (problem s on seed s % 3); got lengths [4]"),
        (lambda: path(rev=rev, hyper={"w_reg": [0.0, -1.0, 0.0]}), "solve_path: the ridge weight and w_sym of every problem must be finite and >= 0"),
        (lambda: path(float("nan")), "solve_path: tol must be finite and >= 0, got nan"),
    ]:
        with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
            call()
