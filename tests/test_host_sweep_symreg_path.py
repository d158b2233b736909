"""main_sweep --symreg_path (the sparsity path of the device STLSQ sweep with the reversed symmetry regulariser) on the CPU:
the flag is popped before the parser, every refusal it adds is written out below word for word and comes before the data set
and the process group, and without the flag every argument combination keeps its answer -- the combination table of
tests/test_host_sweep_stlsq_path.py (the rows of the host sweep tests under every combination of the STLSQ sweep's other
flags, --symreg_stlsq and --stlsq_path off and on) against tests/golden/sweep_refusals_before_symreg_path.json, the answers
``_refusal`` gave on the commit before this flag (recorded answers only: ``answers[row][extras]`` holds four indices into
``texts``, or null)."""
import json
import os

import pytest

from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable
from tests.test_host_sweep_symreg_stlsq import EXTRAS, MORE, combinations

HERE = os.path.dirname(os.path.abspath(__file__))
BEFORE = os.path.join(HERE, "golden", "sweep_refusals_before_symreg_path.json")
NEW = {
    "wsindy": ("--symreg_path is the regularised sparsity path of --method stlsq: the weak-SINDy sweep (--wsindy) has no symmetry "
               "regulariser (drop one of them)"),
    "method": ("--symreg_path is the sparsity path of the sequential least-squares sweep with the reversed symmetry regulariser: "
               "it needs --method stlsq"),
    "device": ("--symreg_path needs --device_stlsq: the path of every seed is one launch on the device (the host route of "
               "--method stlsq runs the threshold loop of the plain fit)"),
    "stlsq_path": ("--symreg_path does not go with --stlsq_path: they are two paths, the regularised joint one and the plain one per "
                   "equation row (give one of them)"),
    "symreg_stlsq": ("--symreg_path does not go with --symreg_stlsq: the path asks for no threshold, the threshold loop for one (give "
                     "one of them)"),
    "constraint": ("--symreg_path does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: the path under the equivariance "
                   "constraint goes rank deficient and is not covered (drop them, or fit with --equiv_stlsq and a threshold)"),
    "weight": ("--symreg_path needs --w_sym_reg > 0: it is the path of the fit with the symmetry regulariser (--stlsq_path is the "
               "path of the plain least-squares fit)"),
    "type": ("--symreg_path covers the reversed symmetry regulariser only (--sym_reg_type r), not 'i': "
             "the other regularisers are not quadratic in the coefficients"),
    "laligan": ("--symreg_path needs --load_laligan: the regulariser's matrices are built from the group action of a saved "
                "LaLiGAN"),
    "fix": "--symreg_path needs --fix_laligan: g(x), J_g(x) are computed once, from a frozen LaLiGAN",
    "grid": ("--symreg_path does not go with --grid / --lbfgs_grid / --wsindy_grid: they are the grids of other sweeps (its own "
             "is --stlsq_grid w_sym_reg=... / w_sindy_reg=...)"),
    "gelsy": ("--symreg_path fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy has no "
              "regularised form"),
    "latent": "--symreg_path does not cover latent fits (--use_latent)",
    "cpu": "--symreg_path runs on the GPU only (no CPU fallback): a HIP device is required",
    "tol_negative": "--path_tol -0.5: the tolerance of the sparsity path must be a finite number >= 0",
    "tol_nan": "--path_tol nan: the tolerance of the sparsity path must be a finite number >= 0",
    "threshold_axis": ("--symreg_path does not take --stlsq_grid threshold=...: the path visits every support a threshold could reach "
                       "and asks for no threshold (its axes are w_sym_reg and w_sindy_reg)"),
    "axis_positive": ("--stlsq_grid w_sym_reg=0,1: every value must be > 0 (a sweep without the regulariser is another run, without "
                      "--symreg_path)"),
    "axis_unknown": "--stlsq_grid lr_sindy=0.1: unknown name 'lr_sindy', the grid axes are w_sindy_reg, w_sym_reg (name=v1,v2,...)",
    "tol_alone": ("--path_tol needs --stlsq_path: it is the tolerance of the sparsity path (the sparsest model within path_tol of "
                  "the best held-out error); the threshold loop takes --threshold"),
}


# ---- without the flag ------------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_combination_keeps_its_answer():
    import inspect

    from symode_amd.main_sweep import _refusal
    assert inspect.signature(_refusal).parameters["symreg_path"].default is False
    before = json.load(open(BEFORE))
    assert sorted(before) == ["answers", "order", "texts"] and all(isinstance(t, str) for t in before["texts"])
    seen = 0
    for key, args, pos, kw in combinations():
        i, j = key.split(".")
        recorded = before["answers"][i][int(j)]
        for at, (sym, path) in enumerate(((False, False), (False, True), (True, False), (True, True))):
            want = None if recorded[at] is None else before["texts"][recorded[at]]
            assert _refusal(args, *pos, symreg_stlsq=sym, stlsq_path=path, **kw) == want, (key, sym, path)
            assert _refusal(args, *pos, symreg_stlsq=sym, stlsq_path=path, symreg_path=False, **kw) == want, (key, sym, path)
            seen += 1
    assert seen == 4 * sum(len(v) for v in before["answers"].values()) == 4 * (len(TABLE) + 2 * len(MORE)) * len(EXTRAS)
    assert not any("symreg_path" in t for t in before["texts"])
    # the words with which --stlsq_path refuses the regulariser are among them
    assert any(t.startswith("--stlsq_path does not go with --w_sym_reg > 0 / --symreg_stlsq:") for t in before["texts"])


# ---- with the flag ---------------------------------------------------------------------------------------------------------------
DEV = dict(device_stlsq=True)
WITH_FLAG = [
    ("stlsq", R, DEV, None),
    ("stlsq", dict(R, lstsq_driver="gels"), DEV, None),
    ("stlsq", R, dict(DEV, path_tol=0.0), None),
    ("stlsq", R, dict(DEV, path_tol=0.1), None),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0.1,1"]), None),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0.1,1", "w_sindy_reg=0,0.01"]), None),
    ("stlsq", R, dict(DEV, wsindy=True), "wsindy"),
    ("stlsq", R, dict(DEV, wsindy_grid=["threshold=0.1"]), "wsindy"),
    ("lbfgs", R, DEV, "method"),
    ("stlsq", R, {}, "device"),
    ("stlsq", R, dict(DEV, stlsq_path=True), "stlsq_path"),
    ("stlsq", R, dict(DEV, symreg_stlsq=True), "symreg_stlsq"),
    ("stlsq", dict(R, eq_constraint=True), DEV, "constraint"),
    ("stlsq", dict(R, eq_constraint=True), dict(DEV, equiv_stlsq=True), "constraint"),
    ("stlsq", R, dict(DEV, min_norm_stlsq=True), "constraint"),
    ("stlsq", {}, DEV, "weight"),
    ("stlsq", dict(R, sym_reg_type="i"), DEV, "type"),
    ("stlsq", dict(R, load_laligan=None), DEV, "laligan"),
    ("stlsq", dict(R, fix_laligan=False), DEV, "fix"),
    ("stlsq", R, dict(DEV, grid=["threshold=0.1"]), "grid"),
    ("stlsq", R, dict(DEV, lbfgs_grid=["w_sym_reg=0.1,1"]), "grid"),
    ("stlsq", dict(R, lstsq_driver="gelsy"), DEV, "gelsy"),
    ("stlsq", dict(R, use_latent=True), DEV, "latent"),
    ("stlsq", R, dict(DEV, path_tol=-0.5), "tol_negative"),
    ("stlsq", R, dict(DEV, path_tol=float("nan")), "tol_nan"),
    ("stlsq", R, dict(DEV, stlsq_grid=["threshold=0.05,0.1"]), "threshold_axis"),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0.1,1", "threshold=0.1"]), "threshold_axis"),
    ("stlsq", R, dict(DEV, stlsq_grid=["w_sym_reg=0,1"]), "axis_positive"),
    ("stlsq", R, dict(DEV, stlsq_grid=["lr_sindy=0.1"]), "axis_unknown"),
    # two apply: the order of the list in _refusal_symreg_path
    ("lbfgs", R, {}, "method"),
    ("stlsq", {}, {}, "device"),
    ("stlsq", {}, dict(DEV, stlsq_path=True), "stlsq_path"),
    ("stlsq", R, dict(DEV, stlsq_path=True, symreg_stlsq=True), "stlsq_path"),
    ("stlsq", dict(eq_constraint=True), DEV, "constraint"),
    ("stlsq", dict(R, lstsq_driver="gelsy", use_latent=True), DEV, "gelsy"),
    ("stlsq", dict(R, use_latent=True), dict(DEV, path_tol=-0.5), "latent"),
]


@pytest.mark.parametrize("row", WITH_FLAG)
def test_refusals_with_the_flag(row):
    from symode_amd.main_sweep import _refusal
    method, over, kw, want = row
    args = _args("lbfgs", "cuda:0", **over)
    before = dict(args)
    got = _refusal(args, method, 1, None, n_seeds=4, symreg_path=True, **kw)
    assert got == (None if want is None else NEW[want])
    assert args == before


def test_a_cpu_device_and_the_other_rules_with_the_flag():
    from symode_amd.main_sweep import MAX_GRID_PROBLEMS, _refusal
    ok = dict(device_stlsq=True, symreg_path=True)
    assert _refusal(_args("lbfgs", "cpu", **R), "stlsq", **ok) == NEW["cpu"]
    assert _refusal(_args("lbfgs", "cpu", **R), "stlsq", path_tol=-0.5, **ok) == NEW["cpu"]
    assert _refusal(_args("lbfgs", "cpu", **R), "stlsq", 2, ENGINE, **ok) is None              # ranks: the matrices are all-reduced
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", 8, None, **ok) is None
    assert _refusal(_args("adam", "cuda:0", **R), "stlsq", **ok) == TEXT["stlsq_opt"]          # what --method stlsq always asked
    assert _refusal(_args("lbfgs", "cuda:0", **R), "nope", **ok) == "--method nope: lbfgs or stlsq"
    too_many = _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", n_seeds=MAX_GRID_PROBLEMS, stlsq_grid=["w_sym_reg=1,2"], **ok)
    assert too_many.startswith("--stlsq_grid: 2 grid points x")
    # --path_tol belongs to either path, and to nothing else
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", device_stlsq=True, symreg_stlsq=True, path_tol=0.0) == NEW["tol_alone"]


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]
SYM = ["--w_sym_reg", "0.1", "--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan"]
ON = ["--symreg_path", "--device_stlsq"]


@pytest.mark.parametrize("argv, text", [
    (STLSQ + ["--symreg_path"] + SYM, NEW["device"]),
    (STLSQ[:4] + ["--n_seeds", "2"] + ON + SYM, NEW["method"]),
    (STLSQ + ON, NEW["weight"]),
    (STLSQ + ON + SYM[:2] + ["--sym_reg_type", "i"] + SYM[4:], NEW["type"]),
    (STLSQ + ON + SYM[:4] + ["--fix_laligan"], NEW["laligan"]),
    (STLSQ + ON + SYM[:6], NEW["fix"]),
    (STLSQ + ON + SYM + ["--stlsq_path"], NEW["stlsq_path"]),
    (STLSQ + ON + SYM + ["--symreg_stlsq"], NEW["symreg_stlsq"]),
    (STLSQ + ON + SYM + ["--eq_constraint"], NEW["constraint"]),
    (STLSQ + ON + SYM + ["--min_norm_stlsq"], NEW["constraint"]),
    (STLSQ + ON + SYM + ["--wsindy"], NEW["wsindy"]),
    (STLSQ + ON + SYM + ["--grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + ON + SYM + ["--lbfgs_grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + ON + SYM + ["--wsindy_grid", "threshold=0.1"], NEW["wsindy"]),
    (STLSQ + ON + SYM + ["--stlsq_grid", "threshold=0.05,0.1"], NEW["threshold_axis"]),
    (STLSQ + ON + SYM + ["--stlsq_grid", "w_sym_reg=0,1"], NEW["axis_positive"]),
    (STLSQ + ON + SYM + ["--lstsq_driver", "gelsy"], NEW["gelsy"]),
    (STLSQ + ON + SYM + ["--use_latent"], NEW["latent"]),
    (STLSQ + ON + SYM + ["--path_tol", "-0.5"], NEW["tol_negative"]),
    (STLSQ + ON + SYM + ["--path_tol", "nan"], NEW["tol_nan"]),
    (STLSQ + ["--device_stlsq", "--path_tol", "0.05"] + SYM, NEW["tol_alone"]),                  # without the flag: as before
    (STLSQ + ["--device_stlsq"] + SYM, TEXT["stlsq_sym"]),
])
def test_the_flag_is_popped_and_refusals_come_before_data_set_and_process_group(argv, text, monkeypatch):
    import torch.distributed as dist
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    monkeypatch.setattr(dist, "init_process_group", _untouchable("init_process_group"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(list(argv), engine=ENGINE)
    assert str(e.value.code) == text


def test_a_cpu_device_is_refused_before_data_set_and_process_group(monkeypatch):
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(STLSQ + ON + SYM + ["--gpu", "-1"])
    assert str(e.value.code) == NEW["cpu"]


@pytest.mark.parametrize("extra", [[], ["--path_tol", "0.1"], ["--stlsq_grid", "w_sym_reg=0.1,1", "--stlsq_grid", "w_sindy_reg=0,0.01"]])
def test_an_accepted_run_reaches_the_data_set_with_the_flags_gone_from_argv(extra, monkeypatch):
    """The parser never sees --symreg_path / --path_tol / --stlsq_grid (it would reject unknown flags): main gets as far as the
    data set."""
    from symode_amd import main_sweep

    class Reached(Exception):
        pass

    def get_dataset(args):
        raise Reached()

    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", get_dataset)
    monkeypatch.setattr(main_sweep, "init_ranks", lambda *a, **k: None)
    with pytest.raises(Reached):
        main_sweep.main(STLSQ + ON + SYM + extra, engine=ENGINE)


def test_the_grid_names_of_the_flag():
    from symode_amd import main_sweep
    assert main_sweep.SYMREG_PATH_GRID_NAMES == {"w_sindy_reg": "w_reg", "w_sym_reg": "w_sym"}
    assert main_sweep.PATH_TOL == 0.02 and main_sweep.SYMREG_STLSQ_MAX_COEFS == 64
    assert "--symreg_path" in main_sweep.__doc__ and "symode_stlsq_path_symreg" in main_sweep.__doc__


def test_more_than_64_coefficients_are_refused_by_name(monkeypatch):
    """d p is known once the library is: _fit_stlsq raises the SystemExit that names the flag, before any data is touched."""
    import types

    from symode_amd import main_sweep
    from symode_amd.coef_map import CoefMap
    template = types.SimpleNamespace(coef=CoefMap(2, 41, None, True, True), latent_dim=2, poly_order=5, include_sine=False,
                                     include_exp=True, flags=2)
    monkeypatch.setattr(main_sweep, "_template", lambda ctx: (template, None, (None, None)))
    monkeypatch.setattr(main_sweep, "SeedSweepSTLSQ", _untouchable("SeedSweepSTLSQ"))
    monkeypatch.setattr(main_sweep, "_rows", _untouchable("_rows"))
    ctx = types.SimpleNamespace(args={"poly_order": 5, "include_sine": False, "include_exp": True}, symreg_path=True)
    with pytest.raises(SystemExit) as e:
        main_sweep._fit_stlsq(ctx)
    assert str(e.value.code) == ("--symreg_path: the library has d p = 2 x 41 = 82 coefficients, the device fit takes at most 64; "
                                 "use --method lbfgs")
    # d p = 64 passes the rule: the fit goes on to the seeds' rows
    template.coef = CoefMap(2, 32, None, True, True)
    with pytest.raises(AssertionError, match="_rows called before the sweep was refused"):
        main_sweep._fit_stlsq(ctx)
