"""main_sweep --stlsq_path / --path_tol and SeedSweepSTLSQ.solve_path (the sparsity path of the device STLSQ sweep) on the CPU:
the flags are popped before the parser, every refusal they add is written out below word for word and comes before the data
set and the process group, and without the flag every argument combination keeps its answer -- the combinations of the
existing host sweep tests are enumerated and compared with the strings ``_refusal`` gave before the flag existed: those of
tests/golden/sweep_refusals_before_symreg_stlsq.json, and tests/golden/sweep_refusals_before_stlsq_path.json, recorded from
the commit before this flag with --symreg_stlsq off and on (key ``<row>.<extras>.<symreg_stlsq>``).  Then
``solve_path(device=False)``, the host twin, against the numpy model of the kernel."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_path_cases as P
from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable
from tests.test_host_sweep_symreg_stlsq import EXTRAS, MORE, combinations

HERE = os.path.dirname(os.path.abspath(__file__))
BEFORE_SYMREG = os.path.join(HERE, "golden", "sweep_refusals_before_symreg_stlsq.json")
BEFORE_PATH = os.path.join(HERE, "golden", "sweep_refusals_before_stlsq_path.json")
NEW = {
    "method": ("--stlsq_path is the sparsity path of the sequential least-squares sweep (backward elimination scored on the "
               "validation set): it needs --method stlsq"),
    "device": ("--stlsq_path needs --device_stlsq: the path of every seed is one launch on the device (the host route of "
               "--method stlsq runs the threshold loop)"),
    "constraint": ("--stlsq_path does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: the path under the "
                   "equivariance constraint is a joint system over the rows and is not covered (drop them, or fit with "
                   "--equiv_stlsq and a threshold)"),
    "symreg": ("--stlsq_path does not go with --w_sym_reg > 0 / --symreg_stlsq: the path with the symmetry regulariser is a joint "
               "system over the rows and is not covered (drop them, or fit with --symreg_stlsq and a threshold)"),
    "wsindy": "--stlsq_path is the path of --method stlsq: the weak-SINDy sweep (--wsindy) is not covered (drop one of them)",
    "grid": ("--stlsq_path does not go with --grid / --lbfgs_grid / --stlsq_grid / --wsindy_grid: the path visits every "
             "support a threshold grid could reach and asks for no threshold (drop the grid)"),
    "gelsy": ("--stlsq_path fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the "
              "host route (drop one of them)"),
    "latent": "--stlsq_path does not cover latent fits (--use_latent)",
    "cpu": "--stlsq_path runs on the GPU only (no CPU fallback): a HIP device is required",
    "tol_negative": "--path_tol -0.5: the tolerance of the sparsity path must be a finite number >= 0",
    "tol_inf": "--path_tol inf: the tolerance of the sparsity path must be a finite number >= 0",
    "tol_nan": "--path_tol nan: the tolerance of the sparsity path must be a finite number >= 0",
    "tol_alone": ("--path_tol needs --stlsq_path: it is the tolerance of the sparsity path (the sparsest model within path_tol of "
                  "the best held-out error); the threshold loop takes --threshold"),
}


# ---- without the flag ------------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_combination_keeps_its_answer():
    from symode_amd.main_sweep import _refusal
    old, new = json.load(open(BEFORE_SYMREG)), json.load(open(BEFORE_PATH))
    seen = 0
    for key, args, pos, kw in combinations():
        for sym in (False, True):
            want = new["answers"][f"{key}.{int(sym)}"]
            want = None if want is None else new["texts"][want]
            assert _refusal(args, *pos, symreg_stlsq=sym, **kw) == want, (key, sym)
            assert _refusal(args, *pos, symreg_stlsq=sym, stlsq_path=False, path_tol=None, **kw) == want, (key, sym)
            seen += 1
        want = old["answers"][key]                              # and the older recording, which knows no --symreg_stlsq
        assert _refusal(args, *pos, stlsq_path=False, **kw) == (None if want is None else old["texts"][want]), key
    assert seen == len(new["answers"]) == 2 * (len(TABLE) + 2 * len(MORE)) * len(EXTRAS)
    assert not any("stlsq_path" in t or "path_tol" in t for t in new["texts"])


# ---- with the flag ---------------------------------------------------------------------------------------------------------------
DEV = dict(device_stlsq=True)
WITH_FLAG = [
    ("stlsq", {}, DEV, None),
    ("stlsq", dict(lstsq_driver="gels"), DEV, None),
    ("stlsq", {}, dict(DEV, path_tol=0.0), None),
    ("stlsq", {}, dict(DEV, path_tol=0.1), None),
    ("lbfgs", {}, DEV, "method"),
    ("stlsq", {}, {}, "device"),
    ("stlsq", dict(eq_constraint=True), DEV, "constraint"),
    ("stlsq", dict(eq_constraint=True), dict(DEV, equiv_stlsq=True), "constraint"),
    ("stlsq", dict(eq_constraint=True), dict(DEV, equiv_stlsq=True, min_norm_stlsq=True), "constraint"),
    ("stlsq", {}, dict(DEV, min_norm_stlsq=True), "constraint"),
    ("stlsq", R, DEV, "symreg"),
    ("stlsq", R, dict(DEV, symreg_stlsq=True), "symreg"),
    ("stlsq", {}, dict(DEV, symreg_stlsq=True), "symreg"),
    ("stlsq", {}, dict(DEV, wsindy=True), "wsindy"),
    ("stlsq", {}, dict(DEV, wsindy_grid=["threshold=0.1"]), "wsindy"),
    ("stlsq", {}, dict(DEV, grid=["threshold=0.1"]), "grid"),
    ("stlsq", {}, dict(DEV, lbfgs_grid=["threshold=0.1"]), "grid"),
    ("stlsq", {}, dict(DEV, stlsq_grid=["threshold=0.05,0.1"]), "grid"),
    ("stlsq", dict(lstsq_driver="gelsy"), DEV, "gelsy"),
    ("stlsq", dict(use_latent=True), DEV, "latent"),
    ("stlsq", {}, dict(DEV, path_tol=-0.5), "tol_negative"),
    ("stlsq", {}, dict(DEV, path_tol=float("inf")), "tol_inf"),
    ("stlsq", {}, dict(DEV, path_tol=float("nan")), "tol_nan"),
    # two apply: the order of the list in _refusal_stlsq_path
    ("lbfgs", {}, {}, "method"),
    ("stlsq", dict(eq_constraint=True), {}, "device"),
    ("stlsq", dict(R, eq_constraint=True), DEV, "constraint"),
    ("stlsq", R, dict(DEV, wsindy=True), "symreg"),
    ("stlsq", {}, dict(DEV, wsindy=True, stlsq_grid=["threshold=0.1"]), "wsindy"),
    ("stlsq", dict(lstsq_driver="gelsy"), dict(DEV, stlsq_grid=["threshold=0.1"]), "grid"),
    ("stlsq", dict(lstsq_driver="gelsy", use_latent=True), DEV, "gelsy"),
    ("stlsq", dict(use_latent=True), dict(DEV, path_tol=-0.5), "latent"),
]


@pytest.mark.parametrize("row", WITH_FLAG)
def test_refusals_with_the_flag(row):
    from symode_amd.main_sweep import _refusal
    method, over, kw, want = row
    args = _args("lbfgs", "cuda:0", **over)
    before = dict(args)
    got = _refusal(args, method, 1, None, n_seeds=4, stlsq_path=True, **kw)
    assert got == (None if want is None else NEW[want])
    assert args == before


def test_a_cpu_device_and_the_other_rules_with_the_flag():
    from symode_amd.main_sweep import _refusal
    ok = dict(device_stlsq=True, stlsq_path=True)
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", **ok) == NEW["cpu"]
    assert _refusal(_args("lbfgs", "cpu", use_latent=True), "stlsq", **ok) == NEW["latent"]
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", path_tol=-0.5, **ok) == NEW["cpu"]
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", 2, ENGINE, **ok) is None                   # ranks: the matrices are all-reduced
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", 8, None, **ok) is None
    assert _refusal(_args("adam", "cuda:0"), "stlsq", **ok) == TEXT["stlsq_opt"]               # what --method stlsq always asked
    assert _refusal(_args("lbfgs", "cuda:0", device_shuffle=True), "stlsq", **ok).startswith("--device_shuffle draws")
    assert _refusal(_args("lbfgs", "cuda:0"), "nope", **ok) == "--method nope: lbfgs or stlsq"


def test_path_tol_without_the_flag_is_refused_whatever_else_is_given():
    from symode_amd.main_sweep import _refusal
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", device_stlsq=True, path_tol=0.05) == NEW["tol_alone"]
    assert _refusal(_args("lbfgs", "cuda:0"), "lbfgs", path_tol=0.05) == NEW["tol_alone"]
    assert _refusal(_args("adam", "cuda:0", **R), "lbfgs", 4, path_tol=-1.0, grid=["nope=1"]) == NEW["tol_alone"]
    assert _refusal(_args("lbfgs", "cuda:0", **R), "stlsq", device_stlsq=True, symreg_stlsq=True, path_tol=0.0) == NEW["tol_alone"]


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]
SYM = ["--w_sym_reg", "0.1", "--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan"]


@pytest.mark.parametrize("argv, text", [
    (STLSQ + ["--stlsq_path"], NEW["device"]),
    (STLSQ[:4] + ["--n_seeds", "2", "--stlsq_path", "--device_stlsq"], NEW["method"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--eq_constraint"], NEW["constraint"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--eq_constraint", "--equiv_stlsq"], NEW["constraint"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--min_norm_stlsq"], NEW["constraint"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq"] + SYM, NEW["symreg"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--symreg_stlsq"] + SYM, NEW["symreg"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--wsindy"], NEW["wsindy"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--stlsq_grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--lbfgs_grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--wsindy_grid", "threshold=0.1"], NEW["wsindy"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--lstsq_driver", "gelsy"], NEW["gelsy"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--use_latent"], NEW["latent"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--path_tol", "-0.5"], NEW["tol_negative"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--path_tol", "inf"], NEW["tol_inf"]),
    (STLSQ + ["--stlsq_path", "--device_stlsq", "--path_tol", "nan"], NEW["tol_nan"]),
    (STLSQ + ["--device_stlsq", "--path_tol", "0.05"], NEW["tol_alone"]),
    (STLSQ + ["--path_tol", "0.05"], NEW["tol_alone"]),
    (STLSQ + ["--device_stlsq"] + SYM, TEXT["stlsq_sym"]),                                       # without the flag: as before
    (STLSQ + ["--eq_constraint"], TEXT["stlsq_eq"]),
])
def test_the_flags_are_popped_and_refusals_come_before_data_set_and_process_group(argv, text, monkeypatch):
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
        main_sweep.main(STLSQ + ["--stlsq_path", "--device_stlsq", "--gpu", "-1"])
    assert str(e.value.code) == NEW["cpu"]


@pytest.mark.parametrize("extra", [["--stlsq_path"], ["--stlsq_path", "--path_tol", "0.1"], ["--path_tol", "0", "--stlsq_path"]])
def test_an_accepted_run_reaches_the_data_set_with_the_flags_gone_from_argv(extra, monkeypatch):
    """The parser never sees --stlsq_path / --path_tol (it would reject unknown flags): main gets as far as the data set."""
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
        main_sweep.main(STLSQ + ["--device_stlsq"] + extra, engine=ENGINE)


def test_the_aggregate_reads_the_seeds_files_and_not_path_npz(tmp_path, monkeypatch, capsys):
    from symode_amd import evaluation
    from symode_amd.main_sweep import _write_results
    monkeypatch.chdir(tmp_path)
    truth = evaluation.truth_table("dosc", 6, False, False)
    Xi = np.stack([truth, truth]).astype(np.float32)
    _write_results(dict(save_dir="run"), [4, 5], Xi, Xi != 0, truth)
    before = evaluation.aggregate_results("run", min_seed=4, max_seed=6)
    np.savez(tmp_path / "eval_results" / "run" / "path.npz", best=np.zeros((2, 2), dtype=np.int32))
    after = evaluation.aggregate_results("run", min_seed=4, max_seed=6)
    assert repr(after) == repr(before) and after["n_runs"] == 2


def test_the_default_tolerance():
    from symode_amd import main_sweep
    assert main_sweep.PATH_TOL == 0.02 == P.TOL_DEFAULT


# ---- SeedSweepSTLSQ.solve_path(device=False): the host twin ----------------------------------------------------------------------
def _sweep(name):
    from symode_amd.sweep import SeedSweepSTLSQ
    from tests.oracle_engine import OracleEngine
    d, G, V, _, _ = P.case(name)
    S, p = G.shape[0], G.shape[1] - d
    sw = SeedSweepSTLSQ(torch.zeros(8, d), torch.zeros(8, d), 1, n_seeds=S, engine=OracleEngine(), idx=torch.zeros(S, 4, dtype=torch.int32))
    sw.p, sw._gram, sw.n_points = p, G.copy(), 200                # the deck's matrices in place of a gather launch
    return sw, V


@pytest.mark.parametrize("name, gamma, tol", [("o3", 0.0, P.TOL_DEFAULT), ("d3_o2_exp", 0.1, 0.0), ("zero_rhs", 0.1, P.TOL_DEFAULT),
                                              ("diag_tie", 0.0, 0.0)])
def test_the_host_twin_against_the_model(name, gamma, tol):
    sw, V = _sweep(name)
    m, r = P.model(name, gamma, tol), P.reference(name, gamma, tol)
    Xi, mask, rec = sw.solve_path(gamma * gamma, V, tol, floor_rel=P.FLOOR_REL, device=False, keep_path=True)
    assert Xi.dtype == torch.float32 and mask.dtype == torch.float32 and tuple(Xi.shape) == tuple(mask.shape) == m["Xi"].shape
    assert np.array_equal(rec["order"], m["order"]) and np.array_equal(rec["best"], m["best"])
    assert np.array_equal(mask.numpy().astype(bool), m["mask"]) and np.array_equal(rec["near"], m["near"])
    assert (np.abs(rec["path_xi"].astype(np.float64) - r["x"]) <= r["coef_bound"]).all()
    assert np.array_equal(Xi.numpy(), np.take_along_axis(rec["path_xi"], rec["best"][:, :, None, None].astype(np.int64), 2)[:, :, 0])
    d, G, _, _, _ = P.case(name)
    p = G.shape[1] - d
    for key, Hs in (("rss_train", G), ("rss_val", V)):
        for s in range(G.shape[0]):
            for j in range(d):
                for t in range(p + 1):
                    v = rec["path_xi"][s, j, t].astype(np.float64)
                    assert abs(rec[key][s, j, t] - P._quad(Hs[s % Hs.shape[0]], p, j, v)) <= P.err_bound(Hs[s % Hs.shape[0]], p, j, v)
    assert sorted(rec) == ["best", "near", "order", "path_xi", "rss_train", "rss_val"]
    assert "path_xi" not in sw.solve_path(gamma * gamma, V, tol, device=False)[2]


def test_one_validation_matrix_serves_all_seeds():
    sw, V = _sweep("o2")
    one = sw.solve_path(0.01, V[:1], 0.02, device=False)
    each = sw.solve_path(0.01, np.repeat(V[:1], 3, axis=0), 0.02, device=False)
    assert torch.equal(one[0], each[0]) and torch.equal(one[1], each[1]) and np.array_equal(one[2]["rss_val"], each[2]["rss_val"])


def test_a_singular_support_gets_the_minimum_norm_answer_and_the_warning():
    from symode_amd import lstsq
    from symode_amd.sindy import stlsq_path_from_gram
    rng = np.random.RandomState(0)
    B = rng.randn(50, 3)
    rows = np.concatenate([B, B[:, :1], B @ np.array([[1.0], [0.5], [0.0]])], axis=1)              # column 3 = column 0
    G = rows.T @ rows
    lstsq._warned_singular = False
    with pytest.warns(RuntimeWarning, match="singular normal equations under the full-rank"):
        Xi, mask, rec = stlsq_path_from_gram(G, G, 0.0, 0.0, 1e-10, 1e-4, 1)
    assert np.isfinite(Xi).all() and np.isfinite(rec["rss_val"]).all()
    full = rec["path_xi"][0, 0]                                                                    # the singular step: all columns
    assert abs(full[0] - full[3]) < 1e-6 and abs(full[0] + full[3] - 1.0) < 1e-6                   # the weight shared: minimum norm
    assert mask[0].sum() == 2 and mask[0, 1] and abs(Xi[0, 1] - 0.5) < 1e-6                        # one of the twins left; an exact fit
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        stlsq_path_from_gram(G, G, 0.1, 0.0, 1e-10, 1e-4, 1)                                       # a ridge makes it regular


def test_solve_path_refuses_by_name():
    sw, V = _sweep("o2")
    for kw, word in ((dict(w_sindy_reg=-1.0), "w_sindy_reg"), (dict(w_sindy_reg=float("nan")), "w_sindy_reg"), (dict(tol=-0.1), "tol"),
                     (dict(tol=float("inf")), "tol"), (dict(floor_rel=-1e-10), "floor_rel")):
        a = dict(dict(w_sindy_reg=0.0, tol=0.02, floor_rel=1e-10), **kw)
        with pytest.raises(ValueError, match=f"solve_path: {word} must be finite and >= 0"):
            sw.solve_path(a["w_sindy_reg"], V, a["tol"], floor_rel=a["floor_rel"], device=False)
    for bad in (V[:2], V[:, :-1, :-1], V[0]):
        with pytest.raises(ValueError, match="solve_path: val_gram must be"):
            sw.solve_path(0.0, bad, 0.02, device=False)
