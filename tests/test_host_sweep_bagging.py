"""main_sweep --bagging / --bag_chunks / --bag_inclusion and SeedSweepSTLSQ.solve_bagged(device=False) on the CPU: the flags are
popped before the parser, every refusal they add is written out below word for word and comes before the data set and the
process group, and without the flags every argument combination keeps its answer -- the combination table of
tests/test_host_sweep_symreg_stlsq.py under every combination of --symreg_stlsq, --stlsq_path and --symreg_path against
tests/golden/sweep_refusals_before_bagging.json, the answers ``_refusal`` gave on the commit before these flags
(``answers[row][extras]`` holds eight indices into ``texts``, or null, in the order of itertools.product over ``order``)."""
import itertools
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests.test_host_sweep_plan import ENGINE, R, TABLE, _args, _untouchable
from tests.test_host_sweep_symreg_stlsq import EXTRAS, MORE, combinations

HERE = os.path.dirname(os.path.abspath(__file__))
BEFORE = os.path.join(HERE, "golden", "sweep_refusals_before_bagging.json")
NEW = {
    "alone_chunks": ("--bag_chunks needs --bagging B: they are the chunk count and the inclusion levels of the bagged threshold fit "
                     "(B bootstrap replicas per seed)"),
    "alone_inclusion": ("--bag_inclusion needs --bagging B: they are the chunk count and the inclusion levels of the bagged "
                        "threshold fit (B bootstrap replicas per seed)"),
    "alone_both": ("--bag_chunks and --bag_inclusion needs --bagging B: they are the chunk count and the inclusion levels of the "
                   "bagged threshold fit (B bootstrap replicas per seed)"),
    "wsindy": "--bagging is the bagged fit of --method stlsq: the weak-SINDy sweep (--wsindy) is not covered (drop one of them)",
    "method": ("--bagging is block-bootstrap bagging of the sequential-threshold least-squares sweep (ensemble SINDy): it needs "
               "--method stlsq"),
    "device": ("--bagging needs --device_stlsq: replicas, replica fits and refit are launches on the device (the host route of "
               "--method stlsq fits one subsample per seed)"),
    "constraint": ("--bagging does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: bagging under the equivariance "
                   "constraint is not covered (drop them, or fit with --equiv_stlsq)"),
    "symreg": ("--bagging does not go with --w_sym_reg > 0 / --symreg_stlsq / --symreg_path: bagging with the symmetry regulariser "
               "needs a joint refit over the rows and is not covered (drop them, or fit with --symreg_stlsq)"),
    "path": ("--bagging does not go with --stlsq_path / --path_tol: the replicas are fit by the threshold loop, the path asks "
             "for no threshold (give one of them)"),
    "grid": ("--bagging does not go with --grid / --lbfgs_grid / --stlsq_grid / --wsindy_grid: its own grid is the list of "
             "inclusion levels, --bag_inclusion v1,v2,... (drop the grid)"),
    "gelsy": ("--bagging fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the host "
              "route (drop one of them)"),
    "latent": "--bagging does not cover latent fits (--use_latent)",
    "cpu": "--bagging runs on the GPU only (no CPU fallback): a HIP device is required",
    "ranks": ("--bagging runs in one process: the chunk matrices of the replicas are not all-reduced over ranks yet (give every "
              "GPU its own block of seeds, python -m symode_amd.main_sweep --seed <first> --n_seeds <count> ... per process)"),
    "replicas": "--bagging 0: the number of bootstrap replicas per seed must be >= 1",
    "chunks": "--bag_chunks 1025: a seed's rows are cut into 1 .. 1024 chunks",
    "chunks_zero": "--bag_chunks 0: a seed's rows are cut into 1 .. 1024 chunks",
    "levels": ("--bag_inclusion 0.5,1.5: the inclusion levels must be a non-empty comma-separated list of multiples of 0.001 in "
               "[0, 1] (the share of replicas a term has to survive in)"),
    "levels_fine": ("--bag_inclusion 0.5005: the inclusion levels must be a non-empty comma-separated list of multiples of 0.001 in "
                    "[0, 1] (the share of replicas a term has to survive in)"),
    "levels_word": ("--bag_inclusion half: the inclusion levels must be a non-empty comma-separated list of multiples of 0.001 in "
                    "[0, 1] (the share of replicas a term has to survive in)"),
    "levels_twice": "--bag_inclusion 0.5,1,0.5: a level is given twice",
    "too_many": "--bagging: 4 seeds x 16384 replicas = 65536 replica problems, one launch takes at most 65535",
}


# ---- without the flags -----------------------------------------------------------------------------------------------------------
def test_without_the_flags_every_combination_keeps_its_answer():
    import inspect

    from symode_amd.main_sweep import _refusal
    for name in ("bagging", "bag_chunks", "bag_inclusion"):
        assert inspect.signature(_refusal).parameters[name].default is None
    before = json.load(open(BEFORE))
    assert sorted(before) == ["answers", "order", "texts"] and before["order"] == ["symreg_stlsq", "stlsq_path", "symreg_path"]
    seen = 0
    for key, args, pos, kw in combinations():
        i, j = key.split(".")
        recorded = before["answers"][i][int(j)]
        for at, (sym, path, spath) in enumerate(itertools.product((False, True), repeat=3)):
            want = None if recorded[at] is None else before["texts"][recorded[at]]
            flags = dict(symreg_stlsq=sym, stlsq_path=path, symreg_path=spath)
            assert _refusal(args, *pos, **flags, **kw) == want, (key, flags)
            assert _refusal(args, *pos, **flags, bagging=None, bag_chunks=None, bag_inclusion=None, **kw) == want, (key, flags)
            seen += 1
    assert seen == 8 * sum(len(v) for v in before["answers"].values()) == 8 * (len(TABLE) + 2 * len(MORE)) * len(EXTRAS)
    assert not any("bagging" in t or "bag_" in t for t in before["texts"])


# ---- with the flags --------------------------------------------------------------------------------------------------------------
DEV = dict(device_stlsq=True, bagging=4)
WITH_FLAG = [
    ("stlsq", {}, DEV, 1, None),
    ("stlsq", dict(lstsq_driver="gels"), DEV, 1, None),
    ("stlsq", {}, dict(DEV, bag_chunks=8), 1, None),
    ("stlsq", {}, dict(DEV, bag_chunks=1), 1, None),
    ("stlsq", {}, dict(DEV, bag_chunks=1024), 1, None),
    ("stlsq", {}, dict(DEV, bag_inclusion="0.5,1"), 1, None),
    ("stlsq", {}, dict(DEV, bag_inclusion="0,0.001,0.999,1"), 1, None),
    ("stlsq", {}, dict(DEV, bagging=16383), 1, None),
    ("stlsq", {}, dict(device_stlsq=True, bag_chunks=8), 1, "alone_chunks"),
    ("stlsq", {}, dict(device_stlsq=True, bag_inclusion="0.5"), 1, "alone_inclusion"),
    ("lbfgs", {}, dict(bag_chunks=8, bag_inclusion="0.5"), 1, "alone_both"),
    ("stlsq", {}, dict(DEV, wsindy=True), 1, "wsindy"),
    ("stlsq", {}, dict(DEV, wsindy_grid=["threshold=0.1"]), 1, "wsindy"),
    ("lbfgs", {}, DEV, 1, "method"),
    ("stlsq", {}, dict(bagging=4), 1, "device"),
    ("stlsq", dict(eq_constraint=True), DEV, 1, "constraint"),
    ("stlsq", dict(eq_constraint=True), dict(DEV, equiv_stlsq=True), 1, "constraint"),
    ("stlsq", {}, dict(DEV, min_norm_stlsq=True), 1, "constraint"),
    ("stlsq", R, DEV, 1, "symreg"),
    ("stlsq", R, dict(DEV, symreg_stlsq=True), 1, "symreg"),
    ("stlsq", R, dict(DEV, symreg_path=True), 1, "symreg"),
    ("stlsq", {}, dict(DEV, stlsq_path=True), 1, "path"),
    ("stlsq", {}, dict(DEV, path_tol=0.05), 1, "path"),
    ("stlsq", {}, dict(DEV, grid=["threshold=0.1"]), 1, "grid"),
    ("stlsq", {}, dict(DEV, lbfgs_grid=["threshold=0.1"]), 1, "grid"),
    ("stlsq", {}, dict(DEV, stlsq_grid=["threshold=0.05,0.1"]), 1, "grid"),
    ("stlsq", dict(lstsq_driver="gelsy"), DEV, 1, "gelsy"),
    ("stlsq", dict(use_latent=True), DEV, 1, "latent"),
    ("stlsq", {}, DEV, 2, "ranks"),
    ("stlsq", {}, DEV, 8, "ranks"),
    ("stlsq", {}, dict(DEV, bagging=0), 1, "replicas"),
    ("stlsq", {}, dict(DEV, bag_chunks=1025), 1, "chunks"),
    ("stlsq", {}, dict(DEV, bag_chunks=0), 1, "chunks_zero"),
    ("stlsq", {}, dict(DEV, bag_inclusion="0.5,1.5"), 1, "levels"),
    ("stlsq", {}, dict(DEV, bag_inclusion="0.5005"), 1, "levels_fine"),
    ("stlsq", {}, dict(DEV, bag_inclusion="half"), 1, "levels_word"),
    ("stlsq", {}, dict(DEV, bag_inclusion="0.5,1,0.5"), 1, "levels_twice"),
    ("stlsq", {}, dict(DEV, bagging=16384), 1, "too_many"),
    # two apply: the order of the list in _refusal_bagging
    ("lbfgs", {}, dict(bagging=4), 1, "method"),
    ("stlsq", dict(eq_constraint=True), dict(bagging=4), 1, "device"),
    ("stlsq", dict(R, eq_constraint=True), DEV, 1, "constraint"),
    ("stlsq", R, dict(DEV, stlsq_path=True), 1, "symreg"),
    ("stlsq", dict(lstsq_driver="gelsy"), dict(DEV, stlsq_grid=["threshold=0.1"]), 1, "grid"),
    ("stlsq", dict(lstsq_driver="gelsy", use_latent=True), DEV, 2, "gelsy"),
    ("stlsq", {}, dict(DEV, bagging=0), 2, "ranks"),
    ("stlsq", {}, dict(DEV, bagging=0, bag_chunks=0), 1, "replicas"),
]


@pytest.mark.parametrize("row", WITH_FLAG)
def test_refusals_with_the_flags(row):
    from symode_amd.main_sweep import _refusal
    method, over, kw, world, want = row
    args = _args("lbfgs", "cuda:0", **over)
    before = dict(args)
    got = _refusal(args, method, world, None, n_seeds=4, **kw)
    assert got == (None if want is None else NEW[want])
    assert args == before


def test_a_cpu_device_and_the_other_rules_with_the_flags():
    from symode_amd.main_sweep import _refusal
    ok = dict(device_stlsq=True, bagging=4)
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", **ok) == NEW["cpu"]
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", 1, ENGINE, **ok) is None                   # the injected test engine
    assert _refusal(_args("lbfgs", "cpu", use_latent=True), "stlsq", **ok) == NEW["latent"]
    assert _refusal(_args("lbfgs", "cpu"), "stlsq", 2, None, **ok) == NEW["cpu"]
    assert _refusal(_args("adam", "cuda:0"), "stlsq", **ok).startswith("main_sweep covers the L-BFGS fits")      # --method stlsq's own
    assert _refusal(_args("lbfgs", "cuda:0"), "nope", **ok) == "--method nope: lbfgs or stlsq"
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", n_seeds=64, device_stlsq=True, bagging=1023) is None
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", n_seeds=64, device_stlsq=True, bagging=1024).startswith(
        "--bagging: 64 seeds x 1024 replicas = 65536 replica problems")


def test_the_defaults():
    from symode_amd import main_sweep
    from symode_amd.sweep import BAG_MAX_CHUNKS
    assert main_sweep.BAG_CHUNKS == 128 <= BAG_MAX_CHUNKS == 1024
    assert main_sweep.BAG_INCLUSION == 1.0                      # profiles/stlsq_bag.txt: the ladder value with the most successes
    assert main_sweep._parse_inclusion("0.5,0.6,0.8,0.9,1.0") == ([0.5, 0.6, 0.8, 0.9, 1.0], None)
    assert main_sweep._parse_inclusion("1") == ([1.0], None) and main_sweep._parse_inclusion("0") == ([0.0], None)


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "4"]
SYM = ["--w_sym_reg", "0.1", "--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan"]
BAG = ["--device_stlsq", "--bagging", "4"]


@pytest.mark.parametrize("argv, text", [
    (STLSQ + ["--bagging", "4"], NEW["device"]),
    (STLSQ[:4] + ["--n_seeds", "4"] + BAG, NEW["method"]),
    (STLSQ + ["--device_stlsq", "--bag_chunks", "8"], NEW["alone_chunks"]),
    (STLSQ + ["--device_stlsq", "--bag_inclusion", "0.5"], NEW["alone_inclusion"]),
    (STLSQ + BAG + ["--eq_constraint"], NEW["constraint"]),
    (STLSQ + BAG + ["--eq_constraint", "--equiv_stlsq"], NEW["constraint"]),
    (STLSQ + BAG + ["--min_norm_stlsq"], NEW["constraint"]),
    (STLSQ + BAG + SYM, NEW["symreg"]),
    (STLSQ + BAG + ["--symreg_stlsq"] + SYM, NEW["symreg"]),
    (STLSQ + BAG + ["--symreg_path"] + SYM, NEW["symreg"]),
    (STLSQ + BAG + ["--stlsq_path"], NEW["path"]),
    (STLSQ + BAG + ["--path_tol", "0.05"], NEW["path"]),
    (STLSQ + BAG + ["--wsindy"], NEW["wsindy"]),
    (STLSQ + BAG + ["--stlsq_grid", "threshold=0.05,0.1"], NEW["grid"]),
    (STLSQ + BAG + ["--grid", "threshold=0.1"], NEW["grid"]),
    (STLSQ + BAG + ["--lbfgs_grid", "threshold=0.1"], NEW["grid"]),
    (STLSQ + BAG + ["--lstsq_driver", "gelsy"], NEW["gelsy"]),
    (STLSQ + BAG + ["--use_latent"], NEW["latent"]),
    (STLSQ + ["--device_stlsq", "--bagging", "0"], NEW["replicas"]),
    (STLSQ + BAG + ["--bag_chunks", "1025"], NEW["chunks"]),
    (STLSQ + BAG + ["--bag_inclusion", "0.5,1.5"], NEW["levels"]),
    (STLSQ + BAG + ["--bag_inclusion", "0.5005"], NEW["levels_fine"]),
    (STLSQ + BAG + ["--bag_inclusion", "half"], NEW["levels_word"]),
    (STLSQ + BAG + ["--bag_inclusion", "0.5,1,0.5"], NEW["levels_twice"]),
    (STLSQ + ["--device_stlsq", "--bagging", "16384"], NEW["too_many"]),
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


@pytest.mark.parametrize("world, device, engine, text", [(2, [], ENGINE, NEW["ranks"]), (1, ["--gpu", "-1"], None, NEW["cpu"])])
def test_ranks_and_a_cpu_device_are_refused_before_data_set_and_process_group(world, device, engine, text, monkeypatch):
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(STLSQ + BAG + device, engine=engine)
    assert str(e.value.code) == text


@pytest.mark.parametrize("extra", [[], ["--bag_chunks", "8"], ["--bag_inclusion", "0.5,1"], ["--bag_inclusion", "0.8", "--bag_chunks", "16"]])
def test_an_accepted_run_reaches_the_data_set_with_the_flags_gone_from_argv(extra, monkeypatch):
    """The parser never sees the three flags (it would reject unknown flags): main gets as far as the data set."""
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
        main_sweep.main(STLSQ + BAG + extra, engine=ENGINE)


# ---- SeedSweepSTLSQ.chunk_grams and solve_bagged(device=False) on the oracle engine ----------------------------------------------
def _sweep(n_rows=403, n_seeds=3, order=2):
    from symode_amd.sweep import SeedSweepSTLSQ
    from tests.oracle_engine import OracleEngine
    rng = np.random.RandomState(11)
    x = rng.uniform(-1.0, 1.0, size=(3 * n_rows, 2))
    dx = np.stack([-0.1 * x[:, 0] + 2.0 * x[:, 1], -2.0 * x[:, 0] - 0.1 * x[:, 1]], axis=1) + 0.02 * rng.randn(3 * n_rows, 2)
    to = lambda a: torch.from_numpy(a.astype(np.float32))                      # noqa: E731
    return SeedSweepSTLSQ(to(x), to(dx), order, n_seeds=n_seeds, subsample=1.0 / 3.0, seed0=3, engine=OracleEngine())


def test_chunk_grams_cuts_ascending_rows_and_refuses_by_name():
    sw = _sweep()
    assert sw.m_local == 403 and sw.seeds == [1_000_003 * 3, 1_000_003 * 4, 1_000_003 * 5]
    chunk = sw.chunk_grams(8).numpy()
    assert chunk.shape == (3, 8, 8, 8)
    L = 403 // 8
    first = sw.engine.aug_gram_gather(sw.x, sw.dx, sw.idx[:, :8 * L].contiguous(), sw.order, sw.flags).numpy()
    G = sw.grams()
    assert np.abs(chunk.sum(axis=1) - first).max() <= 403 * 2.0 ** -52 * np.abs(G).max()
    assert np.abs(first - G).max() > 1e-6                                       # the 3 rows beyond C L are in the refit matrix only
    one = sw.engine.aug_gram_gather(sw.x, sw.dx, sw.idx[1:2, 2 * L:3 * L].contiguous(), sw.order, sw.flags).numpy()
    assert np.array_equal(chunk[1, 2], one[0])                                  # chunk c = rows c L .. (c + 1) L - 1, ascending
    assert tuple(sw.chunk_grams(403).shape) == (3, 403, 8, 8)
    with pytest.raises(ValueError, match="n_chunks = 404 chunks need at least one row each: a seed holds m = 403 rows"):
        sw.chunk_grams(404)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="take 1 .. 1024 chunks"):
            sw.chunk_grams(bad)


def test_more_than_one_rank_is_refused_by_name(monkeypatch):
    import torch.distributed as dist
    sw = _sweep()
    sw.group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="more than one rank is not covered"):
        sw.chunk_grams(8)
    with pytest.raises(ValueError, match="more than one rank is not covered"):
        sw.solve_bagged(0.0, 0.05, 4, n_chunks=8, device=False)


def test_solve_bagged_on_the_host():
    from tests import stlsq_bag_model as M
    from symode_amd.sweep import resample_grams
    from tests.stlsq_cases import host_sweep
    sw = _sweep()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Xi, mask, rec = sw.solve_bagged(0.0, 0.05, 5, n_chunks=8, inclusion=[0.5, 1.0], device=False)
    assert Xi.dtype == torch.float32 and mask.dtype == torch.float32 and tuple(Xi.shape) == tuple(mask.shape) == (6, 2, 6)
    assert sorted(rec) == ["count", "fell", "mean", "std", "valid"]
    assert rec["count"].shape == (3, 2, 6) and rec["valid"].tolist() == [5, 5, 5] and rec["fell"].tolist() == [False] * 6
    # the same numbers from the parts: the model of the entry on the host's replica fits
    rep, _ = resample_grams(sw.chunk_grams(8).numpy(), sw.seeds, 5)
    fits = host_sweep(rep, 2, 0.0, 0.05, 10, n_points=403)
    want = M.bag(sw.grams(), fits[0], fits[1].astype(np.uint8), fits[4], [500] * 3 + [1000] * 3, 0.0)
    assert np.array_equal(mask.numpy() != 0, want["mask"] != 0) and np.array_equal(rec["count"], want["count"])
    assert rec["mean"].tobytes() == want["mean"].tobytes() and rec["std"].tobytes() == want["std"].tobytes()
    assert (np.abs(Xi.numpy().astype(np.float64) - want["xi"]) <= M.row_bound(want["xi"])).all()
    truth = np.zeros((2, 6), dtype=bool)
    truth[:, 1:3] = True
    assert all(np.array_equal(mask.numpy()[s] != 0, truth) for s in range(6))
    one = sw.solve_bagged(0.0, 0.05, 5, n_chunks=8, inclusion=1.0, device=False)
    assert torch.equal(one[0], Xi[3:]) and torch.equal(one[1], mask[3:])        # a value is the list of one
    for kw, word in ((dict(n_replicas=0), "at least one replica"), (dict(inclusion=1.5), "inclusion"), (dict(inclusion=[]), "inclusion"),
                     (dict(threshold=-1.0), "finite and >= 0"), (dict(w_sindy_reg=float("nan")), "finite and >= 0")):
        a = dict(dict(w_sindy_reg=0.0, threshold=0.05, n_replicas=5, inclusion=1.0), **kw)
        with pytest.raises(ValueError, match=word):
            sw.solve_bagged(a["w_sindy_reg"], a["threshold"], a["n_replicas"], n_chunks=8, inclusion=a["inclusion"], device=False)


def test_the_aggregate_reads_the_seeds_files_and_not_bag_npz(tmp_path, monkeypatch):
    from symode_amd import evaluation
    from symode_amd.main_sweep import _write_results
    monkeypatch.chdir(tmp_path)
    truth = evaluation.truth_table("dosc", 6, False, False)
    Xi = np.stack([truth, truth]).astype(np.float32)
    _write_results(dict(save_dir="run"), [4, 5], Xi, Xi != 0, truth)
    before = evaluation.aggregate_results("run", min_seed=4, max_seed=6)
    np.savez(tmp_path / "eval_results" / "run" / "bag.npz", valid=np.zeros(2, dtype=np.int32))
    after = evaluation.aggregate_results("run", min_seed=4, max_seed=6)
    assert repr(after) == repr(before) and after["n_runs"] == 2
