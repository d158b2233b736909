"""main_sweep --lbfgs_grid on the CPU: the flag's popping and parsing, the product order of the grid points, every refusal by
its text, and ``_refusal`` without the flag deciding what it decided before the flag existed (--grid's words included)."""
import pytest

from tests.test_host_sweep_grid import NEEDS_ADAM
from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable

AXES = "lr_sindy, w_sindy_reg, threshold, w_sym_reg"
NEEDS_LBFGS = ("--lbfgs_grid gives every problem of the device L-BFGS trainer its own hyper-parameters on shared Gram matrices: it needs "
               "--sindy_optimizer lbfgs with the default --method lbfgs (the Adam sweep has --grid, the STLSQ sweep takes one value each)")
NEEDS_GRAM = ("--lbfgs_grid needs --gram_closure: the grid points share the seeds' Gram matrices, and the Gram route's results differ "
              "from the streamed route's in the last bits -- a flag must not switch routes silently")
TOGETHER = "--lbfgs_grid and --grid are the grids of two different sweeps (L-BFGS, Adam): give one of them"
NEEDS_REGULARISER = ("--lbfgs_grid w_sym_reg needs the symmetry regulariser on the command line (--w_sym_reg > 0 with --sym_reg_type r "
                     "--load_laligan ... --fix_laligan): without it no regulariser matrices are built")


def _gram(**over):
    return _args("lbfgs", "cuda:0", gram_closure=True, **over)


def test_the_flag_is_repeatable_and_popped_before_the_parser_sees_it():
    from symode_amd.main_sweep import _pop_all
    argv = ["--task", "lv", "--lbfgs_grid", "threshold=0.01,0.05", "--gram_closure", "--lbfgs_grid", "w_sym_reg=0.1,1.0", "--seed", "4",
            "--grid", "lr_sindy=1"]
    assert _pop_all(argv, "--lbfgs_grid") == ["threshold=0.01,0.05", "w_sym_reg=0.1,1.0"]
    assert argv == ["--task", "lv", "--gram_closure", "--seed", "4", "--grid", "lr_sindy=1"]        # --grid is another flag
    assert _pop_all(argv, "--lbfgs_grid") == [] and _pop_all(["--lbfgs_grid"], "--lbfgs_grid") == [""]


def test_parsing_and_product_order():
    from symode_amd.main_sweep import GRID_NAMES, LBFGS_GRID_NAMES, _grid_points, _parse_grid
    assert LBFGS_GRID_NAMES == {"lr_sindy": "lr", "w_sindy_reg": "w_reg", "threshold": "threshold", "w_sym_reg": "w_sym"}
    assert "w_sym_reg" not in GRID_NAMES                                 # --grid keeps its three axes
    from symode_amd.device_lbfgs import HYPER_COLUMNS
    assert tuple(LBFGS_GRID_NAMES.values()) == HYPER_COLUMNS
    axes, why = _parse_grid(["w_sym_reg=0.01,1e-1,1", "threshold=.05,0.1"], LBFGS_GRID_NAMES, "--lbfgs_grid")
    assert why is None and axes == [("w_sym_reg", [0.01, 0.1, 1.0]), ("threshold", [0.05, 0.1])]
    points = _grid_points(axes)                                          # the first axis given is the slowest
    assert points == [{"w_sym_reg": w, "threshold": t} for w in (0.01, 0.1, 1.0) for t in (0.05, 0.1)]
    axes, why = _parse_grid(["lr_sindy=1,0.1", "w_sindy_reg=0", "threshold=0.15,0.01", "w_sym_reg=2"], LBFGS_GRID_NAMES, "--lbfgs_grid")
    assert why is None and [tuple(p.values()) for p in _grid_points(axes)] == [
        (1.0, 0.0, 0.15, 2.0), (1.0, 0.0, 0.01, 2.0), (0.1, 0.0, 0.15, 2.0), (0.1, 0.0, 0.01, 2.0)]


@pytest.mark.parametrize("grid, text", [
    (["treshold=0.1"], f"--lbfgs_grid treshold=0.1: unknown name 'treshold', the grid axes are {AXES} (name=v1,v2,...)"),
    (["batch_size=64"], f"--lbfgs_grid batch_size=64: unknown name 'batch_size', the grid axes are {AXES} (name=v1,v2,...)"),
    ([""], f"--lbfgs_grid : unknown name '', the grid axes are {AXES} (name=v1,v2,...)"),
    (["threshold"], "--lbfgs_grid threshold: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["threshold="], "--lbfgs_grid threshold=: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["w_sym_reg=0.1,,0.2"], "--lbfgs_grid w_sym_reg=0.1,,0.2: the values of w_sym_reg must be a non-empty comma-separated list of numbers"),
    (["lr_sindy=0.1,fast"], "--lbfgs_grid lr_sindy=0.1,fast: the values of lr_sindy must be a non-empty comma-separated list of numbers"),
    (["lr_sindy=0.1,inf"], "--lbfgs_grid lr_sindy=0.1,inf: the values of lr_sindy must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1", "lr_sindy=1", "threshold=0.2"], "--lbfgs_grid threshold is given twice: one value list per name"),
])
def test_a_bad_grid_is_refused_in_the_words_of_the_adam_grid(grid, text):
    from symode_amd.main_sweep import LBFGS_GRID_NAMES, _parse_grid, _refusal
    assert _refusal(_gram(**R), lbfgs_grid=grid) == text
    assert _parse_grid(grid, LBFGS_GRID_NAMES, "--lbfgs_grid") == (None, text)


def test_the_grid_needs_the_gram_form_of_the_lbfgs_sweep():
    from symode_amd.main_sweep import _refusal
    good = ["threshold=0.01,0.05"]
    assert _refusal(_gram(), lbfgs_grid=good) is None
    assert _refusal(_gram(), world=8, lbfgs_grid=good) is None            # point shards: the one all-reduce is before the fit
    assert _refusal(_gram(eq_constraint=True, **R), lbfgs_grid=good + ["w_sym_reg=0.05,0.2"]) is None
    assert _refusal(_args("lbfgs", "cuda:0"), lbfgs_grid=good) == NEEDS_GRAM
    assert _refusal(_args("lbfgs", "cuda:0", gram_closure=False), lbfgs_grid=good) == NEEDS_GRAM
    assert _refusal(_args("adam", "cuda:0", gram_closure=True), lbfgs_grid=good) == NEEDS_LBFGS
    assert _refusal(_gram(), "stlsq", lbfgs_grid=good) == NEEDS_LBFGS
    assert _refusal(_gram(), "stlsq", lbfgs_grid=["nonsense"]) == NEEDS_LBFGS            # ... before the grid itself is read
    assert _refusal(_args("lbfgs", "cuda:0"), lbfgs_grid=["nonsense"]) == NEEDS_GRAM
    # together with --grid, whichever sweep is asked for
    assert _refusal(_gram(), grid=["lr_sindy=1,2"], lbfgs_grid=good) == TOGETHER
    assert _refusal(_args("adam", "cuda:0"), grid=["lr_sindy=1,2"], lbfgs_grid=good) == TOGETHER
    # the regulariser's axis needs the regulariser, and weights that keep it
    assert _refusal(_gram(), lbfgs_grid=["w_sym_reg=0.1,0.2"]) == NEEDS_REGULARISER
    assert _refusal(_gram(**R), lbfgs_grid=["w_sym_reg=0.1,0"]) == \
        "--lbfgs_grid w_sym_reg=0.1,0: every value must be > 0 (a sweep without the regulariser is another run, without --w_sym_reg)"
    assert _refusal(_gram(**R), lbfgs_grid=["w_sym_reg=-1"]).startswith("--lbfgs_grid w_sym_reg=-1: every value must be > 0")
    # the size of the one launch
    many = ["threshold=" + ",".join(["0.1"] * 256), "lr_sindy=" + ",".join(["1"] * 4)]
    assert _refusal(_gram(), lbfgs_grid=many, n_seeds=63) is None and _refusal(_gram(), lbfgs_grid=many) is None      # 64512 problems
    assert _refusal(_gram(), lbfgs_grid=many, n_seeds=64) == \
        "--lbfgs_grid: 1024 grid points x 64 seeds = 65536 problems, one device trainer takes at most 65535"
    # the grid's rules come after all others: what was refused before is refused in the same words
    assert _refusal(_args("adam", "cuda:0", gram_closure=True), "stlsq", lbfgs_grid=good) == TEXT["stlsq_opt"]
    assert _refusal(_gram(use_latent=True), lbfgs_grid=good) == TEXT["latent"]
    assert _refusal(_gram(**dict(R, sym_reg_type="f")), lbfgs_grid=good) == TEXT["not_r"]
    assert _refusal(_gram(**dict(R, fix_laligan=False)), lbfgs_grid=good) == TEXT["not_frozen"]
    assert _refusal(_args("lbfgs", "cpu", gram_closure=True), lbfgs_grid=good) == TEXT["cpu"]
    assert _refusal(_gram(device_shuffle=True), lbfgs_grid=good).startswith("--device_shuffle")
    # ... and --grid says every word it said
    assert _refusal(_gram(), grid=good) == NEEDS_ADAM and _refusal(_gram(), "stlsq", grid=good) == NEEDS_ADAM
    assert _refusal(_args("adam", "cuda:0"), grid=["w_sym_reg=0.1,0.2"]) == \
        "--grid w_sym_reg=0.1,0.2: unknown name 'w_sym_reg', the grid axes are lr_sindy, w_sindy_reg, threshold (name=v1,v2,...)"


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_without_the_flag_the_plan_is_what_it_was(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    want = None if want is None else TEXT[want]
    args = _args(optimiser, device, **over)
    before = dict(args)
    assert _refusal(args, method, world, engine) == want
    assert _refusal(args, method, world, engine, lbfgs_grid=None) == want
    assert _refusal(args, method, world, engine, grid=None, lbfgs_grid=[], n_seeds=50) == want
    assert args == before


@pytest.mark.parametrize("extra, text", [
    (["--lbfgs_grid", "threshold=0.1,0.2"], NEEDS_GRAM),
    (["--gram_closure", "--sindy_optimizer", "adam", "--lbfgs_grid", "threshold=0.1,0.2"], NEEDS_LBFGS),
    (["--gram_closure", "--method", "stlsq", "--lbfgs_grid", "threshold=0.1,0.2"], NEEDS_LBFGS),
    (["--gram_closure", "--lbfgs_grid", "threshold=0.1", "--lbfgs_grid", "threshold=0.2"],
     "--lbfgs_grid threshold is given twice: one value list per name"),
    (["--gram_closure", "--lbfgs_grid", "w_sym_reg=0.1,0.2"], NEEDS_REGULARISER),
    (["--gram_closure", "--sindy_optimizer", "adam", "--grid", "lr_sindy=1,2", "--lbfgs_grid", "threshold=0.1,0.2"], TOGETHER),
    (["--gram_closure", "--n_seeds", "40000", "--lbfgs_grid", "threshold=0.1,0.2"],
     "--lbfgs_grid: 2 grid points x 40000 seeds = 80000 problems, one device trainer takes at most 65535"),
])
def test_main_refuses_a_bad_grid_before_data_set_and_process_group(extra, text, monkeypatch):
    from symode_amd import main_sweep
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    with pytest.raises(SystemExit) as e:
        seeds = [] if "--n_seeds" in extra else ["--n_seeds", "2"]
        main_sweep.main(["--task", "dosc", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--w_sym_reg", "0.0"] + seeds + extra,
                        engine=ENGINE)
    assert str(e.value.code) == text


def test_the_sweep_refuses_a_table_it_cannot_place():
    """SeedSweepLBFGS.fit(hyper=) without the Gram form, and without the device trainer (a CPU closure), by name."""
    import torch
    from types import SimpleNamespace
    from symode_amd.coef_map import CoefMap
    from symode_amd.sweep import SeedSweepLBFGS
    clos = SimpleNamespace(S=2, d=2, p=6, coef=CoefMap(2, 6), engine=None, distributed=False)
    P0 = torch.zeros(4, 12)
    with pytest.raises(ValueError, match="needs the Gram form"):
        SeedSweepLBFGS(clos, 1.0, 0.1, 0).fit(P0, 1, hyper={"lr": [1.0] * 4})
    with pytest.raises(ValueError, match="needs the device trainer"):
        SeedSweepLBFGS(clos, 1.0, 0.1, 0, gram_closure=True).fit(P0, 1, hyper={"lr": [1.0] * 4})
