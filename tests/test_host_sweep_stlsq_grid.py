"""main_sweep --device_stlsq / --stlsq_grid on the CPU: the flags' popping and parsing, product order and problem numbering of
the grid, every refusal by its text, ``_refusal`` without the flags deciding what it decided before they existed (the words
of --grid and --lbfgs_grid included), and the refusals of ``SeedSweepSTLSQ.solve(device=, hyper=)``."""
import pytest

from tests.test_host_sweep_grid import NEEDS_ADAM
from tests.test_host_sweep_lbfgs_grid import NEEDS_LBFGS
from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable

AXES = "threshold, w_sindy_reg"
NEEDS_DEVICE = ("--stlsq_grid needs --device_stlsq: the grid points share the seeds' Gram matrices on the device, and the device fit "
                "is the full-rank driver's, whose results can differ from the host route's in the last bit -- a flag must not switch "
                "routes silently")
NEEDS_STLSQ = ("{}: the device fit of the sequential-threshold least-squares sweep and its grid need --method stlsq (the Adam sweep "
               "has --grid, the L-BFGS sweep --lbfgs_grid)")
TOGETHER = "--stlsq_grid, --grid and --lbfgs_grid are the grids of three different sweeps (STLSQ, Adam, L-BFGS): give one of them"
NO_GELSY = ("--device_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the host route "
            "(drop --device_stlsq)")
GOOD = ["threshold=0.01,0.05"]


def _plain(**over):
    return _args("lbfgs", "cuda:0", **over)


def _refuse(args, method="stlsq", device_stlsq=True, **kw):
    from symode_amd.main_sweep import _refusal
    return _refusal(args, method, device_stlsq=device_stlsq, **kw)


def test_the_flags_are_popped_before_the_parser_sees_them():
    from symode_amd.main_sweep import _pop_all, _pop_flag
    argv = ["--task", "lv", "--stlsq_grid", "threshold=0.01,0.05", "--device_stlsq", "--stlsq_grid", "w_sindy_reg=0,0.1", "--seed", "4",
            "--grid", "lr_sindy=1"]
    assert _pop_all(argv, "--stlsq_grid") == ["threshold=0.01,0.05", "w_sindy_reg=0,0.1"]
    assert _pop_flag(argv, "--device_stlsq") and not _pop_flag(argv, "--device_stlsq")
    assert argv == ["--task", "lv", "--seed", "4", "--grid", "lr_sindy=1"]


def test_parsing_product_order_and_problem_numbering():
    from symode_amd.main_sweep import GRID_NAMES, LBFGS_GRID_NAMES, STLSQ_GRID_NAMES, _grid_points, _grid_problem, _parse_grid
    assert STLSQ_GRID_NAMES == {"threshold": "threshold", "w_sindy_reg": "w_reg"}
    assert len(GRID_NAMES) == 3 and len(LBFGS_GRID_NAMES) == 4                 # the two other grids keep their axes
    axes, why = _parse_grid(["w_sindy_reg=0,1e-1", "threshold=.05,0.1,0.2"], STLSQ_GRID_NAMES, "--stlsq_grid")
    assert why is None and axes == [("w_sindy_reg", [0.0, 0.1]), ("threshold", [0.05, 0.1, 0.2])]
    points = _grid_points(axes)                                                # the first axis given is the slowest
    assert points == [{"w_sindy_reg": w, "threshold": t} for w in (0.0, 0.1) for t in (0.05, 0.1, 0.2)]
    n_seeds = 4                                                                # problem g * n_seeds + k is point g on seed k
    assert [_grid_problem(s, n_seeds) for s in range(len(points) * n_seeds)] == [(g, k) for g in range(6) for k in range(4)]
    # ... which is the table the fit hands to SeedSweepSTLSQ.solve(hyper=): point g's values on rows g * n_seeds .. + n_seeds
    hyper = {STLSQ_GRID_NAMES[name]: [point[name] for point in points for _ in range(n_seeds)] for name in points[0]}
    assert sorted(hyper) == ["threshold", "w_reg"]
    for s in range(len(points) * n_seeds):
        g, k = _grid_problem(s, n_seeds)
        assert (hyper["w_reg"][s], hyper["threshold"][s]) == (points[g]["w_sindy_reg"], points[g]["threshold"]) and k == s % n_seeds


@pytest.mark.parametrize("grid, text", [
    (["treshold=0.1"], f"--stlsq_grid treshold=0.1: unknown name 'treshold', the grid axes are {AXES} (name=v1,v2,...)"),
    (["lr_sindy=1,2"], f"--stlsq_grid lr_sindy=1,2: unknown name 'lr_sindy', the grid axes are {AXES} (name=v1,v2,...)"),
    ([""], f"--stlsq_grid : unknown name '', the grid axes are {AXES} (name=v1,v2,...)"),
    (["threshold"], "--stlsq_grid threshold: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["threshold="], "--stlsq_grid threshold=: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["w_sindy_reg=0.1,,0.2"],
     "--stlsq_grid w_sindy_reg=0.1,,0.2: the values of w_sindy_reg must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1,nan"], "--stlsq_grid threshold=0.1,nan: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1,inf"], "--stlsq_grid threshold=0.1,inf: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1", "w_sindy_reg=1", "threshold=0.2"], "--stlsq_grid threshold is given twice: one value list per name"),
    (["threshold=0.1,-0.05"], "--stlsq_grid threshold=0.1,-0.05: every value must be >= 0"),
    (["threshold=0.1", "w_sindy_reg=-1"], "--stlsq_grid w_sindy_reg=-1: every value must be >= 0"),
])
def test_a_bad_grid_is_refused_by_name(grid, text):
    assert _refuse(_plain(), stlsq_grid=grid) == text


def test_the_rules_of_the_two_flags():
    from symode_amd.main_sweep import _refusal
    assert _refuse(_plain()) is None and _refuse(_plain(), stlsq_grid=GOOD) is None
    assert _refuse(_plain(), world=8, stlsq_grid=GOOD + ["w_sindy_reg=0,0.1"]) is None      # the one all-reduce is before the fit
    assert _refuse(_args("lbfgs", "cpu"), engine=ENGINE) is None                           # _refusal decides; the engine runs it
    assert _refuse(_plain(lstsq_driver="gels"), stlsq_grid=GOOD) is None and _refuse(_plain(lstsq_driver=None)) is None
    # a flag must not switch routes silently
    assert _refuse(_plain(), device_stlsq=False, stlsq_grid=GOOD) == NEEDS_DEVICE
    assert _refuse(_plain(), device_stlsq=False, stlsq_grid=["nonsense"]) == NEEDS_DEVICE    # ... before the grid itself is read
    # without --method stlsq
    assert _refuse(_plain(), "lbfgs") == NEEDS_STLSQ.format("--device_stlsq")
    assert _refuse(_plain(), "lbfgs", device_stlsq=False, stlsq_grid=GOOD) == NEEDS_STLSQ.format("--stlsq_grid")
    assert _refuse(_args("adam", "cuda:0"), "lbfgs", stlsq_grid=GOOD) == NEEDS_STLSQ.format("--device_stlsq and --stlsq_grid")
    assert _refuse(_plain(gram_closure=True), "lbfgs", stlsq_grid=GOOD, lbfgs_grid=GOOD) == NEEDS_STLSQ.format("--device_stlsq and --stlsq_grid")
    # together with the grid of another sweep
    assert _refuse(_plain(), stlsq_grid=GOOD, grid=["lr_sindy=1,2"]) == TOGETHER
    assert _refuse(_plain(), stlsq_grid=GOOD, lbfgs_grid=GOOD) == TOGETHER
    assert _refuse(_plain(), device_stlsq=False, stlsq_grid=GOOD, grid=GOOD, lbfgs_grid=GOOD) == TOGETHER
    # the rank rule is the host route's
    assert _refuse(_plain(lstsq_driver="gelsy")) == NO_GELSY and _refuse(_plain(lstsq_driver="gelsy"), stlsq_grid=GOOD) == NO_GELSY
    assert _refusal(_plain(lstsq_driver="gelsy"), "stlsq") is None                          # ... where it stays available
    # the size of the one launch
    many = ["threshold=" + ",".join(["0.1"] * 256), "w_sindy_reg=" + ",".join(["1"] * 4)]
    assert _refuse(_plain(), stlsq_grid=many, n_seeds=63) is None and _refuse(_plain(), stlsq_grid=many) is None       # 64512 problems
    assert _refuse(_plain(), stlsq_grid=many, n_seeds=64) == \
        "--stlsq_grid: 1024 grid points x 64 seeds = 65536 problems, one launch takes at most 65535"
    # the flags' rules come after all others: what was refused before is refused in the same words
    assert _refuse(_args("adam", "cuda:0"), stlsq_grid=GOOD) == TEXT["stlsq_opt"]
    assert _refuse(_plain(use_latent=True), stlsq_grid=GOOD) == TEXT["latent"]
    assert _refuse(_args("lbfgs", "cpu"), stlsq_grid=GOOD) == TEXT["cpu"]
    assert _refuse(_plain(**R), stlsq_grid=GOOD) == TEXT["stlsq_sym"]
    assert _refuse(_plain(eq_constraint=True)) == TEXT["stlsq_eq"]
    assert _refuse(_plain(device_shuffle=True)).startswith("--device_shuffle")
    # ... and the two other grids say every word they said
    assert _refusal(_plain(), "stlsq", grid=GOOD) == NEEDS_ADAM and _refuse(_plain(), grid=GOOD) == NEEDS_ADAM
    assert _refusal(_plain(gram_closure=True), "stlsq", lbfgs_grid=GOOD) == NEEDS_LBFGS
    assert _refuse(_plain(gram_closure=True), lbfgs_grid=GOOD) == NEEDS_LBFGS
    assert "the L-BFGS and STLSQ sweeps take one value each" in NEEDS_ADAM and "the STLSQ sweep takes one value each" in NEEDS_LBFGS


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_without_the_flags_the_plan_is_what_it_was(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    want = None if want is None else TEXT[want]
    args = _args(optimiser, device, **over)
    before = dict(args)
    assert _refusal(args, method, world, engine) == want
    assert _refusal(args, method, world, engine, device_stlsq=False, stlsq_grid=None) == want
    assert _refusal(args, method, world, engine, grid=None, lbfgs_grid=[], n_seeds=50, device_stlsq=False, stlsq_grid=[]) == want
    assert args == before


@pytest.mark.parametrize("extra, text", [
    (["--method", "stlsq", "--stlsq_grid", "threshold=0.1,0.2"], NEEDS_DEVICE),
    (["--device_stlsq"], NEEDS_STLSQ.format("--device_stlsq")),
    (["--device_stlsq", "--stlsq_grid", "threshold=0.1,0.2"], NEEDS_STLSQ.format("--device_stlsq and --stlsq_grid")),
    (["--method", "stlsq", "--device_stlsq", "--lstsq_driver", "gelsy"], NO_GELSY),
    (["--method", "stlsq", "--device_stlsq", "--stlsq_grid", "threshold=0.1", "--stlsq_grid", "threshold=0.2"],
     "--stlsq_grid threshold is given twice: one value list per name"),
    (["--method", "stlsq", "--device_stlsq", "--stlsq_grid", "threshold=0.1,0.2", "--grid", "lr_sindy=1,2"], TOGETHER),
    (["--method", "stlsq", "--device_stlsq", "--stlsq_grid", "threshold=-0.1"], "--stlsq_grid threshold=-0.1: every value must be >= 0"),
    (["--method", "stlsq", "--device_stlsq", "--n_seeds", "40000", "--stlsq_grid", "threshold=0.1,0.2"],
     "--stlsq_grid: 2 grid points x 40000 seeds = 80000 problems, one launch takes at most 65535"),
])
def test_main_refuses_before_data_set_and_process_group(extra, text, monkeypatch):
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


def test_the_sweep_refuses_what_its_device_route_does_not_cover():
    """SeedSweepSTLSQ.solve: ``hyper`` without ``device=True`` and ``device=True`` with gelsy, by name and before any Gram is
    built (the engine below has no Gram entry at all); a table the route cannot place."""
    import inspect
    from types import SimpleNamespace

    import numpy as np
    import torch

    from symode_amd.sweep import SeedSweepSTLSQ
    sig = inspect.signature(SeedSweepSTLSQ.solve).parameters
    assert sig["device"].default is False and sig["hyper"].default is None
    assert inspect.signature(SeedSweepSTLSQ.grams).parameters["device"].default is False
    eng = SimpleNamespace(lib_size=lambda d, order, flags: 10)
    sw = SeedSweepSTLSQ(torch.zeros(8, 2), torch.zeros(8, 2), 3, n_seeds=3, subsample=0.5, seed0=0, engine=eng,
                        idx=torch.zeros(3, 4, dtype=torch.int32))
    table = {"w_reg": [0.0] * 6, "threshold": [0.1] * 6}
    with pytest.raises(ValueError, match="hyper .* needs device=True"):
        sw.solve(0.0, 0.1, hyper=table)
    with pytest.raises(ValueError, match="hyper .* needs device=True"):
        sw.solve(0.0, 0.1, lstsq_driver="gels", hyper=table)
    with pytest.raises(ValueError, match=r"device=True fits with the full-rank driver \(gels\) only, not lstsq_driver='gelsy'"):
        sw.solve(0.0, 0.1, lstsq_driver="gelsy", device=True)
    with pytest.raises(ValueError, match="not lstsq_driver='gelsy'"):                   # CPU data: gelsy is the default driver
        sw.solve(0.0, 0.1, device=True)
    # tables the device route cannot place: matrices handed in on the host, so these too are decided before any launch
    sw._gram, sw.n_points = np.zeros((3, 12, 12)), 4
    for bad, words in [({"lr": [1.0] * 6}, "the per-problem columns of the STLSQ sweep are w_reg and threshold"),
                       ({}, "the per-problem columns"),
                       ({"w_reg": [0.0] * 6, "threshold": [0.1] * 3}, "one value per problem"),
                       ({"threshold": [0.1] * 4}, "a multiple of the 3 seeds"),
                       ({"threshold": [0.1] * 2}, "a multiple of the 3 seeds"),
                       ({"threshold": [0.1, -0.1, 0.1]}, "finite and >= 0"),
                       ({"w_reg": [0.0, float("nan"), 0.0]}, "finite and >= 0")]:
        with pytest.raises(ValueError, match=words):
            sw.solve(0.0, 0.1, lstsq_driver="gels", device=True, hyper=bad)
    assert sw.grams() is sw._gram                                                  # the host copy is what it was
