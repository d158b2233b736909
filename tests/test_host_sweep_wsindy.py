"""The host side of ``main_sweep --wsindy``: the windows are main_wsindy's draws, the plan's refusals word for word, the
older refusals untouched when the new keywords keep their defaults, grid parsing and problem order."""
import numpy as np
import pytest

from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable

CMD = "python -m symode_amd.main_wsindy --seed $i ... for each seed (the per_seed loop of run_scripts/sweep.sh)"
W = {
    "grid_alone": "--wsindy_grid needs --wsindy: it is the grid of the weak-SINDy sweep (the other sweeps have --grid, --lbfgs_grid, "
                  "--stlsq_grid)",
    "method": "--wsindy is a fit of its own (weak form, sequential-threshold least squares on the device): drop --method stlsq",
    "latent": f"--wsindy does not cover latent fits (--use_latent); run {CMD}",
    "sym": f"--wsindy sweeps the plain weak-form least-squares fit (w_sym_reg 0), main_wsindy has no symmetry regulariser; run {CMD}",
    "eq": f"--wsindy sweeps the unconstrained library (no --eq_constraint); run {CMD}",
    "gelsy": ("--wsindy fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the host; "
              f"run {CMD}"),
    "shuffle": "--device_shuffle draws the epoch order of the minibatch Adam fit: the weak-SINDy sweep has no epoch order (drop it)",
    "device_stlsq": "--device_stlsq is the device fit of --method stlsq: the weak-SINDy sweep always fits on the device (drop it)",
    "grids": ("--grid, --lbfgs_grid and --stlsq_grid are the grids of three other sweeps (Adam, L-BFGS, STLSQ): the weak-SINDy "
              "sweep takes --wsindy_grid"),
    "ranks": ("main_sweep runs the weak-SINDy fits in one process (no collective over seeds): give every GPU its own block of "
              "seeds, python -m symode_amd.main_sweep --wsindy --seed <first> --n_seeds <count> ... per process"),
    "cpu": TEXT["cpu"],
    "seeds": "--wsindy: 65536 seeds = 65536 problems, one launch takes at most 65535",
}


def test_windows_are_the_draws_of_main_wsindy():
    from symode_amd.sweep import weak_windows
    for n_ics, n_steps in ((6, 200), (1, 10), (50, 1000)):
        n_t = int(0.8 * n_steps)
        got = weak_windows(range(50), n_ics, n_steps, n_t)
        assert got.shape == (50, 2) and np.issubdtype(got.dtype, np.integer)
        for seed in range(50):
            np.random.seed(seed)                                       # main_wsindy.py:21, 26-27
            start = np.random.randint(0, n_steps - int(0.8 * n_steps))
            traj = np.random.randint(0, n_ics)
            assert got[seed].tolist() == [traj, start], seed
    # a seed's window is a function of the seed alone
    assert np.array_equal(weak_windows([7, 3], 6, 200, 160), weak_windows(range(50), 6, 200, 160)[[7, 3]])
    with pytest.raises(ValueError):
        weak_windows([0], 6, 200, 200)


def _refuse(over=None, method="lbfgs", world=1, device="cuda:0", engine=None, optimiser="adam", **kw):
    from symode_amd.main_sweep import _refusal
    args = _args(optimiser, device, **(over or {}))                   # (adam: the parser's default, which the weak configs leave)
    before = dict(args)
    kw.setdefault("wsindy", True)
    got = _refusal(args, method, world, engine, **kw)
    assert args == before
    return got


def test_the_weak_sweep_is_accepted_whatever_the_optimiser_flag():
    for optimiser in ("adam", "lbfgs", "sgd"):
        assert _refuse(optimiser=optimiser) is None
        assert _refuse(optimiser=optimiser, n_seeds=50, wsindy_grid=["threshold=0.1,0.2"]) is None
    assert _refuse(device="cpu", engine=ENGINE) is None
    assert _refuse(dict(sindy_reg_type="none")) is None                 # an Adam rule: not asked of the weak sweep
    assert _refuse(dict(lstsq_driver="gels"), n_seeds=65535) is None


def test_every_refusal_word_for_word():
    assert _refuse(wsindy=False, wsindy_grid=["threshold=0.1"]) == W["grid_alone"]
    assert _refuse(method="stlsq") == W["method"]
    assert _refuse(method="newton") == TEXT["method"]
    assert _refuse(dict(use_latent=True)) == W["latent"]
    assert _refuse(R) == W["sym"]
    assert _refuse(dict(eq_constraint=True)) == W["eq"]
    assert _refuse(dict(lstsq_driver="gelsy")) == W["gelsy"]
    assert _refuse(dict(device_shuffle=True)) == W["shuffle"]
    assert _refuse(device_stlsq=True) == W["device_stlsq"]
    for other in ("grid", "lbfgs_grid", "stlsq_grid"):
        assert _refuse(**{other: ["threshold=0.1"]}) == W["grids"], other
        assert _refuse(wsindy_grid=["threshold=0.1"], **{other: ["threshold=0.1"]}) == W["grids"], other
    assert _refuse(world=2) == W["ranks"]
    assert _refuse(device="cpu") == W["cpu"]
    assert _refuse(n_seeds=65536) == W["seeds"]
    # with a config, the per-seed command names it
    assert _refuse(dict(use_latent=True, config="dosc/noise20_wsindy.cfg")) == W["latent"].replace(
        "--seed $i ...", "--seed $i --config dosc/noise20_wsindy.cfg")
    # the order: the flag pair, the method, the fit's rules, the other flags, ranks, device
    assert _refuse(dict(R, use_latent=True, eq_constraint=True), world=2, device="cpu") == W["latent"]
    assert _refuse(dict(R, eq_constraint=True), world=2) == W["sym"]
    assert _refuse(dict(device_shuffle=True), world=2, device="cpu", device_stlsq=True) == W["shuffle"]
    assert _refuse(world=2, device="cpu") == W["ranks"]


def test_grid_refusals_word_for_word():
    g = lambda *specs, **kw: _refuse(wsindy_grid=list(specs), n_seeds=kw.pop("n_seeds", 4), **kw)       # noqa: E731
    assert g("lr_sindy=0.1") == ("--wsindy_grid lr_sindy=0.1: unknown name 'lr_sindy', the grid axes are threshold, w_sindy_reg "
                                 "(name=v1,v2,...)")
    assert g("threshold=0.1", "threshold=0.2") == "--wsindy_grid threshold is given twice: one value list per name"
    for spec in ("threshold", "threshold=", "threshold=0.1,,0.2", "threshold=a", "w_sindy_reg=inf", "w_sindy_reg=0.1,nan"):
        name = spec.partition("=")[0]
        assert g(spec) == (f"--wsindy_grid {spec}: the values of {name} must be a non-empty comma-separated list of numbers"), spec
    assert g("threshold=0.1,-0.2") == "--wsindy_grid threshold=0.1,-0.2: every value must be >= 0"
    assert g("w_sindy_reg=-1") == "--wsindy_grid w_sindy_reg=-1: every value must be >= 0"
    assert g("threshold=" + ",".join(["0.1"] * 256), "w_sindy_reg=" + ",".join(["0"] * 64), n_seeds=4) == (
        "--wsindy_grid: 16384 grid points x 4 seeds = 65536 problems, one launch takes at most 65535")
    assert g("threshold=0.1,0.2", "w_sindy_reg=0,1e-3,1e-2") is None


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_the_older_refusals_are_unchanged_with_the_new_keywords_at_their_defaults(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    args = _args(optimiser, device, **over)
    want = None if want is None else TEXT[want]
    assert _refusal(args, method, world, engine) == want
    assert _refusal(args, method, world, engine, wsindy=False, wsindy_grid=None) == want


def test_grid_parsing_and_product_order():
    from symode_amd.main_sweep import WSINDY_GRID_NAMES, _grid_points, _grid_problem, _parse_grid
    assert WSINDY_GRID_NAMES == {"threshold": "threshold", "w_sindy_reg": "w_reg"}
    axes, why = _parse_grid(["w_sindy_reg=0,1e-3", "threshold=0.1,0.2,0.3"], WSINDY_GRID_NAMES, "--wsindy_grid")
    assert why is None and axes == [("w_sindy_reg", [0.0, 1e-3]), ("threshold", [0.1, 0.2, 0.3])]
    points = _grid_points(axes)                                           # the first axis given is the slowest
    assert points == [dict(w_sindy_reg=w, threshold=t) for w in (0.0, 1e-3) for t in (0.1, 0.2, 0.3)]
    assert [_grid_problem(s, 4) for s in (0, 3, 4, 23)] == [(0, 0), (0, 3), (1, 0), (5, 3)]


@pytest.mark.parametrize("extra, text", [
    (["--wsindy", "--eq_constraint"], W["eq"]),
    (["--wsindy", "--method", "stlsq"], W["method"]),
    (["--wsindy_grid", "threshold=0.1"], W["grid_alone"]),
    (["--wsindy", "--wsindy_grid", "threshold=0.1,-1"], "--wsindy_grid threshold=0.1,-1: every value must be >= 0"),
])
def test_an_invalid_weak_sweep_is_refused_before_data_set_and_process_group(extra, text, monkeypatch):
    import torch.distributed as dist
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    monkeypatch.setattr(dist, "init_process_group", _untouchable("init_process_group"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(["--task", "dosc", "--n_seeds", "2"] + extra, engine=ENGINE)
    assert str(e.value.code) == text
