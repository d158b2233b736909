"""main_sweep --grid on the CPU: the flag's parsing and the product order of the grid points, every refusal by its text,
the problem-to-(grid point, seed) map, and ``_refusal`` without ``grid`` deciding what it decided before the flag existed."""
import pytest

from tests.test_host_sweep_plan import ENGINE, TABLE, TEXT, _args, _untouchable

NEEDS_ADAM = ("--grid gives every problem of the minibatch Adam launch its own hyper-parameters: it needs --sindy_optimizer adam "
              "(with the default --method lbfgs); the L-BFGS and STLSQ sweeps take one value each")


def test_the_flag_is_repeatable_and_popped_before_the_parser_sees_it():
    from symode_amd.main_sweep import _pop_all
    argv = ["--task", "dosc", "--grid", "threshold=0.01,0.05", "--n_seeds", "3", "--grid", "lr_sindy=0.1,1.0", "--seed", "4"]
    assert _pop_all(argv, "--grid") == ["threshold=0.01,0.05", "lr_sindy=0.1,1.0"]
    assert argv == ["--task", "dosc", "--n_seeds", "3", "--seed", "4"]
    assert _pop_all(argv, "--grid") == [] and _pop_all(["--grid"], "--grid") == [""]      # a flag without its value: refused below


def test_parsing_and_product_order():
    from symode_amd.main_sweep import GRID_NAMES, _grid_points, _parse_grid
    assert GRID_NAMES == {"lr_sindy": "lr", "w_sindy_reg": "w_reg", "threshold": "threshold"}
    axes, why = _parse_grid(["threshold=0.01,5e-2,.075", "lr_sindy=0.1,1"])
    assert why is None and axes == [("threshold", [0.01, 0.05, 0.075]), ("lr_sindy", [0.1, 1.0])]
    points = _grid_points(axes)                                        # the first axis given is the slowest
    assert points == [{"threshold": t, "lr_sindy": lr} for t in (0.01, 0.05, 0.075) for lr in (0.1, 1.0)]
    assert list(points[0]) == ["threshold", "lr_sindy"]
    axes, why = _parse_grid(["lr_sindy=1,0.1", "w_sindy_reg=0", "threshold=0.15,0.01"])
    assert why is None and [tuple(p.values()) for p in _grid_points(axes)] == [(1.0, 0.0, 0.15), (1.0, 0.0, 0.01), (0.1, 0.0, 0.15),
                                                                              (0.1, 0.0, 0.01)]
    assert _grid_points(_parse_grid(["w_sindy_reg=0.5"])[0]) == [{"w_sindy_reg": 0.5}]


def test_the_problem_to_point_and_seed_map():
    from symode_amd.main_sweep import _grid_problem
    n_seeds, G = 3, 4
    assert [_grid_problem(q, n_seeds) for q in range(G * n_seeds)] == [(g, k) for g in range(G) for k in range(n_seeds)]
    assert all(g * n_seeds + k == q for q in range(G * n_seeds) for g, k in [_grid_problem(q, n_seeds)])


@pytest.mark.parametrize("grid, text", [
    (["treshold=0.1"], "--grid treshold=0.1: unknown name 'treshold', the grid axes are lr_sindy, w_sindy_reg, threshold "
                       "(name=v1,v2,...)"),
    (["w_sym_reg=0.1,0.2"], "--grid w_sym_reg=0.1,0.2: unknown name 'w_sym_reg', the grid axes are lr_sindy, w_sindy_reg, threshold "
                            "(name=v1,v2,...)"),
    (["threshold"], "--grid threshold: the values of threshold must be a non-empty comma-separated list of numbers"),
    ([""], "--grid : unknown name '', the grid axes are lr_sindy, w_sindy_reg, threshold (name=v1,v2,...)"),
    (["threshold="], "--grid threshold=: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1,,0.2"], "--grid threshold=0.1,,0.2: the values of threshold must be a non-empty comma-separated list of numbers"),
    (["lr_sindy=0.1,fast"], "--grid lr_sindy=0.1,fast: the values of lr_sindy must be a non-empty comma-separated list of numbers"),
    (["lr_sindy=0.1,nan"], "--grid lr_sindy=0.1,nan: the values of lr_sindy must be a non-empty comma-separated list of numbers"),
    (["threshold=0.1", "lr_sindy=1", "threshold=0.2"], "--grid threshold is given twice: one value list per name"),
])
def test_a_bad_grid_is_refused_by_name(grid, text):
    from symode_amd.main_sweep import _parse_grid, _refusal
    assert _refusal(_args("adam", "cuda:0"), grid=grid) == text
    assert _parse_grid(grid) == (None, text)


def test_the_grid_needs_the_adam_sweep():
    from symode_amd.main_sweep import _refusal
    good = ["threshold=0.01,0.05"]
    assert _refusal(_args("adam", "cuda:0"), grid=good) is None
    assert _refusal(_args("adam", "cuda:0", eq_constraint=True, device_shuffle=True), grid=good) is None
    assert _refusal(_args("lbfgs", "cuda:0"), grid=good) == NEEDS_ADAM
    assert _refusal(_args("lbfgs", "cuda:0"), "stlsq", grid=good) == NEEDS_ADAM
    assert _refusal(_args("lbfgs", "cuda:0"), grid=["nonsense"]) == NEEDS_ADAM         # ... before the grid itself is read
    # the grid's rules come after all others: what was refused before is refused in the same words
    assert _refusal(_args("adam", "cuda:0"), "stlsq", grid=good) == TEXT["stlsq_opt"]
    assert _refusal(_args("adam", "cuda:0", w_sym_reg=0.1), grid=good) == TEXT["adam_sym"]
    assert _refusal(_args("adam", "cuda:0", use_latent=True), grid=good) == TEXT["latent"]
    assert _refusal(_args("adam", "cuda:0"), world=2, grid=good) == TEXT["adam_ranks"]
    assert _refusal(_args("adam", "cpu"), grid=good) == TEXT["cpu"]
    assert _refusal(_args("lbfgs", "cuda:0", device_shuffle=True), grid=good).startswith("--device_shuffle")


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_without_a_grid_the_plan_is_what_it_was(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    want = None if want is None else TEXT[want]
    assert _refusal(_args(optimiser, device, **over), method, world, engine) == want
    assert _refusal(_args(optimiser, device, **over), method, world, engine, grid=None) == want
    assert _refusal(_args(optimiser, device, **over), method, world, engine, grid=[]) == want


@pytest.mark.parametrize("extra, text", [
    (["--sindy_optimizer", "lbfgs", "--grid", "threshold=0.1,0.2"], NEEDS_ADAM),
    (["--sindy_optimizer", "adam", "--grid", "threshold=0.1", "--grid", "threshold=0.2"],
     "--grid threshold is given twice: one value list per name"),
    (["--sindy_optimizer", "adam", "--grid", "batch_size=64,256"],
     "--grid batch_size=64,256: unknown name 'batch_size', the grid axes are lr_sindy, w_sindy_reg, threshold (name=v1,v2,...)"),
])
def test_main_refuses_a_bad_grid_before_data_set_and_process_group(extra, text, monkeypatch):
    from symode_amd import main_sweep
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(["--task", "dosc", "--ae_arch", "none", "--n_seeds", "2"] + extra, engine=ENGINE)
    assert str(e.value.code) == text
