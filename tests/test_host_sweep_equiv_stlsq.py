"""main_sweep --equiv_stlsq (the device STLSQ sweep under the equivariance constraint): the flag is popped before the parser,
every refusal it adds is written out below word for word, and without it every argument combination keeps its answer -- the
table of tests/test_host_sweep_plan.py is imported, not edited."""
import pytest

from tests.test_host_sweep_plan import ENGINE, R, TABLE, TEXT, _args, _untouchable

NEW = {
    "wsindy": ("--equiv_stlsq is the constrained fit of --method stlsq: the weak-SINDy sweep (--wsindy) fits the unconstrained "
               "library (drop one of them)"),
    "method": "--equiv_stlsq is the constrained fit of the sequential-threshold least-squares sweep: it needs --method stlsq",
    "device": ("--equiv_stlsq needs --device_stlsq: the constrained fit of the sweep runs on the device (the host route of "
               "--method stlsq sweeps the unconstrained library)"),
    "constraint": ("--equiv_stlsq needs --eq_constraint: it fits under the equivariance constraint (drop --equiv_stlsq for the "
                   "unconstrained library)"),
    "gelsy": ("--equiv_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the "
              "host (python -m symode_amd.main_sindy per seed)"),
    "sym": ("--equiv_stlsq sweeps the constrained least-squares fit without a symmetry regulariser (w_sym_reg 0): use "
            "--method lbfgs with the regulariser"),
    "latent": "--equiv_stlsq does not cover latent fits (--use_latent)",
}
EQ = dict(eq_constraint=True)


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_without_the_flag_every_row_of_the_plan_keeps_its_answer(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    args = _args(optimiser, device, **over)
    assert _refusal(args, method, world, engine) == _refusal(args, method, world, engine, equiv_stlsq=False) == (
        None if want is None else TEXT[want])


# (method, overrides, device_stlsq, wsindy, stlsq_grid) -> the refusal with --equiv_stlsq, None = the sweep runs
WITH_FLAG = [
    ("stlsq", EQ, True, False, None, None),
    ("stlsq", dict(EQ, constrain_constant=True), True, False, None, None),
    ("stlsq", dict(EQ, lstsq_driver="gels"), True, False, None, None),
    ("stlsq", EQ, True, False, ["threshold=0.05,0.1", "w_sindy_reg=0,0.1"], None),
    ("lbfgs", EQ, True, False, None, "method"),
    ("lbfgs", EQ, False, False, None, "method"),
    ("stlsq", EQ, False, False, None, "device"),
    ("stlsq", {}, True, False, None, "constraint"),
    ("stlsq", dict(EQ, lstsq_driver="gelsy"), True, False, None, "gelsy"),
    ("stlsq", dict(R, eq_constraint=True), True, False, None, "sym"),
    ("stlsq", dict(EQ, use_latent=True), True, False, None, "latent"),
    ("lbfgs", EQ, False, True, None, "wsindy"),
    ("stlsq", EQ, True, True, None, "wsindy"),
    # two apply: the order of the list in the issue
    ("lbfgs", {}, False, False, None, "method"),
    ("stlsq", {}, False, False, None, "device"),
    ("stlsq", dict(lstsq_driver="gelsy"), True, False, None, "constraint"),
    ("stlsq", dict(R, eq_constraint=True, lstsq_driver="gelsy"), True, False, None, "gelsy"),
    ("stlsq", dict(R, eq_constraint=True, use_latent=True), True, False, None, "sym"),
]


@pytest.mark.parametrize("row", WITH_FLAG)
def test_refusals_with_the_flag(row):
    from symode_amd.main_sweep import _refusal
    method, over, device_stlsq, wsindy, stlsq_grid, want = row
    args = _args("lbfgs", "cuda:0", **over)
    before = dict(args)
    got = _refusal(args, method, 1, None, device_stlsq=device_stlsq, wsindy=wsindy, stlsq_grid=stlsq_grid, n_seeds=4, equiv_stlsq=True)
    assert got == (None if want is None else NEW[want])
    assert args == before


def test_the_other_rules_still_apply_with_the_flag():
    from symode_amd.main_sweep import _refusal
    ok = dict(device_stlsq=True, equiv_stlsq=True)
    assert _refusal(_args("adam", "cuda:0", **EQ), "stlsq", **ok) == TEXT["stlsq_opt"]
    assert _refusal(_args("lbfgs", "cpu", **EQ), "stlsq", **ok) == TEXT["cpu"]
    assert _refusal(_args("lbfgs", "cpu", **EQ), "stlsq", 2, ENGINE, **ok) is None                 # ranks: the Gram matrices are all-reduced
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", grid=["threshold=0.1"], **ok).startswith("--grid gives every problem")
    assert "--stlsq_grid nope=1" in _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", stlsq_grid=["nope=1"], **ok)
    # and the refusal the flag lifts is lifted by nothing else
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", device_stlsq=True) == TEXT["stlsq_eq"]


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]


@pytest.mark.parametrize("extra, text", [
    (["--equiv_stlsq", "--eq_constraint"], NEW["device"]),
    (["--equiv_stlsq", "--device_stlsq"], NEW["constraint"]),
    (["--device_stlsq", "--eq_constraint", "--equiv_stlsq", "--lstsq_driver", "gelsy"], NEW["gelsy"]),
    (["--device_stlsq", "--equiv_stlsq", "--eq_constraint", "--wsindy"], NEW["wsindy"]),
    (["--device_stlsq", "--eq_constraint"], TEXT["stlsq_eq"]),                                   # without the flag: as before
    (["--eq_constraint"], TEXT["stlsq_eq"]),
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
    """The parser never sees --equiv_stlsq (it would reject an unknown flag): main gets as far as the data set."""
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
        main_sweep.main(STLSQ + ["--device_stlsq", "--equiv_stlsq", "--eq_constraint"], engine=ENGINE)


def test_more_than_64_free_parameters_are_refused_by_name(monkeypatch):
    """r' is known once Q exists: _fit_stlsq raises the SystemExit that names it."""
    import types

    import torch

    from symode_amd import main_sweep
    from symode_amd.coef_map import CoefMap
    coef = CoefMap(2, 41, torch.zeros(82, 63), True, True)                     # r' = 63 + 2
    template = types.SimpleNamespace(coef=coef, poly_order=5, include_sine=False, include_exp=False)
    monkeypatch.setattr(main_sweep, "_template", lambda ctx: (template, None, None))
    monkeypatch.setattr(main_sweep, "SeedSweepSTLSQ", _untouchable("SeedSweepSTLSQ"))
    ctx = types.SimpleNamespace(args={"poly_order": 5, "include_sine": False, "include_exp": False}, equiv_stlsq=True)
    with pytest.raises(SystemExit) as e:
        main_sweep._fit_stlsq(ctx)
    assert str(e.value.code) == ("--equiv_stlsq: the constraint leaves r' = 65 free parameters (63 columns of Q + 2 constants), the "
                                 "device fit takes at most 64; use --method lbfgs")
