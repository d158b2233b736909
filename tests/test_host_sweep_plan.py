"""main_sweep's plan: ``_refusal`` is the one place that decides whether a sweep runs -- a pure function of the parsed
arguments, the method, the number of ranks and the injected test engine -- and ``main`` asks it before a process group, a
data file or a device is touched.  The texts below are the driver's messages written out in full, and where two refusals
apply the one listed is the one ``main`` raised when four of them still sat behind the data set and the process group."""
import pytest

CMD = "python -m symode_amd.main --seed $i ... for each seed (the per_seed loop of run_scripts/sweep.sh)"
TEXT = {
    "method": "--method newton: lbfgs or stlsq",
    "stlsq_opt": f"main_sweep covers the L-BFGS fits (--sindy_optimizer lbfgs); run {CMD}",
    "optimiser": f"main_sweep covers the L-BFGS and Adam fits (--sindy_optimizer lbfgs | adam); run {CMD}",
    "latent": f"main_sweep does not cover latent fits (--use_latent); run {CMD}",
    "adam_sym": f"main_sweep covers Adam fits without a symmetry regulariser (w_sym_reg 0) only; run {CMD}",
    "not_r": ("main_sweep covers the reversed symmetry regulariser only (--sym_reg_type r), not 'f': its closure runs the "
              f"autoencoder on Xi-dependent inputs; run {CMD}"),
    "not_loaded": ("main_sweep needs --load_laligan with the symmetry regulariser: without it every per-seed process fits "
                   f"against its own random autoencoder; run {CMD}"),
    "not_frozen": f"main_sweep needs --fix_laligan with the symmetry regulariser (g(x), J_g(x) computed once); run {CMD}",
    "adam_ranks": ("main_sweep runs the Adam fits in one process (no collective over seeds): give every GPU its own block of "
                   "seeds, python -m symode_amd.main_sweep --seed <first> --n_seeds <count> ... per process"),
    "cpu": "symode_amd runs the SINDy path on the GPU only (no CPU fallback): a HIP device is required",
    "stlsq_sym": "--method stlsq sweeps the plain least-squares fit (use --method lbfgs with the symmetry regulariser)",
    "stlsq_eq": "--method stlsq sweeps the unconstrained library (use --method lbfgs for EquivSINDy-c)",
}
ENGINE = object()                       # stands for the injected test engine: it is never called
R = dict(w_sym_reg=0.1, sym_reg_type="r", load_laligan="x", fix_laligan=True)      # the reversed regulariser as it is swept

# (method, optimiser, overrides of the plain config, world, device, engine) -> the refusal, None = the sweep runs
TABLE = [
    # accepted today
    ("lbfgs", "lbfgs", {}, 1, "cuda:0", None, None),
    ("lbfgs", "lbfgs", {}, 8, "cuda:0", None, None),
    ("lbfgs", "lbfgs", dict(eq_constraint=True), 2, "cuda:0", None, None),
    ("lbfgs", "lbfgs", R, 1, "cuda:0", None, None),
    ("lbfgs", "lbfgs", dict(R, eq_constraint=True), 2, "cuda:0", None, None),
    ("lbfgs", "lbfgs", {}, 3, "cpu", ENGINE, None),                       # the CPU rehearsal with a test engine
    ("stlsq", "lbfgs", {}, 1, "cuda:0", None, None),
    ("stlsq", "lbfgs", {}, 8, "cuda:0", None, None),
    ("stlsq", "lbfgs", {}, 2, "cpu", ENGINE, None),
    ("lbfgs", "adam", {}, 1, "cuda:0", None, None),
    ("lbfgs", "adam", dict(eq_constraint=True), 1, "cuda:0", None, None),
    ("lbfgs", "adam", {}, 1, "cpu", ENGINE, None),
    ("lbfgs", "lbfgs", dict(sym_reg_type="f"), 1, "cuda:0", None, None),   # a regulariser's type without a weight is no regulariser
    # one refusal applies
    ("newton", "lbfgs", {}, 1, "cuda:0", None, "method"),
    ("stlsq", "adam", {}, 1, "cuda:0", None, "stlsq_opt"),
    ("lbfgs", "sgd", {}, 1, "cuda:0", None, "optimiser"),
    ("lbfgs", "lbfgs", dict(use_latent=True), 1, "cuda:0", None, "latent"),
    ("lbfgs", "adam", dict(use_latent=True), 1, "cuda:0", None, "latent"),
    ("lbfgs", "adam", R, 1, "cuda:0", None, "adam_sym"),
    ("lbfgs", "lbfgs", dict(R, sym_reg_type="f"), 1, "cuda:0", None, "not_r"),
    ("lbfgs", "lbfgs", dict(R, load_laligan=None), 1, "cuda:0", None, "not_loaded"),
    ("lbfgs", "lbfgs", dict(R, fix_laligan=False), 1, "cuda:0", None, "not_frozen"),
    ("lbfgs", "adam", {}, 2, "cuda:0", None, "adam_ranks"),
    ("lbfgs", "lbfgs", {}, 1, "cpu", None, "cpu"),
    ("stlsq", "lbfgs", {}, 1, "cpu", None, "cpu"),
    ("stlsq", "lbfgs", R, 1, "cuda:0", None, "stlsq_sym"),
    ("stlsq", "lbfgs", dict(eq_constraint=True), 1, "cuda:0", None, "stlsq_eq"),
    ("stlsq", "lbfgs", dict(eq_constraint=True), 2, "cpu", ENGINE, "stlsq_eq"),
    # two or more apply: the winner is the one main() reached first
    ("newton", "sgd", dict(use_latent=True), 1, "cpu", None, "method"),
    ("stlsq", "adam", dict(use_latent=True), 2, "cpu", None, "stlsq_opt"),
    ("stlsq", "sgd", {}, 1, "cuda:0", None, "stlsq_opt"),
    ("lbfgs", "sgd", dict(use_latent=True), 1, "cuda:0", None, "optimiser"),
    ("lbfgs", "adam", dict(R, use_latent=True), 2, "cpu", None, "latent"),
    ("lbfgs", "adam", R, 2, "cpu", None, "adam_sym"),
    ("lbfgs", "lbfgs", dict(R, sym_reg_type="f", load_laligan=None, fix_laligan=False), 1, "cpu", None, "not_r"),
    ("lbfgs", "lbfgs", dict(R, load_laligan=None, fix_laligan=False), 1, "cpu", None, "not_loaded"),
    ("lbfgs", "lbfgs", dict(R, fix_laligan=False), 1, "cpu", None, "not_frozen"),
    ("stlsq", "lbfgs", dict(R, sym_reg_type="f"), 1, "cuda:0", None, "not_r"),           # before the STLSQ rules
    ("stlsq", "lbfgs", dict(R, load_laligan=None, eq_constraint=True), 1, "cuda:0", None, "not_loaded"),
    ("lbfgs", "adam", {}, 2, "cpu", None, "adam_ranks"),                                # several ranks, then the device
    ("lbfgs", "adam", {}, 2, "cpu", ENGINE, "adam_ranks"),
    ("stlsq", "lbfgs", R, 1, "cpu", None, "cpu"),                                       # the device, then the STLSQ rules
    ("stlsq", "lbfgs", dict(eq_constraint=True), 1, "cpu", None, "cpu"),
    ("stlsq", "lbfgs", dict(R, eq_constraint=True), 1, "cuda:0", None, "stlsq_sym"),    # the weight, then the constraint
    ("stlsq", "lbfgs", dict(R, eq_constraint=True), 4, "cpu", ENGINE, "stlsq_sym"),
]


def _args(optimiser, device, **over):
    a = {"config": None, "sindy_optimizer": optimiser, "use_latent": False, "w_sym_reg": 0.0, "sym_reg_type": "i",
         "load_laligan": None, "fix_laligan": False, "sindy_reg_type": "l1", "eq_constraint": False, "device": device}
    a.update(over)
    return a


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-{'-'.join(f'{k}={v}' for k, v in r[2].items()) or 'plain'}-"
                                                      f"w{r[3]}-{r[4]}{'-engine' if r[5] is not None else ''}")
def test_refusal_table(row):
    from symode_amd.main_sweep import _refusal
    method, optimiser, over, world, device, engine, want = row
    args = _args(optimiser, device, **over)
    before = dict(args)
    got = _refusal(args, method, world, engine)
    assert got == (None if want is None else TEXT[want])
    assert args == before                                                  # it decides; it changes nothing


def test_refusal_accepts_the_partial_dicts_of_the_older_tests():
    """Keys the function did not read before the late refusals moved into it are optional."""
    from symode_amd.main_sweep import _refusal
    args = {"sindy_optimizer": "lbfgs", "use_latent": False, "w_sym_reg": 0.0, "sym_reg_type": "i", "load_laligan": None,
            "fix_laligan": False}
    assert _refusal(args) is None and _refusal(args, "stlsq") is None and _refusal(args, "stlsq", 8) is None
    assert _refusal(dict(args, config="dosc/noise20_sindy.cfg", use_latent=True)) == TEXT["latent"].replace(
        "--seed $i ...", "--seed $i --config dosc/noise20_sindy.cfg")


def _untouchable(name):
    def touched(*a, **k):
        raise AssertionError(f"{name} called before the sweep was refused")
    return touched


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]


@pytest.mark.parametrize("extra, text", [
    (["--eq_constraint"], TEXT["stlsq_eq"]),
    (["--w_sym_reg", "0.1", "--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan"], TEXT["stlsq_sym"]),
])
@pytest.mark.parametrize("world", [1, 2])
def test_an_invalid_stlsq_sweep_is_refused_before_data_set_and_process_group(extra, text, world, monkeypatch):
    import torch.distributed as dist
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    monkeypatch.setattr(dist, "init_process_group", _untouchable("init_process_group"))
    monkeypatch.setattr(dist, "barrier", _untouchable("barrier"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(STLSQ + extra, engine=ENGINE)
    assert str(e.value.code) == text
