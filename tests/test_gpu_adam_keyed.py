"""The keyed epoch entries (symode_adam_epochs_keyed / _reversed_keyed / _latent_keyed: the row of every batch slot computed
inside the launch from an order seed) against their table siblings fed the table the numpy twin device_adam.epoch_order
builds, on identical state: params, m, v, step, mask, xi and the log BIT FOR BIT.  The table path is the one pinned against
fp64 and torch.optim.Adam elsewhere; no tolerance appears here.  Operands and injected state come from the generators of
tests/adam_cases.py and tests/adam_latent_cases.py; d = 2, order 2, three problems, three epochs with a thresholding event
inside the launch (st_freq = 2), non-default betas and eps."""
import numpy as np
import pytest
import torch

from tests import adam_cases as C
from tests import adam_latent_cases as LC
from tests.trainer_cases import _bytes_equal

from symode_amd.device_adam import epoch_order

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIB = (2, 2, 0)
S, EPOCHS = 3, 3
SEEDS = [5, 2 ** 40 + 3, -2]
KEYS = ("params", "m", "v", "step", "mask", "xi", "log")
KINDS = ("plain", "reversed", "latent")
SHAPES = [(5, 1), (5, 77), (5, 300), (5, 2000), (300, 77), (300, 300), (300, 2000), (1025, 77), (1025, 300), (1025, 2000)]


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd.get_engine()


_ORDERS, _DATA = {}, {}


def _table(n, batch, seeds, n_epochs, epoch0=0, shuffle=True):
    """The twin's (n_epochs, len(seeds), steps, batch) int32 table; every order is computed once for the module."""
    steps = (n + batch - 1) // batch
    t = np.full((n_epochs, len(seeds), steps * batch), -1, dtype=np.int32)
    for e in range(n_epochs):
        for k, seed in enumerate(seeds):
            key = (seed, epoch0 + e, n)
            if shuffle and key not in _ORDERS:
                _ORDERS[key] = epoch_order(*key)
            t[e, k, :n] = _ORDERS[key] if shuffle else np.arange(n)
    return torch.from_numpy(t.reshape(n_epochs, len(seeds), steps, batch))


def _data(kind, n):
    """n rows of the generators' 600-row fields (repeated beyond 600), on the device."""
    if (kind, n) not in _DATA:
        rows = torch.arange(n) % C.N_SRC
        f = LC.field(2) if kind == "latent" else C.field(2)
        _DATA[kind, n] = {k: (v if k == "L" else v[:, rows] if k in ("gx", "jgx") else v[rows]).contiguous().to(DEV)
                          for k, v in f.items()}
    return _DATA[kind, n]


def _cfg(kind, form="xi", **kw):
    kw = dict(dict(st_freq=2, threshold=0.1), **kw)
    if kind == "latent":
        return LC._cfg(LIB, "weighted", form, 1, 2, **kw)                # n_gen = 1, D_obs = d + 2
    return C._cfg(LIB, "weighted", "rev2" if kind == "reversed" else "plain", form, **kw)


def _state(cfg, seed=0, starts=(0, 9, 999)):
    p, dp = C.lib_dims(LIB)
    n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + LIB[0]
    return C._state(S, n_par, LIB[0], p, list(starts), ["ones", "half", "ones"], True, torch.Generator().manual_seed(4000 + seed))


def _launch(eng, kind, cfg, state, n, batch, seeds, n_epochs=EPOCHS, epoch0=0, keyed=True, shuffle=True, table=None):
    """One launch of the keyed entry, or of its sibling on the twin's table, on fresh copies of ``state``."""
    f = _data(kind, n)
    p, m, v, step, mask = (state[k].to(DEV).clone() for k in C.STATE_KEYS)
    kw = dict(lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], w_x=cfg["w_x"], w_reg=cfg["w_reg"], l1=cfg["l1"],
              threshold=cfg["threshold"], st_freq=cfg["st_freq"], epoch0=epoch0, near_band=cfg["near_band"],
              q_eff=None if cfg["q"] is None else cfg["q"].to(DEV), allow_constant=cfg["allow_const"])
    if keyed:
        how, suffix = (seeds, n_epochs, batch), "_keyed"
        kw["shuffle"] = shuffle
    else:
        table = _table(n, batch, seeds, n_epochs, epoch0, shuffle) if table is None else table
        how, suffix = (table.to(DEV).contiguous(),), ""
    tail = (*how, p, m, v, step, mask, cfg["order"], cfg["flags"])
    if kind == "plain":
        xi, log = getattr(eng, "adam_epochs" + suffix)(f["x"], f["dx"], *tail, **kw)
    elif kind == "reversed":
        n_g = cfg["n_g"]
        xi, log = getattr(eng, "adam_epochs_reversed" + suffix)(f["x"], f["dx"], f["gx"][:n_g].contiguous(), f["jgx"][:n_g].contiguous(),
                                                                 *tail, w_sym=cfg["w_sym"], **kw)
    else:
        xi, log = getattr(eng, "adam_epochs_latent" + suffix)(f["z"], f["dz"], f["B"], f["y"], f["e"], cfg["D_obs"],
                                                               f["L"][:cfg["n_gen"]].contiguous(), *tail, w_z=cfg["w_z"],
                                                               w_sym=cfg["w_sym"], **kw)
    torch.cuda.synchronize()
    return dict(params=p.cpu(), m=m.cpu(), v=v.cpu(), step=step.cpu(), mask=mask.cpu(), xi=xi.cpu(), log=log.cpu())


def _differ(a, b, keys=KEYS):
    return [k for k in keys if a[k].shape != b[k].shape or not _bytes_equal(a[k], b[k])]


@pytest.mark.parametrize("own", [False, True], ids=["one_seed", "seed_per_problem"])
@pytest.mark.parametrize("n, batch", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", KINDS)
def test_the_keyed_entry_equals_its_sibling_on_the_twins_table(eng, kind, n, batch, own):
    cfg, seeds = _cfg(kind), SEEDS if own else SEEDS[:1]
    state = _state(cfg)
    got = _launch(eng, kind, cfg, state, n, batch, seeds)
    want = _launch(eng, kind, cfg, state, n, batch, seeds, keyed=False)
    assert _differ(got, want) == []
    steps = (n + batch - 1) // batch
    assert got["step"].tolist() == [s + EPOCHS * steps for s in (0, 9, 999)]              # every step was taken
    assert (got["log"][:, :, 5] == torch.tensor([0.0, 1.0, 0.0])[:, None]).all()           # the event of epoch 1, inside the launch
    assert not _bytes_equal(got["params"], state["params"])
    if own and n > 5:
        assert not torch.equal(got["log"][:, 0, 0], got["log"][:, 2, 0])


@pytest.mark.parametrize("kind", KINDS)
def test_under_the_constraint(eng, kind):
    cfg = _cfg(kind, form="q5c")                                                           # q_eff with 5 columns, constants added
    assert cfg["q"] is not None and cfg["allow_const"]
    state = _state(cfg, seed=1)
    got = _launch(eng, kind, cfg, state, 300, 77, SEEDS)
    assert _differ(got, _launch(eng, kind, cfg, state, 300, 77, SEEDS, keyed=False)) == []
    assert got["step"].tolist() == [12, 21, 1011]


@pytest.mark.parametrize("kind", KINDS)
def test_a_problem_that_enters_frozen_comes_back_untouched(eng, kind):
    cfg = _cfg(kind)
    state = _state(cfg, seed=2)
    state["step"][1] = -10
    got = _launch(eng, kind, cfg, state, 300, 77, SEEDS)
    assert _differ(got, _launch(eng, kind, cfg, state, 300, 77, SEEDS, keyed=False)) == []
    assert _differ({k: got[k][1] for k in C.STATE_KEYS}, {k: state[k][1] for k in C.STATE_KEYS}, C.STATE_KEYS) == []
    assert int(got["step"][1]) == -10 and (got["log"][:, 1, 4] == 1).all() and (got["log"][:, 1, 2] == 0).all()
    assert got["step"].tolist()[::2] == [12, 1011]


@pytest.mark.parametrize("n, batch", [(300, 77), (1025, 300)])
@pytest.mark.parametrize("kind", KINDS)
def test_four_epochs_in_one_launch_equal_one_plus_three(eng, kind, n, batch):
    cfg = _cfg(kind)
    state = _state(cfg, seed=3)
    whole = _launch(eng, kind, cfg, state, n, batch, SEEDS, n_epochs=4)
    a = _launch(eng, kind, cfg, state, n, batch, SEEDS, n_epochs=1)
    b = _launch(eng, kind, cfg, {k: a[k] for k in C.STATE_KEYS}, n, batch, SEEDS, n_epochs=3, epoch0=1)
    assert _differ(whole, b, keys=C.STATE_KEYS + ("xi",)) == []
    assert _bytes_equal(whole["log"], torch.cat([a["log"], b["log"]]))
    assert whole["log"][:, 0, 6].tolist() == [0.0, 1.0, 2.0, 3.0] and whole["log"][:, 0, 5].tolist() == [0.0, 1.0, 0.0, 1.0]
    # the epoch number is part of the key: the continuation without epoch0 walks other rows
    wrong = _launch(eng, kind, dict(cfg, st_freq=0), state, n, batch, SEEDS, n_epochs=1, epoch0=1)
    right = _launch(eng, kind, dict(cfg, st_freq=0), state, n, batch, SEEDS, n_epochs=1, epoch0=0)
    assert _differ(wrong, right, keys=("params",)) == ["params"]


@pytest.mark.parametrize("kind", KINDS)
def test_without_shuffle_the_rows_come_in_order(eng, kind):
    cfg = _cfg(kind)
    state = _state(cfg, seed=4)
    got = _launch(eng, kind, cfg, state, 300, 77, SEEDS[:1], shuffle=False)
    steps = torch.arange(4 * 77, dtype=torch.int32)
    steps[300:] = -1
    table = steps.view(1, 1, 4, 77).expand(EPOCHS, 1, 4, 77).contiguous()
    assert _differ(got, _launch(eng, kind, cfg, state, 300, 77, SEEDS[:1], keyed=False, table=table)) == []
    assert _differ(got, _launch(eng, kind, cfg, state, 300, 77, SEEDS[:1]), keys=("params",)) == ["params"]


# ------------------------------------------------------------------------------------------------ DeviceAdam.fit
def _trainer(eng, kind, n, batch):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    f, (p, _) = _data(kind, n), C.lib_dims(LIB)
    kw = {}
    if kind == "reversed":
        kw["reversed_sym"] = (f["gx"][:2].contiguous(), f["jgx"][:2].contiguous(), 0.25)
    if kind == "latent":
        kw["latent"] = (f["B"], f["y"], f["e"], 4, f["L"][:1].contiguous(), 0.37, 2e-3)
    x, dx = (f["z"], f["dz"]) if kind == "latent" else (f["x"], f["dx"])
    return DeviceAdam(x, dx, LIB[1], False, False, CoefMap(2, p), 3e-2, 0.6, 0.05, 0.1, 2, batch, betas=(0.8, 0.95), eps=1e-3,
                      engine=eng, **kw)


@pytest.mark.parametrize("per_launch", [1, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_fit_with_order_seeds_equals_fit_on_the_device_tables(eng, kind, per_launch):
    n, batch, n_epochs = 300, 77, 5
    tr = _trainer(eng, kind, n, batch)
    p0 = _state(_cfg(kind), seed=5)["params"]
    tables = eng.adam_order_table(n, batch, SEEDS, n_epochs, device=torch.device(DEV))
    assert torch.equal(tables.cpu(), _table(n, batch, SEEDS, n_epochs))
    orders = [tables[e].reshape(S, -1)[:, :n].long() for e in range(n_epochs)]
    recs = {"orders": [], "seeds": []}

    def note(name):
        def on_epoch(epoch, rec):
            state = None if rec["state"] is None else {k: v.detach().cpu().clone() for k, v in rec["state"].items()}
            recs[name].append((epoch, {k: np.array(v) for k, v in rec.items() if k != "state"}, state))
        return on_epoch

    want = tr.fit(p0, n_epochs, iter(orders), on_epoch=note("orders"), epochs_per_launch=per_launch)
    got = tr.fit(p0, n_epochs, order_seeds=SEEDS, on_epoch=note("seeds"), epochs_per_launch=per_launch)
    for k in ("Xi", "mask", "params", "m", "v", "step", "nan"):
        assert _bytes_equal(got[k].cpu(), want[k].cpu()), k
    assert got["log"].shape == (n_epochs, S, 10 if kind == "latent" else 8) and got["log"].tobytes() == want["log"].tobytes()
    assert [r[0] for r in recs["seeds"]] == list(range(n_epochs)) == [r[0] for r in recs["orders"]]
    for (_, a, sa), (_, b, sb) in zip(recs["seeds"], recs["orders"]):
        assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
        assert (sa is None) == (sb is None) and (sa is None or all(_bytes_equal(sa[k], sb[k]) for k in sa))
    assert sum(r[2] is not None for r in recs["seeds"]) == (n_epochs if per_launch == 1 else 1)
    # continued with epoch0 and the state: the fit in one go
    first = tr.fit(p0, 2, order_seeds=SEEDS, epochs_per_launch=per_launch)
    rest = tr.fit(first["params"], 3, order_seeds=SEEDS, mask0=first["mask"], epoch0=2, state=(first["m"], first["v"], first["step"]),
                  epochs_per_launch=per_launch)
    assert all(_bytes_equal(rest[k].cpu(), got[k].cpu()) for k in ("Xi", "mask", "params", "m", "v", "step"))


def test_fit_takes_the_orders_or_the_seeds(eng):
    tr = _trainer(eng, "plain", 300, 77)
    p0 = _state(_cfg("plain"))["params"]
    with pytest.raises(ValueError, match="one of them"):
        tr.fit(p0, 1)
    with pytest.raises(ValueError, match="one of them"):
        tr.fit(p0, 1, iter([]), order_seeds=SEEDS)
    with pytest.raises(ValueError, match="1 or 3 seeds"):
        tr.fit(p0, 1, order_seeds=SEEDS[:2])


# ------------------------------------------------------------------------------------------------ main_sweep --device_shuffle
def test_main_sweep_device_shuffle_is_the_direct_fit_on_the_seeds(eng, tmp_path, monkeypatch, capsys):
    from symode_amd import dataset as D, main_sweep
    from symode_amd.device_adam import DeviceAdam
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples, noise-free
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)
    seen = {}
    fit_adam = main_sweep._fit_adam

    def spy(ctx):
        with monkeypatch.context() as mp:
            mp.setattr(torch, "argsort", lambda *a, **k: pytest.fail("--device_shuffle sorts no keys"))
            mp.setattr(torch, "rand", lambda *a, **k: pytest.fail("--device_shuffle draws no keys"))
            seen["ctx"], seen["result"] = ctx, fit_adam(ctx)
        return seen["result"]

    monkeypatch.setattr(main_sweep, "_fit_adam", spy)
    argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "adam", "--device_shuffle",
            "--batch_size", "256", "--lr_sindy", "0.01", "--w_sindy_x", "1.0", "--w_sindy_z", "0.0", "--w_sindy_reg", "0.001",
            "--w_sym_reg", "0.0", "--poly_order", "2", "--st_freq", "2", "--threshold", "5e-2", "--num_epochs", "2",
            "--seed", "4", "--n_seeds", "3", "--save_dir", "keyed"]
    res = main_sweep.main(argv)
    assert res["n_runs"] == 3 and "2 epochs x 5 Adam steps of 256 rows" in capsys.readouterr().out
    ctx, result = seen["ctx"], seen["result"]
    assert ctx.seeds == [4, 5, 6]
    template, P0, _ = main_sweep._template(ctx)
    tr = DeviceAdam(ctx.x_all, ctx.dx_all, 2, False, False, template.coef, 0.01, 1.0, 0.001, 5e-2, 2, 256)
    out = tr.fit(P0, 2, order_seeds=ctx.seeds)
    assert torch.equal(out["Xi"], result.Xi) and torch.equal(out["mask"], result.mask)
    one = tr.fit(P0[1:2], 2, order_seeds=[5])                                    # seed 5's fit is a function of 5 alone
    assert torch.equal(one["Xi"][0], result.Xi[1])
    for k, s in enumerate(ctx.seeds):
        saved = np.load(tmp_path / "eval_results" / "keyed" / f"seed{s}.npz")
        assert saved["coefficients"].shape == (2, 6) and np.isfinite(saved["coefficients"]).all()
        assert np.array_equal(saved["coefficients"], np.where(out["mask"][k].cpu().numpy() != 0, out["Xi"][k].cpu().numpy(), 0.0))
    assert not torch.equal(result.Xi[0], result.Xi[1])


def test_the_drivers_refuse_the_flag_where_no_adam_epoch_runs():
    from symode_amd import main as main_mod, main_sweep
    base = ["--task", "dosc", "--ae_arch", "none", "--device_shuffle", "--n_seeds", "2"]
    with pytest.raises(SystemExit, match="--device_shuffle draws the epoch order of the minibatch Adam fit inside its launch"):
        main_sweep.main(base + ["--sindy_optimizer", "lbfgs"])
    with pytest.raises(SystemExit, match="--device_shuffle draws the epoch order of the minibatch Adam fit inside its launch"):
        main_sweep.main(base + ["--sindy_optimizer", "lbfgs", "--method", "stlsq"])
    with pytest.raises(SystemExit, match="--device_shuffle draws the epoch order of the device Adam fit inside its launch: it "
                                         "needs --device_adam"):
        main_mod.main(["--task", "dosc", "--ae_arch", "none", "--sindy_optimizer", "adam", "--device_shuffle"])
