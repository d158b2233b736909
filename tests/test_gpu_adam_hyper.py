"""A hyper-parameter grid in one epoch launch (symode_adam_run with ``hyper``: every problem its own lr, w_reg, threshold and
w_sym) against the scalar entries, which are the ones pinned against fp64 and torch.optim.Adam elsewhere: everything here is
BIT FOR BIT through ``_bytes_equal``, no tolerance appears.  Library (2, 2, 0), 300 rows of the generators' fields (tests/
adam_cases.py, tests/adam_latent_cases.py), four problems, three epochs with a thresholding event inside the launch
(st_freq = 2), non-default betas and eps; batch 77 (one chunk, a short last batch) and 300 (two chunks, 256 + 44); plain,
reversed with two group elements, latent with one generator and D_obs = d + 2; unconstrained and under a q_eff; on the index
table and on the order seeds."""
import json

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
N, S, EPOCHS = 300, 4, 3
SEEDS = [5, 2 ** 40 + 3, -2, 11]
KEYS = ("params", "m", "v", "step", "mask", "xi", "log")
KINDS = ("plain", "reversed", "latent")
BATCHES = (77, 300)
FORMS = ("xi", "q5c")                      # unconstrained; q_eff with 5 columns, constants added
# all sixteen values differ, from problem to problem and from column to column; problem 1 has w_sym = 0
VARIED = [[0.03, 0.05, 0.25, 0.2], [0.01, 0.007, 0.015, 0.0], [0.04, 0.002, 0.3, 0.5], [0.02, 0.033, 0.06, 0.125]]


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd.get_engine()


_ORDERS, _DATA, _SOLO = {}, {}, {}


def _table(batch, seeds, n_epochs, epoch0=0):
    """The numpy twin's (n_epochs, len(seeds), steps, batch) int32 table; every order is computed once for the module."""
    steps = (N + batch - 1) // batch
    t = np.full((n_epochs, len(seeds), steps * batch), -1, dtype=np.int32)
    for e in range(n_epochs):
        for k, seed in enumerate(seeds):
            key = (seed, epoch0 + e, N)
            if key not in _ORDERS:
                _ORDERS[key] = epoch_order(*key)
            t[e, k, :N] = _ORDERS[key]
    return torch.from_numpy(t.reshape(n_epochs, len(seeds), steps, batch))


def _data(kind):
    if kind not in _DATA:
        f = LC.field(2) if kind == "latent" else C.field(2)
        _DATA[kind] = {k: (v if k == "L" else v[:, :N] if k in ("gx", "jgx") else v[:N]).contiguous().to(DEV) for k, v in f.items()}
    return _DATA[kind]


def _cfg(kind, form="xi", **kw):
    kw = dict(dict(st_freq=2, threshold=0.1), **kw)
    if kind == "latent":
        return LC._cfg(LIB, "weighted", form, 1, 2, **kw)                # n_gen = 1, D_obs = d + 2
    return C._cfg(LIB, "weighted", "rev2" if kind == "reversed" else "plain", form, **kw)


def _state(cfg, seed=0):
    """Four problems with their own parameters, moments and step counts, every mask ones; problems 0 and 1 start from the
    SAME state, so whatever sets them apart after a launch is their hyper-parameters (and, keyed, their order seeds)."""
    p, dp = C.lib_dims(LIB)
    n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + LIB[0]
    st = C._state(S, n_par, LIB[0], p, [9, 9, 0, 999], ["ones"] * S, True, torch.Generator().manual_seed(6000 + seed))
    for k in ("params", "m", "v"):
        st[k][1] = st[k][0]
    return st


def _scalars(cfg):
    return [cfg["lr"], cfg["w_reg"], cfg["threshold"], cfg["w_sym"]]


def _launch(eng, kind, cfg, state, batch, seeds, *, keyed, row=None, hyper=None, n_epochs=EPOCHS, epoch0=0):
    """One launch on fresh copies of ``state``: the scalar entry with ``row`` = [lr, w_reg, threshold, w_sym] (None: those of
    ``cfg``), or symode_adam_run with the (S, 4) table ``hyper`` -- then the four scalars are handed over as NaN, which a
    launch that read one of them would not survive."""
    f = _data(kind)
    p, m, v, step, mask = (state[k].to(DEV).clone() for k in C.STATE_KEYS)
    lr, w_reg, threshold, w_sym = [float("nan")] * 4 if hyper is not None else _scalars(cfg) if row is None else row
    kw = dict(lr=lr, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], w_x=cfg["w_x"], w_reg=w_reg, l1=cfg["l1"],
              threshold=threshold, st_freq=cfg["st_freq"], epoch0=epoch0, near_band=cfg["near_band"],
              q_eff=None if cfg["q"] is None else cfg["q"].to(DEV), allow_constant=cfg["allow_const"])
    if hyper is not None:
        kw["hyper"] = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    if keyed:
        how, suffix = (seeds, n_epochs, batch), "_keyed"
    else:
        how, suffix = (_table(batch, seeds, n_epochs, epoch0).to(DEV).contiguous(),), ""
    tail = (*how, p, m, v, step, mask, cfg["order"], cfg["flags"])
    if kind == "plain":
        xi, log = getattr(eng, "adam_epochs" + suffix)(f["x"], f["dx"], *tail, **kw)
    elif kind == "reversed":
        n_g = cfg["n_g"]
        xi, log = getattr(eng, "adam_epochs_reversed" + suffix)(f["x"], f["dx"], f["gx"][:n_g].contiguous(), f["jgx"][:n_g].contiguous(),
                                                                 *tail, w_sym=w_sym, **kw)
    else:
        xi, log = getattr(eng, "adam_epochs_latent" + suffix)(f["z"], f["dz"], f["B"], f["y"], f["e"], cfg["D_obs"],
                                                               f["L"][:cfg["n_gen"]].contiguous(), *tail, w_z=cfg["w_z"],
                                                               w_sym=w_sym, **kw)
    torch.cuda.synchronize()
    return dict(params=p.cpu(), m=m.cpu(), v=v.cpu(), step=step.cpu(), mask=mask.cpu(), xi=xi.cpu(), log=log.cpu())


def _differ(a, b, keys=KEYS):
    return [k for k in keys if a[k].shape != b[k].shape or not _bytes_equal(a[k], b[k])]


def _problem(out, s):
    """Problem ``s`` of a launch's results, shaped as a launch of that problem alone."""
    return {k: (out[k][:, s:s + 1] if k == "log" else out[k][s:s + 1]) for k in KEYS}


def _solo(eng, kind, form, batch, keyed, s):
    """The scalar entry launched on problem ``s`` alone (S = 1, its own table row or order seed) with row s of VARIED: the
    reference of the varied tests, computed once for the module and left unchanged."""
    key = (kind, form, batch, keyed, s)
    if key not in _SOLO:
        cfg = _cfg(kind, form)
        one = {k: v[s:s + 1].clone() for k, v in _state(cfg).items()}
        _SOLO[key] = _launch(eng, kind, cfg, one, batch, SEEDS[s:s + 1], keyed=keyed, row=VARIED[s])
    return _SOLO[key]


GRID = [(kind, form, batch, keyed) for kind in KINDS for form in FORMS for batch in BATCHES for keyed in (False, True)]
GRID_IDS = [f"{kind}-{form}-b{batch}-{'keyed' if keyed else 'table'}" for kind, form, batch, keyed in GRID]


@pytest.mark.parametrize("kind, form, batch, keyed", GRID, ids=GRID_IDS)
def test_a_uniform_table_is_the_scalar_entry(eng, kind, form, batch, keyed):
    cfg = _cfg(kind, form)
    assert cfg["l1"] and (cfg["q"] is None) == (form == "xi")
    state = _state(cfg)
    want = _launch(eng, kind, cfg, state, batch, SEEDS, keyed=keyed)
    got = _launch(eng, kind, cfg, state, batch, SEEDS, keyed=keyed, hyper=[_scalars(cfg)] * S)
    assert _differ(got, want) == []
    steps = (N + batch - 1) // batch
    assert got["step"].tolist() == [t + EPOCHS * steps for t in (9, 9, 0, 999)]             # every step was taken
    assert (got["log"][:, :, 5] == torch.tensor([0.0, 1.0, 0.0])[:, None]).all()           # the event of epoch 1, inside the launch
    assert not _bytes_equal(got["params"], state["params"])


@pytest.mark.parametrize("kind, form, batch, keyed", GRID, ids=GRID_IDS)
def test_a_varied_table_gives_every_problem_its_own_scalar_launch(eng, kind, form, batch, keyed):
    assert len({v for row in VARIED for v in row}) == 16 and VARIED[1][3] == 0.0
    cfg = _cfg(kind, form)
    solo = [_solo(eng, kind, form, batch, keyed, s) for s in range(S)]
    # the precondition, on the scalar runs: the thresholds tell at least two problems apart -- 0 and 1, which start alike, at
    # 0.25 and 0.015 -- and row 2's threshold of 0.3 leaves its problem fewer coefficients than row 1's 0.015 leaves
    masks = [o["mask"].reshape(-1) for o in solo]
    assert not torch.equal(masks[0], masks[1]) and masks[2].sum() < masks[1].sum()
    assert all(float(o["log"][1, 0, 5]) == 1.0 for o in solo)
    got = _launch(eng, kind, cfg, _state(cfg), batch, SEEDS, keyed=keyed, hyper=VARIED)
    for s in range(S):
        assert _differ(_problem(got, s), solo[s]) == [], s
    if kind != "plain":                                                  # column 3 is read: w_sym = 0 is not row 0's 0.2
        other = _launch(eng, kind, cfg, _state(cfg), batch, SEEDS, keyed=keyed, hyper=[r[:3] + [VARIED[0][3]] for r in VARIED])
        assert _differ(_problem(other, 1), solo[1], keys=("params",)) == ["params"]
        assert _differ(_problem(other, 0), solo[0]) == []


@pytest.mark.parametrize("kind", KINDS)
def test_the_plain_kind_does_not_read_column_three(eng, kind):
    cfg = _cfg(kind)
    got = _launch(eng, kind, cfg, _state(cfg), 77, SEEDS, keyed=True, hyper=VARIED)
    nan = _launch(eng, kind, cfg, _state(cfg), 77, SEEDS, keyed=True, hyper=[r[:3] + [float("nan")] for r in VARIED])
    if kind == "plain":
        assert _differ(got, nan) == []
    else:                                                                # a NaN weight reaches the loss: every problem ends frozen
        assert (nan["step"] < 0).all() and (got["step"] > 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_the_varied_keyed_launch_cut_into_one_plus_two_epochs(eng, kind):
    cfg = _cfg(kind)
    state = _state(cfg, seed=1)
    whole = _launch(eng, kind, cfg, state, 77, SEEDS, keyed=True, hyper=VARIED)
    a = _launch(eng, kind, cfg, state, 77, SEEDS, keyed=True, hyper=VARIED, n_epochs=1)
    b = _launch(eng, kind, cfg, {k: a[k] for k in C.STATE_KEYS}, 77, SEEDS, keyed=True, hyper=VARIED, n_epochs=2, epoch0=1)
    assert _differ(whole, b, keys=C.STATE_KEYS + ("xi",)) == []
    assert _bytes_equal(whole["log"], torch.cat([a["log"], b["log"]]))
    assert whole["log"][:, 0, 6].tolist() == [0.0, 1.0, 2.0] and whole["log"][:, 0, 5].tolist() == [0.0, 1.0, 0.0]


def test_the_binding_refuses_a_table_it_cannot_hand_over(eng):
    from symode_amd import SymodeError
    cfg = _cfg("plain")
    good = torch.tensor(VARIED, dtype=torch.float32, device=DEV)
    for bad in (good.cpu(), good.double(), good[:3], good[:, :3], good.t().contiguous().t(), VARIED, good.reshape(-1)):
        f = _data("plain")
        p, m, v, step, mask = (_state(cfg)[k].to(DEV).clone() for k in C.STATE_KEYS)
        with pytest.raises(SymodeError, match=r"hyper must be a contiguous \(4, 4\) fp32 tensor"):
            eng.adam_epochs_keyed(f["x"], f["dx"], SEEDS, 1, 77, p, m, v, step, mask, 2, 0, lr=0.1, hyper=bad)
        assert int(step.sum()) == 9 + 9 + 0 + 999                                          # refused before the launch


# ------------------------------------------------------------------------------------------------ DeviceAdam.fit(hyper=...)
def _trainer(eng, kind, row=None):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    f, (p, _) = _data(kind), C.lib_dims(LIB)
    lr, w_reg, threshold, w_sym = [3e-2, 0.05, 0.1, 0.25 if kind == "reversed" else 2e-3] if row is None else row
    kw = {}
    if kind == "reversed":
        kw["reversed_sym"] = (f["gx"][:2].contiguous(), f["jgx"][:2].contiguous(), w_sym)
    if kind == "latent":
        kw["latent"] = (f["B"], f["y"], f["e"], 4, f["L"][:1].contiguous(), 0.37, w_sym)
    x, dx = (f["z"], f["dz"]) if kind == "latent" else (f["x"], f["dx"])
    return DeviceAdam(x, dx, LIB[1], False, False, CoefMap(2, p), lr, 0.6, w_reg, threshold, 2, 77, betas=(0.8, 0.95), eps=1e-3,
                      engine=eng, **kw)


@pytest.mark.parametrize("kind, keyed", [("reversed", True), ("latent", False), ("plain", True)],
                         ids=["reversed-order_seeds", "latent-orders", "plain-order_seeds"])
def test_fit_with_hyper_equals_one_trainer_per_row(eng, kind, keyed, monkeypatch):
    n_epochs = 3
    p0 = _state(_cfg(kind), seed=2)["params"]
    rows = [r if kind != "plain" else r[:3] + [0.0] for r in VARIED]
    hyper = {name: [r[c] for r in rows] for c, name in enumerate(("lr", "w_reg", "threshold", "w_sym")) if kind != "plain" or c < 3}
    tables = _table(77, SEEDS, n_epochs).to(DEV)
    orders = [tables[e].reshape(S, -1)[:, :N].long() for e in range(n_epochs)]
    how = (lambda s: dict(order_seeds=SEEDS[s])) if keyed else (lambda s: dict(orders=iter([o[s] for o in orders])))
    tr = _trainer(eng, kind)
    built = []
    table_of = tr.hyper_table
    monkeypatch.setattr(tr, "hyper_table", lambda *a: built.append(table_of(*a)) or built[-1])
    got = tr.fit(p0, n_epochs, epochs_per_launch=2, hyper=hyper, **how(slice(None)))        # two launches, one table
    assert len(built) == 1 and torch.equal(built[0].cpu(), torch.tensor(rows))
    for s in range(S):
        one = slice(s, s + 1)
        want = _trainer(eng, kind, rows[s]).fit(p0[one], n_epochs, epochs_per_launch=2, **how(one))
        for k in ("Xi", "mask", "params", "m", "v", "step"):
            assert _bytes_equal(got[k][one].cpu(), want[k].cpu()), (s, k)
        assert got["log"][:, one].tobytes() == want["log"].tobytes(), s
    assert not torch.equal(got["mask"][0], got["mask"][2])
    # a key left out is the trainer's scalar: the fit with every column spelled out
    part = tr.fit(p0, n_epochs, hyper={"threshold": hyper["threshold"]}, **how(slice(None)))
    full = tr.fit(p0, n_epochs, hyper=dict({"lr": [tr.lr] * S, "w_reg": [tr.w_reg] * S}, threshold=hyper["threshold"]), **how(slice(None)))
    assert all(_bytes_equal(part[k].cpu(), full[k].cpu()) for k in ("Xi", "mask", "params", "m", "v", "step"))


# ------------------------------------------------------------------------------------------------ main_sweep --grid
THRESHOLDS, LRS = ("5e-2", "0.2"), ("0.01", "0.05")


def _sweep(main_sweep, save_dir, extra):
    argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "adam", "--batch_size", "256",
            "--w_sindy_x", "1.0", "--w_sindy_z", "0.0", "--w_sindy_reg", "0.001", "--w_sym_reg", "0.0", "--poly_order", "2",
            "--st_freq", "2", "--num_epochs", "2", "--seed", "4", "--n_seeds", "3", "--save_dir", save_dir]
    return main_sweep.main(argv + extra)


@pytest.mark.parametrize("shuffle", [["--device_shuffle"], []], ids=["device_shuffle", "host_shuffle"])
def test_main_sweep_grid_is_main_sweep_at_every_point(eng, shuffle, tmp_path, monkeypatch, capsys):
    from symode_amd import dataset as D, main_sweep
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples, noise-free
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)
    res = _sweep(main_sweep, "grid", shuffle + ["--grid", "threshold=" + ",".join(THRESHOLDS), "--grid", "lr_sindy=" + ",".join(LRS)])
    out = capsys.readouterr().out
    assert sorted(res) == [0, 1, 2, 3] and all(r["n_runs"] == 3 for r in res.values())
    assert "grid of 4 points x 3 seeds" in out and "grid 3: 3 seeds, 2 epochs x 5 Adam steps of 256 rows" in out
    root = tmp_path / "eval_results"
    listed = json.loads((root / "grid" / "grid.json").read_text())
    points = [(float(t), float(lr)) for t in THRESHOLDS for lr in LRS]                    # the first axis given is the slowest
    assert [(p["threshold"], p["lr_sindy"]) for p in listed["points"]] == points
    assert [p["grid"] for p in listed["points"]] == [0, 1, 2, 3] and listed["axes"][0][0] == "threshold"
    assert all(p["w_sindy_reg"] == 0.001 and 0.0 <= p["success_rate"] <= 1.0 for p in listed["points"])
    assert sorted(p.name for p in (root / "grid").iterdir()) == ["grid.json", "grid0", "grid1", "grid2", "grid3"]
    coefs = []
    for g, (t, lr) in enumerate(points):
        scalar = _sweep(main_sweep, f"point{g}", shuffle + ["--threshold", THRESHOLDS[g // 2], "--lr_sindy", LRS[g % 2]])
        assert scalar["n_runs"] == 3
        # without --grid the directory has the old layout
        assert sorted(p.name for p in (root / f"point{g}").iterdir()) == ["seed4.npz", "seed5.npz", "seed6.npz"]
        for s in (4, 5, 6):
            want, got = np.load(root / f"point{g}" / f"seed{s}.npz"), np.load(root / "grid" / f"grid{g}" / f"seed{s}.npz")
            assert got["coefficients"].shape == (2, 6) and np.isfinite(got["coefficients"]).all()
            assert got["coefficients"].tobytes() == want["coefficients"].tobytes(), (g, s)
            assert set(got.files) == set(want.files) | {"threshold", "lr_sindy", "w_sindy_reg"}
            assert (float(got["threshold"]), float(got["lr_sindy"]), float(got["w_sindy_reg"])) == (t, lr, 0.001)
            coefs.append(got["coefficients"])
    capsys.readouterr()
    assert not np.array_equal(coefs[0], coefs[1]) and not np.array_equal(coefs[0], coefs[3])   # seeds differ, and so do the points


def test_main_sweep_grid_with_eval_ltp_scores_and_ranks_the_points(eng, tmp_path, monkeypatch, capsys):
    from symode_amd import dataset as D, main_sweep
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)
    res = _sweep(main_sweep, "scored", ["--device_shuffle", "--lr_sindy", "0.01", "--eval_ltp", "--ltp_bound_rel", "0.1",
                                        "--grid", "threshold=" + ",".join(THRESHOLDS)])
    out = capsys.readouterr().out
    assert sorted(res) == [0, 1] and "grid of 2 points x 3 seeds" in out
    listed = json.loads((tmp_path / "eval_results" / "scored" / "grid.json").read_text())["points"]
    assert [p["threshold"] for p in listed] == [0.05, 0.2] and all(p["lr_sindy"] == 0.01 for p in listed)
    per_point = []
    for g in (0, 1):
        med = []
        for s in (4, 5, 6):
            got = np.load(tmp_path / "eval_results" / "scored" / f"grid{g}" / f"seed{s}.npz")
            assert got["ltp_mean_error"].shape == (3,) and got["ltp_horizon"].shape == (3,) and got["val_mse"].shape == ()
            med.append(np.median(got["ltp_mean_error"]))
        med = np.array(med)
        per_point.append(float(np.median(np.where(np.isfinite(med), med, np.inf))))
        want = per_point[-1] if np.isfinite(per_point[-1]) else None
        assert listed[g]["ltp_median_error"] == want and ("val_mse" in listed[g])
    best = int(np.argmin(per_point))                                  # the first of equals
    assert f"best by validation roll-out error: grid {best} (lr_sindy=0.01 w_sindy_reg=0.001 threshold={[0.05, 0.2][best]:g})" in out
