"""The cases of the latent Adam step tests (symode_adam_epochs_latent), drawn in the pattern of tests/adam_cases.py and run
through the same kind of driver: ``tests/test_gpu_adam_latent_steps.py`` plays them on the device,
``tests/test_host_adam_latent_model.py`` replays them on the CPU with the float32 model standing where the device stands.
Every launch is one epoch of one or two minibatch steps checked on its own against the fp64 model
(tests/adam_latent_model.py) from the float32 state that went into it.

A "device" is anything with ``launch(tables, state, cfg) -> (state, xi, log)`` as in adam_cases; ``cfg`` carries ``w_z``,
``D_obs`` and ``n_gen`` next to the settings of adam_cases, and ``log`` is (1, S, 10).
"""
import functools
import math

import torch

from tests import adam_cases as C
from tests import adam_latent_model as M
from tests.adam_cases import (BATCHES, COND_MAX, FORMS, MASKS, N_SRC, PADS, PROBLEMS, STARTS, STATE_KEYS, STEPS, Case,  # noqa: F401
                              _deck, _q_of, _rows, _state, lib_dims, libs_of, one_problem, same_bits)
from tests.trainer_cases import Report, _bytes_equal, _dev  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances.  Derived, not chosen, as in adam_cases: tests/test_host_adam_latent_model.py replays every case below with
# the model in float32, every sum taken one term after the other, against the model in fp64 from the same float32 state,
# takes per field the worst deviation relative to the field's largest magnitude in that problem, and asserts that each
# constant here is 4 x that figure (rounded up to two digits; x 4 because the device adds per-thread partial sums, a wave
# butterfly and four wave partials where the replay adds sequentially).  The replay figures and the worst the MI355X run
# showed are in profiles/adam_latent_steps.txt.
# ---------------------------------------------------------------------------------------------------------------------
TOL = {"params": 9.5e-7, "m": 1.5e-5, "v": 5.4e-6, "xi": 3.7e-6, "mse_z": 1.2e-6, "mse_x": 2.5e-6, "sym": 2.0e-6, "l1": 5.6e-7}

LIBS = C.LIBS
N_GENS = [0, 1, 3]
D_EXTRA = [0, 2]                                                        # D_obs - d
HYPER = {"default": {}, "weighted": dict(lr=3e-2, betas=(0.8, 0.95), eps=1e-3, w_z=0.37, w_x=0.6, w_sym=2e-3, w_reg=0.05),
         "beta1_0": dict(betas=(0.0, 0.999)), "no_l1": dict(l1=False, w_sym=5e-4), "w_z4": dict(w_z=4.0, w_x=0.0)}
W_SYM = 1e-3                                                            # the regulariser is a SUM over the batch's rows
PER_LIB = 27


# ---------------------------------------------------------------------------------------------------------------------
# data: z, dz the noisy quadratic field of adam_cases; B, y, e random; rotation and scaling generators
# ---------------------------------------------------------------------------------------------------------------------
def _field(d):
    f = C.field(d)
    g = torch.Generator().manual_seed(300 + d)
    B = (torch.eye(d)[None] + 0.3 * torch.randn(N_SRC, d, d, generator=g)).contiguous()
    y = torch.randn(N_SRC, d, generator=g)
    e = 0.5 * torch.rand(N_SRC, generator=g)
    rot, scale, third = torch.zeros(d, d), torch.eye(d), torch.diag(torch.tensor([(-0.5) ** k for k in range(d)]))
    if d == 1:
        rot[0, 0] = -0.7
    else:
        rot[0, 1], rot[1, 0] = -1.0, 1.0
        third[0, d - 1] = 0.25
    return dict(z=f["x"], dz=f["dx"], B=B, y=y, e=e, L=torch.stack([rot, scale, third]).contiguous())


_FIELDS = {}


def field(d):
    if d not in _FIELDS:
        _FIELDS[d] = _field(d)
    return _FIELDS[d]


def data_of(cfg):
    """The float32 operands of a launch: e None with D_obs == d, L the first n_gen generators (None without)."""
    f = field(cfg["d"])
    n_gen = cfg["n_gen"]
    return dict(z=f["z"], dz=f["dz"], B=f["B"], y=f["y"], e=f["e"] if cfg["D_obs"] > cfg["d"] else None,
                L=f["L"][:n_gen].contiguous() if n_gen else None)


# ---------------------------------------------------------------------------------------------------------------------
# one launch by the model
# ---------------------------------------------------------------------------------------------------------------------
def predict(tables, state, cfg, s, dt=torch.float64, sequential=False, mutant=None):
    """Problem ``s`` through the launch (one epoch).  Returns (state', xi, log row as 10 Python floats, margins, steps)."""
    data = data_of(cfg)
    st = {k: state[k][s].reshape(-1).to(dt) for k in ("params", "m", "v", "mask")}
    st["step"] = int(state["step"][s])
    tab = tables[0, s if tables.shape[1] > 1 else 0]
    recs = []
    for k in range(tab.shape[0]):
        st, rec = M.step(st, tab[k], data, cfg, sequential, mutant)
        if rec is not None:
            recs.append(rec)
    xi = M.xi_of(st["params"], cfg)
    st, ev, mg = M.epoch_end(st, xi, cfg, cfg["epoch0"])
    nan = float("nan")
    mean = lambda key: float(sum(float(r[key]) for r in recs) / len(recs)) if recs else nan  # noqa: E731
    row = [mean("mse_x"), mean("l1"), float(len(recs)), float(ev["near"]), float(st["step"] < 0), float(ev["event"]),
           float(cfg["epoch0"]), mean("sym"), mean("mse_z"), 0.0]
    return st, xi, row, mg, len(recs)


class ModelDevice:
    """The model standing where the device stands: float32 with sequential sums (the replay), or any dtype with a mutant."""

    def __init__(self, dt=torch.float32, sequential=True, mutant=None):
        self.dt, self.sequential, self.mutant = dt, sequential, mutant

    def launch(self, tables, state, cfg):
        S = state["params"].shape[0]
        out = {k: state[k].clone() for k in STATE_KEYS}
        xi, log = torch.zeros_like(state["mask"]), torch.zeros(1, S, 10)
        for s in range(S):
            st, x, row, _, _ = predict(tables, state, cfg, s, self.dt, self.sequential, self.mutant)
            for k in ("params", "m", "v", "mask"):
                out[k][s] = st[k].to(torch.float32).reshape(out[k][s].shape)
            out["step"][s] = st["step"]
            xi[s], log[0, s] = x.to(torch.float32), torch.tensor(row)
        return out, xi, log


_REFERENCE = {}                                                         # (case name, problem) -> the fp64 prediction, computed once


def check_launch(rep, case, dev, tol=None):
    """Play ``case`` on ``dev`` and compare with the fp64 model.  Returns what the device returned."""
    tol = TOL if tol is None else tol
    cfg, tables, state = case.cfg, case.tables, case.state
    before = {k: v.clone() for k, v in state.items()}
    out, xi, log = dev.launch(tables, state, cfg)
    assert tuple(log.shape) == (1, state["params"].shape[0], 10), (case.name, tuple(log.shape))
    for k in STATE_KEYS:
        assert _bytes_equal(state[k], before[k]), (case.name, k, "the device wrapper changed the case's own state")
    for s in range(state["params"].shape[0]):
        where = (case.name, s)
        if where not in _REFERENCE:
            _REFERENCE[where] = predict(tables, state, cfg, s)
        want, want_xi, row, mg, steps = _REFERENCE[where]
        rep.launches += 1
        rep.unsettled += [where + m for m in mg if m[0] not in case.exact and M.unsettled([m], tol["xi"])]
        if int(out["step"][s]) != want["step"]:
            rep.mismatch.append(where + ("step", int(out["step"][s]), want["step"]))
        if not torch.equal(out["mask"][s].reshape(-1).double(), want["mask"]):
            rep.mismatch.append(where + ("mask", out["mask"][s].reshape(-1).tolist(), want["mask"].tolist()))
        for col, name in ((2, "steps"), (3, "near"), (4, "frozen"), (5, "event"), (6, "epoch"), (9, "unused")):
            if float(log[0, s, col]) != row[col]:
                rep.mismatch.append(where + ("log column %d (%s)" % (col, name), float(log[0, s, col]), row[col]))
        if steps == 0:                                       # padding alone, frozen, or frozen by this launch: bit for bit as found
            for k in ("params", "m", "v"):
                if not _bytes_equal(out[k][s], state[k][s]):
                    rep.mismatch.append(where + (k, "changed although no step was taken", None))
        for k in ("params", "m", "v"):
            rep.dev(k, _dev(out[k][s], want[k]), where)
        rep.dev("xi", _dev(xi[s], want_xi), where)
        for col, k in ((0, "mse_x"), (1, "l1"), (7, "sym"), (8, "mse_z")):
            rep.dev(k, _dev(log[0, s, col], torch.tensor(row[col], dtype=torch.float64)), where)
    return out, xi, log


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(lib, hyper, form, n_gen, d_extra, **extra):
    p, dp = lib_dims(lib)
    q, allow = _q_of(form, dp)
    kw = dict(dict(w_sym=W_SYM), **HYPER[hyper])
    kw.update(extra)
    cfg = M.make_cfg(*lib, D_obs=lib[0] + d_extra, n_gen=n_gen, map=None if q is None else (q.double(), q.shape[1], p, allow), **kw)
    cfg.update(entry="latent", q=q, allow_const=allow)
    return cfg


def cancellation(case):
    """adam_cases.cancellation on this entry's gradient: under the constraint, sum_j |Q_jc| |g_xi_j| over the largest
    |(Q^T g_xi)_c|, the worst over the problems and steps of the launch, by the fp64 model alone; 1 without the constraint."""
    cfg, worst = case.cfg, 1.0
    if cfg["map"] is None:
        return worst
    Q, r = cfg["map"][0], cfg["map"][1]
    data = data_of(cfg)
    for s in range(case.state["params"].shape[0]):
        st = {k: case.state[k][s].reshape(-1).double() for k in ("params", "m", "v", "mask")}
        st["step"] = int(case.state["step"][s])
        tab = case.tables[0, s if case.tables.shape[1] > 1 else 0]
        for k in range(tab.shape[0]):
            rows = M.valid_rows(tab[k], N_SRC)
            if rows and st["step"] >= 0 and bool(st["mask"].any()):
                g, g_xi = M.loss_and_grad(st["params"], st["mask"], rows, data, cfg)[3:]
                worst = max(worst, float((Q.abs().T @ g_xi.abs()).max()) / max(float(g[:r].abs().max()), 1e-300))
            st, _ = M.step(st, tab[k], data, cfg)
    return worst


def grid_cases(libs=LIBS):
    return _grid(tuple(libs))


@functools.lru_cache(maxsize=None)
def _grid(libs):
    """Per library PER_LIB cases with every axis drawn from its own shuffled deck, and the three fixed pairings of
    adam_cases (513 columns with the middle chunk padding, one valid row among 256 columns, padding alone)."""
    out = []
    for lib in libs:
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(9000 + 100 * lib[0] + 10 * lib[1] + lib[2])
        n = PER_LIB + 3
        deck = {k: _deck(v, n, gen) for k, v in (("batch", BATCHES), ("pad", PADS), ("form", FORMS), ("mask", MASKS), ("start", STARTS),
                                                   ("hyper", list(HYPER)), ("n_gen", N_GENS), ("d_extra", D_EXTRA),
                                                   ("problems", PROBLEMS), ("steps", STEPS))}
        for k in range(n):
            batch, pad = deck["batch"][k], deck["pad"][k]
            if k >= PER_LIB:
                batch, pad = [(513, "middle"), (256, "one_valid"), (65, "all_pad")][k - PER_LIB]
            form, hyper, steps, n_gen, d_extra = deck["form"][k], deck["hyper"][k], deck["steps"][k], deck["n_gen"][k], deck["d_extra"][k]
            S, own = deck["problems"][k]
            cfg = _cfg(lib, hyper, form, n_gen, d_extra, epoch0=k % 3)
            n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + d
            first = STARTS.index(deck["start"][k])
            starts = [STARTS[(first + s) % len(STARTS)] for s in range(S)]
            masks = [MASKS[(MASKS.index(deck["mask"][k]) + s) % len(MASKS)] for s in range(S)]
            name = (f"d{lib[0]}o{lib[1]}f{lib[2]}-{k}-b{batch}-{pad}-{form}-{deck['mask'][k]}-t{starts[0]}-{hyper}-g{n_gen}-D{d + d_extra}"
                    f"-S{S}{'own' if own else ''}-{steps}")
            for draw in range(20):                           # state and tables are drawn again while the beta gradient cancels
                state = _state(S, n_par, d, p, starts, masks, cfg["l1"], gen)
                tabs = []
                for _ in range(S if own else 1):
                    last = _rows(batch, pad, gen)
                    if steps == "one":
                        tabs.append(last[None])
                    elif steps == "pad_then_one":
                        tabs.append(torch.stack([_rows(batch, "all_pad", gen), last]))
                    else:
                        tabs.append(torch.stack([_rows(batch, "none" if pad == "all_pad" else pad, gen), last]))
                case = Case(name, cfg, torch.stack(tabs)[None].contiguous(), state, (), None)
                if cancellation(case) <= COND_MAX:
                    break
            else:
                raise AssertionError(f"{name}: no well-conditioned draw")
            out.append(case)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# freezing: S = 3, problem 1 holds an inf parameter at t = 9
# ---------------------------------------------------------------------------------------------------------------------
FREEZE_LIBS = [((2, 2, 2), 1, 0), ((3, 3, 1), 3, 2)]                    # (library, n_gen, D_obs - d)


def freeze_cases(libs=None):
    out = []
    for lib, n_gen, d_extra in FREEZE_LIBS:
        if libs is not None and lib not in libs:
            continue
        p, dp = lib_dims(lib)
        gen = torch.Generator().manual_seed(83 + dp)
        cfg = _cfg(lib, "weighted", "xi", n_gen, d_extra)
        state = _state(3, dp, lib[0], p, [1, 9, 999], ["ones", "ones", "half"], True, gen)
        state["params"][1, dp // 2] = float("inf")
        tables = torch.stack([_rows(65, "tail", gen)[None] for _ in range(3)])[None].contiguous()
        out.append(Case(f"freeze-d{lib[0]}o{lib[1]}f{lib[2]}-g{n_gen}-D{lib[0] + d_extra}", cfg, tables, state, (), None))
    return out


def check_freeze(rep, case, dev):
    """The frozen problem keeps its state bit for bit and gets step = -10; the neighbours equal their own launches bit for bit."""
    out, xi, log = check_launch(rep, case, dev)
    bad = [k for k in ("params", "m", "v", "mask") if not _bytes_equal(out[k][1], case.state[k][1])]
    assert bad == [] and int(out["step"][1]) == -10 and float(log[0, 1, 4]) == 1.0 and float(log[0, 1, 2]) == 0.0, (case.name, bad, out["step"])
    assert all(math.isnan(float(log[0, 1, c])) for c in (0, 1, 7, 8)), (case.name, log[0, 1])
    for s in (0, 2):
        one = one_problem(case, s)
        o1, x1, l1 = check_launch(rep, one, dev)
        got = {k: v[s:s + 1] for k, v in out.items()}
        assert same_bits(got, o1) == [] and _bytes_equal(xi[s:s + 1], x1) and _bytes_equal(log[:, s:s + 1], l1), (case.name, s)
        assert int(o1["step"][0]) == int(case.state["step"][s]) + 1


# ---------------------------------------------------------------------------------------------------------------------
# the epoch end: the placed coefficients of adam_cases around the threshold
# ---------------------------------------------------------------------------------------------------------------------
THRESHOLD, NEAR_BAND, EPOCH_LR = C.THRESHOLD, C.NEAR_BAND, C.EPOCH_LR
EPOCH_LIBS = C.EPOCH_LIBS


def epoch_cases(libs=None):
    """st_freq = 1 events (unconstrained and constrained, with and without generators), st_freq = 2 met and missed by epoch0."""
    out = []
    S = 2
    for lib in EPOCH_LIBS:
        if libs is not None and lib not in libs:
            continue
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(950 + dp)
        xi, mask, near, after = C._placed(S, dp)
        variants = [("xi", 0, 0, 1, 0), ("xi", 3, 2, 1, 5), ("qfc", 1, 0, 1, 2), ("qfc", 3, 2, 1, 0), ("xi", 1, 2, 2, 1), ("xi", 1, 0, 2, 2)]
        for form, n_gen, d_extra, st_freq, epoch0 in variants:
            cfg = _cfg(lib, "default", form, n_gen, d_extra, lr=EPOCH_LR, threshold=THRESHOLD, near_band=NEAR_BAND, st_freq=st_freq, epoch0=epoch0)
            if cfg["q"] is None:
                params = xi.float()
            else:                                            # [beta | const] with reshape(Q beta) + const = the placed Xi (adam_cases)
                const = 0.05 * torch.randn(S, d, generator=gen)
                rest = xi.clone()
                rest[:, ::p] -= const.double()
                params = torch.cat([(rest @ cfg["q"].double()).float(), const], dim=1).contiguous()
            state = _state(S, params.shape[1], d, p, [9, 0], ["ones", "ones"], False, gen)
            state["params"], state["mask"] = params, mask.clone()
            event = (epoch0 + 1) % st_freq == 0
            expect = dict(near=near if event else [0] * S, mask=after if event else mask, event=event)
            tables = _rows(64, "tail", gen)[None, None, None].contiguous()
            out.append(Case(f"epoch-d{lib[0]}o{lib[1]}f{lib[2]}-{form}-g{n_gen}-D{d + d_extra}-st{st_freq}-e{epoch0}", cfg, tables, state, (), expect))
    return out


def check_epoch(rep, case, dev):
    out, xi, log = check_launch(rep, case, dev)
    e = case.expect
    assert [int(v) for v in log[0, :, 3]] == e["near"] and torch.equal(out["mask"], e["mask"]), (case.name, log[0, :, 3], e["near"])
    assert all(float(v) == float(e["event"]) for v in log[0, :, 5]), (case.name, log[0, :, 5])


# ---------------------------------------------------------------------------------------------------------------------
# structure, bit for bit: one launch of 1 epoch x 2 steps equals two launches of 1 x 1 step
# ---------------------------------------------------------------------------------------------------------------------
STRUCTURE_LIBS = C.STRUCTURE_LIBS


def structure_cases(libs=None):
    """n_gen 0 / 3 x Xi and [beta | const] x batch 64, 257, 513, dealt out over the two libraries as in adam_cases."""
    out = []
    combos = [(n_gen, form, batch) for n_gen in (0, 3) for form in ("xi", "q5c") for batch in (64, 257, 513)]
    both = libs is None or all(lib in libs for lib in STRUCTURE_LIBS)
    for k, lib in enumerate(STRUCTURE_LIBS):
        if libs is not None and lib not in libs:
            continue
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(550 + dp)
        for n_gen, form, batch in (combos[k::2] if both else combos):
            cfg = _cfg(lib, "weighted", form, n_gen, 2 if batch != 257 else 0)
            n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + d
            state = _state(2, n_par, d, p, [0, 9], ["ones", "half"], True, gen)
            tables = torch.stack([torch.stack([_rows(batch, "scattered", gen), _rows(batch, "tail", gen)]) for _ in range(2)])[None]
            out.append(Case(f"structure-d{lib[0]}o{lib[1]}f{lib[2]}-g{n_gen}-{form}-b{batch}", cfg, tables.contiguous(), state, (), None))
    return out


def check_structure(case, dev):
    """params, m, v, step, mask and xi of the 2-step launch against step 0 then step 1 as launches of their own."""
    whole, xi_w, _ = dev.launch(case.tables, case.state, case.cfg)
    a, _, _ = dev.launch(case.tables[:, :, :1].contiguous(), case.state, case.cfg)
    b, xi_b, _ = dev.launch(case.tables[:, :, 1:].contiguous(), a, case.cfg)
    assert same_bits(whole, b) == [] and _bytes_equal(xi_w, xi_b), (case.name, same_bits(whole, b))
    assert whole["step"].tolist() == (case.state["step"] + 2).tolist(), (case.name, whole["step"])
