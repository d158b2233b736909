"""The cases of the Adam step tests, and the one driver both sides run them through.

``tests/test_gpu_adam_steps.py`` plays them on the device, ``tests/test_host_adam_model.py`` replays them on the CPU with
the float32 model standing where the device stands.  Every launch is one epoch of one or two minibatch steps and is checked
on its own: the fp64 model (tests/adam_model.py) is handed the float32 state that went into the launch and predicts the
state, Xi and the log row after it -- teacher forcing, no trajectory drift.  After one step ``m`` and ``v`` carry the
gradient itself, (1 - b1) g and (1 - b2) g^2 on top of what was injected, so a wrong gradient scale shows at once.

A "device" is anything with ``launch(tables, state, cfg) -> (state, xi, log)``: ``tables`` (1, S or 1, n_steps, batch) int32,
``state`` a dict of CPU tensors ``params m v`` (S, n) float32, ``step`` (S,) int32, ``mask`` (S, d p) float32 (not modified),
``cfg`` the model's settings plus ``entry`` ("plain" / "reversed"), ``n_g`` and ``q`` (the float32 Q_eff or None); it returns the
state after the launch, ``xi`` (S, d p) and ``log`` (1, S, 8), all on the CPU.
"""
import functools
import math
from collections import namedtuple

import torch

from tests import adam_model as M
from tests.trainer_cases import Report, _bytes_equal, _dev, householder_q

N_SRC = 600
W_SYM = 0.25

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances.  Derived, not chosen: tests/test_host_adam_model.py replays every case below with the model in float32,
# every sum taken one term after the other, against the model in fp64 from the same float32 state, takes per field the
# worst deviation relative to the field's largest magnitude in that problem, and asserts that each constant here is 4 x
# that figure (rounded up to two digits; x 4 because the device adds per-thread partial sums, a wave butterfly and four
# wave partials where the replay adds sequentially).  The replay figures and the worst the MI355X run showed are in
# profiles/adam_steps.txt.
# ---------------------------------------------------------------------------------------------------------------------
TOL = {"params": 5.8e-7, "m": 2.5e-6, "v": 4.8e-6, "xi": 1.8e-6, "mse": 2.2e-6, "l1": 5.3e-7, "sym": 4.0e-6}
STATE_KEYS = ("params", "m", "v", "step", "mask")


# ---------------------------------------------------------------------------------------------------------------------
# data: the noisy quadratic field of tests/test_gpu_adam.py on 600 rows, three group elements
# ---------------------------------------------------------------------------------------------------------------------
def _rot(angle, d):
    R = torch.eye(d, dtype=torch.float64)
    if d == 1:
        R[0, 0] = -math.cos(angle)                     # no plane to rotate in: a contracting reflection, g(x) far from x
    else:
        R[0, 0], R[0, 1], R[1, 0], R[1, 1] = math.cos(angle), -math.sin(angle), math.sin(angle), math.cos(angle)
    return R


def _field(d):
    g = torch.Generator().manual_seed(100 + d)
    x = (torch.rand(N_SRC, d, generator=g) - 0.5) * 3.0
    A = torch.randn(d, d, generator=g)
    B = torch.randn(d, d * (d + 1) // 2, generator=g) * 0.5
    quad = torch.stack([x[:, i] * x[:, j] for i in range(d) for j in range(i, d)], dim=1)
    dx = x @ A.T + quad @ B.T + 0.05 * torch.randn(N_SRC, d, generator=g)
    x, dx = x.contiguous(), dx.contiguous()
    # g1 = R(0.3) x, g2 = R(-0.2) x + 0.1 sin x (tests/test_gpu_adam_reversed.py), g3 = R(0.5) (x + 0.1 sin x)
    xd = x.double()
    R1, R2, R3 = _rot(0.3, d), _rot(-0.2, d), _rot(0.5, d)
    gx = torch.stack([xd @ R1.T, xd @ R2.T + 0.1 * torch.sin(xd), (xd + 0.1 * torch.sin(xd)) @ R3.T])
    eye = torch.eye(d, dtype=torch.float64)
    jgx = torch.stack([R1.expand(N_SRC, d, d), R2[None] + 0.1 * torch.diag_embed(torch.cos(xd)),
                       R3[None] @ (eye[None] + 0.1 * torch.diag_embed(torch.cos(xd)))])
    return dict(x=x, dx=dx, gx=gx.float().contiguous(), jgx=jgx.float().contiguous())


_FIELDS = {}


def field(d):
    if d not in _FIELDS:
        _FIELDS[d] = _field(d)
    return _FIELDS[d]


def data_of(cfg):
    """The float32 operands of a launch: x, dx and the first n_g group elements (None without)."""
    f = field(cfg["d"])
    n_g = cfg["n_g"] if cfg["entry"] == "reversed" else 0
    return dict(x=f["x"], dx=f["dx"], gx=f["gx"][:n_g].contiguous() if n_g else None, jgx=f["jgx"][:n_g].contiguous() if n_g else None)


# ---------------------------------------------------------------------------------------------------------------------
# one launch by the model: the reference (fp64) and the stand-in device (float32, sequential sums)
# ---------------------------------------------------------------------------------------------------------------------
def predict(tables, state, cfg, s, dt=torch.float64, sequential=False, mutant=None):
    """Problem ``s`` through the launch (one epoch).  Returns (state', xi, log row as 8 Python floats, margins, steps)."""
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
    st, ev, mg = M.epoch_end(st, xi, cfg, cfg["epoch0"], mutant)
    nan = float("nan")
    mean = lambda key: float(sum(float(r[key]) for r in recs) / len(recs)) if recs else nan  # noqa: E731
    with_reg = cfg["entry"] == "reversed" and cfg["n_g"] > 0
    row = [mean("mse"), mean("l1"), float(len(recs)), float(ev["near"]), float(st["step"] < 0), float(ev["event"]),
           float(cfg["epoch0"]), mean("sym") if with_reg else 0.0]
    return st, xi, row, mg, len(recs)


class ModelDevice:
    """The model standing where the device stands: float32 with sequential sums (the replay), or any dtype with a mutant."""

    def __init__(self, dt=torch.float32, sequential=True, mutant=None):
        self.dt, self.sequential, self.mutant = dt, sequential, mutant

    def launch(self, tables, state, cfg):
        S = state["params"].shape[0]
        out = {k: state[k].clone() for k in STATE_KEYS}
        xi, log = torch.zeros_like(state["mask"]), torch.zeros(1, S, 8)
        for s in range(S):
            st, x, row, _, _ = predict(tables, state, cfg, s, self.dt, self.sequential, self.mutant)
            for k in ("params", "m", "v", "mask"):
                out[k][s] = st[k].to(torch.float32).reshape(out[k][s].shape)
            out["step"][s] = st["step"]
            xi[s], log[0, s] = x.to(torch.float32), torch.tensor(row)
        return out, xi, log


# ---------------------------------------------------------------------------------------------------------------------
# the driver: one launch against the fp64 model
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name cfg tables state exact expect")         # exact: margin names equal by construction; expect: dict or None
_REFERENCE = {}                                                         # (case name, problem) -> the fp64 prediction, computed once


def check_launch(rep, case, dev, tol=None):
    """Play ``case`` on ``dev`` and compare with the fp64 model.  Returns what the device returned."""
    tol = TOL if tol is None else tol
    cfg, tables, state = case.cfg, case.tables, case.state
    before = {k: v.clone() for k, v in state.items()}
    out, xi, log = dev.launch(tables, state, cfg)
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
        for col, name in ((2, "steps"), (3, "near"), (4, "frozen"), (5, "event"), (6, "epoch")):
            if float(log[0, s, col]) != row[col]:
                rep.mismatch.append(where + ("log column %d (%s)" % (col, name), float(log[0, s, col]), row[col]))
        if steps == 0:                                       # padding alone, frozen, or frozen by this launch: bit for bit as found
            for k in ("params", "m", "v"):
                if not _bytes_equal(out[k][s], state[k][s]):
                    rep.mismatch.append(where + (k, "changed although no step was taken", None))
        for k in ("params", "m", "v"):
            rep.dev(k, _dev(out[k][s], want[k]), where)
        rep.dev("xi", _dev(xi[s], want_xi), where)
        for col, k in ((0, "mse"), (1, "l1"), (7, "sym")):
            rep.dev(k, _dev(log[0, s, col], torch.tensor(row[col], dtype=torch.float64)), where)
    return out, xi, log


def same_bits(a, b, keys=STATE_KEYS):
    return [k for k in keys if not _bytes_equal(a[k], b[k])]


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------
LIBS = [(1, 3, 0), (2, 2, 2), (2, 5, 0), (3, 3, 0), (3, 3, 1), (3, 4, 1), (4, 2, 0), (4, 3, 3)]
BATCHES = [1, 63, 64, 65, 256, 257, 513]
PADS = ["none", "tail", "scattered", "middle", "one_valid", "all_pad"]
FORMS = ["xi", "xi", "q1c", "q5c", "qmc", "q1", "q5", "qm"]             # q<r>[c]: Q_eff with r columns (m: d p - 1, f: d p), c: constants added
MASKS = ["ones", "half", "row_off", "zero"]
STARTS = [0, 1, 9, 999, 100000]                                         # t found in the state; 0: fresh, m = v = 0
HYPER = {"default": {}, "weighted": dict(lr=3e-2, betas=(0.8, 0.95), eps=1e-3, w_x=0.37, w_reg=0.05), "beta1_0": dict(betas=(0.0, 0.999)),
         "no_l1": dict(l1=False), "w_x4": dict(w_x=4.0)}
ENTRIES = ["plain", "rev0", "rev1", "rev3"]
PROBLEMS = [(1, False), (3, False), (3, True)]                          # (S, one table per problem)
STEPS = ["one", "one", "one", "one", "pad_then_one", "two"]
PER_LIB = 27                                                            # drawn cases per library, + 3 fixed pairings
JUNK = [-1, N_SRC, N_SRC + 5, -2 ** 31]


def lib_dims(lib):
    cfg = M.make_cfg(*lib)
    p = M.terms(cfg)
    return p, lib[0] * p


def _deck(values, n, gen):
    """``values`` repeated to n entries and shuffled: every value comes up about equally often."""
    reps = (list(range(len(values))) * (n // len(values) + 1))[:n]
    order = torch.randperm(n, generator=gen).tolist()
    return [values[reps[i]] for i in order]


def _rows(batch, pad, gen):
    rows = torch.randint(0, N_SRC, (batch,), generator=gen, dtype=torch.int64)          # with replacement: duplicates
    junk = torch.tensor(JUNK, dtype=torch.int64)
    if pad == "tail" and batch > 1:
        rows[batch - max(1, batch // 5):] = -1
    elif pad == "scattered" and batch > 1:
        hit = torch.rand(batch, generator=gen) < 0.3
        hit[int(torch.randint(0, batch, (1,), generator=gen))] = False
        rows[hit] = junk[torch.randint(0, 4, (int(hit.sum()),), generator=gen)]
    elif pad == "middle" and batch > 2:
        lo, hi = (256, 512) if batch > 512 else (batch // 3, 2 * batch // 3)               # 513: the whole middle chunk
        rows[lo:hi] = junk[torch.arange(hi - lo) % 4]
    elif pad == "one_valid":
        keep = int(torch.randint(0, batch, (1,), generator=gen))
        one = rows[keep].clone()
        rows[:] = -1
        rows[keep] = one
    elif pad == "all_pad":
        rows = junk[torch.arange(batch) % 4]
    return rows.to(torch.int32)


def _q_of(form, dp):
    if form == "xi":
        return None, True
    r = {"m": dp - 1, "f": dp}[form[1]] if form[1] in "mf" else int(form[1])
    return householder_q(dp, max(r, 1)), form.endswith("c")


def _mask(kind, d, p, gen):
    mk = torch.ones(d, p)
    if kind == "half":
        mk = (torch.rand(d, p, generator=gen) < 0.5).float()
    elif kind == "row_off":
        mk[int(torch.randint(0, d, (1,), generator=gen))] = 0.0
    elif kind == "zero":
        mk.zero_()
    return mk.reshape(-1)


def _state(S, n, d, p, starts, masks, l1, gen):
    params = 0.3 * torch.randn(S, n, generator=gen)
    if l1:                                                   # exact zeros (and a -0) among the parameters: sign(0) = 0
        for s in range(S):
            j = torch.randperm(n, generator=gen)[:3].tolist()
            params[s, j[0]] = 0.0
            if n > 2:
                params[s, j[1]] = -0.0
    m = 0.3 * torch.randn(S, n, generator=gen)
    v = m * m * (0.5 + 1.5 * torch.rand(S, n, generator=gen))
    step = torch.tensor(starts, dtype=torch.int32)
    fresh = step == 0
    m[fresh], v[fresh] = 0.0, 0.0
    mask = torch.stack([_mask(masks[s], d, p, gen) for s in range(S)])
    return dict(params=params, m=m, v=v, step=step, mask=mask)


def _cfg(lib, hyper, entry, form, **extra):
    p, dp = lib_dims(lib)
    q, allow = _q_of(form, dp)
    kw = dict(HYPER[hyper], **extra)
    rev = entry != "plain"
    cfg = M.make_cfg(*lib, w_sym=W_SYM if rev else 0.0, map=None if q is None else (q.double(), q.shape[1], p, allow), **kw)
    cfg.update(entry="reversed" if rev else "plain", n_g=int(entry[3:]) if rev else 0, q=q, allow_const=allow)
    return cfg


COND_MAX = 32.0


def cancellation(case):
    """Under the constraint the beta gradient is Q^T g_xi: sum_j |Q_jc| |g_xi_j| over the largest |(Q^T g_xi)_c|, the worst over
    the problems and steps of the launch, by the fp64 model alone.  A draw where this is large measures the rounding of
    a cancelling dot product (in m and v, relative to their largest entry), not the trainer; 1 without the constraint."""
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
                _, _, g, g_xi = M.loss_and_grad(st["params"], st["mask"], rows, data, cfg)
                worst = max(worst, float((Q.abs().T @ g_xi.abs()).max()) / max(float(g[:r].abs().max()), 1e-300))
            st, _ = M.step(st, tab[k], data, cfg)
    return worst


def grid_cases(libs=LIBS):
    return _grid(tuple(libs))


@functools.lru_cache(maxsize=None)
def _grid(libs):
    """The covering set: per library PER_LIB cases with every axis drawn from its own shuffled deck, and three fixed
    pairings (513 columns with the middle chunk padding, one valid row among 256 columns, padding alone)."""
    out = []
    for li, lib in enumerate(libs):
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(7000 + 100 * lib[0] + 10 * lib[1] + lib[2])
        n = PER_LIB + 3
        deck = {k: _deck(v, n, gen) for k, v in (("batch", BATCHES), ("pad", PADS), ("form", FORMS), ("mask", MASKS), ("start", STARTS),
                                                   ("hyper", list(HYPER)), ("entry", ENTRIES), ("problems", PROBLEMS), ("steps", STEPS))}
        for k in range(n):
            batch, pad = deck["batch"][k], deck["pad"][k]
            if k >= PER_LIB:
                batch, pad = [(513, "middle"), (256, "one_valid"), (65, "all_pad")][k - PER_LIB]
            form, hyper, entry, steps = deck["form"][k], deck["hyper"][k], deck["entry"][k], deck["steps"][k]
            S, own = deck["problems"][k]
            cfg = _cfg(lib, hyper, entry, form, epoch0=k % 3)
            n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + d
            first = STARTS.index(deck["start"][k])
            starts = [STARTS[(first + s) % len(STARTS)] for s in range(S)]
            masks = [MASKS[(MASKS.index(deck["mask"][k]) + s) % len(MASKS)] for s in range(S)]
            name = f"d{lib[0]}o{lib[1]}f{lib[2]}-{k}-b{batch}-{pad}-{form}-{deck['mask'][k]}-t{starts[0]}-{hyper}-{entry}-S{S}{'own' if own else ''}-{steps}"
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
FREEZE_LIBS = [((2, 2, 2), "plain"), ((3, 3, 1), "rev3")]


def freeze_cases(libs=None):
    out = []
    for lib, entry in FREEZE_LIBS:
        if libs is not None and lib not in libs:
            continue
        p, dp = lib_dims(lib)
        gen = torch.Generator().manual_seed(81 + dp)
        cfg = _cfg(lib, "weighted", entry, "xi")
        state = _state(3, dp, lib[0], p, [1, 9, 999], ["ones", "ones", "half"], True, gen)
        state["params"][1, dp // 2] = float("inf")
        tables = torch.stack([_rows(65, "tail", gen)[None] for _ in range(3)])[None].contiguous()
        out.append(Case(f"freeze-d{lib[0]}o{lib[1]}f{lib[2]}-{entry}", cfg, tables, state, (), None))
    return out


def one_problem(case, s):
    """Problem ``s`` of ``case`` as a launch of its own."""
    tables = case.tables[:, s:s + 1] if case.tables.shape[1] > 1 else case.tables
    return Case(case.name + f"/problem{s}", case.cfg, tables.contiguous(), {k: v[s:s + 1].clone() for k, v in case.state.items()}, case.exact, None)


def check_freeze(rep, case, dev):
    """The frozen problem keeps its state bit for bit and gets step = -10; the neighbours equal their own launches bit for bit."""
    out, xi, log = check_launch(rep, case, dev)
    bad = [k for k in ("params", "m", "v", "mask") if not _bytes_equal(out[k][1], case.state[k][1])]
    assert bad == [] and int(out["step"][1]) == -10 and float(log[0, 1, 4]) == 1.0 and float(log[0, 1, 2]) == 0.0, (case.name, bad, out["step"])
    assert math.isnan(float(log[0, 1, 0])) and math.isnan(float(log[0, 1, 1])), (case.name, log[0, 1])
    for s in (0, 2):
        one = one_problem(case, s)
        o1, x1, l1 = check_launch(rep, one, dev)
        got = {k: v[s:s + 1] for k, v in out.items()}
        assert same_bits(got, o1) == [] and _bytes_equal(xi[s:s + 1], x1) and _bytes_equal(log[:, s:s + 1], l1), (case.name, s)
        assert int(o1["step"][0]) == int(case.state["step"][s]) + 1


# ---------------------------------------------------------------------------------------------------------------------
# the epoch end: coefficients placed around the threshold, a mask that already has zeros
# ---------------------------------------------------------------------------------------------------------------------
THRESHOLD, NEAR_BAND, EPOCH_LR = 0.1, 1e-2, 1e-6
EPOCH_LIBS = [(2, 2, 2), (3, 3, 1)]
_PLACES = [THRESHOLD + NEAR_BAND / 2, -(THRESHOLD + NEAR_BAND / 2), THRESHOLD - NEAR_BAND / 2, -(THRESHOLD - NEAR_BAND / 2),
           THRESHOLD + 2 * NEAR_BAND, -(THRESHOLD + 2 * NEAR_BAND), THRESHOLD - 2 * NEAR_BAND, -(THRESHOLD - 2 * NEAR_BAND), 0.5, -0.02]


def _placed(S, dp):
    """Xi (S, dp) cycling through _PLACES, a mask with zeros on every kind of place, and per problem the coefficients that
    are near (|.| within the band, mask set) and the mask after a strict threshold."""
    xi, mask = torch.zeros(S, dp, dtype=torch.float64), torch.ones(S, dp)
    near, after = [], torch.zeros(S, dp)
    for s in range(S):
        n = 0
        for j in range(dp):
            k = (j + 3 * s) % len(_PLACES)
            xi[s, j] = _PLACES[k]
            mask[s, j] = 0.0 if (j + s) % 3 == 0 else 1.0
            n += int(k < 4 and mask[s, j] > 0)
            after[s, j] = float(abs(_PLACES[k]) > THRESHOLD and mask[s, j] > 0)
        near.append(n)
    return xi, mask, near, after


def epoch_cases(libs=None):
    """st_freq = 1 events (unconstrained and constrained, plain and reversed entry), st_freq = 2 met and missed by epoch0,
    and one launch that cannot move (w_x = 0, no L1, fresh moments) with coefficients AT the threshold and one float32 step
    to either side: exact in any dtype, and the only way to see whether > is strict."""
    out = []
    S = 2
    for lib in EPOCH_LIBS:
        if libs is not None and lib not in libs:
            continue
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(900 + dp)
        xi, mask, near, after = _placed(S, dp)
        variants = [("xi", "plain", 1, 0), ("xi", "rev3", 1, 5), ("qfc", "plain", 1, 2), ("qfc", "rev1", 1, 0), ("xi", "plain", 2, 1), ("xi", "plain", 2, 2)]
        for form, entry, st_freq, epoch0 in variants:
            cfg = _cfg(lib, "default", entry, form, lr=EPOCH_LR, threshold=THRESHOLD, near_band=NEAR_BAND, st_freq=st_freq, epoch0=epoch0)
            if cfg["q"] is None:
                params = xi.float()
            else:                                            # [beta | const] with reshape(Q beta) + const = the placed Xi: Q is the whole
                const = 0.05 * torch.randn(S, d, generator=gen)              # reflection (r = d p), so beta = Q^T (Xi - const) is no larger than Xi
                rest = xi.clone()
                rest[:, ::p] -= const.double()
                params = torch.cat([(rest @ cfg["q"].double()).float(), const], dim=1).contiguous()
            state = _state(S, params.shape[1], d, p, [9, 0], ["ones", "ones"], False, gen)
            state["params"], state["mask"] = params, mask.clone()
            event = (epoch0 + 1) % st_freq == 0
            expect = dict(near=near if event else [0] * S, mask=after if event else mask, event=event)
            tables = _rows(64, "tail", gen)[None, None, None].contiguous()
            out.append(Case(f"epoch-d{lib[0]}o{lib[1]}f{lib[2]}-{form}-{entry}-st{st_freq}-e{epoch0}", cfg, tables, state, (), expect))
    lib = EPOCH_LIBS[0]
    if libs is None or lib in libs:
        d, (p, dp) = lib[0], lib_dims(lib)
        cfg = _cfg(lib, "no_l1", "plain", "xi", lr=EPOCH_LR, w_x=0.0, threshold=THRESHOLD, near_band=NEAR_BAND, st_freq=1)
        t32 = torch.tensor(THRESHOLD, dtype=torch.float32)
        up, down = torch.nextafter(t32, torch.tensor(1.0)), torch.nextafter(t32, torch.tensor(0.0))
        params = torch.full((1, dp), 0.5)
        params[0, :6] = torch.stack([t32, -t32, up, -up, down, -down])
        state = dict(params=params, m=torch.zeros(1, dp), v=torch.zeros(1, dp), step=torch.zeros(1, dtype=torch.int32), mask=torch.ones(1, dp))
        after = torch.ones(1, dp)
        after[0, [0, 1, 4, 5]] = 0.0
        gen = torch.Generator().manual_seed(77)
        out.append(Case("epoch-at-the-threshold", cfg, _rows(64, "none", gen)[None, None, None].contiguous(), state,
                        ("threshold", "near_hi", "near_lo"), dict(near=[6], mask=after, event=True)))
    return out


def check_epoch(rep, case, dev):
    out, xi, log = check_launch(rep, case, dev)
    e = case.expect
    assert [int(v) for v in log[0, :, 3]] == e["near"] and torch.equal(out["mask"], e["mask"]), (case.name, log[0, :, 3], e["near"])
    assert all(float(v) == float(e["event"]) for v in log[0, :, 5]), (case.name, log[0, :, 5])


# ---------------------------------------------------------------------------------------------------------------------
# structure, bit for bit: one launch of 1 epoch x 2 steps equals two launches of 1 x 1 step
# ---------------------------------------------------------------------------------------------------------------------
STRUCTURE_LIBS = [(2, 5, 0), (3, 3, 1)]


def structure_cases(libs=None):
    """Plain and reversed (n_g = 3) entry x Xi and [beta | const] x batch 64, 257, 513: the twelve combinations dealt out
    over the two libraries (all twelve on one of them where the other is not compiled)."""
    out = []
    combos = [(entry, form, batch) for entry in ("plain", "rev3") for form in ("xi", "q5c") for batch in (64, 257, 513)]
    both = libs is None or all(lib in libs for lib in STRUCTURE_LIBS)
    for k, lib in enumerate(STRUCTURE_LIBS):
        if libs is not None and lib not in libs:
            continue
        d, (p, dp) = lib[0], lib_dims(lib)
        gen = torch.Generator().manual_seed(500 + dp)
        for entry, form, batch in (combos[k::2] if both else combos):
            cfg = _cfg(lib, "weighted", entry, form)
            n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + d
            state = _state(2, n_par, d, p, [0, 9], ["ones", "half"], True, gen)
            tables = torch.stack([torch.stack([_rows(batch, "scattered", gen), _rows(batch, "tail", gen)]) for _ in range(2)])[None]
            out.append(Case(f"structure-d{lib[0]}o{lib[1]}f{lib[2]}-{entry}-{form}-b{batch}", cfg, tables.contiguous(), state, (), None))
    return out


def check_structure(case, dev):
    """params, m, v, step, mask and xi of the 2-step launch against step 0 then step 1 as launches of their own."""
    whole, xi_w, _ = dev.launch(case.tables, case.state, case.cfg)
    a, _, _ = dev.launch(case.tables[:, :, :1].contiguous(), case.state, case.cfg)
    b, xi_b, _ = dev.launch(case.tables[:, :, 1:].contiguous(), a, case.cfg)
    assert same_bits(whole, b) == [] and _bytes_equal(xi_w, xi_b), (case.name, same_bits(whole, b))
    assert whole["step"].tolist() == (case.state["step"] + 2).tolist(), (case.name, whole["step"])


def libs_of(cases):
    return sorted({(c.cfg["d"], c.cfg["order"], c.cfg["flags"]) for c in cases})
