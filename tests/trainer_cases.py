"""The cases of the trainer step tests, and the one driver both sides run them through.

``tests/test_gpu_trainer_steps.py`` plays them on the device, ``tests/test_host_trainer_model.py`` replays them on the CPU
with the float32 model standing where the device stands.  Either way every launch is checked on its own: the fp64 model
(tests/trainer_model.py) is handed the state found before the launch (float32 values) and the closure output that was
handed over, and predicts the state after it -- teacher forcing, no trajectory drift.

A "device" here is anything with ``load(hs)``, ``read() -> hs``, ``put(name, tensor)``, ``update(mode)``,
``epoch_end(epoch)`` and ``logs() -> dict``; ``hs`` is the state block as a dict of CPU tensors in the device's dtypes and
shapes (``field_shapes``).  ``ModelDevice`` is the float32 model behind that interface.
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import sindy_oracle as O
from tests import trainer_model as M

LOG_RING = 8
SENTINEL = -7.0                                      # what the log rows hold before a launch writes them

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances.  Derived, not chosen: tests/test_host_trainer_model.py replays every case below with the model in float32
# against the model in float64 from the same float32 state, takes per field the worst deviation relative to the field's
# largest magnitude in that problem, and asserts that each constant here is 4 x that figure (rounded up to two digits;
# x 4 because the device adds wave sums in butterfly order and fused, the model sequentially).  A field whose replay
# deviation is 0 (copies, resets, counters kept in floats) gets 0: the device has to match it exactly.
# The measured figures, and the worst the MI355X run showed, are in profiles/trainer_steps.txt.
# ---------------------------------------------------------------------------------------------------------------------
STEP_TOL = {
    "params": 3.7e-5, "xi": 4.0e-5, "g": 1.3e-5, "loss": 4.6e-7, "d": 9.2e-5, "t": 1.5e-6, "h_diag": 1.4e-5, "prev_g": 1.3e-5,
    "prev_loss": 4.6e-7, "l1_last": 6.6e-7, "old_dirs": 7.5e-5, "old_stps": 2.3e-7, "ro": 1.7e-5,
}
EPOCH_TOL = {"prev": 0.0, "pprev": 0.0, "h_diag": 0.0, "update_norm": 1.2e-7, "update_norm_2": 2.4e-7}
# A branch is settled for the device when its two sides differ, relatively, by more than the tolerance of the field the
# compared quantity is made of (the curvature y.s is 1 / ro; g.d is judged as d).
MARGIN_FIELD = {"tol_grad": "g", "step_size": "d", "loss_change_hi": "loss", "loss_change_lo": "loss", "curvature": "ro", "descent": "d",
                "tol_update": "update_norm", "tol_update_2": "update_norm_2", "threshold": "xi", "near_hi": "xi", "near_lo": "xi"}


def unsettled(margins, exact=()):
    tol = dict(STEP_TOL, **EPOCH_TOL)
    return [m for m in margins if m[0] not in exact and M.unsettled([m], tol[MARGIN_FIELD[m[0]]])]


# The free-running check: |Xi_fp32 - Xi_fp64| / max |Xi_fp64| of oracle.lbfgs_fit on the CPU (worst epoch and case) x 4.
FREE_RUN_TOL = 3.6e-5

FLOAT_FIELDS = ("params", "xi", "g", "loss", "d", "t", "h_diag", "prev_g", "prev_loss", "l1_last")
INT_FIELDS = ("act", "n_iter", "head", "count", "done")
EPOCH_INT_FIELDS = ("n_iters", "n_iter", "head", "count", "done", "nan", "finished", "epochs", "near")
_DTYPES = {"act": torch.uint8, "n_iter": torch.int64, "head": torch.int64, "count": torch.int64, "n_iters": torch.int32,
           "done": torch.uint8, "nan": torch.uint8, "finished": torch.uint8, "epochs": torch.int32, "near": torch.int32}


def field_shapes(S, n, dp, H):
    v, x = (S, n), (S, dp)
    return {"params": v, "xi": x, "mask": x, "cl_loss": (S, 2), "cl_grad": x, "g": v, "loss": (S,), "act": (S,), "n_iter": (S,),
            "d": v, "t": (S,), "old_dirs": (S, H, n), "old_stps": (S, H, n), "ro": (S, H), "head": (S,), "count": (S,),
            "h_diag": (S,), "prev_g": v, "prev_loss": (S,), "prev": v, "pprev": v, "n_iters": (S,), "done": (S,), "nan": (S,),
            "finished": (S,), "epochs": (S,), "near": (S,), "l1_last": (S,), "test_grad": x}


def blank_state(S, n, dp, H):
    """What symode_trainer_init leaves, before parameters and mask: zeros, h_diag = 1."""
    hs = {k: torch.zeros(shape, dtype=_DTYPES.get(k, torch.float32)) for k, shape in field_shapes(S, n, dp, H).items()}
    hs["h_diag"].fill_(1.0)
    return hs


def lib_terms(d, order, flags):
    return O.term_count(d, order, bool(flags & 1), bool(flags & 2))


def householder_q(dp, r):
    """(dp, r) float32 with orthonormal columns (dp < r: orthonormal rows), dense, made without a factorisation so that
    every machine gets the same bits: the first columns of the reflection I - 2 v v^T / |v|^2."""
    m = max(dp, r)
    v = torch.cos(torch.arange(1, m + 1, dtype=torch.float64) * 0.7) + 0.3
    Hm = torch.eye(m, dtype=torch.float64) - 2.0 * torch.outer(v, v) / float((v * v).sum())
    return Hm[:dp, :r].to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic closure
# ---------------------------------------------------------------------------------------------------------------------
class Quadratic:
    """Per problem two convex quadratics in z = Xi * mask: f_k(z) = 0.5 (z - c_k)^T A_k (z - c_k), A_k = 0.5 I + B_k^T B_k / 8,
    evaluated in fp64 and rounded to float32; the gradient handed over is mask * d(f_0 + w_pair f_1)/dz (f_0's alone
    without ``pair``), so masked entries are exactly 0."""

    def __init__(self, S, dp, seed, pair, w_pair):
        g = torch.Generator().manual_seed(seed)
        self.B = torch.randn(2, S, 8, dp, generator=g, dtype=torch.float64)
        self.c = 0.5 * torch.randn(2, S, dp, generator=g, dtype=torch.float64)
        self.pair, self.w_pair, self.S = pair, M.f32(w_pair), S

    def half(self, k, z):
        e = z - self.c[k]
        Ae = 0.5 * e + torch.einsum("skj,sk->sj", self.B[k], torch.einsum("skj,sj->sk", self.B[k], e)) / 8.0
        return 0.5 * (e * Ae).sum(1), Ae

    def __call__(self, xi, mask):
        """xi, mask (S, dp) in any dtype -> (loss (S, 2) fp64, grad (S, dp) fp64)"""
        m = mask.reshape(self.S, -1).double()
        z = xi.reshape(self.S, -1).double() * m
        f0, g0 = self.half(0, z)
        f1, g1 = self.half(1, z)
        grad = g0 + self.w_pair * g1 if self.pair else g0
        return torch.stack([f0, f1], 1), grad * m


def put_closure(dev, loss2, grad, pair):
    """Hand a closure result over as the closure kernels do: (S, 2) = (mse, regulariser) with the pair; the mse alone in the
    FIRST S floats of the block without it (the rest is then not the kernels' to read: it gets decoys)."""
    S = loss2.shape[0]
    cl = loss2.to(torch.float32).clone()
    if not pair:
        flat = 1000.0 + torch.arange(2 * S, dtype=torch.float32)
        flat[:S] = loss2[:, 0].to(torch.float32)
        cl = flat.view(S, 2)
    dev.put("cl_loss", cl)
    dev.put("cl_grad", grad.to(torch.float32))


def closure_of(hs, s, pair):
    """(mse, regulariser) of problem s as handed over, and its gradient."""
    S = hs["cl_loss"].shape[0]
    cl = hs["cl_loss"][s] if pair else torch.stack([hs["cl_loss"].reshape(-1)[s], torch.zeros(())])
    assert S == hs["cl_grad"].shape[0]
    return cl, hs["cl_grad"][s]


# ---------------------------------------------------------------------------------------------------------------------
# state block <-> the model's state of one problem
# ---------------------------------------------------------------------------------------------------------------------
def problem_state(hs, s, dt, cfg):
    st = {k: hs[k][s].reshape(-1).to(dt) for k in ("params", "mask", "g", "d", "prev_g", "prev", "pprev")}
    st["xi"] = st["params"].clone() if cfg["map"] is None else hs["xi"][s].reshape(-1).to(dt)
    for k in ("loss", "t", "h_diag", "prev_loss", "l1_last"):
        st[k] = hs[k][s].to(dt)
    for k in ("act", "n_iter", "head", "done", "n_iters", "nan", "finished", "epochs", "near"):
        st[k] = int(hs[k][s])
    st["pairs"] = M.pairs_from_ring(hs["old_dirs"][s].to(dt), hs["old_stps"][s].to(dt), hs["ro"][s].to(dt), st["head"], int(hs["count"][s]))
    return st


def _counted(st):
    """The device's ``count`` of a model state: the pairs it holds."""
    st["count"] = len(st["pairs"])
    return st


def store_problem(hs, s, st, cfg):
    """The model's state into the block, as float32 (ModelDevice)."""
    for k in ("params", "mask", "g", "d", "prev_g", "prev", "pprev", "loss", "t", "h_diag", "prev_loss", "l1_last"):
        hs[k][s] = st[k].to(torch.float32).reshape(hs[k][s].shape)
    if cfg["map"] is not None:
        hs["xi"][s] = st["xi"].to(torch.float32)
    for k in ("act", "n_iter", "done", "n_iters", "nan", "finished", "epochs", "near"):
        hs[k][s] = st[k]
    f = [(y.float(), v.float(), r.float()) for y, v, r in st["pairs"]]
    hs["head"][s], hs["count"][s] = M.pairs_to_ring(f, st["head"], hs["old_dirs"][s], hs["old_stps"][s], hs["ro"][s])


class ModelDevice:
    """The float32 model standing where the device stands."""

    def __init__(self, S, n, dp, H, cfg, pair):
        self.cfg, self.pair, self.S, self.dims = cfg, pair, S, (S, n, dp, H)
        self.hs = blank_state(S, n, dp, H)
        self.log = torch.full((LOG_RING, S, 8), SENTINEL)
        self.log_xi, self.log_mask = torch.full((LOG_RING, S, dp), SENTINEL), torch.full((LOG_RING, S, dp), SENTINEL)
        self.log_params = torch.full((LOG_RING, S, n), SENTINEL)

    def load(self, hs):
        self.hs = {k: v.clone() for k, v in hs.items()}
        if self.cfg["map"] is None:
            self.hs["xi"] = self.hs["params"].clone()

    def read(self):
        if self.cfg["map"] is None:
            self.hs["xi"] = self.hs["params"].clone()
        return {k: v.clone() for k, v in self.hs.items()}

    def put(self, name, tensor):
        self.hs[name] = tensor.to(self.hs[name].dtype).reshape(self.hs[name].shape).clone()

    def update(self, mode):
        hs = self.read()
        for s in range(self.S):
            cl, gr = closure_of(hs, s, self.pair)
            st, _ = M.update(problem_state(hs, s, torch.float32, self.cfg), cl, gr, self.cfg, mode)
            store_problem(self.hs, s, st, self.cfg)

    def epoch_end(self, epoch):
        hs, slot = self.read(), epoch % LOG_RING
        for s in range(self.S):
            cl, _ = closure_of(hs, s, self.pair)
            st, rec, _ = M.epoch_end(problem_state(hs, s, torch.float32, self.cfg), cl, self.cfg, epoch)
            store_problem(self.hs, s, st, self.cfg)
            self.log[slot, s, 0], self.log[slot, s, 7] = rec["code"], epoch
            if rec["code"] != M.EVENT_IDLE:
                self.log[slot, s, 1:7] = torch.tensor([rec[k] for k in ("mse", "sym", "l1", "update_norm", "update_norm_2", "near")])
                self.log_xi[slot, s], self.log_mask[slot, s], self.log_params[slot, s] = rec["xi"].float(), rec["mask"].float(), rec["params"].float()

    def logs(self):
        return {k: getattr(self, k).clone() for k in ("log", "log_xi", "log_mask", "log_params")}


# ---------------------------------------------------------------------------------------------------------------------
# comparing one launch with the fp64 model
# ---------------------------------------------------------------------------------------------------------------------
def _dev(got, want):
    """max |got - want| / max |want| over the finite entries; the NaN patterns have to be the same."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    if not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    ok = ~torch.isnan(want)
    if not bool(ok.any()):
        return 0.0
    if not torch.equal(torch.isinf(got[ok]), torch.isinf(want[ok])):
        return float("inf")
    ok = ok & ~torch.isinf(want)
    if not bool(ok.any()):
        return 0.0
    return float((got[ok] - want[ok]).abs().max()) / max(float(want[ok].abs().max()), M.TINY)


def _bytes_equal(a, b):
    return torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


class Report:
    """What a run of cases showed: worst deviation per field, discrete mismatches, unsettled margins, launches checked."""

    def __init__(self):
        self.worst, self.mismatch, self.unsettled, self.launches, self.events = {}, [], [], 0, []

    def dev(self, field, value, where):
        if value > self.worst.get(field, (-1.0, None))[0]:
            self.worst[field] = (value, where)

    def over(self, tol):
        return {k: v for k, v in self.worst.items() if k in tol and not v[0] <= tol[k]}


def check_update(rep, where, cfg, pair, hs0, hs1, mode, exact=()):
    """One update launch: ``hs0`` the block before it (closure output included), ``hs1`` after it."""
    S = hs0["params"].shape[0]
    outcomes = []
    for s in range(S):
        cl, gr = closure_of(hs0, s, pair)
        st0 = problem_state(hs0, s, torch.float64, cfg)
        st, mg = M.update(st0, cl, gr, cfg, mode)
        st = _counted(st)
        rep.launches += 1
        rep.unsettled += [(where, s) + m for m in unsettled(mg, exact)]
        got = _counted(problem_state(hs1, s, torch.float64, cfg))
        for k in INT_FIELDS:
            if got[k] != st[k]:
                rep.mismatch.append((where, s, k, got[k], st[k]))
        for k in FLOAT_FIELDS:
            rep.dev(k, _dev(got[k], st[k]), (where, s))
        touched = st["n_iter"] != st0["n_iter"]              # the launch went into an iteration
        if touched:
            if len(got["pairs"]) == len(st["pairs"]):
                for (y, v, r), (wy, wv, wr) in zip(got["pairs"], st["pairs"]):
                    rep.dev("old_dirs", _dev(y, wy), (where, s))
                    rep.dev("old_stps", _dev(v, wv), (where, s))
                    rep.dev("ro", _dev(r, wr), (where, s))
        # bytes of what the model leaves untouched
        fresh = any(m[0] == "curvature" and m[1] > m[2] for m in mg)       # a pair was stored: one ring slot is the launch's
        H = hs0["ro"].shape[1]
        slot = (st["head"] + len(st["pairs"]) - 1) % H if fresh else -1
        for k in ("old_dirs", "old_stps", "ro"):
            keep = [j for j in range(H) if j != slot]
            if not _bytes_equal(hs0[k][s][keep], hs1[k][s][keep]):
                rep.mismatch.append((where, s, k, "a slot the launch does not own changed", slot))
        for k in hs0:
            if k in ("old_dirs", "old_stps", "ro", "xi") or k in INT_FIELDS or k == "count":
                continue
            same = (k not in st) or (torch.is_tensor(st[k]) and torch.equal(st[k], st0[k]) and not torch.isnan(st[k]).any()) \
                or (not torch.is_tensor(st[k]) and st[k] == st0[k])
            if k in ("t", "h_diag") and touched:
                continue                                     # rewritten by every iteration, possibly with the same value
            if same and not _bytes_equal(hs0[k][s], hs1[k][s]):
                rep.mismatch.append((where, s, k, "changed although the model leaves it", None))
        outcomes.append((st["act"], st["n_iter"], len(st["pairs"])))
    return outcomes


def check_epoch(rep, where, cfg, pair, hs0, hs1, logs0, logs1, epoch, exact=()):
    """One epoch launch; ``logs*``: the record arrays before and after it."""
    S, slot = hs0["params"].shape[0], epoch % LOG_RING
    codes = []
    for s in range(S):
        cl, _ = closure_of(hs0, s, pair)
        st0 = problem_state(hs0, s, torch.float64, cfg)
        st, rec, mg = M.epoch_end(st0, cl, cfg, epoch)
        st = _counted(st)
        rep.launches += 1
        rep.unsettled += [(where, s) + m for m in unsettled(mg, exact)]
        got = _counted(problem_state(hs1, s, torch.float64, cfg))
        row = logs1["log"][slot, s]
        codes.append(rec["code"])
        if int(row[0]) != rec["code"] or float(row[0]) != float(rec["code"]):
            rep.mismatch.append((where, s, "code", float(row[0]), rec["code"]))
        if float(row[7]) != float(epoch):
            rep.mismatch.append((where, s, "record epoch", float(row[7]), epoch))
        for k in EPOCH_INT_FIELDS:
            if got[k] != st[k]:
                rep.mismatch.append((where, s, k, got[k], st[k]))
        if not torch.equal(got["mask"], st["mask"]):
            rep.mismatch.append((where, s, "mask", got["mask"].tolist(), st["mask"].tolist()))
        for k in ("prev", "pprev", "h_diag"):
            rep.dev(k, _dev(got[k], st[k]), (where, s))
        if rec["code"] == M.EVENT_IDLE:                      # (-1, untouched ..., epoch), no detail rows, no state byte changed
            if not _bytes_equal(row[1:7], logs0["log"][slot, s, 1:7]):
                rep.mismatch.append((where, s, "idle record", row.tolist(), None))
            for k in ("log_xi", "log_mask", "log_params"):
                if not _bytes_equal(logs0[k][slot, s], logs1[k][slot, s]):
                    rep.mismatch.append((where, s, k, "idle problem's row written", None))
            for k in hs0:
                if not _bytes_equal(hs0[k][s], hs1[k][s]):
                    rep.mismatch.append((where, s, k, "idle problem's state changed", None))
            continue
        want_row = {1: rec["mse"], 2: rec["sym"], 3: rec["l1"], 6: float(rec["near"])}
        for col, v in want_row.items():                      # copies of float32 inputs and a count: exact
            if float(row[col]) != float(torch.tensor(v, dtype=torch.float32)):
                rep.mismatch.append((where, s, f"record column {col}", float(row[col]), v))
        rep.dev("update_norm", _dev(row[4], torch.tensor(rec["update_norm"], dtype=torch.float64)), (where, s))
        rep.dev("update_norm_2", _dev(row[5], torch.tensor(rec["update_norm_2"], dtype=torch.float64)), (where, s))
        for k in ("xi", "mask", "params"):                   # the rows are copies of the state after the event
            want = got[k].to(torch.float32)
            if not _bytes_equal(logs1["log_" + k][slot, s], want) and not (torch.isnan(want).any() and _dev(logs1["log_" + k][slot, s], want) == 0.0):
                rep.mismatch.append((where, s, "log_" + k, None, None))
        if not _bytes_equal(got["xi"].float(), st0["xi"].float()) and not torch.isnan(st0["xi"]).any():
            rep.mismatch.append((where, s, "xi", "the epoch launch does not write Xi", None))
        for k in ("g", "loss", "d", "t", "prev_g", "prev_loss", "l1_last", "old_dirs", "old_stps", "ro", "cl_loss", "cl_grad", "act", "test_grad", "params"):
            if not _bytes_equal(hs0[k][s], hs1[k][s]):
                rep.mismatch.append((where, s, k, "changed although the epoch logic leaves it", None))
    for k in ("log", "log_xi", "log_mask", "log_params"):    # the other slots of the ring
        keep = [j for j in range(LOG_RING) if j != slot]
        if not _bytes_equal(logs0[k][keep], logs1[k][keep]):
            rep.mismatch.append((where, -1, k, "a slot of another epoch changed", None))
    rep.events.append((where, codes))
    return codes


# ---------------------------------------------------------------------------------------------------------------------
# the update cases
# ---------------------------------------------------------------------------------------------------------------------
UPDATE_LIBS = [(1, 3, 0), (2, 3, 0), (2, 5, 0), (3, 3, 3), (3, 4, 0), (4, 3, 0), (4, 3, 3)]
S_UPDATE, MAX_ITER = 3, 4


def update_cases(libs=UPDATE_LIBS):
    """(d, order, flags, map kind, history, l1, pair): maps none / q5c (r = 5, constants) / q5 (r = 5, constants not read) /
    q100c (r = 100, constants; dp >= 105); history 3 and 100; l1 and pair each on half of the cases, crossing under the map."""
    out, k = [], 0
    for d, order, flags in libs:
        dp = d * lib_terms(d, order, flags)
        for kind in ["none", "q5c", "q5"] + (["q100c"] if dp >= 105 else []):
            for history in (3, 100):
                out.append((d, order, flags, kind, history, bool(k & 1), bool((k >> 1) & 1)))
                k += 1
    return out


def case_id(case):
    d, order, flags, kind, history, l1, pair = case
    return f"d{d}o{order}f{flags}-{kind}-H{history}" + ("-l1" if l1 else "") + ("-pair" if pair else "")


Setup = namedtuple("Setup", "cfg Q allow_const n dp p closure P0 mask0")      # Q (dp, r) or None; P0 (S, n), mask0 (S, dp)


def case_setup(case, lr=0.5):
    """The Setup of an update case."""
    d, order, flags, kind, history, l1, pair = case
    p = lib_terms(d, order, flags)
    dp = d * p
    seed = 1000 * d + 100 * order + 10 * flags + history + {"none": 0, "q5c": 1, "q5": 2, "q100c": 3}[kind]
    Q, allow_const, mp = None, True, None
    if kind != "none":
        r = 100 if kind == "q100c" else 5
        Q, allow_const = householder_q(dp, r), kind != "q5"
        mp = (Q.double(), r, p, allow_const)
    n = dp if Q is None else Q.shape[1] + d
    cfg = M.make_cfg(lr=lr, history=history, w_x=2.0 if l1 else 1.0, w_reg=1e-3 if l1 else 0.0, l1=l1, pair=pair,
                     w_pair=0.37 if pair else 0.0, map=mp, d=d)
    g = torch.Generator().manual_seed(seed)
    P0 = 0.5 * torch.randn(S_UPDATE, n, generator=g)
    mask0 = (torch.rand(S_UPDATE, dp, generator=g) > 0.2).float()
    return Setup(cfg, Q, allow_const, n, dp, p, Quadratic(S_UPDATE, dp, seed + 7, pair, cfg["w_pair"]), P0, mask0)


def start_state(cfg, n, dp, H, P0, mask0):
    hs = blank_state(P0.shape[0], n, dp, H)
    hs["params"], hs["prev"], hs["pprev"], hs["mask"] = P0.clone(), P0.clone(), P0.clone(), mask0.clone()
    hs["xi"] = torch.stack([M.xi_of(P0[s].double(), cfg).float() for s in range(P0.shape[0])])
    return hs


def drive_update_case(case, dev, rep, setup=None):
    """Two epochs of BEGIN, ACCEPT x 3 with the closure played by hand; between them problems 0 and 1 get the reset an epoch
    event makes (n_iter, head, count = 0, h_diag = 1; the pairs stay in the ring, stale) and problem 2 carries on."""
    su = setup or case_setup(case)
    cfg, closure, pair = su.cfg, su.closure, su.cfg["pair"]
    for epoch in range(2):
        for it in range(MAX_ITER):
            hs = dev.read()
            put_closure(dev, *closure(hs["xi"], hs["mask"]), pair)
            hs0 = dev.read()
            mode = M.BEGIN if it == 0 else M.ACCEPT
            dev.update(mode)
            check_update(rep, (case_id(case), epoch, it), cfg, pair, hs0, dev.read(), mode)
        if epoch == 0:
            hs = dev.read()
            for k, v in (("n_iter", 0), ("head", 0), ("count", 0), ("h_diag", 1.0)):
                hs[k][:2] = v
                dev.put(k, hs[k])


# ---------------------------------------------------------------------------------------------------------------------
# crafted single update launches (library (2, 3, 0): dp = 20, no map unless said)
# ---------------------------------------------------------------------------------------------------------------------
def _mid_run_state(cfg, n, dp, H, S, seed, map_q=None):
    """A state two iterations into a step: one stored pair, prev_g / d / t / prev_loss of the last move; all exact float32."""
    g = torch.Generator().manual_seed(seed)
    hs = blank_state(S, n, dp, H)
    hs["params"] = 0.5 * torch.randn(S, n, generator=g)
    hs["mask"] = torch.ones(S, dp)
    hs["xi"] = torch.stack([M.xi_of(hs["params"][s].double(), cfg).float() for s in range(S)])
    hs["prev"], hs["pprev"] = hs["params"].clone(), hs["params"].clone()
    hs["d"], hs["prev_g"] = -0.3 * torch.randn(S, n, generator=g), torch.randn(S, n, generator=g)
    hs["g"] = hs["prev_g"].clone()
    hs["t"].fill_(cfg["lr"])
    hs["act"].fill_(1)
    hs["n_iter"].fill_(2)
    hs["count"].fill_(1)
    hs["old_stps"][:, 0] = 0.1 * torch.randn(S, n, generator=g)
    hs["old_dirs"][:, 0] = 2.0 * hs["old_stps"][:, 0] + 0.05 * torch.randn(S, n, generator=g)
    hs["ro"][:, 0] = 1.0 / (hs["old_dirs"][:, 0].double() * hs["old_stps"][:, 0].double()).sum(1).float()
    hs["h_diag"].fill_(0.7)
    hs["loss"].fill_(3.0)
    hs["prev_loss"].fill_(3.0)
    hs["l1_last"].fill_(5.0)
    return hs, g


# one crafted launch sequence: the state ``hs``, the closure output handed over, the modes launched in turn, the margin names
# that are exact by construction, and (act, n_iter, pairs) per problem expected after the first launch
Crafted = namedtuple("Crafted", "name cfg pair hs cl_loss cl_grad modes exact expect")


def crafted_cases():
    """The Crafted launches (library (2, 3, 0))."""
    n = dp = 20
    H, out = 3, []
    cfg = M.make_cfg(lr=0.5, history=H, d=2)
    tg = cfg["tol_grad"]
    up = float(np.nextafter(np.float32(tg), np.float32(1.0)))

    # the gradient maximum equal to tol_grad (stops), one ulp above (goes on), and all zero (stops): BEGIN
    hs = start_state(cfg, n, dp, H, 0.5 * torch.randn(3, n, generator=torch.Generator().manual_seed(1)), torch.ones(3, dp))
    gr = torch.zeros(3, dp)
    gr[0, 3], gr[0, 11], gr[1, 3], gr[1, 11] = tg, -0.5 * tg, -up, 0.5 * tg
    out.append(Crafted("tol_grad edge and zero gradient", cfg, False, hs, torch.tensor([[1.0, 0.0]] * 3), gr, [M.BEGIN], ("tol_grad",),
                [(0, 0, 0), (0, 1, 0), (0, 0, 0)]))        # (problem 1 enters the iteration; g.d = -|g|^2 > -tol_change ends it there)

    # ys <= 1e-10: y = 0 exactly (problem 0), negative curvature (problem 1); problem 2 stores a pair.  ACCEPT
    hs, g = _mid_run_state(cfg, n, dp, H, 3, seed=2)
    gr = hs["prev_g"].clone()
    gr[1] = hs["prev_g"][1] - 0.5 * hs["d"][1]
    gr[2] = hs["prev_g"][2] + 0.5 * hs["d"][2]
    out.append(Crafted("curvature guard", cfg, False, hs, torch.tensor([[2.0, 0.0]] * 3), gr, [M.ACCEPT], (), [(1, 3, 1), (1, 3, 1), (1, 3, 2)]))

    # |loss - prev_loss| one ulp below tol_change (stops), equal to it and one ulp above (go on): ACCEPT, exact in float32
    cfg2 = M.make_cfg(lr=0.5, history=H, d=2, tol_change=2.0 ** -20)
    hs, g = _mid_run_state(cfg2, n, dp, H, 3, seed=3)
    hs["prev_loss"].fill_(1.0)
    gr = hs["prev_g"] + 0.5 * hs["d"]
    cl = torch.tensor([[1.0 + 7 * 2.0 ** -23, 0.0], [1.0 + 8 * 2.0 ** -23, 0.0], [1.0 + 9 * 2.0 ** -23, 0.0]])
    out.append(Crafted("loss change edge", cfg2, False, hs, cl, gr, [M.ACCEPT], ("loss_change_hi", "loss_change_lo"), [(0, 2, 1), (1, 3, 2), (1, 3, 2)]))

    # a NaN gradient entry: BEGIN (no stop, the parameter goes to NaN), ACCEPT (no pair from a NaN curvature, everything NaN)
    hs = start_state(cfg, n, dp, H, 0.5 * torch.randn(2, n, generator=torch.Generator().manual_seed(4)), torch.ones(2, dp))
    gr = torch.randn(2, dp, generator=torch.Generator().manual_seed(5))
    gr[0, 7] = float("nan")
    out.append(Crafted("NaN gradient at BEGIN", cfg, False, hs, torch.tensor([[1.0, 0.0]] * 2), gr, [M.BEGIN], (), [(1, 1, 0), (1, 1, 0)]))
    hs, g = _mid_run_state(cfg, n, dp, H, 2, seed=6)
    gr = hs["prev_g"] + 0.5 * hs["d"]
    gr[0, 13] = float("nan")
    out.append(Crafted("NaN gradient at ACCEPT", cfg, False, hs, torch.tensor([[2.0, 0.0]] * 2), gr, [M.ACCEPT], (), [(1, 3, 1), (1, 3, 2)]))

    # done = 1 at BEGIN: act becomes 0 and nothing else changes; the following ACCEPT changes nothing.  Problem 1 is not done.
    hs, g = _mid_run_state(cfg, n, dp, H, 2, seed=7)
    hs["done"][0] = 1
    gr = hs["prev_g"] + 0.5 * hs["d"]
    # (problem 1's ACCEPT sees the same closure value again: loss == prev_loss exactly, it stops there)
    out.append(Crafted("done at BEGIN", cfg, False, hs, torch.tensor([[2.0, 0.0]] * 2), gr, [M.BEGIN, M.ACCEPT], ("loss_change_hi", "loss_change_lo"),
                [(0, 2, 1), (1, 3, 2)]))

    # n_iter = 0 with stale pairs, head and count: the first-iteration step length and an empty memory.  Under the map too.
    for mp_kind in ("none", "q5c"):
        Q = None if mp_kind == "none" else householder_q(dp, 5)
        cfg3 = M.make_cfg(lr=0.5, history=H, d=2, map=None if Q is None else (Q.double(), 5, 10, True))
        n3 = dp if Q is None else 7
        hs, g = _mid_run_state(cfg3, n3, dp, H, 2, seed=8)
        hs["n_iter"].fill_(0)
        hs["head"].fill_(2)
        hs["count"].fill_(3)
        hs["old_dirs"], hs["old_stps"] = torch.randn(2, H, n3, generator=g), torch.randn(2, H, n3, generator=g)
        hs["ro"] = torch.randn(2, H, generator=g)
        gr = torch.randn(2, dp, generator=g)
        gr[1] *= 0.01                                        # sum |g| < 1: the step length is capped at lr
        out.append(Crafted(f"stale memory at n_iter 0 ({mp_kind})", cfg3, False, hs, torch.tensor([[2.0, 0.0]] * 2), gr, [M.BEGIN], (),
                    [(1, 1, 0), (1, 1, 0)]))

    # a parameter exactly 0 (and -0) under l1: sign(0) = 0.  BEGIN and a following ACCEPT, pair on.
    cfg4 = M.make_cfg(lr=0.5, history=H, d=2, w_x=2.0, w_reg=1e-3, l1=True, pair=True, w_pair=0.37)
    P0 = 0.5 * torch.randn(2, n, generator=torch.Generator().manual_seed(9))
    P0[0, 0], P0[0, 5], P0[1, 19] = 0.0, -0.0, 0.0
    hs = start_state(cfg4, n, dp, H, P0, torch.ones(2, dp))
    gr = torch.randn(2, dp, generator=torch.Generator().manual_seed(10))
    gr[0, 0] = gr[0, 5] = gr[1, 19] = 0.0                    # so that the zero parameters stay where they are
    out.append(Crafted("zero parameter under l1", cfg4, True, hs, torch.tensor([[2.0, 0.5]] * 2), gr, [M.BEGIN], (), [(1, 1, 0), (1, 1, 0)]))
    return out


def drive_crafted(crafted, dev, rep):
    name, cfg, pair, hs, cl, gr, modes, exact, expect = crafted
    dev.load(hs)
    put_closure(dev, cl.double(), gr.double(), pair)
    outcomes = None
    for k, mode in enumerate(modes):
        hs0 = dev.read()
        dev.update(mode)
        got = check_update(rep, (name, k), cfg, pair, hs0, dev.read(), mode, exact)
        outcomes = outcomes or got
    return outcomes


# ---------------------------------------------------------------------------------------------------------------------
# the epoch cases: the state written by hand, one problem per event
# ---------------------------------------------------------------------------------------------------------------------
EPOCH_LIBS = [(1, 3, 0), (2, 3, 0), (3, 4, 0), (4, 3, 0)]              # n = d p = 4, 20, 105, 140 without the map
S_EPOCH, ST_FREQ, TOL_UPDATE, THRESHOLD = 6, 5, 1e-3, 0.1
WANT_CODES = [M.EVENT_CONV, M.EVENT_FINAL, M.EVENT_FREQ, M.EVENT_NONE, M.EVENT_NAN, M.EVENT_IDLE]


def epoch_cases(libs=EPOCH_LIBS):
    """(d, order, flags, mapped, pair, epoch)"""
    return [(d, o, f, mapped, pair, epoch) for d, o, f in libs for mapped in (False, True)
            for pair, epoch in ((False, 1), (True, LOG_RING + 3))]


def epoch_setup(case):
    """(cfg, Q, n, dp, hs, cl_loss (S, 2)) -- problems: 0 conv without final, 1 final, 2 period hit, 3 period miss, 4 NaN, 5 done.
    Under the map |delta beta| = |delta const| = 0.6 tol where a tensor has to look moved: sqrt(a + b) = 0.85 tol < tol <
    1.2 tol = sqrt(a) + sqrt(b), so only the sum of the per-tensor norms gives the event wanted."""
    d, order, flags, mapped, pair, epoch = case
    p = lib_terms(d, order, flags)
    dp, S, H = d * p, S_EPOCH, 3
    Q = householder_q(dp, 5) if mapped else None
    n = 5 + d if mapped else dp
    cfg = M.make_cfg(history=H, pair=pair, w_pair=0.37 if pair else 0.0, map=None if Q is None else (Q.double(), 5, p, True),
                     threshold=THRESHOLD, tol_update=TOL_UPDATE, st_freq=ST_FREQ, d=d)
    thr, band, tol = cfg["threshold"], cfg["near_band"], cfg["tol_update"]
    g = torch.Generator().manual_seed(17 * dp + (3 if mapped else 0) + (1 if pair else 0))
    hs, _ = _mid_run_state(cfg, n, dp, H, S, seed=11 + dp)
    hs["n_iter"] = torch.tensor([3, 4, 5, 6, 7, 8])
    hs["head"], hs["count"] = torch.tensor([1, 2, 0, 1, 2, 0]), torch.tensor([3, 2, 1, 3, 2, 1])
    hs["near"] = torch.tensor([3, 4, 5, 6, 7, 8], dtype=torch.int32)
    hs["epochs"].fill_(epoch)
    hs["n_iters"] = torch.tensor([2, 3, ST_FREQ - 1, ST_FREQ - 2, 1, 9], dtype=torch.int32)
    # coefficients: magnitudes far from the threshold and its band (|.| in [0.15, 0.6] or [0.01, 0.08]), then the edge values
    sgn = torch.where(torch.rand(S, dp, generator=g) < 0.5, -1.0, 1.0)
    big = torch.rand(S, dp, generator=g) < 0.5
    xi = sgn * torch.where(big, 0.15 + 0.45 * torch.rand(S, dp, generator=g), 0.01 + 0.07 * torch.rand(S, dp, generator=g))
    mask = (torch.rand(S, dp, generator=g) > 0.25).float()
    t32 = np.float32(thr)
    special = [(float(t32), 1.0), (float(np.nextafter(t32, np.float32(1))), 1.0), (-float(np.nextafter(t32, np.float32(0))), 1.0),
               (float(np.float32(thr + 0.5 * band)), 0.0), (-float(np.float32(thr - 0.5 * band)), 1.0), (0.5, 0.0)]
    for s in range(S):
        for k in range(min(len(special), dp)):
            v, m = special[(k + s) % len(special)]
            j = (k * max(dp // len(special), 1) + s) % dp if dp >= len(special) else k
            xi[s, j], mask[s, j] = v, m
    hs["mask"] = mask
    if mapped:
        hs["xi"] = xi
        hs["params"] = 0.5 * torch.randn(S, n, generator=g)
    else:
        hs["params"] = xi.clone()
        hs["xi"] = xi.clone()
    P = hs["params"]

    def moved(by_beta, by_const):
        q = P.clone()
        q[:, 0] += by_beta
        q[:, n - 1] += by_const
        if n > 64:                                           # the lanes' second component moves as well
            q[:, 70] += by_beta
        return q
    far, near_ = moved(0.3, 0.2), moved(0.05 * tol, 0.05 * tol if mapped else 0.0)
    split = moved(0.6 * tol, 0.6 * tol) if mapped else moved(1.2 * tol, 0.0)
    hs["prev"], hs["pprev"] = far.clone(), far.clone()
    hs["prev"][0], hs["pprev"][0] = near_[0], split[0]        # conv, not final (merged norms would call it final)
    hs["prev"][1], hs["pprev"][1] = near_[1], near_[1]        # final
    hs["prev"][2], hs["prev"][3] = split[2], split[3]         # not converged (merged norms would call it converged)
    hs["params"][4, n - 1 if n <= 64 else 66] = float("nan")
    if not mapped:
        hs["xi"] = hs["params"].clone()
    hs["done"][5], hs["finished"][5] = 1, 1
    cl = torch.rand(S, 2, generator=g) + 0.5
    return cfg, Q, n, dp, hs, cl


def drive_epoch_case(case, dev, rep):
    cfg, Q, n, dp, hs, cl = epoch_setup(case)
    pair, epoch = case[4], case[5]
    dev.load(hs)
    put_closure(dev, cl.double(), torch.zeros(S_EPOCH, dp, dtype=torch.float64), pair)
    hs0, logs0 = dev.read(), dev.logs()
    dev.epoch_end(epoch)
    exact = ("threshold", "near_hi", "near_lo")              # float32 inputs against float32 constants; |xi| - thr is exact near thr
    return check_epoch(rep, ("epoch",) + tuple(case), cfg, pair, hs0, dev.read(), logs0, dev.logs(), epoch, exact)


# ---------------------------------------------------------------------------------------------------------------------
# the free-running check for the large libraries: oracle.lbfgs_fit on the same data
# ---------------------------------------------------------------------------------------------------------------------
FREE_RUN_CASES = [(3, 4, 0, True), (4, 3, 0, False)]                    # (d, order, flags, mapped: Q with r = 5 and constants)
FREE_RUN_EPOCHS, FREE_RUN_POINTS, FREE_RUN_LR, FREE_RUN_TOL_UPDATE = 3, 257, 0.2, 1e-6


def free_run_data(case):
    """x, dx (257, d), Q (dp, 5) or None, P0 (n,): float32, so that oracle and device start from the same numbers."""
    d, order, flags, mapped = case
    p = lib_terms(d, order, flags)
    g = torch.Generator().manual_seed(100 * d + order)
    x = 0.6 * torch.randn(FREE_RUN_POINTS, d, generator=g)
    truth = torch.randn(d, p, generator=g) * (torch.rand(d, p, generator=g) < 0.3)
    dx = (O.theta(x.double(), order) @ truth.double().T).float() + 0.05 * torch.randn(FREE_RUN_POINTS, d, generator=g)
    Q = householder_q(d * p, 5) if mapped else None
    P0 = 0.3 * torch.randn(5 + d if mapped else d * p, generator=g)
    return x, dx, Q, P0


def free_run_oracle(case, dt):
    """oracle.lbfgs_fit in ``dt`` over FREE_RUN_EPOCHS epochs of max_iter = 4, history 3, no periodic thresholding."""
    d, order, flags, mapped = case
    x, dx, Q, P0 = free_run_data(case)
    reg = O.OracleRegressor(d, order, bool(flags & 1), bool(flags & 2), Xi0=torch.zeros(d, lib_terms(d, order, flags)))
    reg.mask = reg.mask.to(dt)
    if mapped:
        reg.constraint, reg.Q, reg.use_kron_product, reg.allow_constant = True, Q.to(dt), True, True
        reg.beta = P0[:5].to(dt).clone().requires_grad_(True)
        reg.const = P0[5:].to(dt).reshape(d, 1).clone().requires_grad_(True)
        reg.Xi = None
    else:
        reg.Xi = P0.to(dt).reshape(d, -1).clone().requires_grad_(True)
    return O.lbfgs_fit(reg, x.to(dt), dx.to(dt), FREE_RUN_EPOCHS, FREE_RUN_LR, sindy_reg_type="none", st_freq=0, tol=FREE_RUN_TOL_UPDATE,
                       max_iter=4, history_size=3)
