"""One launch of the device L-BFGS trainer as plain torch, for ONE problem, in the dtype of the state it is handed.

``update`` is one optimiser launch (``symode_trainer_update``): torch.optim.LBFGS.step without line search, cut where the
device cuts it -- BEGIN is the top of ``step()`` (take the closure's value, optimality test) followed by one iteration of its
loop up to the move; ACCEPT is the bottom of that loop (take the re-evaluated value, the three stopping tests) followed by
the next iteration up to the move.  ``epoch_end`` is one epoch launch (``symode_trainer_epoch_end``): the statements of
``oracle.sindy_oracle.lbfgs_fit`` after ``opt.step`` (train.py:694-725).  Both are written from those two sources and
from include/symode.h, not from the kernels, and know nothing of lanes, rings or staging.

Every comparison that decides a branch is reported as a margin ``(name, lhs, rhs)`` (both as Python floats): a test may
only trust a launch whose margins are settled (``unsettled``), because a float32 device and a float64 model may then not
fall on different sides.  Comparisons whose left side is a difference of two close numbers are reported in the form that
shows the cancellation (``loss`` against ``prev_loss +- tol_change``, ``|xi|`` against ``threshold +- band``).

State of one problem (a dict): ``params xi mask g d prev_g`` vectors; ``loss t h_diag prev_loss l1_last`` 0-dim tensors;
``act n_iter head done`` ints; ``pairs``: list of ``(y, s, ro)``, oldest first.  The epoch logic adds ``prev pprev``
vectors and ``n_iters nan finished epochs near`` ints.  Unconstrained problems have ``xi is params`` in value: the model
keeps them equal.  ``head`` is the device's ring position of the oldest pair; the model only states when it moves (one
slot per eviction, to 0 with an empty memory) so that ``pairs_to_ring`` can lay the pairs out as the device does.
"""
import math

import torch

BEGIN, ACCEPT = 2, 1                                  # the mode argument of symode_trainer_update (include/symode.h)
EVENT_NONE, EVENT_CONV, EVENT_FREQ, EVENT_FINAL, EVENT_NAN, EVENT_IDLE = 0, 1, 2, 3, 4, -1
CURVATURE_GUARD = 1e-10                               # torch/optim/lbfgs.py: `if ys > 1e-10`
TINY = 1e-30


def f32(v):
    """A Python float rounded through float32: what the device's descriptor holds."""
    return float(torch.tensor(v, dtype=torch.float32))


def make_cfg(lr=1.0, tol_grad=1e-7, tol_change=1e-9, history=100, w_x=1.0, w_reg=0.0, l1=True, pair=False, w_pair=0.0,
             map=None, threshold=0.1, tol_update=1e-3, near_band=1e-4, st_freq=0, d=1):
    """``map``: None or ``(Q_eff (dp, r), r, p, allow_const)``; ``d``: equations (rows of Xi).  Float settings are rounded
    through float32 so that model and device compare against the same numbers."""
    return dict(lr=f32(lr), tol_grad=f32(tol_grad), tol_change=f32(tol_change), history=int(history), w_x=f32(w_x),
                w_reg=f32(w_reg) if l1 else 0.0, l1=bool(l1), pair=bool(pair), w_pair=f32(w_pair), map=map,
                threshold=f32(threshold), tol_update=f32(tol_update), near_band=f32(near_band), st_freq=int(st_freq), d=int(d))


def unsettled(margins, rel):
    """The margins a relative float tolerance ``rel`` cannot decide (exactly equal sides are the caller's to vouch for)."""
    bad = []
    for name, lhs, rhs in margins:
        if math.isnan(lhs) or math.isnan(rhs):
            continue                                  # a NaN compares false in every dtype
        if not abs(lhs - rhs) > rel * max(abs(lhs), abs(rhs), TINY):
            bad.append((name, lhs, rhs))
    return bad


def _copy(state):
    out = {}
    for k, v in state.items():
        if torch.is_tensor(v):
            out[k] = v.clone()
        elif k == "pairs":
            out[k] = [(y.clone(), s.clone(), ro.clone()) for y, s, ro in v]
        else:
            out[k] = v
    return out


def xi_of(params, cfg):
    """Xi (flat, (d, p) row-major) at ``params``: the parameters themselves, or Q beta (+ const in column 0)."""
    if cfg["map"] is None:
        return params.clone()
    Q, r, p, allow_const = cfg["map"]
    xi = (Q.to(params.dtype) @ params[:r]).clone()
    if allow_const:
        xi[::p] += params[r:]
    return xi


def grad_of(g_xi, cfg):
    """d/dparams from d/dXi: Q^T g_xi for beta, column 0 of every equation for the constants (zero when the model does not
    read them)."""
    if cfg["map"] is None:
        return g_xi.clone()
    Q, r, p, allow_const = cfg["map"]
    g_beta = Q.to(g_xi.dtype).T @ g_xi
    g_const = g_xi[::p].clone() if allow_const else torch.zeros(cfg["d"], dtype=g_xi.dtype)
    return torch.cat([g_beta, g_const])


def update(state, cl_loss, cl_grad, cfg, mode):
    """One ``symode_trainer_update`` launch -- the TRAINER's route only: that entry point always forms
    w_x * data + w_reg * |params|_1 (w_reg = 0 when ``l1`` is off) and always keeps ``l1_last``, and so does this model.  The
    sweep's entry point (symode_lbfgs_step) is the same launch without map, pair and l1_last: with its ``l1`` set it is
    tied to this one byte for byte (tests/test_gpu_trainer_steps.py); its l1 == 0 call (no w_x) is NOT described here.  ``cl_loss`` (2,) = (mse, regulariser) [the second is ignored without ``pair``],
    ``cl_grad`` (dp,) = d(data term)/dXi.  Returns (state', margins)."""
    st, mg = _copy(state), []
    dt = st["params"].dtype
    cl_loss, cl_grad = cl_loss.to(dt), cl_grad.to(dt)
    if mode == BEGIN:
        if st["done"]:                                # the epoch logic has finished this problem: the step is not taken
            st["act"] = 0
            return st, mg
    elif not st["act"]:                               # stopped earlier in this step()
        return st, mg
    # --- the closure: objective = w_x * (mse + w_pair * reg) + w_reg * |params|_1          (lbfgs_fit.closure)
    data = cl_loss[0] + cfg["w_pair"] * cl_loss[1] if cfg["pair"] else cl_loss[0]
    l1n = st["params"].abs().sum()
    loss = cfg["w_x"] * data + cfg["w_reg"] * l1n
    g = cfg["w_x"] * grad_of(cl_grad, cfg) + cfg["w_reg"] * torch.sign(st["params"])      # torch.sign(0) = 0
    st["g"], st["loss"], st["l1_last"] = g, loss, l1n
    # --- stopping tests (a NaN maximum compares false: it stops nothing)
    gmax = g.abs().max()
    mg.append(("tol_grad", float(gmax), cfg["tol_grad"]))
    stop = bool(gmax <= cfg["tol_grad"])
    if mode == ACCEPT and not stop:
        dmax = (st["d"] * st["t"]).abs().max()
        mg.append(("step_size", float(dmax), cfg["tol_change"]))
        stop = bool(dmax <= cfg["tol_change"])
        if not stop:
            mg.append(("loss_change_hi", float(loss), float(st["prev_loss"] + cfg["tol_change"])))
            mg.append(("loss_change_lo", float(loss), float(st["prev_loss"] - cfg["tol_change"])))
            stop = bool((loss - st["prev_loss"]).abs() < cfg["tol_change"])
    if stop:
        st["act"] = 0
        return st, mg
    # --- one iteration of the loop, up to the move
    st["n_iter"] += 1
    if st["n_iter"] == 1:
        st["pairs"], st["head"] = [], 0
        st["h_diag"] = torch.ones((), dtype=dt)
    else:
        y = g - st["prev_g"]
        s = st["d"] * st["t"]
        ys = y.dot(s)
        mg.append(("curvature", float(ys), CURVATURE_GUARD))
        if bool(ys > CURVATURE_GUARD):
            if len(st["pairs"]) == cfg["history"]:
                st["pairs"].pop(0)
                st["head"] = (st["head"] + 1) % cfg["history"]
            st["pairs"].append((y, s, 1.0 / ys))
            st["h_diag"] = ys / y.dot(y)
    q = -g
    al = [None] * len(st["pairs"])
    for i in range(len(st["pairs"]) - 1, -1, -1):
        y, s, ro = st["pairs"][i]
        al[i] = s.dot(q) * ro
        q = q - al[i] * y
    dvec = q * st["h_diag"]
    for i, (y, s, ro) in enumerate(st["pairs"]):
        be = y.dot(dvec) * ro
        dvec = dvec + s * (al[i] - be)
    st["d"] = dvec
    st["prev_g"], st["prev_loss"] = g.clone(), loss.clone()
    if st["n_iter"] == 1:
        inv = 1.0 / g.abs().sum()                     # `min(1., 1. / flat_grad.abs().sum()) * lr`: Python's min, so that
        st["t"] = (inv if bool(inv < 1.0) else torch.ones((), dtype=dt)) * cfg["lr"]      # a NaN sum gives lr
    else:
        st["t"] = torch.tensor(cfg["lr"], dtype=dt)
    gtd = g.dot(dvec)
    mg.append(("descent", float(gtd), -cfg["tol_change"]))
    if bool(gtd > -cfg["tol_change"]):
        st["act"] = 0
        return st, mg
    st["params"] = st["params"] + st["t"] * dvec
    st["xi"] = xi_of(st["params"], cfg)
    st["act"] = 1
    return st, mg


def _tensors(v, cfg):
    """The parameter tensors of the model: [Xi], or [beta, const] under the map."""
    if cfg["map"] is None:
        return [v]
    r = cfg["map"][1]
    return [v[:r], v[r:]]


def epoch_end(state, cl_loss, cfg, epoch):
    """One ``symode_trainer_epoch_end`` launch.  ``cl_loss`` (2,): the last closure's (mse, regulariser), for the record.
    Returns (state', record, margins); record = dict(code, mse, sym, l1, update_norm, update_norm_2, near, epoch) and,
    unless idle, the rows ``xi mask params`` after the event."""
    st, mg = _copy(state), []
    if st["done"]:
        return st, dict(code=EVENT_IDLE, epoch=epoch), mg
    dt = st["params"].dtype
    zero = torch.zeros((), dtype=dt)
    st["epochs"] = epoch + 1
    n_it = st["n_iters"] + 1                                                                # :694
    upd = sum((torch.linalg.vector_norm(a - b) for a, b in zip(_tensors(st["params"], cfg), _tensors(st["prev"], cfg))), zero)
    upd2 = sum((torch.linalg.vector_norm(a - b) for a, b in zip(_tensors(st["params"], cfg), _tensors(st["pprev"], cfg))), zero)
    rec = dict(mse=float(cl_loss[0]), sym=float(cl_loss[1]) if cfg["pair"] else 0.0, l1=float(st["l1_last"]),
               update_norm=float(upd), update_norm_2=float(upd2), near=0, epoch=epoch)
    event = EVENT_NONE
    if bool(torch.isnan(st["params"]).any()):                                               # :697
        st["nan"], st["done"], st["n_iters"] = 1, 1, n_it
        event = EVENT_NAN
    else:
        mg.append(("tol_update", float(upd), cfg["tol_update"]))
        if bool(upd < cfg["tol_update"]):                                                   # :705
            mg.append(("tol_update_2", float(upd2), cfg["tol_update"]))
            event = EVENT_FINAL if bool(upd2 < cfg["tol_update"]) else EVENT_CONV           # :709
        elif cfg["st_freq"] > 0 and n_it % cfg["st_freq"] == 0:                             # :720
            event = EVENT_FREQ
        if event == EVENT_FINAL:
            st["finished"], st["done"], st["n_iters"] = 1, 1, n_it
        elif event in (EVENT_CONV, EVENT_FREQ):
            st["n_iters"] = 0
            a = st["xi"].abs()                                                              # set_threshold (sindy.py:192-194)
            live = st["mask"] > 0
            thr, band = cfg["threshold"], cfg["near_band"]
            for j in range(a.numel()):
                mg.append(("threshold", float(a[j]), thr))
                if bool(live[j]):
                    mg.append(("near_hi", float(a[j]), float(torch.tensor(thr, dtype=dt) + band)))
                    mg.append(("near_lo", float(a[j]), float(torch.tensor(thr, dtype=dt) - band)))
            near = int((((a - thr).abs() < band) & live).sum())
            st["near"] += near
            rec["near"] = near
            st["mask"] = ((a > thr) & live).to(dt)
            st["n_iter"], st["pairs"], st["head"] = 0, [], 0                                # a fresh optimiser (:717 / :723)
            st["h_diag"] = torch.ones((), dtype=dt)
            if event == EVENT_CONV:
                st["pprev"] = st["params"].clone()                                          # :718
        else:
            st["n_iters"] = n_it
        if event != EVENT_FINAL:
            st["prev"] = st["params"].clone()                                               # :725
    rec["code"] = event
    rec["xi"], rec["mask"], rec["params"] = st["xi"].clone(), st["mask"].clone(), st["params"].clone()
    return st, rec, mg


# ---------------------------------------------------------------------------------------------------------------------
# logical pair order <-> the device's ring (head, count, slot (head + k) % H)
# ---------------------------------------------------------------------------------------------------------------------
def pairs_from_ring(old_dirs, old_stps, ro, head, count):
    """Pairs of one problem, oldest first, from its ring arrays old_dirs / old_stps (H, n) and ro (H,)."""
    H = old_dirs.shape[0]
    return [(old_dirs[(head + k) % H].clone(), old_stps[(head + k) % H].clone(), ro[(head + k) % H].clone()) for k in range(count)]


def pairs_to_ring(pairs, head, old_dirs, old_stps, ro):
    """Write ``pairs`` (oldest first) into the ring arrays in place, the oldest at slot ``head``; other slots keep what
    they hold.  Returns (head, count)."""
    H = old_dirs.shape[0]
    assert len(pairs) <= H
    for k, (y, s, r) in enumerate(pairs):
        slot = (head + k) % H
        old_dirs[slot], old_stps[slot], ro[slot] = y, s, r
    return head, len(pairs)
