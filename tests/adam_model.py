"""One minibatch step and the epoch end of the device Adam trainer as plain torch, for ONE problem, in the dtype asked for.

``step`` is one batch of ``symode_adam_epochs`` / ``symode_adam_epochs_reversed``: the loss include/symode.h writes out,
its gradient with respect to the raw parameters in closed form, and torch.optim.Adam.step as that header words it
(train.py:491-547 of the reference).  ``epoch_end`` is the thresholding event after an epoch (sindy.py:192-194).  Both are
written from those sources, not from the kernel, and know nothing of threads, waves or staging.  Theta comes from
``oracle.sindy_oracle``.

State of one problem (a dict): ``params m v`` vectors (n,), ``mask`` (d p,), ``step`` an int (< 0: frozen at step
-step - 1).  ``data``: ``x dx`` (n_src, d) and, for the reversed regulariser, ``gx`` (n_g, n_src, d), ``jgx``
(n_g, n_src, d, d) -- or ``gx = None``.

``epoch_end`` reports every comparison that decides something as a margin ``(name, lhs, rhs)``, as tests/trainer_model.py
does: a float32 device and the fp64 model may only be compared where neither can fall on the other side.

``mutant`` switches ONE deliberate mistake on (tests/test_host_adam_model.py proves with them that the cases notice such
a mistake); None is the model.
"""
import torch

from oracle import sindy_oracle as O
from tests.trainer_model import f32, unsettled  # noqa: F401  (unsettled: re-exported for the cases)

MUTANTS = ("data_grad_x2", "l1_dropped", "l1_sign0_is_1", "reg_weight_times_w_x", "reg_grad_dropped", "pads_in_divisor",
           "d_missing_in_divisor", "mask_not_on_grad", "const_grad_wrong_column", "eps_inside_sqrt", "no_bias_correction_1",
           "no_bias_correction_2", "t_not_carried", "l1_logged_after_update", "threshold_not_strict", "near_ignores_mask")


def make_cfg(d, order, flags, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, w_x=1.0, w_reg=1e-3, l1=True, w_sym=0.0, map=None,
             threshold=0.1, st_freq=0, near_band=1e-4, epoch0=0):
    """``map``: None (the parameters are Xi) or ``(Q_eff (d p, r) fp64, r, p, allow_constant)``.  Float settings are rounded
    through float32: model and device work with the same numbers."""
    return dict(d=int(d), order=int(order), flags=int(flags), lr=f32(lr), beta1=f32(betas[0]), beta2=f32(betas[1]), eps=f32(eps),
                w_x=f32(w_x), w_reg=f32(w_reg), l1=bool(l1), w_sym=f32(w_sym), map=map, threshold=f32(threshold),
                st_freq=int(st_freq), near_band=f32(near_band), epoch0=int(epoch0))


def terms(cfg):
    return O.term_count(cfg["d"], cfg["order"], bool(cfg["flags"] & 1), bool(cfg["flags"] & 2))


def xi_of(params, cfg):
    """Xi (flat, (d, p) row-major): the parameters, or reshape(Q beta) plus const in column 0 (sindy.py:169-176)."""
    if cfg["map"] is None:
        return params.clone()
    Q, r, p, allow_const = cfg["map"]
    xi = Q.to(params.dtype) @ params[:r]
    if allow_const:
        xi = xi.clone()
        xi[::p] += params[r:]
    return xi


def grad_of(g_xi, cfg, mutant=None):
    """d/dparams from d/dXi: Q^T g for beta, column 0 of every row for const (zero when const is not read)."""
    if cfg["map"] is None:
        return g_xi.clone()
    Q, r, p, allow_const = cfg["map"]
    col = 1 if mutant == "const_grad_wrong_column" else 0
    g_const = g_xi[col::p].clone() if allow_const else torch.zeros(cfg["d"], dtype=g_xi.dtype)
    return torch.cat([Q.to(g_xi.dtype).T @ g_xi, g_const])


def _total(t, sequential):
    """Sum over the first axis; ``sequential``: one term after the other in the tensor's dtype (the float32 replay)."""
    if t.shape[0] == 0:
        return torch.zeros(t.shape[1:], dtype=t.dtype)
    return t.cumsum(0)[-1] if sequential else t.sum(0)


def valid_rows(batch_rows, n_src):
    """The entries in [0, n_src), in table order, duplicates kept; everything else is padding."""
    return [int(i) for i in batch_rows.tolist() if 0 <= int(i) < n_src]


def loss_and_grad(params, mask, rows, data, cfg, sequential=False, mutant=None, n_entries=None):
    """(mse, sym, d loss / d params without the L1 term, the same with respect to Xi) at ``rows`` (valid row numbers); dtype
    of ``params``."""
    dt = params.dtype
    d, p = cfg["d"], terms(cfg)
    sine, exp_ = bool(cfg["flags"] & 1), bool(cfg["flags"] & 2)
    x, dx = data["x"].to(dt)[rows], data["dx"].to(dt)[rows]
    W = (xi_of(params, cfg) * mask).view(d, p)
    th = O.theta(x, cfg["order"], sine, exp_)
    h = th @ W.T
    res = h - dx
    count = (n_entries if mutant == "pads_in_divisor" else len(rows)) * (1 if mutant == "d_missing_in_divisor" else d)
    mse = _total((res * res).reshape(-1, 1), sequential)[0] / count
    g_mse = 2.0 * _total(res[:, :, None] * th[:, None, :], sequential) / count
    if mutant == "data_grad_x2":
        g_mse = 2.0 * g_mse
    sym, g_sym = torch.zeros((), dtype=dt), torch.zeros(d, p, dtype=dt)
    if data.get("gx") is not None:
        for gx, jg in zip(data["gx"], data["jgx"]):
            tg = O.theta(gx.to(dt)[rows], cfg["order"], sine, exp_)
            J = jg.to(dt)[rows]
            rr = torch.einsum("bij,bj->bi", J, h) - tg @ W.T                 # J_g h(x) - h(g x)
            sym = sym + _total((rr * rr).reshape(-1, 1), sequential)[0] / count
            jtr = torch.einsum("bji,bj->bi", J, rr)
            g_sym = g_sym + 2.0 * _total(jtr[:, :, None] * th[:, None, :] - rr[:, :, None] * tg[:, None, :], sequential) / count
    w_sym = cfg["w_sym"] * cfg["w_x"] if mutant == "reg_weight_times_w_x" else cfg["w_sym"]
    g_xi = cfg["w_x"] * g_mse + (0.0 if mutant == "reg_grad_dropped" else w_sym) * g_sym
    g_xi = g_xi.reshape(-1)
    if mutant != "mask_not_on_grad":
        g_xi = g_xi * mask                                                    # the model reads Xi * mask
    return mse, sym, grad_of(g_xi, cfg, mutant), g_xi


def step(state, batch_rows, data, cfg, sequential=False, mutant=None):
    """One minibatch step.  Returns (state', record): record None when no step is taken (padding alone, a frozen problem,
    or a non-finite mse + sym, which freezes the problem: state untouched but step = -t - 1); else dict(mse, l1, sym)."""
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
    rows = valid_rows(batch_rows, data["x"].shape[0])
    if st["step"] < 0 or not rows:
        return st, None
    p, dt = st["params"], st["params"].dtype
    mse, sym, g, _ = loss_and_grad(p, st["mask"], rows, data, cfg, sequential, mutant, n_entries=int(batch_rows.numel()))
    if not bool(torch.isfinite(mse + sym)):
        st["step"] = -st["step"] - 1
        return st, None
    l1 = p.abs().sum()
    if cfg["l1"] and mutant != "l1_dropped":
        sgn = torch.sign(p)                                                   # sign(0) = 0
        if mutant == "l1_sign0_is_1":
            sgn = torch.where(p == 0, torch.ones_like(p), sgn)
        g = g + cfg["w_reg"] * sgn
    b1, b2 = cfg["beta1"], cfg["beta2"]
    t = (0 if mutant == "t_not_carried" else st["step"]) + 1
    m = b1 * st["m"] + (1.0 - b1) * g
    v = b2 * st["v"] + (1.0 - b2) * g * g
    bc1 = 1.0 if mutant == "no_bias_correction_1" else 1.0 - b1 ** t         # Python floats: fp64 in either replay
    bc2 = 1.0 if mutant == "no_bias_correction_2" else 1.0 - b2 ** t
    if mutant == "eps_inside_sqrt":
        denom = torch.sqrt(v / bc2 + cfg["eps"])
    else:
        denom = torch.sqrt(v) / torch.tensor(bc2, dtype=dt).sqrt() + cfg["eps"]
    st["params"] = p - torch.tensor(cfg["lr"] / bc1, dtype=dt) * (m / denom)
    st["m"], st["v"], st["step"] = m, v, t
    if mutant == "l1_logged_after_update":
        l1 = st["params"].abs().sum()
    return st, dict(mse=mse, l1=l1, sym=sym)


def epoch_end(state, xi, cfg, epoch, mutant=None):
    """The thresholding event after global epoch ``epoch`` at coefficients ``xi`` (unmasked).  Returns
    (state', dict(event, near), margins)."""
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
    mg = []
    event = st["step"] >= 0 and cfg["st_freq"] > 0 and (epoch + 1) % cfg["st_freq"] == 0
    near = 0
    if event:
        dt = xi.dtype
        a, live = xi.abs(), st["mask"] > 0
        thr, band = torch.tensor(cfg["threshold"], dtype=dt), torch.tensor(cfg["near_band"], dtype=dt)
        for j in range(a.numel()):
            if bool(live[j]):                                                 # a zero stays zero whatever |Xi| is
                mg.append(("threshold", float(a[j]), float(thr)))
                mg.append(("near_hi", float(a[j]), float(thr + band)))
                mg.append(("near_lo", float(a[j]), float(thr - band)))
        counted = torch.ones_like(live) if mutant == "near_ignores_mask" else live
        near = int((((a - thr).abs() < band) & counted).sum())
        keep = (a >= thr) if mutant == "threshold_not_strict" else (a > thr)
        st["mask"] = (keep & live).to(st["mask"].dtype)
    return st, dict(event=int(event), near=near), mg
