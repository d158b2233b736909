"""One minibatch step of the device Adam trainer's latent branch as plain torch, for ONE problem, in the dtype asked for.

``step`` is one batch of ``symode_adam_epochs_latent``: the loss include/symode.h writes out for that entry, its gradient
with respect to the raw parameters in closed form, and torch.optim.Adam.step as the header words it for
``symode_adam_epochs`` (train.py:491-547 of the reference, the ``use_latent`` branch).  Written from those sources, not from
the kernel; the pieces that do not depend on the loss -- the coefficient map, the parameter gradient from d/dXi, the sums,
the row filter and the epoch end -- are those of tests/adam_model.py.

``data``: ``z dz y`` (n_src, d), ``B`` (n_src, d, d), ``e`` (n_src,) or None (D_obs == d), ``L`` (n_gen, d, d) or None.
``cfg``: ``adam_model.make_cfg`` plus ``w_z``, ``D_obs``, ``n_gen``; its ``w_x`` weighs mse_x, its ``w_sym`` the regulariser.

``mutant`` switches ONE deliberate mistake on (tests/test_host_adam_latent_model.py proves with them that the cases notice
such a mistake); None is the model.
"""
import torch

from oracle import sindy_oracle as O
from tests import adam_model as M
from tests.adam_model import epoch_end, f32, grad_of, terms, unsettled, valid_rows, xi_of  # noqa: F401  (re-exported for the cases)

MUTANTS = ("sym_divided_by_rows", "x_term_in_gradient", "sym_grad_dropped", "lt_u_term_dropped", "e_dropped_from_log",
           "D_for_d_in_x_divisor", "z_weight_on_sym", "mask_not_on_sym_grad")


def make_cfg(d, order, flags, w_z=1.0, D_obs=None, n_gen=0, **kw):
    cfg = M.make_cfg(d, order, flags, **kw)
    cfg.update(w_z=f32(w_z), D_obs=int(d if D_obs is None else D_obs), n_gen=int(n_gen))
    return cfg


def theta_jvp(z, v, order, include_sine, include_exp):
    """J_Theta(z) v, column for column in the library order of ``O.theta``: the product rule along the same left-to-right
    products, cos z * v and exp z * v for the two optional blocks."""
    d = z.shape[-1]
    blocks = [torch.zeros(*z.shape[:-1], 1, dtype=z.dtype), v]
    prev = {(i,): (z[..., i], v[..., i]) for i in range(d)}
    for n in range(2, order + 1):
        cur, cols = {}, []
        for tup in O.poly_tuples(d, n):
            a, da = prev[tup[:-1]]
            k = tup[-1]
            cur[tup] = (a * z[..., k], da * z[..., k] + a * v[..., k])
            cols.append(cur[tup][1].reshape(*z.shape[:-1], 1))
        blocks.append(torch.cat(cols, dim=-1))
        prev = cur
    if include_sine:
        blocks.append(torch.cos(z) * v)
    if include_exp:
        blocks.append(torch.exp(z) * v)
    return torch.cat(blocks, dim=-1)


def loss_and_grad(params, mask, rows, data, cfg, sequential=False, mutant=None):
    """(mse_z, mse_x, sym, d loss / d params without the L1 term, the same with respect to Xi) at ``rows`` (valid row
    numbers); dtype of ``params``."""
    dt = params.dtype
    d, p, D = cfg["d"], terms(cfg), cfg["D_obs"]
    sine, exp_ = bool(cfg["flags"] & 1), bool(cfg["flags"] & 2)
    z, dz, B, y = (data[k].to(dt)[rows] for k in ("z", "dz", "B", "y"))
    n = len(rows)
    W = (xi_of(params, cfg) * mask).view(d, p)
    th = O.theta(z, cfg["order"], sine, exp_)
    h = th @ W.T
    r_z = h - dz
    r_x = torch.einsum("bij,bj->bi", B, h) - y
    mse_z = M._total((r_z * r_z).reshape(-1, 1), sequential)[0] / (n * d)
    x_terms = torch.zeros(n, 1, dtype=dt)                     # per row: |r_x|^2, then e_b
    for i in range(d):
        x_terms[:, 0] = x_terms[:, 0] + r_x[:, i] * r_x[:, i]
    if data.get("e") is not None and D > d and mutant != "e_dropped_from_log":
        x_terms = x_terms + data["e"].to(dt)[rows].reshape(-1, 1)
    mse_x = M._total(x_terms, sequential)[0] / (n * (d if mutant == "D_for_d_in_x_divisor" else D))
    g_z = 2.0 * M._total(r_z[:, :, None] * th[:, None, :], sequential) / (n * d)
    sym, g_sym = torch.zeros((), dtype=dt), torch.zeros(d, p, dtype=dt)
    if data.get("L") is not None:
        for L in data["L"].to(dt):
            dth = theta_jvp(z, z @ L.T, cfg["order"], sine, exp_)
            u = dth @ W.T - h @ L.T                                           # W J_Theta(z)(L z) - L h
            sym = sym + M._total((u * u).reshape(-1, 1), sequential)[0]
            ltu = torch.zeros_like(u) if mutant == "lt_u_term_dropped" else u @ L     # (L^T u) per row
            g_sym = g_sym + 2.0 * M._total(u[:, :, None] * dth[:, None, :] - ltu[:, :, None] * th[:, None, :], sequential)
    if mutant == "sym_divided_by_rows":
        sym, g_sym = sym / n, g_sym / n
    w_sym = cfg["w_sym"] * cfg["w_z"] if mutant == "z_weight_on_sym" else cfg["w_sym"]
    if mutant == "sym_grad_dropped":
        w_sym = 0.0
    mk = mask.view(d, p)
    g_xi = cfg["w_z"] * g_z * mk + w_sym * g_sym * (1.0 if mutant == "mask_not_on_sym_grad" else mk)
    if mutant == "x_term_in_gradient":
        btr = torch.einsum("bji,bj->bi", B, r_x)
        g_xi = g_xi + cfg["w_x"] * 2.0 * M._total(btr[:, :, None] * th[:, None, :], sequential) / (n * D) * mk
    g_xi = g_xi.reshape(-1)
    return mse_z, mse_x, sym, grad_of(g_xi, cfg), g_xi


def step(state, batch_rows, data, cfg, sequential=False, mutant=None):
    """One minibatch step.  Returns (state', record): record None when no step is taken (padding alone, a frozen problem,
    or a non-finite w_z mse_z + w_x mse_x + w_sym sym, which freezes the problem: state untouched but step = -t - 1); else
    dict(mse_z, mse_x, sym, l1)."""
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
    rows = valid_rows(batch_rows, data["z"].shape[0])
    if st["step"] < 0 or not rows:
        return st, None
    p, dt = st["params"], st["params"].dtype
    mse_z, mse_x, sym, g, _ = loss_and_grad(p, st["mask"], rows, data, cfg, sequential, mutant)
    if not bool(torch.isfinite(cfg["w_z"] * mse_z + cfg["w_x"] * mse_x + cfg["w_sym"] * sym)):
        st["step"] = -st["step"] - 1
        return st, None
    l1 = p.abs().sum()
    if cfg["l1"]:
        g = g + cfg["w_reg"] * torch.sign(p)                                  # sign(0) = 0
    b1, b2 = cfg["beta1"], cfg["beta2"]
    t = st["step"] + 1
    m = b1 * st["m"] + (1.0 - b1) * g
    v = b2 * st["v"] + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t                                   # Python floats: fp64 in either replay
    denom = torch.sqrt(v) / torch.tensor(bc2, dtype=dt).sqrt() + cfg["eps"]
    st["params"] = p - torch.tensor(cfg["lr"] / bc1, dtype=dt) * (m / denom)
    st["m"], st["v"], st["step"] = m, v, t
    return st, dict(mse_z=mse_z, mse_x=mse_x, sym=sym, l1=l1)
