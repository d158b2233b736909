"""The regulariser operators as plain torch in closed form, in the dtype asked for: the materialised reversed symmetry
regulariser (S4, ``symode_symreg_reversed`` / ``symode_symreg_reversed_batched``) first, the S2 / S3 operators
(``symode_forward_jvp``, ``symode_vjp``, ``symode_jvp_vjp``, ``symode_euler_jvp``, ``symode_euler_jvp_vjp``) and the roll-out
error further down, each under its own heading.

S4.  Written from the formula include/symode.h documents at ``symode_symreg_reversed``, not from the kernel, and knowing nothing of
chunks, waves, partial rows or slabs:

    u    = J_g(x_n) h(x_n) - h(g x_n)                     per problem, group element and point; h = Theta(.) W^T, W = xi * mask
    loss = inv_count * sum_g sum_n |u|^2                  inv_count = 1 / (n d) unless given (a rank holding a shard of the points)
    grad = 2 inv_count * sum_g sum_n ((J_g^T u) Theta(x_n)^T - u Theta(g x_n)^T) * mask

``inv_count`` reaches the device as a float32 argument, so it is an INPUT like the points: the model takes the float32 value
of it (``round_inv=False``: the number as given, for the comparison with the oracle's exact mean).

Next to (loss, grad) ``evaluate`` returns the YARDSTICKS: the same sums with every term replaced by its absolute value,
``a = |J_g| (|Theta(x)| |W|^T) + |Theta(g x)| |W|^T`` standing where ``u`` stands: inv_count * sum a^2 and 2 inv_count *
sum ((|J_g|^T a) |Theta(x)|^T + a |Theta(g x)|^T) * mask.  A float32 evaluation is judged against them, not against the result
(J_g = I with g x = x gives u = 0 and a float32 value that is pure rounding), and ENTRY BY ENTRY: entry (j, q) of grad against
entry (j, q) of its yardstick, never against the largest one -- the high-order columns are hundreds of times smaller than the
constant column and would hide behind it.  A zero yardstick (no group element, a masked entry) demands the exact zero.

``sequential``: every sum one term after the other in the tensor's dtype, points outermost, group elements inside, as a single
thread would add them (the float32 replay of tests/test_host_regulariser_model.py); the matrix products are then written out
as one multiply and one add per term, and sin / exp are taken in fp64 and rounded (``symreg_linear_model.theta_jvp``): the
replay consists of IEEE operations alone and gives the same figures on any CPU.

``mutant`` switches ONE deliberate mistake on; None is the model.
"""
import torch

from tests.symreg_linear_model import PPT, _apply, _total, terms, theta_jvp

S4_MUTANTS = ("jg_transposed", "jgx_group_stride_n_d", "divisor_n", "generator_0_only", "problem_0_xi", "grad_jg_for_jg_t",
              "mask_on_grad_not_on_xi", "mask_on_xi_not_on_grad", "last_ragged_point_dropped", "last_chunk_twice")


def s4_mutant_applies(mutant, d, n_g, S, n, has_mask, default_inv):
    """Does ``mutant`` read or compute anything else than the model on a case of this shape?"""
    if n_g == 0:
        return False                                     # nothing is summed at all
    if mutant in ("jg_transposed", "grad_jg_for_jg_t"):
        return d > 1
    if mutant == "jgx_group_stride_n_d":
        return d > 1 and n_g > 1
    if mutant == "divisor_n":
        return d > 1 and default_inv
    if mutant == "generator_0_only":
        return n_g > 1
    if mutant == "problem_0_xi":
        return S > 1
    if mutant.startswith("mask"):
        return has_mask
    if mutant == "last_ragged_point_dropped":
        return n % PPT[d] != 0
    if mutant == "last_chunk_twice":
        return n >= PPT[d]
    raise ValueError(mutant)


def _theta(z, order, flags):
    return theta_jvp(z, torch.zeros_like(z), order, flags)[0]


def _matvec(J, h, sequential, transpose=False):
    """J (n, d, d) times h (n, d) per point (``transpose``: J^T h); ``sequential``: one term after the other."""
    if transpose:
        J = J.transpose(1, 2)
    if not sequential:
        return torch.einsum("nij,nj->ni", J, h)
    out = []
    for i in range(J.shape[1]):
        t = J[:, i, 0] * h[:, 0]
        for j in range(1, J.shape[2]):
            t = t + J[:, i, j] * h[:, j]
        out.append(t)
    return torch.stack(out, dim=1)


def _points(n, d, mutant):
    """The point indices the sums run over."""
    idx = list(range(n))
    ppt = PPT[d]
    if mutant == "last_ragged_point_dropped" and n % ppt:
        idx = idx[:-1]
    if mutant == "last_chunk_twice" and n >= ppt:
        full = (n // ppt) * ppt
        idx = idx + list(range(full - ppt, full))
    return torch.tensor(idx, dtype=torch.long)


def _one_problem(x, gx, jgx, W, mk, inv, order, flags, sequential, mutant):
    """x (n, d), gx (n_g, n, d), jgx (n_g, n, d, d), W, mk (d, p) -> loss, grad, loss_yard, grad_yard, the largest a (the mask not yet on grad)."""
    n, d = x.shape
    p = W.shape[1]
    dt = x.dtype
    n_g = gx.shape[0]
    if mutant == "jgx_group_stride_n_d" and n_g > 1:     # group g read n d floats after group g - 1, where n d d are right
        flat = jgx.reshape(-1)
        jgx = torch.stack([flat[g * n * d:g * n * d + n * d * d].reshape(n, d, d) for g in range(n_g)])
    if mutant == "generator_0_only":
        gx, jgx, n_g = gx[:1], jgx[:1], min(n_g, 1)
    if n_g == 0:
        zero = torch.zeros((), dtype=dt)
        return zero, torch.zeros(d, p, dtype=dt), zero.clone(), torch.zeros(d, p, dtype=dt), zero.clone()
    keep = _points(n, d, mutant)
    x = x[keep]
    th = _theta(x, order, flags)
    h, ha = _apply(th, W, sequential), th.abs() @ W.abs().T
    sq, ysq, gt, ygt = [], [], [], []
    for g in range(n_g):
        J = jgx[g][keep]
        thg = _theta(gx[g][keep], order, flags)
        hg, hga = _apply(thg, W, sequential), thg.abs() @ W.abs().T
        u = _matvec(J, h, sequential, transpose=mutant == "jg_transposed") - hg
        a = _matvec(J.abs(), ha, False) + hga
        jtu = _matvec(J, u, sequential, transpose=mutant != "grad_jg_for_jg_t")
        jta = _matvec(J.abs(), a, False, transpose=True)
        sq.append(u * u)
        ysq.append(a * a)
        gt.append(jtu[:, :, None] * th[:, None, :] - u[:, :, None] * thg[:, None, :])
        ygt.append(jta[:, :, None] * th.abs()[:, None, :] + a[:, :, None] * thg.abs()[:, None, :])
    flat = lambda parts: torch.stack(parts, dim=1).reshape(-1)                 # noqa: E731  points outermost, then group elements
    rows = lambda parts: torch.stack(parts, dim=1).reshape(-1, d, p)           # noqa: E731
    loss = inv * _total(flat(sq)[:, None], sequential)[0]
    loss_yard = inv * _total(flat(ysq)[:, None], False)[0]
    grad = (2.0 * inv) * _total(rows(gt), sequential)
    grad_yard = (2.0 * inv) * _total(rows(ygt), False) * mk
    return loss, grad, loss_yard, grad_yard, torch.stack(ysq).max().sqrt() if len(keep) else torch.zeros((), dtype=dt)


def evaluate_s4(x, gx, jgx, xi, mask, order, flags, inv_count=None, dt=torch.float64, sequential=False, mutant=None, round_inv=True):
    """x (S, n, d), gx (S, n_g, n, d), jgx (S, n_g, n, d, d), xi (S, d, p), mask (S, d, p) or None [one problem: without the
    leading axis], float32 (or anything) -> dict of ``loss`` (S,), ``grad`` (S, d, p), ``loss_yard``, ``grad_yard`` in ``dt``
    [one problem: a scalar and (d, p)], and ``majorant``: the largest component of ``a`` at any point."""
    batched = x.dim() == 3
    if not batched:
        x, gx, jgx, xi = x[None], gx[None], jgx[None], xi[None]
        mask = None if mask is None else mask[None]
    S, n, d = x.shape
    p = terms(d, order, flags)
    inv = 1.0 / (n if mutant == "divisor_n" and inv_count is None else n * d) if inv_count is None else float(inv_count)
    if round_inv:
        inv = float(torch.tensor(inv, dtype=torch.float32))
    out = []
    for s in range(S):
        xi_s = xi[0 if mutant == "problem_0_xi" else s].to(dt).reshape(d, p)
        mk = torch.ones(d, p, dtype=dt) if mask is None else mask[s].to(dt).reshape(d, p)
        W = xi_s if mutant == "mask_on_grad_not_on_xi" else xi_s * mk
        loss, grad, ly, gy, am = _one_problem(x[s].to(dt), gx[s].to(dt), jgx[s].to(dt), W, mk, inv, order, flags, sequential, mutant)
        out.append((loss, grad if mutant == "mask_on_xi_not_on_grad" else grad * mk, ly, gy, am))
    loss, grad, ly, gy, am = (torch.stack(f) for f in zip(*out))
    if not batched:
        loss, grad, ly, gy = loss[0], grad[0], ly[0], gy[0]
    return dict(loss=loss, grad=grad, loss_yard=ly, grad_yard=gy, majorant=am.max())


def fractions(got, ref, yard):
    """|got - ref| / yard entry by entry; where the yardstick is zero: 0 for the exact zero, inf for anything else (a NaN is
    inf everywhere: it is no deviation to rank)."""
    got, ref, yard = (torch.as_tensor(t, dtype=torch.float64).detach().reshape(-1) for t in (got, ref, yard))
    err = (got - ref).abs()
    frac = torch.where(yard > 0, err / yard.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), frac)


def deviation_s4(got_loss, got_grad, ref):
    """(loss, grad) deviation of a result from the fp64 model ``ref``: the worst entry-by-entry fraction of the yardsticks."""
    return float(fractions(got_loss, ref["loss"], ref["loss_yard"]).max()), float(fractions(got_grad, ref["grad"], ref["grad_yard"]).max())


# ---------------------------------------------------------------------------------------------------------------------
# S2 / S3: the regressor's forward and reverse modes and the Euler flow with its tangent map
# ---------------------------------------------------------------------------------------------------------------------
# From the formulas include/symode.h documents at symode_forward_jvp, symode_vjp, symode_jvp_vjp, symode_euler_jvp and
# symode_euler_jvp_vjp, W = xi * mask:
#
#   forward_jvp    out = Theta(x) W^T,  jv = (J_Theta(x) v) W^T
#   vjp            grad_x = J_Theta(x)^T W^T g,  grad_xi = (g^T Theta(x)) * mask
#   jvp_vjp        grad_x_i = sum_q (g_out W)_q d_i Theta_q + sum_q (g_jv W)_q sum_k d_i d_k Theta_q v_k,
#                  grad_v_k = sum_q (g_jv W)_q d_k Theta_q,  grad_xi = (g_out^T Theta + g_jv^T (J_Theta v)) * mask
#   euler_jvp      K steps (x, t) <- (x + dt out(x), t + dt jv(x, t)), both right-hand sides at the OLD x
#   euler_jvp_vjp  the adjoints (a, b) of (x_K, t_K) walk the steps backwards: step k is jvp_vjp at (x_k, t_k) with
#                  g_out = dt a, g_jv = dt b; a += grad_x, b += grad_v, grad_xi accumulates
#
# The forward side takes Theta and J_Theta v from ``symreg_linear_model.theta_jvp``; the reverse side is written by hand on
# the first and second derivatives of every column (``library_derivatives``), so that it runs in float32 term by term.
# tests/test_host_regulariser_model.py checks it against fp64 autograd through the forward side on every case.
#
# YARDSTICKS: the same computation on (|x|, |v|, |g|, |W|) with the library's majorant in the library's place -- the
# monomials at |x| are the absolute values of the monomials, sinh / cosh / sinh stand for sin / cos / -sin (the power series
# with every term replaced by its absolute value), exp stays.  For the one-step operators that is every term of every sum
# replaced by its absolute value; for the flow it is the majorant recursion on |x|, |t|, |W|, and for its reverse sweep the
# same sweep on the majorant states.  Reduced outputs (grad_xi) are judged entry by entry; per-point outputs (n, d) point by
# point, the largest error among a point's d components against the largest yardstick among them (``point_fractions``).
OPS = {"forward_jvp": ("out", "jv"), "vjp": ("grad_x", "grad_xi"), "jvp_vjp": ("grad_x", "grad_v", "grad_xi"),
       "euler_jvp": ("x_out", "t_out"), "euler_jvp_vjp": ("grad_x", "grad_v", "grad_xi")}
REDUCED = ("grad_xi",)

OPS_MUTANTS = ("tangent_step_uses_updated_x", "sweep_uses_state_k_plus_1", "last_step_state_dropped", "second_order_term_missing",
               "second_order_roles_swapped", "dt_on_one_adjoint_only", "sine_second_derivative_sign", "exp_second_derivative_zero",
               "mask_on_grad_not_on_xi", "mask_on_xi_not_on_grad", "last_ragged_point_dropped", "last_chunk_twice", "g_out_null_as_ones")


def ops_mutant_applies(mutant, op, d, order, flags, n, K, has_mask, g_out_given):
    """Does ``mutant`` compute anything else than the model for this operator on a case of this shape?"""
    euler, reverse = op.startswith("euler"), op in ("vjp", "jvp_vjp", "euler_jvp_vjp")
    second = op in ("jvp_vjp", "euler_jvp_vjp") and (not euler or K >= 1)        # the operators that read second derivatives
    if euler and K == 0 and not mutant.startswith("last_"):
        return False                                     # no step: nothing is computed
    if mutant == "tangent_step_uses_updated_x":
        return euler and (order >= 2 or flags != 0)      # (a linear right-hand side has the same Jacobian everywhere)
    if mutant in ("sweep_uses_state_k_plus_1", "last_step_state_dropped", "dt_on_one_adjoint_only"):
        return op == "euler_jvp_vjp"
    if mutant == "second_order_term_missing":
        return second and (order >= 2 or flags != 0)
    if mutant == "second_order_roles_swapped":
        return second and (order >= 2 or flags != 0) and d > 1
    if mutant == "sine_second_derivative_sign":
        return second and bool(flags & 1)
    if mutant == "exp_second_derivative_zero":
        return second and bool(flags & 2)
    if mutant == "mask_on_grad_not_on_xi":
        return has_mask
    if mutant == "mask_on_xi_not_on_grad":
        return has_mask and reverse and (not euler or K >= 1)
    if mutant == "last_ragged_point_dropped":
        return n % PPT[d] != 0
    if mutant == "last_chunk_twice":
        return reverse and n >= PPT[d] and (not euler or K >= 1)
    if mutant == "g_out_null_as_ones":
        return op == "jvp_vjp" and not g_out_given
    raise ValueError(mutant)


def library_derivatives(x, order, flags, majorant=False, mutant=None):
    """(Theta (n, p), d_i Theta_q (n, p, d), d_i d_k Theta_q (n, p, d, d)), columns in the oracle's order, by the product
    rule along the recurrence column(i1..in) = column(i1..i(n-1)) * x[in].  ``majorant``: sinh, cosh, sinh for sin, cos, -sin."""
    from oracle import sindy_oracle as O
    n, d = x.shape
    zero, one = torch.zeros(n, dtype=x.dtype), torch.ones(n, dtype=x.dtype)
    cols = [(one, torch.zeros(n, d, dtype=x.dtype), torch.zeros(n, d, d, dtype=x.dtype))]
    prev = {}
    for i in range(d):
        g = torch.zeros(n, d, dtype=x.dtype)
        g[:, i] = 1.0
        prev[(i,)] = (x[:, i], g, torch.zeros(n, d, d, dtype=x.dtype))
        cols.append(prev[(i,)])
    for deg in range(2, order + 1):
        cur = {}
        for tup in O.poly_tuples(d, deg):
            pv, pg, ph = prev[tup[:-1]]
            k = tup[-1]
            xk = x[:, k]
            g = pg * xk[:, None]
            g[:, k] = g[:, k] + pv
            h = ph * xk[:, None, None]
            h[:, :, k] = h[:, :, k] + pg
            h[:, k, :] = h[:, k, :] + pg
            cur[tup] = (pv * xk, g, h)
            cols.append(cur[tup])
        prev = cur
    fn = lambda f, a: f(a.double()).to(a.dtype)  # noqa: E731
    def single(i, val, first, second):
        g, h = torch.zeros(n, d, dtype=x.dtype), torch.zeros(n, d, d, dtype=x.dtype)
        g[:, i], h[:, i, i] = first, second
        cols.append((val, g, h))
    if flags & 1:
        for i in range(d):
            s, c = fn(torch.sinh if majorant else torch.sin, x[:, i]), fn(torch.cosh if majorant else torch.cos, x[:, i])
            single(i, s, c, s if majorant or mutant == "sine_second_derivative_sign" else -s)
    if flags & 2:
        for i in range(d):
            e = fn(torch.exp, x[:, i])
            single(i, e, e, zero if mutant == "exp_second_derivative_zero" else e)
    return tuple(torch.stack(part, dim=1) for part in zip(*cols))


def _over_columns(c, A, sequential):
    """sum_q c[:, q] A[:, q, i] -> (n, d); ``sequential``: one term after the other."""
    if not sequential:
        return torch.einsum("nq,nqi->ni", c, A)
    out = []
    for i in range(A.shape[2]):
        t = c[:, 0] * A[:, 0, i]
        for q in range(1, A.shape[1]):
            t = t + c[:, q] * A[:, q, i]
        out.append(t)
    return torch.stack(out, dim=1)


def _along(A, v, sequential):
    """sum_k A[..., k] v[:, k] over the last axis of A (n, ..., d); ``sequential``: one term after the other."""
    shape = (v.shape[0],) + (1,) * (A.dim() - 2)
    t = A[..., 0] * v[:, 0].reshape(shape)
    for k in range(1, v.shape[1]):
        t = t + A[..., k] * v[:, k].reshape(shape)
    return t


def _forward(x, v, W, order, flags, sequential, majorant):
    """(out, jv) at (x, v)"""
    if majorant:
        th, G, _ = library_derivatives(x, order, flags, majorant=True)
        dth = _along(G, v, False)
    else:
        th, dth = theta_jvp(x, v, order, flags)
    return _apply(th, W, sequential), _apply(dth, W, sequential)


def _reverse(x, v, g_out, g_jv, W, order, flags, sequential, majorant, mutant):
    """One step backwards: (grad_x, grad_v, the (n, d, p) terms of grad_xi) of (out, jv) at (x, v) under (g_out, g_jv)."""
    th, G, H = library_derivatives(x, order, flags, majorant, mutant)
    dth = _along(G, v, sequential)
    c_out, c_jv = _apply(g_out, W.T, sequential), _apply(g_jv, W.T, sequential)          # (n, p): sum_j g_j W_jq
    if mutant == "second_order_term_missing":
        second = torch.zeros_like(x)
    elif mutant == "second_order_roles_swapped":         # v in the place of g_jv and g_jv in the place of v
        second = _over_columns(_apply(v, W.T, sequential), _along(H, g_jv, sequential), sequential)
    else:
        second = _over_columns(c_jv, _along(H, v, sequential), sequential)
    grad_x = _over_columns(c_out, G, sequential) + second
    grad_v = _over_columns(c_jv, G, sequential)
    return grad_x, grad_v, g_out[:, :, None] * th[:, None, :] + g_jv[:, :, None] * dth[:, None, :]


def _run(op, x, v, ga, gb, W, K, dt, order, flags, sequential, majorant, mutant):
    """The per-point outputs of ``op`` and the (n, d, p) terms of its grad_xi (None for the forward operators)."""
    zeros = torch.zeros_like(x)
    if op == "forward_jvp":
        out, jv = _forward(x, v, W, order, flags, sequential, majorant)
        return dict(out=out, jv=jv), None
    if op == "vjp":
        grad_x, _, rows = _reverse(x, zeros, ga, zeros, W, order, flags, sequential, majorant, mutant)
        return dict(grad_x=grad_x), rows
    if op == "jvp_vjp":
        if ga is None:
            ga = torch.ones_like(x) if mutant == "g_out_null_as_ones" else zeros
        grad_x, grad_v, rows = _reverse(x, v, ga, gb, W, order, flags, sequential, majorant, mutant)
        return dict(grad_x=grad_x, grad_v=grad_v), rows
    states, t = [], v
    for _ in range(K):
        states.append((x, t))
        h, jt = _forward(x, t, W, order, flags, sequential, majorant)
        if mutant == "tangent_step_uses_updated_x":
            jt = _forward(x + dt * h, t, W, order, flags, sequential, majorant)[1]
        x, t = x + dt * h, t + dt * jt
    states.append((x, t))
    if op == "euler_jvp":
        return dict(x_out=x, t_out=t), None
    a, b, rows = ga, gb, torch.zeros(x.shape[0], W.shape[0], W.shape[1], dtype=x.dtype)
    for k in reversed(range(K)):
        if mutant == "last_step_state_dropped" and k == K - 1:
            continue
        xk, tk = states[k + 1 if mutant == "sweep_uses_state_k_plus_1" else k]
        gx, gv, r = _reverse(xk, tk, dt * a, b if mutant == "dt_on_one_adjoint_only" else dt * b, W, order, flags, sequential, majorant, mutant)
        a, b, rows = a + gx, b + gv, rows + r
    return dict(grad_x=a, grad_v=b), rows


def evaluate_op(op, x, v, ga, gb, xi, mask, order, flags, K=0, dt=0.0, dtype=torch.float64, sequential=False, mutant=None, yardsticks=True):
    """``op`` of OPS on x, v, ga, gb (n, d) [ga: g of vjp, g_out (None allowed) of jvp_vjp, g_x of the flow; gb: g_jv, g_t],
    xi, mask (d, p): dict of the operator's fields and of ``<field>_yard`` in ``dtype``.  ``dt`` is taken as given: hand in a
    number float32 holds exactly.  ``yardsticks=False``: the fields alone."""
    n, d = x.shape
    p = terms(d, order, flags)
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    x, v, ga, gb, xi = cast(x), cast(v), cast(ga), cast(gb), xi.to(dtype).reshape(d, p)
    mk = torch.ones(d, p, dtype=dtype) if mask is None else mask.to(dtype).reshape(d, p)
    W = xi if mutant == "mask_on_grad_not_on_xi" else xi * mk
    points, rows = _run(op, x, v, ga, gb, W, K, dt, order, flags, sequential, False, mutant)
    absolute = lambda t: None if t is None else t.abs()  # noqa: E731
    if not yardsticks:
        ypoints, yrows = {k: torch.zeros_like(t) for k, t in points.items()}, None if rows is None else torch.zeros_like(rows)
    else:
        ypoints, yrows = _run(op, x.abs(), absolute(v), absolute(ga), absolute(gb), (xi * mk).abs(), K, dt, order, flags, False, True, None)
    ppt = PPT[d]
    out = {}
    if mutant == "last_ragged_point_dropped" and n % ppt:
        points = {k: torch.cat([t[:-1], torch.zeros_like(t[-1:])]) for k, t in points.items()}        # never written
    for k in points:
        out[k], out[k + "_yard"] = points[k], ypoints[k]
    if rows is not None:
        if mutant == "last_ragged_point_dropped" and n % ppt:
            rows = rows[:-1]
        if mutant == "last_chunk_twice" and n >= ppt:
            full = (n // ppt) * ppt
            rows = torch.cat([rows, rows[full - ppt:full]])
        grad_xi = _total(rows, sequential)
        out["grad_xi"] = grad_xi if mutant == "mask_on_xi_not_on_grad" else grad_xi * mk
        out["grad_xi_yard"] = _total(yrows, False) * mk
    out["majorant"] = max(float(t.max()) for t in list(ypoints.values()) + ([yrows] if yrows is not None else []))
    return out


def point_fractions(got, ref, yard):
    """Per point: the largest |got - ref| among the point's d components over the largest yardstick among them; a zero
    yardstick demands the exact value, a NaN is inf."""
    got, ref, yard = (torch.as_tensor(t, dtype=torch.float64).detach() for t in (got, ref, yard))
    return fractions((got - ref).abs().amax(dim=1), torch.zeros(got.shape[0], dtype=torch.float64), yard.amax(dim=1))


def deviation_op(op, got, ref):
    """{field: worst fraction of the yardstick} of the results ``got`` (a dict, or the operator's outputs in order)."""
    if not isinstance(got, dict):
        got = dict(zip(OPS[op], got))
    return {f: float((fractions if f in REDUCED else point_fractions)(got[f], ref[f], ref[f + "_yard"]).max()) for f in OPS[op]}


# ---------------------------------------------------------------------------------------------------------------------
# The roll-out error (``symode_rollout_error``): a judge of the integrator that shares no code with it
# ---------------------------------------------------------------------------------------------------------------------
def rollout_error(x_true, xi, mask, order, flags, dt, method, dtype=torch.float64, sequential=False):
    """x_true (n_ics, n_steps + 1, d), xi / mask (S, d, p) -> (err (S, n_ics, n_steps), its yardstick): every model integrated
    from x_true[:, 0] by explicit Euler or classical RK4 steps of dx/dt = Theta(x) W^T, and after step k
    err = mean_j (x_true[i, k + 1, j] - x_pred[j])^2.  The yardstick: mean_j (|x_true| + X)^2 with X the same integration of the
    majorant system from |x_true[:, 0]| (every stage of it is a sum of positive terms)."""
    S, d, p = xi.shape
    n_steps = x_true.shape[1] - 1
    xt = x_true.to(dtype)
    err, yard = [], []
    for s in range(S):
        mk = torch.ones(d, p, dtype=dtype) if mask is None else mask[s].to(dtype)
        W = xi[s].to(dtype) * mk
        for W_, major, sink in ((W, False, err), (W.abs(), True, yard)):
            def f(a):
                if major:
                    return library_derivatives(a, order, flags, majorant=True)[0] @ W_.T
                return _apply(theta_jvp(a, torch.zeros_like(a), order, flags)[0], W_, sequential)
            x = xt[:, 0].abs() if major else xt[:, 0]
            steps = []
            for k in range(n_steps):
                if method == "euler":
                    x = x + dt * f(x)
                else:
                    k1 = f(x)
                    k2 = f(x + dt / 2 * k1)
                    k3 = f(x + dt / 2 * k2)
                    k4 = f(x + dt * k3)
                    x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
                diff = xt[:, k + 1].abs() + x if major else xt[:, k + 1] - x
                sq = diff * diff
                total = sq[:, 0]
                for j in range(1, d):
                    total = total + sq[:, j]
                steps.append(total * (1.0 / d) if dtype == torch.float32 and not major else total / d)
            sink.append(torch.stack(steps, dim=1))
    return torch.stack(err), torch.stack(yard)
