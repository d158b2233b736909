"""The linear-latent symmetry regulariser (S1, ``symode_symreg_linear``) as plain torch in closed form, in the dtype asked for.

Written from the formula include/symode.h and csrc/kernels.hpp document, not from the kernel, and knowing nothing of chunks,
waves or partial rows:

    u    = Xi_m (J_Theta(z) L z) - L (Xi_m Theta(z))            per point and generator, Xi_m = Xi * mask
    loss = sum |u|^2 over points and generators, NOT divided by anything
    grad = 2 sum (u dth^T - (L^T u) th^T) * mask,                dth = J_Theta(z) L z

Next to (loss, grad) ``evaluate`` returns the YARDSTICKS: the same two sums with every term replaced by its absolute value,
``a = |jv| + |L h|`` standing where ``u`` stands (``jv = Xi_m dth``, ``h = Xi_m th``): sum a^2 and 2 sum (a |dth|^T + (|L|^T a)
|th|^T) * mask.  A float32 evaluation is judged against them, not against the result: for an equivariant field the result is
zero and its float32 value pure rounding.

``sequential``: every sum one term after the other in the tensor's dtype, points outermost, generators inside, as a single
thread would add them (the float32 replay of tests/test_host_symreg_linear_model.py); the matrix products too are then
written out as one multiply and one add per term.  Below fp64, sin, cos and exp are taken in fp64 and rounded, i.e. the
correctly rounded value of the dtype.  Together: the replay consists of IEEE operations alone and gives the same figures on
any CPU, whatever its BLAS kernels and vector math library do in float32.

``mutant`` switches ONE deliberate mistake on; None is the model.
"""
import torch

from oracle import sindy_oracle as O

PPT = {1: 4, 2: 2, 3: 4, 4: 1}                          # points per 16-byte chunk

MUTANTS = ("first_generator_only", "further_generators_transposed", "further_generators_stride_d", "l_u_for_lt_u", "grad_factor_1",
           "loss_divided_by_n_d", "mask_on_grad_not_on_xi", "mask_on_xi_not_on_grad", "last_ragged_point_dropped", "last_chunk_twice",
           "sine_derivative_sign", "exp_derivative_zero")


def terms(d, order, flags):
    return O.term_count(d, order, bool(flags & 1), bool(flags & 2))


def theta_jvp(z, v, order, flags, mutant=None):
    """(Theta(z), J_Theta(z) v), columns in the oracle's order: the product rule along the recurrence
    column(i1..in) = column(i1..i(n-1)) * z[in] that ``oracle.sindy_oracle.theta`` builds its columns with."""
    d = z.shape[-1]
    one = torch.ones(z.shape[0], dtype=z.dtype)
    cols, dcols = [one], [torch.zeros_like(one)]
    prev = {(i,): (z[:, i], v[:, i]) for i in range(d)}
    for i in range(d):
        cols.append(z[:, i])
        dcols.append(v[:, i])
    for n in range(2, order + 1):
        cur = {}
        for tup in O.poly_tuples(d, n):
            c, dc = prev[tup[:-1]]
            k = tup[-1]
            cur[tup] = (c * z[:, k], dc * z[:, k] + c * v[:, k])
            cols.append(cur[tup][0])
            dcols.append(cur[tup][1])
        prev = cur
    fn = lambda f, a: f(a.double()).to(a.dtype)  # noqa: E731
    if flags & 1:
        sign = -1.0 if mutant == "sine_derivative_sign" else 1.0
        for i in range(d):
            cols.append(fn(torch.sin, z[:, i]))
            dcols.append(sign * fn(torch.cos, z[:, i]) * v[:, i])
    if flags & 2:
        for i in range(d):
            e = fn(torch.exp, z[:, i])
            cols.append(e)
            dcols.append(torch.zeros_like(e) if mutant == "exp_derivative_zero" else e * v[:, i])
    return torch.stack(cols, dim=1), torch.stack(dcols, dim=1)


def _total(t, sequential):
    """Sum over the first axis; ``sequential``: one term after the other in the tensor's dtype."""
    if t.shape[0] == 0:
        return torch.zeros(t.shape[1:], dtype=t.dtype)
    return t.cumsum(0)[-1] if sequential else t.sum(0)


def _apply(a, B, sequential):
    """a (n, k) times B^T for B (m, k): a @ B.T; ``sequential``: sum_k a[:, k] B[j, k] one term after the other."""
    if not sequential:
        return a @ B.T
    out = []
    for j in range(B.shape[0]):
        t = a[:, 0] * B[j, 0]
        for k in range(1, a.shape[1]):
            t = t + a[:, k] * B[j, k]
        out.append(t)
    return torch.stack(out, dim=1)


def _generators(L, d, mutant):
    """The (n_gen, d, d) matrices the formula reads out of the flat row-major table."""
    n_gen = L.shape[0]
    if mutant == "first_generator_only":
        return L[:1]
    if mutant == "further_generators_transposed" and n_gen > 1:
        return torch.cat([L[:1], L[1:].transpose(1, 2)])
    if mutant == "further_generators_stride_d" and n_gen > 1:
        flat = L.reshape(-1)
        return torch.stack([flat[g * d:g * d + d * d].reshape(d, d) for g in range(n_gen)])
    return L


def _points(z, d, mutant):
    n = z.shape[0]
    ppt = PPT[d]
    if mutant == "last_ragged_point_dropped" and n % ppt:
        return z[:-1]
    if mutant == "last_chunk_twice" and n >= ppt:
        full = (n // ppt) * ppt
        return torch.cat([z, z[full - ppt:full]])
    return z


def evaluate(z, xi, mask, L, order, flags, dt=torch.float64, sequential=False, mutant=None):
    """z (n, d), xi (d, p), mask (d, p) or None, L (n_gen, d, d), all float32 (or anything) -> dict of ``loss``, ``grad`` (d, p),
    ``loss_yard``, ``grad_yard`` (d, p) in ``dt``."""
    d = z.shape[-1]
    n = z.shape[0]
    p = terms(d, order, flags)
    z, xi = _points(z.to(dt), d, mutant), xi.to(dt).reshape(d, p)
    mk = torch.ones(d, p, dtype=dt) if mask is None else mask.to(dt).reshape(d, p)
    W = xi if mutant == "mask_on_grad_not_on_xi" else xi * mk
    Ls = _generators(L.to(dt).reshape(-1, d, d), d, mutant)
    if Ls.shape[0] == 0:
        zero = torch.zeros((), dtype=dt)
        return dict(loss=zero, grad=torch.zeros(d, p, dtype=dt), loss_yard=zero.clone(), grad_yard=torch.zeros(d, p, dtype=dt))
    sq, ysq, gt, ygt = [], [], [], []
    for Lg in Ls:
        v = _apply(z, Lg, sequential)
        th, dth = theta_jvp(z, v, order, flags, mutant)
        h, jv = _apply(th, W, sequential), _apply(dth, W, sequential)
        lh = _apply(h, Lg, sequential)
        u = jv - lh
        a = jv.abs() + lh.abs()
        ltu = _apply(u, Lg if mutant == "l_u_for_lt_u" else Lg.T, sequential)
        lta = a @ Lg.abs()
        sq.append(u * u)
        ysq.append(a * a)
        gt.append(u[:, :, None] * dth[:, None, :] - ltu[:, :, None] * th[:, None, :])
        ygt.append(a[:, :, None] * dth.abs()[:, None, :] + lta[:, :, None] * th.abs()[:, None, :])
    flat = lambda parts: torch.stack(parts, dim=1).reshape(-1, 1)              # noqa: E731  points outermost, then generators
    rows = lambda parts: torch.stack(parts, dim=1).reshape(-1, d, p)            # noqa: E731
    loss, loss_yard = _total(flat(sq), sequential)[0], _total(flat(ysq), False)[0]
    factor = 1.0 if mutant == "grad_factor_1" else 2.0
    grad, grad_yard = factor * _total(rows(gt), sequential), 2.0 * _total(rows(ygt), False) * mk
    if mutant != "mask_on_xi_not_on_grad":
        grad = grad * mk
    if mutant == "loss_divided_by_n_d":
        loss = loss / (n * d)
    return dict(loss=loss, grad=grad, loss_yard=loss_yard, grad_yard=grad_yard)


def deviation(got_loss, got_grad, ref):
    """(loss, grad) deviation of a result from the fp64 model ``ref`` as fractions of the yardsticks: |loss - ref| / loss_yard
    and max |grad - ref| / max grad_yard.  A zero yardstick (no generator, a mask of zeros) demands the exact zero: inf else."""
    def frac(err, yard):
        if yard == 0.0:
            return 0.0 if err == 0.0 else float("inf")
        return err / yard
    dl = abs(float(got_loss) - float(ref["loss"]))
    dg = float((got_grad.double().reshape(ref["grad"].shape) - ref["grad"].double()).abs().max())
    if not (dl == dl and dg == dg):                                              # a NaN is no deviation to rank
        return float("inf"), float("inf")
    return frac(dl, float(ref["loss_yard"])), frac(dg, float(ref["grad_yard"].max()))
