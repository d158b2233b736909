"""The deck of the STLSQ tests with the reversed symmetry regulariser, with no GPU in it.  Every case is a pair (G, R) of raw
fp64 sums: G = [Theta | dx]^T [Theta | dx] and R = sum_g sum_n B^T B, B[i, (j, a)] = J_g[i, j] theta_a(x) - [i == j] theta_a(g x)
(the regulariser as gram_closure states it), rows and columns of R in Xi's (d, p) row-major order.

  osc_*      the damped oscillator dx = [[-0.1, -1], [1, -0.1]] x, N_POINTS seeded points in [-1, 1]^2 rounded to fp32,
             targets with 50 % relative noise, two rotations as group elements (the system commutes with them): orders 2, 3
             and 5 (n = 12, 20, 42) and order 2 plus exp (p = 8);
  osc3_o3    its d = 3 extension (a decaying third coordinate, rotations about its axis), order 3: n = 60;
  spd_*      a random positive definite pair with no compiled library behind it, at the lane limit n = d p = 64: d = 4, p = 16
             and d = 1, p = 64.  The targets follow a sparse model v, and R = B^T B with B v = 0, so the regulariser agrees
             with the model as a symmetry would.

``python -m tests.stlsq_symreg_cases`` prints what the CPU test asserts on the deck; the seeds were chosen with it."""
import functools

import numpy as np
import torch

N_POINTS, NOISE, BAND = 400, 0.5, 1e-4
THRESHOLD = 0.05
GAMMAS = (0.0, 0.1)
W_SYMS = (0.0, 0.1, 1.0, 10.0)
MAX_ITERS = (1, 2, 10)
COND_BOUND = 1e6            # of every pass's system; with n <= 64 the solve's term of the bound stays under 2e-6 max|v|
GAP = 100                   # no coefficient of a deciding pass within GAP * bound of the threshold
ANGLES = (0.4, 1.3)
# name -> (d, order, include_exp, seed)
OSC = {"osc_o2": (2, 2, False, 0), "osc_o3": (2, 3, False, 0), "osc_o5": (2, 5, False, 0), "osc_o2_exp": (2, 2, True, 0),
       "osc3_o3": (3, 3, False, 0)}
# name -> (d, p, seed)
SPD = {"spd_d4_p16": (4, 16, 0), "spd_d1_p64": (1, 64, 0)}
DECK = tuple(OSC) + tuple(SPD)


def _rotation(d, angle):
    J = np.eye(d)
    J[:2, :2] = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
    return J


def rev_gram(th, thgs, Js):
    """sum_g sum_n B^T B in fp64: th (N, p) the library at x, thgs[g] (N, p) at g x, Js[g] (N, d, d) or (d, d) the Jacobian."""
    N, p = th.shape
    d = Js[0].shape[-1]
    R = np.zeros((d * p, d * p))
    for thg, J in zip(thgs, Js):
        J = np.broadcast_to(J, (N, d, d))
        B = J[:, :, :, None] * th[:, None, None, :] - np.eye(d)[None, :, :, None] * thg[:, None, None, :]      # (N, i, j, a)
        B = B.reshape(N * d, d * p)
        R += B.T @ B
    return R


@functools.lru_cache(maxsize=None)
def pair(name, variant=0):
    """(G (p+d, p+d), R (d p, d p), d) of the case, fp64.  ``variant``: another draw of points and noise (the sets of a table)."""
    if name in SPD:
        d, p, seed = SPD[name]
        rng = np.random.RandomState(1000 + seed + 7 * d + 100 * variant)
        A = rng.randn(600, p + d)
        A[:, 0] = 1.0
        v = rng.uniform(0.6, 1.5, (d, p)) * rng.choice([-1.0, 1.0], (d, p))
        v[:, 1::2] = 0.02 * rng.choice([-1.0, 1.0], v[:, 1::2].shape)           # every other entry is under the threshold
        A[:, p:] = A[:, :p] @ v.T + 0.1 * rng.randn(600, d)
        B = 0.3 * rng.randn(300, d * p)
        vf = v.reshape(-1)
        B -= np.outer(B @ vf, vf) / (vf @ vf)
        return A.T @ A, B.T @ B, d
    from oracle import sindy_oracle as O
    d, order, exp, seed = OSC[name]
    rng = np.random.RandomState(seed + 10 * order + d + 100 * variant)
    x = rng.uniform(-1.0, 1.0, (N_POINTS, d)).astype(np.float32)
    M = np.zeros((d, d))
    M[:2, :2] = [[-0.1, -1.0], [1.0, -0.1]]
    if d == 3:
        M[2, 2] = -0.3
    dx = x.astype(np.float64) @ M.T
    dx = (dx + NOISE * dx.std() * rng.randn(N_POINTS, d)).astype(np.float32)
    th = O.theta(torch.from_numpy(x), order, False, exp).double().numpy()
    Js = [_rotation(d, a) for a in ANGLES]
    thgs = [O.theta(torch.from_numpy((x.astype(np.float64) @ J.T).astype(np.float32)), order, False, exp).double().numpy() for J in Js]
    a = np.concatenate([th, dx.astype(np.float64)], axis=1)
    return a.T @ a, rev_gram(th, thgs, Js), d


@functools.lru_cache(maxsize=None)
def modelled(name, gamma, w_sym, max_iter):
    """(the model's result, its trace) on the case: computed once, shared by the CPU and the GPU tests."""
    from tests import stlsq_symreg_model as M
    G, R, d = pair(name)
    trace = []
    out = M.sweep(G, R, d, gamma, THRESHOLD, w_sym, max_iter, band=BAND, trace=trace)
    return out, trace


def truth(name):
    """The oscillator's true support (d, p) bool."""
    d, order, exp, _ = OSC[name]
    p = pair(name)[0].shape[0] - d
    m = np.zeros((d, p), dtype=bool)
    m[0, 1], m[0, 2], m[1, 1], m[1, 2] = True, True, True, True
    if d == 3:
        m[2, 3] = True
    return m


if __name__ == "__main__":
    from tests import stlsq_symreg_model as M
    for name in DECK:
        G, R, d = pair(name)
        for gamma in GAMMAS:
            for w in W_SYMS:
                out, trace = modelled(name, gamma, w, 10)
                conds = [np.linalg.cond(t[2]) if t[4] else 1.0 for t in trace]
                gaps = []
                for t in trace:
                    if t[4]:
                        v = np.array([t[1][j, k] for j, k in t[4]], dtype=np.float64)
                        gaps.append((np.abs(np.abs(v) - M.f32(THRESHOLD)) / M.xi_bound(v, np.linalg.cond(t[2]), len(v))).min())
                ok = "" if name in SPD else " truth %s" % bool(np.array_equal(out["mask"], truth(name)))
                print(name, "gamma", gamma, "w_sym", w, "passes", out["passes"], "near", out["near"], "fell", out["fell"], "n",
                      [len(t[4]) for t in trace], "cond %.3g" % max(conds), "min gap / bound %.3g" % min(gaps) + ok)
