"""The weak-SINDy seed sweep restated in fp64 on the host, with no GPU in it: windows -> Z = [G | b] -> N = Z^T M Z -> the
threshold loop on ``stlsq_solve_from_gram`` with gamma = fp32(sqrt(w_sindy_reg)), the value the device launch takes.  The
data of the fit tests are made here as well.  ``python -m tests.weak_sweep_model`` prints, for the per-seed route
(WSINDyWrapper + train_WSINDy on tests.oracle_engine.OracleEngine), the conditions the GPU fit test asserts on its inputs."""
import functools

import numpy as np
import torch

from symode_amd.engine import FLAG_EXP, FLAG_SINE
from symode_amd.sindy import near_threshold_cases, stlsq_solve_from_gram

N_ICS, N_STEPS, N_T, DT, K, ORDER = 6, 200, 160, 0.02, 50, 3
NOISE, DATA_SEED = 0.02, 0
FIT_POINTS = ((1e-4, 0.2), (1e-3, 0.3))                    # (w_sindy_reg, threshold)
MAX_ITER = 10


def theta(x, order, flags=0):
    from oracle import sindy_oracle as O
    return O.theta(x, order, bool(flags & FLAG_SINE), bool(flags & FLAG_EXP))


@functools.lru_cache(maxsize=None)
def dosc_data(n_ics=N_ICS, n_steps=N_STEPS, dt=DT, noise=NOISE, seed=DATA_SEED):
    """(n_ics, n_steps, 2) fp32: damped-oscillator trajectories (dx = -0.1 x - y, dy = x - 0.1 y, fp64 RK4 in torch on
    the CPU) from initial conditions on radius 0.5 .. 2, plus Gaussian noise of ``noise`` times the data's std."""
    gen = torch.Generator().manual_seed(seed)
    r = 0.5 + 1.5 * torch.rand(n_ics, generator=gen, dtype=torch.float64)
    th = 2 * np.pi * torch.rand(n_ics, generator=gen, dtype=torch.float64)
    A = torch.tensor([[-0.1, -1.0], [1.0, -0.1]], dtype=torch.float64)
    f = lambda z: z @ A.T                                                  # noqa: E731
    z = torch.stack([r * torch.cos(th), r * torch.sin(th)], dim=1)
    out = [z]
    for _ in range(n_steps - 1):
        k1 = f(z)
        k2 = f(z + 0.5 * dt * k1)
        k3 = f(z + 0.5 * dt * k2)
        k4 = f(z + dt * k3)
        z = z + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        out.append(z)
    x = torch.stack(out, dim=1)
    x = x + noise * x.std() * torch.randn(x.shape, generator=gen, dtype=torch.float64)
    return x.float()


def z_of_window(xw, V, V_drv, order, flags=0):
    """Z = [V Theta(x) | -V' x] (K, p+d) fp64 from the oracle's fp32 Theta: what the contraction computes, up to summation order."""
    G = V.double() @ theta(xw, order, flags).double()
    b = -V_drv.double() @ xw.double()
    return torch.cat([G, b], dim=1).numpy()


def normal(Z, M):
    return Z.T @ (M @ Z)


def normals(x3, windows, n_t, V, V_drv, M, order, flags=0):
    """(S, p+d, p+d) fp64: N of every window [trajectory, start]."""
    return np.stack([normal(z_of_window(x3[tr, st:st + n_t], V, V_drv, order, flags), M) for tr, st in np.asarray(windows).tolist()])


def fit(N, d, n_points, w_sindy_reg, threshold, max_iter=MAX_ITER):
    """The threshold loop on one window's N: Xi (d, p) fp32, mask bool, passes, near-threshold coefficients met."""
    p = N.shape[0] - d
    gamma = float(np.float32(np.sqrt(w_sindy_reg)))
    mask, near = np.ones((d, p), dtype=bool), 0
    for it in range(max_iter):
        xi, _ = stlsq_solve_from_gram(N, n_points, mask, gamma, d, "gels")
        xi32 = xi.astype(np.float32)
        near += len(near_threshold_cases(xi32, mask, threshold))
        new = np.logical_and(np.abs(xi32) > np.float32(threshold), mask)
        done = np.array_equal(new, mask)
        mask = new
        if done:
            break
    return xi32, mask, it + 1, near


def sweep(Ns, d, n_points, w_sindy_reg, threshold, max_iter=MAX_ITER):
    """``fit`` over (S, p+d, p+d): Xi (S, d, p) fp32, mask (S, d, p) bool, passes (S,), near (S,)."""
    out = [fit(N, d, n_points, w_sindy_reg, threshold, max_iter) for N in Ns]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def per_seed(x3, windows, n_t, dt, order, w_sindy_reg, threshold, device="cpu", engine=None, max_iter=MAX_ITER, k=K):
    """The per-seed route: WSINDyWrapper + the loop of train_WSINDy (driver gels) on every copied window.
    Xi (S, d, p) fp32, mask bool, passes, near: the coefficients within sindy.NEAR_THRESHOLD_BAND of the threshold, over all passes."""
    from symode_amd import sindy as S
    d = x3.shape[-1]
    out = []
    for tr, st in np.asarray(windows).tolist():
        xw = x3[tr, st:st + n_t].contiguous().to(device)
        reg = S.SINDyRegression(d, order, False, False, threshold=threshold, device=device, lstsq_driver="gels",
                                **({} if engine is None else {"engine": engine}))
        wr = S.WSINDyWrapper(reg, torch.arange(n_t) * dt, n_t * dt, num_test_funcs=k, device=device)
        near = 0
        for it in range(max_iter):
            before = reg.mask.detach().cpu().numpy() > 0
            _, conv = wr.solve(xw, w_sindy_reg, threshold, lstsq_driver="gels")
            near += len(near_threshold_cases(reg.Xi.detach().cpu().numpy(), before, threshold))
            if conv:
                break
        out.append((reg.Xi.detach().cpu().numpy().copy(), reg.mask.detach().cpu().numpy() > 0, it + 1, near))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def conditions(mask, passes, near):
    """What the fit tests assert of the per-seed side: no coefficient near the threshold, a seed with >= 2 passes, at least
    half the supports neither empty nor full."""
    size = mask.reshape(len(mask), -1).sum(axis=1)
    partial = int(((size > 0) & (size < mask[0].size)).sum())
    return bool((near == 0).all()), bool((passes >= 2).any()), 2 * partial >= len(mask)


if __name__ == "__main__":
    from symode_amd.sindy import weak_test_functions
    from symode_amd.sweep import weak_windows
    from tests.oracle_engine import OracleEngine
    x3 = dosc_data()
    win = weak_windows(range(8), N_ICS, N_STEPS, N_T)
    _, _, V, V_drv, M = weak_test_functions(torch.arange(N_T) * DT, N_T * DT, K, "trig", "cpu")
    Ns = normals(x3, win, N_T, V, V_drv, M, ORDER)
    for w, thr in FIT_POINTS:
        xi, mask, passes, near = per_seed(x3, win, N_T, DT, ORDER, w, thr, engine=OracleEngine())
        mxi, mmask, mpasses, _ = sweep(Ns, 2, N_T, w, thr)
        err = max(np.abs(a - b).max() / np.abs(a).max() for a, b in zip(xi, mxi))
        print((w, thr), "passes", passes.tolist(), "support", mask.reshape(8, -1).sum(1).tolist(), "near", near.tolist(),
              "conditions", conditions(mask, passes, near), "model: masks", np.array_equal(mask, mmask), "passes",
              np.array_equal(passes, mpasses), "err %.3g" % err,
              "cond(G^T M G + w I) <= %.3g" % max(np.linalg.cond(N[:-2, :-2] + w * np.eye(len(N) - 2)) for N in Ns))
