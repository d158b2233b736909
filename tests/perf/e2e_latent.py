"""The latent closure kernel against the fused reversed closure, and the latent fit on the fused route against host_params.

    python tests/perf/e2e_latent.py [--out profiles/latent_closure.txt] [--problems 8192] [--epochs 10]

One process:
  (a) symode_loss_grad_latent against symode_loss_grad_reversed at n_g = 1 on the SAME buffers (z = x, dz = dx, y = g(x),
      B = J_g(x): both read 40 bytes per point at d = 2, the latent kernel evaluates the library once per point, the
      reversed one twice) at the bench shape: 50 x 2500 points per problem, d = 2, orders 3 and 5, `--problems` resident
      problems.  HIP events around one launch, 3 warm-up launches, 20 timed launches alternating the two kernels; median
      and min.  The yardstick is the reversed closure of this build in this run: exit status 1 if the latent kernel's
      median is above the reversed kernel's by more than the larger of the two spreads (max - min of the 20 launches).
  (b) train_SIGED_lbfgs(use_latent=True) on 125 000 damped-oscillator points through a near-identity 2 -> 2 autoencoder,
      `--epochs` epochs, nothing logged or saved inside the call: fused_latent=True against the host_params route, wall clock
      around the synchronised call (operands included), one warm-up call each, median of 3.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"


def kernel_times(eng, order, n_problems, n, reps=20, warm=3):
    g = torch.Generator(device=DEV).manual_seed(order)
    z = torch.randn(n_problems, n, 2, generator=g, device=DEV)
    dz = torch.randn(n_problems, n, 2, generator=g, device=DEV)
    y = torch.randn(n_problems, n, 2, generator=g, device=DEV)
    B = torch.randn(n_problems, n, 2, 2, generator=g, device=DEV)
    p = eng.lib_size(2, order, 0)
    xi = 0.3 * torch.randn(n_problems, 2, p, generator=g, device=DEV)
    mask = torch.ones_like(xi)
    out_l = (torch.empty(n_problems, 2, device=DEV), torch.empty(n_problems, 2, p, device=DEV))
    out_r = (torch.empty(n_problems, 2, device=DEV), torch.empty(n_problems, 2, p, device=DEV))
    calls = {"latent": lambda: eng.loss_grad_latent(z, dz, B, y, xi, mask, order, 0, w_pair=0.5, out=out_l),
             "reversed": lambda: eng.loss_grad_reversed(z, dz, y[:, None], B[:, None], xi, mask, order, 0, w_sym=0.5, out=out_r)}
    times = {k: [] for k in calls}
    for it in range(warm + reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warm:
                times[k].append(a.elapsed_time(b) * 1e3)
    return times, n_problems * n * 40


def fit_seconds(S, x, dx, ae, fused, epochs):
    torch.manual_seed(0)
    reg = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
    ident = torch.nn.Identity()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S.train.train_SIGED_lbfgs(
        train_loader=[(x, dx)], test_loader=[], num_epochs=epochs, device=DEV, log_interval=10 ** 9, save_interval=10 ** 9,
        save_dir="perf", autoencoder=ae, generator=ident, regressor=reg, regressor_dst=None, use_latent=True,
        distill_latent=False, lr_sindy=0.1, w_sindy_z=1.0, w_sindy_x=0.5, sindy_reg_type="l1", w_sindy_reg=1e-3,
        sym_reg_type="i", w_sym_reg=0.0, st_freq=100, threshold=0.05, int_t=0.1, int_dt=0.01, print_eq=False,
        fused_latent=fused)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_closure.txt"))
    ap.add_argument("--problems", type=int, default=8192)
    ap.add_argument("--points", type=int, default=50 * 2500)
    ap.add_argument("--epochs", type=int, default=10)
    a = ap.parse_args()
    import symode_amd as S
    from oracle import sindy_oracle as O
    from tests.latent_cases import near_identity_autoencoder
    eng = S.get_engine()
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"(a) one launch, HIP events, 3 warm-up + 20 timed launches alternating the two kernels; {a.problems} problems x "
             f"{a.points} points, d = 2, the same buffers for both kernels (40 B/point)"]
    ok = True
    for order in (3, 5):
        t, nbytes = kernel_times(eng, order, a.problems, a.points)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(max(v) - min(v) for v in t.values())
        for k, v in t.items():
            lines.append(f"  order {order} {k:9s} median {med[k]:10.1f} us  min {min(v):10.1f} us  max {max(v):10.1f} us  "
                         f"{nbytes / med[k] / 1e6:6.2f} TB/s at the median")
        slower = med["latent"] - med["reversed"]
        lines.append(f"  order {order} latent - reversed (median) {slower:+.1f} us; spread of the 20 launches {spread:.1f} us")
        ok = ok and slower <= spread
        torch.cuda.empty_cache()
    rng = np.random.RandomState(0)
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(250, rng), 0.02, 500)
    x = torch.from_numpy(xs.reshape(-1, 2)).float().to(DEV)
    dx = torch.from_numpy(dxs.reshape(-1, 2)).float().to(DEV) + 0.01 * torch.randn(x.shape, device=DEV)
    ae = near_identity_autoencoder(0, device=DEV)
    lines.append(f"(b) train_SIGED_lbfgs(use_latent=True), {x.shape[0]} points, order 3, {a.epochs} epochs, wall clock around the "
                 f"synchronised call, one warm-up call, median of 3")
    fit = {}
    for name, fused in (("host_params", False), ("fused_latent", True)):
        fit_seconds(S, x, dx, ae, fused, a.epochs)
        fit[name] = statistics.median(fit_seconds(S, x, dx, ae, fused, a.epochs) for _ in range(3))
        lines.append(f"  {name:12s} {fit[name]:8.3f} s  ({fit[name] / a.epochs * 1e3:8.2f} ms per epoch)")
    lines.append(f"  host_params / fused_latent = {fit['host_params'] / fit['fused_latent']:.2f}")
    lines.append(f"latent kernel no slower than the reversed closure beyond the spread: {ok}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
