"""Minibatch Adam fit, wall time per epoch: the tensor-op loop of train_SIGED against the device trainer.

    python tests/perf/e2e_adam.py [--out profiles/adam_trainer.json] [--quick]

Data: the damped oscillator by the reference's recipe size (250 trajectories x 500 samples = 125 000 rows, 20 % noise),
orders 2 and 5, batch 256 (489 steps per epoch) and 8192 (16 steps), in one process:
  (a) train.train_SIGED as it is by default: one Python iteration per minibatch;
  (b) train.train_SIGED(device_adam=True): whole epochs per launch (16 at a time when nothing is logged in between);
  (k) the bare symode_adam_epochs launch on a prepared index table, HIP events: us per minibatch step of the kernel,
      for one problem and for 64 problems with their own shuffles;
  (s) DeviceAdam.fit for 64 seeds with their own shuffles (keys from 64 generators, one argsort per epoch, as main_sweep
      draws them) against 64 x (b).
(a) and (b) are wall clock around the whole call (synchronised), divided by the epochs of the call, median over repeated
calls after one warm-up call; neither logs, evaluates the test loss or saves inside the timed call.  The yardstick is (a)
in the same run: (b) must be faster than (a) at batch 256, and (s) must cost less than 64 x (b); exit status 1 otherwise.
Kernel registers / LDS / scratch for the record come from a separate rocprofv3 --kernel-trace --stats run with --quick.
"""
import argparse
import json
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


def dosc_rows(n_ics=250, n_steps=500, noise=0.2):
    from oracle import sindy_oracle as O
    rng = np.random.RandomState(0)
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(n_ics, rng), 0.02, n_steps)
    xs = xs + noise * xs.std() * rng.randn(*xs.shape)
    return torch.from_numpy(xs.reshape(-1, 2)).float(), torch.from_numpy(dxs.reshape(-1, 2)).float()


def train_call(S, x, dx, order, batch, epochs, device_adam):
    from symode_amd.dataset import DeviceBatches
    torch.manual_seed(0)
    reg = S.SINDyRegression(2, order, False, False, threshold=0.05, device=DEV)
    loader = DeviceBatches([x, dx], x.shape[0], batch, True, DEV)
    ident = torch.nn.Identity()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S.train.train_SIGED(train_loader=loader, test_loader=[], num_epochs=epochs, device=DEV, log_interval=10 ** 9,
                        save_interval=10 ** 9, save_dir="perf", autoencoder=ident, discriminator=ident, generator=ident, lr_ae=0,
                        lr_d=0, lr_g=0, w_recon=0, w_gan=0, w_reg_norm=0, w_reg_ortho=0, w_reg_closure=0, use_original_x=False,
                        gan_st_freq=0, gan_st_thres=0.0, ae_arch="none", regressor=reg, use_latent=False, lr_sindy=1e-3,
                        w_sindy_z=0.0, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=1e-2, w_sym_reg=0.0, st_freq=100,
                        threshold=0.05, int_t=0.1, int_dt=0.01, device_adam=device_adam)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs * 1e6


def median_epoch_us(fn, reps):
    fn()
    return statistics.median(fn() for _ in range(reps))


def kernel_step_us(S, x, dx, order, batch, n_problems, epochs, reps=5):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    eng = S.get_engine()
    p = eng.lib_size(2, order, 0)
    tr = DeviceAdam(x, dx, order, False, False, CoefMap(2, p), 1e-3, 1.0, 1e-2, 0.05, 100, batch)
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = torch.stack([tr.table(torch.argsort(torch.rand(n_problems, x.shape[0], generator=g, device=DEV), dim=1))
                       for _ in range(epochs)]).contiguous()
    params = (torch.randn(n_problems, 2 * p, generator=torch.Generator().manual_seed(1)) * 0.3).to(DEV)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step, mask = torch.zeros(n_problems, dtype=torch.int32, device=DEV), torch.ones(n_problems, 2, p, device=DEV)

    def launch():
        eng.adam_epochs(x, dx, idx, params, m, v, step, mask, order, 0, lr=1e-3, w_reg=1e-2, threshold=0.05, st_freq=100)
    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times) / (epochs * tr.steps), tr.steps


def sweep_epoch_us(S, x, dx, order, batch, n_seeds, epochs, reps):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    p = S.get_engine().lib_size(2, order, 0)
    coef = CoefMap(2, p)
    tr = DeviceAdam(x, dx, order, False, False, coef, 1e-3, 1.0, 1e-2, 0.05, 100, batch)
    inits = torch.stack([coef.draw(torch.Generator().manual_seed(s)) for s in range(n_seeds)]).to(DEV)
    keys = torch.empty(n_seeds, x.shape[0], device=DEV)

    def call():
        gens = [torch.Generator(device=DEV).manual_seed(s) for s in range(n_seeds)]

        def orders():
            for _ in range(epochs):
                for k, g in enumerate(gens):
                    torch.rand(x.shape[0], generator=g, out=keys[k])
                yield torch.argsort(keys, dim=1, stable=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.fit(inits, epochs, orders())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / epochs * 1e6
    return median_epoch_us(call, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_trainer.json"))
    ap.add_argument("--quick", action="store_true", help="device path and bare launches only, one repetition (for a kernel trace)")
    a = ap.parse_args()
    import symode_amd as S
    x, dx = (t.to(DEV).contiguous() for t in dosc_rows())
    res = {"device": torch.cuda.get_device_name(0), "rows": x.shape[0],
           "timing": "(a), (b), (s): wall clock around the synchronised call / epochs, one warm-up call, median of the repeated "
                     "calls; (k): HIP events around one launch of 16 epochs, one warm-up, median of 5"}
    ok = True
    for order in (2, 5):
        for batch in (256, 8192):
            r = {}
            if not a.quick:
                r["a_tensor_op_epoch_us"] = median_epoch_us(lambda: train_call(S, x, dx, order, batch, 2, False), 3)
            r["b_device_adam_epoch_us"] = median_epoch_us(lambda: train_call(S, x, dx, order, batch, 16, True), 1 if a.quick else 5)
            k1, steps = kernel_step_us(S, x, dx, order, batch, 1, 16, 1 if a.quick else 5)
            k64, _ = kernel_step_us(S, x, dx, order, batch, 64, 16, 1 if a.quick else 5)
            r.update(steps_per_epoch=steps, k_kernel_step_us_1_problem=k1, k_kernel_step_us_64_problems=k64)
            if not a.quick:
                r["a_over_b"] = r["a_tensor_op_epoch_us"] / r["b_device_adam_epoch_us"]
                r["a_step_us"] = r["a_tensor_op_epoch_us"] / steps
                r["b_step_us"] = r["b_device_adam_epoch_us"] / steps
                if batch == 256:
                    r["s_64_seeds_epoch_us"] = sweep_epoch_us(S, x, dx, order, batch, 64, 16, 3)
                    r["s_over_64_b"] = r["s_64_seeds_epoch_us"] / (64 * r["b_device_adam_epoch_us"])
                    ok = ok and r["a_over_b"] > 1.0 and r["s_over_64_b"] < 1.0
            res[f"order{order}_batch{batch}"] = r
            print(f"order {order} batch {batch}", json.dumps(r), flush=True)
    if not a.quick:
        res["device_path_faster_at_batch_256_and_64_seeds_cheaper_than_64_fits"] = bool(ok)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
