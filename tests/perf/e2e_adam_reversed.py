"""Minibatch Adam fit under the reversed symmetry regulariser, wall time per step: a tensor-op loop against the device trainer.

    python tests/perf/e2e_adam_reversed.py [--out profiles/adam_reversed_e2e.txt]

Data: the damped oscillator by the reference's recipe size (250 trajectories x 500 samples = 125 000 rows, 20 % noise),
order 3, one synthetic LINEAR group element g(x) = exp(0.01 so2) x behind an identity autoencoder of stock layers (so
model_utils takes its usual route through encoder, group element and decoder), w_sym 0.1, batch 256 (489 steps per epoch)
and 4096 (31 steps), in one process:
  (a) the loop a user has today: per minibatch  w_x * mse + w_sym * model_utils.symmreg_r + w_reg * l1,  backward,
      torch.optim.Adam.step on a SINDyRegression (symmreg_r computes g(x), J_g(x) of each new batch, then one fused launch);
  (b) DeviceAdam(reversed_sym=...).fit: g(x), J_g(x) once over the data set (timed apart), then whole epochs per launch;
  (k) the bare symode_adam_epochs_reversed launch of 16 epochs on a prepared index table, HIP events.
(a) and (b) are wall clock around the synchronised call divided by its steps, median over repeated calls after one warm-up
call.  No threshold: the file records what was measured."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.perf.e2e_adam import DEV, dosc_rows, median_epoch_us  # noqa: E402

ORDER, LR, W_X, W_REG, W_SYM = 3, 1e-3, 1.0, 1e-2, 0.1


class LinearAE(torch.nn.Module):
    """encode = decode = identity, from the layers mlp_jvp covers; z_mean is the (zero) bias of encoder[-2]."""

    def __init__(self, d):
        super().__init__()
        def eye():
            lin = torch.nn.Linear(d, d)
            with torch.no_grad():
                lin.weight.copy_(torch.eye(d))
                lin.bias.zero_()
            return lin
        self.encoder = torch.nn.Sequential(eye(), torch.nn.Identity())
        self.decoder = torch.nn.Sequential(eye())
        for q in self.parameters():
            q.requires_grad = False

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z):
        return self.decoder(z)


class Rotation(torch.nn.Module):
    """One group element exp(scale * so2) on each of the two components of the stacked latent."""

    def __init__(self, device=DEV):
        super().__init__()
        self.device = device

    def get_deterministic_group_elems(self, split_channel=False, scale=1.0):
        L = torch.tensor([[0.0, 1.0], [-1.0, 0.0]], device=self.device)
        return [torch.block_diag(*[torch.matrix_exp(scale * L)] * 2)]


def loop_step_us(S, x, dx, ae, gen, batch, max_steps):
    from symode_amd.dataset import DeviceBatches
    from symode_amd.model_utils import symmreg_r
    torch.manual_seed(0)
    reg = S.SINDyRegression(2, ORDER, False, False, threshold=0.05, device=DEV)
    opt = torch.optim.Adam(reg.parameters(), lr=LR)
    loader = DeviceBatches([x, dx], x.shape[0], batch, True, DEV)
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    for xb, dxb in loader:
        xb = xb.contiguous()
        loss = W_X * reg.mse_loss(xb, dxb) + W_SYM * symmreg_r(xb, ae, gen, reg, require_grad=True) \
            + W_REG * sum(torch.norm(q, 1) for q in reg.parameters())
        opt.zero_grad()
        loss.backward()
        opt.step()
        steps += 1
        if steps == max_steps:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def device_trainer(S, x, dx, rev, batch):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    p = S.get_engine().lib_size(2, ORDER, 0)
    coef = CoefMap(2, p)
    return DeviceAdam(x, dx, ORDER, False, False, coef, LR, W_X, W_REG, 0.05, 100, batch, reversed_sym=rev), coef


def fit_step_us(S, x, dx, rev, batch, epochs):
    tr, coef = device_trainer(S, x, dx, rev, batch)
    init = coef.draw(torch.Generator().manual_seed(0))[None].to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.fit(init, epochs, (torch.randperm(x.shape[0], generator=g, device=DEV)[None] for _ in range(epochs)))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (epochs * tr.steps) * 1e6


def kernel_step_us(S, x, dx, rev, batch, epochs=16, reps=5):
    tr, coef = device_trainer(S, x, dx, rev, batch)
    eng = S.get_engine()
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = torch.stack([tr.table(torch.randperm(x.shape[0], generator=g, device=DEV)[None]) for _ in range(epochs)]).contiguous()
    params = coef.draw(torch.Generator().manual_seed(0))[None].to(DEV).contiguous()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step, mask = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, 2, coef.p, device=DEV)
    times = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.adam_epochs_reversed(x, dx, rev[0], rev[1], idx, params, m, v, step, mask, ORDER, 0, w_sym=rev[2], lr=LR, w_x=W_X,
                                 w_reg=W_REG, threshold=0.05, st_freq=100)
        b.record()
        b.synchronize()
        if k:
            times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times) / (epochs * tr.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_reversed_e2e.txt"))
    a = ap.parse_args()
    import symode_amd as S
    from symode_amd.model_utils import symmetry_operands
    x, dx = (t.to(DEV).contiguous() for t in dosc_rows())
    ae, gen = LinearAE(2).to(DEV), Rotation()
    rows = torch.arange(x.shape[0], device=DEV)[None]
    symmetry_operands(x[:4096], rows[:, :4096], ae, gen)                      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, gx, jgx, _, _ = symmetry_operands(x, rows, ae, gen)
    torch.cuda.synchronize()
    pre_us = (time.perf_counter() - t0) * 1e6
    rev = (gx, jgx, W_SYM)
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"rows {x.shape[0]}, d 2, order {ORDER}, one linear group element, w_sym {W_SYM}; us per minibatch step",
             "(a), (b): wall clock around the synchronised call / steps, one warm-up call, median of 3; (k): HIP events around",
             "one launch of 16 epochs, one warm-up, median of 5",
             f"g(x), J_g(x) over the whole set, once per fit (not in (b)): {pre_us:.0f} us"]
    for batch in (256, 4096):
        steps = (x.shape[0] + batch - 1) // batch
        a_us = median_epoch_us(lambda: loop_step_us(S, x, dx, ae, gen, batch, 200), 3)
        b_us = median_epoch_us(lambda: fit_step_us(S, x, dx, rev, batch, 16), 3)
        k_us = kernel_step_us(S, x, dx, rev, batch)
        lines.append(f"batch {batch} ({steps} steps per epoch): (a) tensor-op loop {a_us:.1f}   (b) DeviceAdam.fit {b_us:.2f}   "
                     f"(k) kernel alone {k_us:.2f}   (a) / (b) {a_us / b_us:.1f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:5]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
