"""Minibatch Adam fit on the --use_latent branch, time per step: the tensor-op loop against the device trainer.

    python tests/perf/e2e_adam_latent.py [--out profiles/adam_latent.txt]

Data: the damped oscillator by the reference's recipe size (250 trajectories x 500 samples = 125 000 rows, 20 % noise)
behind a small frozen autoencoder in eval mode (mlp, hidden 16, 2 layers, batch norm, D = d = 2), one so(2) generator,
order 2 and order 3, batch 256 (489 steps per epoch) and 4096 (31 steps), in one process:
  (a) the loop train_SIGED(use_latent=True) runs today, per minibatch: encoder pass, compute_dz, regressor, compute_dx, the
      two MSEs, model_utils.symmreg_linear, the L1 term, backward, torch.optim.Adam.step;
  (b) DeviceAdam(latent=...).fit: whole epochs per launch, shuffles and index tables included;
  (o) model_utils.latent_operands(per_row=True) over the whole set, once per fit, not part of (b).
HIP events around a block of steps (a: 20 steps, b: 2 epochs) divided by its steps; 3 warm-up blocks, median of 20.  No
threshold: the file records what was measured."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.perf.e2e_adam import DEV, dosc_rows  # noqa: E402

LR, W_Z, W_X, W_REG, W_SYM = 1e-3, 1.0, 1.0, 1e-2, 1e-4
WARMUP, REPS, LOOP_BLOCK, FIT_EPOCHS = 3, 20, 20, 2


class So2(torch.nn.Module):
    def get_full_basis_list(self):
        return [torch.tensor([[0.0, -1.0], [1.0, 0.0]], device=DEV)]


def autoencoder(x):
    from symode_amd.autoencoder import AutoEncoder
    torch.manual_seed(11)
    ae = AutoEncoder(ae_arch="mlp", input_dim=2, latent_dim=2, hidden_dim=16, n_layers=2, n_comps=1, batch_norm=True,
                     activation="ReLU").to(DEV)
    ae.train()
    with torch.no_grad():
        ae(x[::8])
    ae.eval()
    for q in ae.parameters():
        q.requires_grad = False
    return ae


def timed(block, steps):
    """us per step: HIP events around ``block()``, WARMUP blocks first, median of REPS."""
    times = []
    for k in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        block()
        b.record()
        b.synchronize()
        if k >= WARMUP:
            times.append(a.elapsed_time(b) * 1e3 / steps)
    return statistics.median(times)


def loop_step_us(S, x, dx, ae, gen, order, batch):
    from symode_amd.dataset import DeviceBatches
    from symode_amd.model_utils import symmreg_linear
    torch.manual_seed(0)
    reg = S.SINDyRegression(2, order, False, False, threshold=0.05, device=DEV)
    opt = torch.optim.Adam(reg.parameters(), lr=LR)
    loader = DeviceBatches([x, dx], x.shape[0], batch, True, DEV)
    batches = iter(())

    def block():
        nonlocal batches
        for _ in range(LOOP_BLOCK):
            item = next(batches, None)
            if item is None:
                batches = iter(loader)
                item = next(batches)
            xb, dxb = item
            z, _ = ae(xb)
            dz = ae.compute_dz(xb, dxb)
            dz_pred = reg(z)
            dx_pred = ae.compute_dx(z, dz_pred)
            loss = W_Z * torch.nn.functional.mse_loss(dz_pred, dz) + W_X * torch.nn.functional.mse_loss(dx_pred, dxb) \
                + W_SYM * symmreg_linear(z, reg, gen.get_full_basis_list()) + W_REG * sum(torch.norm(q, 1) for q in reg.parameters())
            opt.zero_grad()
            loss.backward()
            opt.step()

    return timed(block, LOOP_BLOCK)


def fit_step_us(S, x, ops, L, order, batch):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    z, dz, B, y, e, D = ops
    coef = CoefMap(2, S.get_engine().lib_size(2, order, 0))
    tr = DeviceAdam(z, dz, order, False, False, coef, LR, W_X, W_REG, 0.05, 100, batch, latent=(B, y, None, D, L, W_Z, W_SYM))
    init = coef.draw(torch.Generator().manual_seed(0))[None].to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)

    def block():
        tr.fit(init, FIT_EPOCHS, (torch.randperm(z.shape[0], generator=g, device=DEV)[None] for _ in range(FIT_EPOCHS)))

    return timed(block, FIT_EPOCHS * tr.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_latent.txt"))
    a = ap.parse_args()
    import symode_amd as S
    from symode_amd.model_utils import latent_operands
    x, dx = (t.to(DEV).contiguous() for t in dosc_rows())
    ae, gen = autoencoder(x), So2()
    ops = None

    def operands():
        nonlocal ops
        ops = latent_operands(x, dx, ae, per_row=True)

    o_us = timed(operands, 1)
    L = torch.stack(gen.get_full_basis_list()).contiguous()
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"rows {x.shape[0]}, D = d = 2, one so(2) generator, w_z {W_Z} w_x {W_X} w_sym {W_SYM}; us per minibatch step",
             f"HIP events around a block ((a) {LOOP_BLOCK} steps, (b) {FIT_EPOCHS} epochs) / its steps, {WARMUP} warm-up blocks, median of {REPS}",
             f"(o) latent_operands(per_row=True) over the whole set, once per fit (not in (b)): {o_us:.0f} us"]
    for order in (2, 3):
        for batch in (256, 4096):
            steps = (x.shape[0] + batch - 1) // batch
            a_us = loop_step_us(S, x, dx, ae, gen, order, batch)
            b_us = fit_step_us(S, x, ops, L, order, batch)
            lines.append(f"order {order} batch {batch} ({steps} steps per epoch): (a) tensor-op loop {a_us:.1f}   (b) DeviceAdam.fit {b_us:.2f}   "
                         f"(a) / (b) {a_us / b_us:.1f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
