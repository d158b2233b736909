"""Shared by the latent-closure tests (test infrastructure, not product code): a plain torch restatement of the formula of
symode_loss_grad_latent, seeded autoencoders, and the one fit case of tests/test_gpu_latent.py."""
import numpy as np
import torch

from oracle import sindy_oracle as O


def closure_from_operands(z, dz, B, y, Xi, mask, order, w_pair, sine=False, exp=False):
    """(loss2 (2,), grad (d, p)) as include/symode.h states them, in the dtype of the operands:
    loss2 = (mean |h - dz|^2, mean |B h - y|^2) both under 1 / (n d), grad = d(loss2[0] + w_pair loss2[1]) / dXi, masked."""
    Xi = Xi.detach().clone().requires_grad_(True)
    n, d = z.shape
    with torch.enable_grad():
        h = O.theta(z, order, sine, exp) @ (Xi * mask).T
        l0 = (h - dz).square().sum() / (n * d)
        l1 = (torch.einsum("nab,nb->na", B, h) - y).square().sum() / (n * d)
        (g,) = torch.autograd.grad(l0 + w_pair * l1, Xi)
    return torch.stack([l0.detach(), l1.detach()]), g


def seeded_autoencoder(input_dim, latent_dim, n_comps, seed, hidden=16, dtype=torch.float32, device="cpu"):
    """A small random 'mlp' autoencoder, batch norm on with non-trivial running statistics, frozen, in eval mode."""
    from symode_amd.autoencoder import AutoEncoder
    torch.manual_seed(seed)
    ae = AutoEncoder(ae_arch="mlp", input_dim=input_dim, hidden_dim=hidden, latent_dim=latent_dim, n_layers=2, n_comps=n_comps,
                     activation="Tanh", activation_args=[], batch_norm=True, ortho_ae=False)
    with torch.no_grad():
        for m in ae.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.1 * torch.randn_like(m.running_mean))
                m.running_var.copy_(1.0 + 0.5 * torch.rand_like(m.running_var))
                m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                m.bias.copy_(0.1 * torch.randn_like(m.bias))
    for p in ae.parameters():
        p.requires_grad = False
    return ae.to(device=device, dtype=dtype).eval()


def near_identity_autoencoder(seed, hidden=8, device="cpu"):
    """2 -> 2 'mlp' autoencoder, one hidden Tanh layer, whose encoder and decoder are seeded perturbations of the identity
    (tanh in its near-linear range): invertible-ish, so the latent dynamics of a polynomial system stay close to polynomial
    and the fitted coefficients stay O(1).  Frozen, eval mode."""
    from symode_amd.autoencoder import AutoEncoder
    torch.manual_seed(seed)
    ae = AutoEncoder(ae_arch="mlp", input_dim=2, hidden_dim=hidden, latent_dim=2, n_layers=1, n_comps=1, activation="Tanh",
                     activation_args=[], batch_norm=True, ortho_ae=False)
    with torch.no_grad():
        for seq in (ae.encoder, ae.decoder):
            lin = [m for m in seq.modules() if isinstance(m, torch.nn.Linear)]
            lin[0].weight.copy_(0.05 * torch.randn(hidden, 2))
            lin[0].weight[:2] += 0.3 * torch.eye(2)
            lin[0].bias.zero_()
            lin[1].weight.copy_(0.05 * torch.randn(2, hidden))
            lin[1].weight[:, :2] += torch.eye(2) / 0.3
            lin[1].bias.zero_()
    for p in ae.parameters():
        p.requires_grad = False
    return ae.to(device).eval()


def random_points(n, n_comps, input_dim, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    shape = (n, n_comps, input_dim) if n_comps > 1 else (n, input_dim)
    return torch.randn(*shape, generator=g).to(dtype), torch.randn(*shape, generator=g).to(dtype)


# ------------------------------------------------------------------------ the fit case
# Chosen on the CPU ('plain' route, oracle engine, twice): masks repeat, no coefficient within 1e-3 of the threshold at
# any event, final convergence at epoch 7.  The L1 weight is 0 (the term stays in the records): with 1e-3 the masked raw
# parameters drift through the L-BFGS memory under sign flips of their L1 gradient and loss_sindy_reg jumps between 2.5
# and 38 from epoch to epoch on the existing host_params route itself -- a chaotic case, not an admissible one.
FIT = dict(order=2, threshold=0.05, st_freq=10, epochs=30, lr=0.1, w_sindy_z=1.0, w_sindy_x=0.5, w_sindy_reg=0.0, seed=3,
           noise=0.01, n_ics=8, n_steps=250, dt=0.02)


def fit_data():
    """Damped oscillator, 2 000 points, derivative noise FIT['noise']; fitted through near_identity_autoencoder."""
    rng = np.random.RandomState(FIT["seed"])
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(FIT["n_ics"], rng), FIT["dt"], FIT["n_steps"])
    x = torch.from_numpy(xs.reshape(-1, 2)).float()
    dx = torch.from_numpy(dxs.reshape(-1, 2)).float()
    dx = dx + FIT["noise"] * torch.from_numpy(rng.randn(*dx.shape)).float()
    Xi0 = 0.1 * torch.from_numpy(rng.randn(2, 6)).float()
    return x, dx, Xi0


def run_fit(symode_amd, device, engine=None, fused_latent=False, host_lbfgs=True):
    """train_SIGED_lbfgs(use_latent=True) on the fit case: (regressor, stdout-independent list of logged records)."""
    x, dx, Xi0 = fit_data()
    ae = near_identity_autoencoder(FIT["seed"], device=device)
    kw = {} if engine is None else {"engine": engine}
    r = symode_amd.SINDyRegression(2, FIT["order"], False, False, threshold=FIT["threshold"], device=device, **kw)
    r.Xi.data = Xi0.to(device)
    ident = torch.nn.Identity()
    symode_amd.train.train_SIGED_lbfgs(
        train_loader=[(x.to(device), dx.to(device))], test_loader=[(x, dx)], num_epochs=FIT["epochs"], device=device,
        log_interval=2, save_interval=10 ** 9, save_dir="latent", autoencoder=ae, generator=ident, regressor=r,
        regressor_dst=None, use_latent=True, distill_latent=False, lr_sindy=FIT["lr"], w_sindy_z=FIT["w_sindy_z"],
        w_sindy_x=FIT["w_sindy_x"], sindy_reg_type="l1", w_sindy_reg=FIT["w_sindy_reg"], sym_reg_type="i", w_sym_reg=0.0,
        st_freq=FIT["st_freq"], threshold=FIT["threshold"], int_t=0.1, int_dt=0.01, print_eq=False, host_lbfgs=host_lbfgs,
        fused_latent=fused_latent)
    return r


def events(stdout):
    """The convergence / thresholding / NaN messages of a transcript, in order."""
    keys = ("Convergence reached", "Max number of LBFGS", "Final convergence", "NaN encountered")
    return [line for line in stdout.splitlines() if any(k in line for k in keys)]
