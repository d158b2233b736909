"""Training loops of the SINDy path -- the ``train_*(**args)`` surface of the reference's train.py.

Control flow (epochs, convergence tests, thresholding events, optimizer resets, NaN guard,
checkpoint names) follows train.py:382-887 statement by statement; the arithmetic inside the
closures runs on the HIP engine:

  * ``MSELoss()(regressor(x), dx)`` + backward  ->  ``regressor.mse_loss(x, dx)``: ONE fused kernel
    (Theta never materialised), the Xi-gradient comes out of the same pass;
  * ``odeint`` / jvp-through-odeint of the symmetry terms -> fused integrator / analytic tangent flow;
  * ``solve_SINDy_one_step`` -> fp64 Gram (MFMA) + host solve.

``train_lassi`` (joint autoencoder + LieGAN symmetry discovery with a latent SINDy model, BASELINE
config 5) keeps the autoencoder, generator and discriminator on stock PyTorch-ROCm, as north_star asks; its
SINDy branch -- ``regressor(z)`` with backward into the encoder, or the latent least-squares solve whose
residual is differentiable w.r.t. z -- runs on the HIP engine.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .batched import allreduce_sums
from .model_utils import (_EulerFlow, make_fsymmreg_pttrain, make_rsymmreg_pttrain, make_symmreg_pttrain, odeint,
                          symmreg_linear)
from .sindy import solve_SINDy, solve_SINDy_one_step

try:                                    # wandb is optional (absent offline; README: WANDB_MODE=disabled)
    import wandb
except Exception:                       # pragma: no cover
    class _NoWandb:
        @staticmethod
        def log(*a, **k):
            pass

        @staticmethod
        def init(*a, **k):
            pass

        @staticmethod
        def finish(*a, **k):
            pass
    wandb = _NoWandb()


def _as_float(d):
    return {k: (v.item() if torch.is_tensor(v) else float(v)) for k, v in d.items()}


def _save(regressor, save_dir, name):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return                                              # sharded fits: every rank holds the same model, rank 0 writes it
    os.makedirs(f'saved_models/{save_dir}', exist_ok=True)
    torch.save(regressor.state_dict(), f'saved_models/{save_dir}/{name}')


class _RunningMeans:
    """Per-epoch means of the logged scalars."""

    def __init__(self, keys):
        self.values = {k: [] for k in keys}

    def add(self, key, value):
        self.values[key].append(value.item() if torch.is_tensor(value) else float(value))

    def means(self):
        return {k: (float(np.mean(v)) if len(v) else float('nan')) for k, v in self.values.items()}

    def line(self, prefix, shown):
        m = self.means()
        return ', '.join([prefix] + [f'{k}: {m[k]:.4f}' for k in self.values if shown.get(k, False)])


_LASSI_TRAIN_KEYS = ('loss_ae', 'loss_g', 'loss_reg_norm', 'loss_reg_ortho', 'loss_reg_closure', 'loss_d_real', 'loss_d_fake',
                     'loss_ae_rel', 'loss_sindy_x', 'loss_sindy_z', 'loss_sindy_reg')
_LASSI_TEST_KEYS = ('test_loss_ae', 'test_loss_g', 'test_loss_d_real', 'test_loss_d_fake', 'test_loss_sindy_x', 'test_loss_sindy_z')


def _latent_generators(generator, n_comps):
    """The generator's current basis cut to one component: the (d, d) blocks the regressor is constrained by
    (train.py:162-164, main.py:69-73)."""
    full = generator.get_full_basis_list()
    d = full[0].shape[-1] // n_comps
    return [L[:d, :d].detach().cpu() for L in full]


def train_lassi(
    autoencoder, discriminator, generator, train_loader, test_loader,
    num_epochs, lr_ae, lr_d, lr_g, w_recon, w_gan, w_reg_norm, w_reg_sim, w_reg_ortho, w_reg_closure,
    use_original_x, gan_st_freq, gan_st_thres, ae_arch,
    include_sindy, regressor, lr_sindy, w_sindy_z, w_sindy_x, sindy_reg_type, w_sindy_reg, st_freq, threshold,
    device, log_interval, save_interval, save_dir, **kwargs
):
    """Joint training of autoencoder, Lie generator, discriminator and a latent SINDy model on multi-timestep
    batches x, dx (B, n_timesteps, input_dim) -- reference train.py:16-253, same arguments, same per-batch loss,
    same epoch events (generator / regressor thresholding, checkpoints under saved_models/<save_dir>/*_{epoch}.pt).

    SINDy branch: with ``w_sindy_x > 0`` the regressor is trained by Adam (lr x10 after each of the first three
    epochs) on  w_z * MSE(regressor(z), dz) + w_x^2 * MSE(J_dec dz_pred, dx)  (the reference scales loss_sindy_x by
    w_sindy_x twice, train.py:145, 148) + L1; otherwise its parameters are frozen and re-solved every batch by
    sequential-threshold least squares on (z_0, dz_0), the solve's residual being the loss that reaches the encoder;
    under the equivariance constraint Q is rebuilt when the learned generators have moved by more than 0.1 (summed
    Frobenius distance) or on the last batch of an epoch.
    """
    train_ae = (ae_arch != 'none')
    opt = {'d': torch.optim.Adam(discriminator.parameters(), lr=lr_d), 'g': torch.optim.Adam(generator.parameters(), lr=lr_g)}
    if train_ae:
        opt['ae'] = torch.optim.Adam(autoencoder.parameters(), lr=lr_ae)
    scheduler = None
    fit_by_adam = include_sindy and w_sindy_x > 0.0
    if fit_by_adam:
        opt['sindy'] = torch.optim.Adam(regressor.parameters(), lr=lr_sindy)
        scheduler = torch.optim.lr_scheduler.MultiStepLR(opt['sindy'], milestones=[1, 2, 3], gamma=10)
    elif include_sindy:
        for p in regressor.parameters():
            p.requires_grad = False
    else:
        w_sindy_z = w_sindy_x = w_sindy_reg = 0.0
    bce, mse = torch.nn.BCELoss(), torch.nn.MSELoss()

    shown = dict(zip(_LASSI_TRAIN_KEYS, [w > 0 for w in (w_recon, w_gan, w_reg_norm, w_reg_ortho, w_reg_closure, w_gan, w_gan,
                                                         w_recon, w_sindy_x, w_sindy_z, w_sindy_reg)]))
    shown_test = dict(zip(_LASSI_TEST_KEYS, [w > 0 for w in (w_recon, w_gan, w_gan, w_gan, w_sindy_x, w_sindy_z)]))

    def sindy_terms(log, x, dx, z, last_batch):
        """loss contribution of the latent SINDy model for one batch"""
        dz = autoencoder.compute_dz(x, dx)
        if fit_by_adam:
            dz_pred = regressor(z)
            dx_pred = autoencoder.compute_dx(z, dz_pred)
            on_z = mse(dz_pred, dz)
            on_x = w_sindy_x * mse(dx_pred, dx)
            log.add('loss_sindy_z', on_z)
            log.add('loss_sindy_x', on_x)
            total = w_sindy_z * on_z + w_sindy_x * on_x
            if sindy_reg_type != 'l1':
                raise ValueError(f'Unknown regularization type: {sindy_reg_type}')
            l1 = sum(torch.norm(p, 1) for p in regressor.parameters())
            log.add('loss_sindy_reg', l1)
            return total + w_sindy_reg * l1
        if regressor.constraint:
            with torch.no_grad():
                current = _latent_generators(generator, kwargs['n_comps'])
                moved = sum(torch.norm(a - b) for a, b in zip(current, regressor.L_list))
                if moved > 0.1 or last_batch:
                    regressor.update_Q(current)
        residual = solve_SINDy(regressor, z[:, 0], dz[:, 0], w_sindy_reg, threshold)
        log.add('loss_sindy_z', residual)
        log.add('loss_sindy_x', 0.0)
        log.add('loss_sindy_reg', 0.0)
        return w_sindy_z * residual

    n_batches = len(train_loader)
    for epoch in range(num_epochs):
        log = _RunningMeans(_LASSI_TRAIN_KEYS)
        for m in (autoencoder, discriminator, generator):
            m.train()
        if include_sindy:
            regressor.train()
        for i, (x, dx) in enumerate(train_loader):
            x = x.to(device)
            if include_sindy:
                dx = dx.to(device)
            real = torch.ones((x.shape[0], 1), device=device)
            fake = torch.zeros((x.shape[0], 1), device=device)

            # autoencoder
            z, xhat = autoencoder(x)
            loss_ae = mse(xhat, x)
            log.add('loss_ae', loss_ae)
            log.add('loss_ae_rel', loss_ae / mse(x, torch.zeros_like(x)))
            loss = w_recon * loss_ae

            # generator: a random group element moves the latent batch; the critic should not notice
            zt = generator(z)
            xt = autoencoder.decode(zt) if use_original_x else None
            loss_g = bce(discriminator(zt, None, xt), real)
            log.add('loss_g', loss_g)
            loss = loss + w_gan * loss_g
            if not np.isclose(w_reg_norm, 0.0):
                reg = generator.reg_norm()
                loss = loss + w_reg_norm * reg
            elif not np.isclose(w_reg_sim, 0.0):             # or: transformed and original latents should differ
                reg = torch.abs(torch.nn.CosineSimilarity(dim=-1)(zt, z).mean())
                loss = loss + w_reg_sim * reg
            else:
                reg = 0.0
            log.add('loss_reg_norm', reg)
            for key, weight, term in (('loss_reg_ortho', w_reg_ortho, generator.reg_ortho),
                                      ('loss_reg_closure', w_reg_closure, generator.reg_closure)):
                if not np.isclose(weight, 0.0):
                    value = term()
                    loss = loss + weight * value
                    log.add(key, value)
                else:
                    log.add(key, 0.0)

            # discriminator on detached latents
            xd = xhat.detach() if use_original_x else None
            xtd = xt.detach() if use_original_x else None
            loss_d_real = bce(discriminator(z.detach(), xd), real)      # (sic) second positional slot, as train.py:132-133
            loss_d_fake = bce(discriminator(zt.detach(), xtd), fake)
            log.add('loss_d_real', loss_d_real)
            log.add('loss_d_fake', loss_d_fake)
            loss = loss + (loss_d_real + loss_d_fake) / 2

            if include_sindy:
                loss = loss + sindy_terms(log, x, dx, z, last_batch=(i == n_batches - 1))
            else:
                for key in ('loss_sindy_z', 'loss_sindy_x', 'loss_sindy_reg'):
                    log.add(key, 0.0)

            for o in opt.values():
                o.zero_grad()
            loss.backward()
            for name in ('ae', 'd', 'g', 'sindy'):
                if name in opt:
                    opt[name].step()

        if scheduler is not None:
            scheduler.step()
        if gan_st_freq > 0 and (epoch + 1) % gan_st_freq == 0:
            generator.set_threshold(gan_st_thres)
        if fit_by_adam and st_freq > 0 and (epoch + 1) % st_freq == 0:
            regressor.set_threshold(threshold)

        record = log.means()
        if (epoch + 1) % log_interval == 0:
            print(log.line(f'Epoch {epoch}', shown))
            for m in (autoencoder, discriminator, generator):
                m.eval()
            tlog = _RunningMeans(_LASSI_TEST_KEYS)
            for x, dx in test_loader:
                x, dx = x.to(device), dx.to(device)
                with torch.no_grad():
                    real = torch.ones((x.shape[0], 1), device=device)
                    fake = torch.zeros((x.shape[0], 1), device=device)
                    z, xhat = autoencoder(x)
                    zt = generator(z)
                    xt = autoencoder.decode(zt)
                    d_fake = discriminator(zt, None, xt if use_original_x else None)
                    d_real = discriminator(z, None, x if use_original_x else None)
                    tlog.add('test_loss_ae', mse(xhat, x))
                    tlog.add('test_loss_g', bce(d_fake, real))
                    tlog.add('test_loss_d_real', bce(d_real, real))
                    tlog.add('test_loss_d_fake', bce(d_fake, fake))
                if include_sindy:
                    dz = autoencoder.compute_dz(x, dx)          # functional jvp: builds its own graph, returns detached
                    with torch.no_grad():
                        dz_pred = regressor(z)
                    dx_pred = autoencoder.compute_dx(z, dz_pred)
                    tlog.add('test_loss_sindy_z', mse(dz_pred, dz))
                    tlog.add('test_loss_sindy_x', mse(dx_pred, dx))
                else:
                    tlog.add('test_loss_sindy_z', 0.0)
                    tlog.add('test_loss_sindy_x', 0.0)
            record.update(tlog.means())
            print(tlog.line(f'Epoch {epoch}', shown_test))
            if kwargs.get('print_li'):
                print(generator.getLi())
            if include_sindy:
                regressor.print()
        wandb.log(record)

        if (epoch + 1) % save_interval == 0:
            out = f'saved_models/{save_dir}'
            os.makedirs(out, exist_ok=True)
            torch.save(autoencoder.state_dict(), f'{out}/autoencoder_{epoch}.pt')
            torch.save(discriminator.state_dict(), f'{out}/discriminator_{epoch}.pt')
            torch.save(generator.state_dict(), f'{out}/generator_{epoch}.pt')
            torch.save(generator.masks, f'{out}/generator_mask_{epoch}.pt')
            if include_sindy:
                torch.save(regressor.state_dict(), f'{out}/regressor_{epoch}.pt')
                torch.save(regressor.L_list, f'{out}/regressor_lie_list_{epoch}.pt')
    return record


class _HostShadow:
    """Host-resident optimisation variables of a regressor whose data lives in HBM.

    L-BFGS on a dozen parameters is dozens of tiny tensor ops per inner iteration; on device
    tensors every one of them is a kernel launch or a sync (measured: 3.6 ms per closure for
    dosc 50x2500x2, against 12 us of kernel time).  The shadow keeps ``Xi`` (or ``beta``/``const``)
    and the mask on the host, evaluates the closure with ONE fused launch -- coefficients go up
    through a pinned buffer, ``[loss | dloss/dXi]`` comes back through another -- and lets autograd
    carry the gradient through ``get_Xi`` on the host.  ``sync()`` writes the state back into the
    regressor (called before every print / save / threshold and at the end), so callers see
    the reference's semantics.
    """

    def __init__(self, regressor, x, dx, reversed_sym=None, numpy_vars=True, use_graph=True, zero_copy=True):
        self.reg, self.x, self.dx = regressor, x, dx
        self.params = [p.detach().cpu().clone().requires_grad_(True) for p in regressor.parameters()]
        self.coef = regressor.coef.to('cpu')
        # numpy mode: ONE flat float32 vector aliases every host parameter (torch views of the same memory)
        self.flat = None
        if numpy_vars:
            self.flat = np.concatenate([p.detach().numpy().reshape(-1) for p in self.params]).astype(np.float32)
            self.params = [v for v in self.coef.split(torch.from_numpy(self.flat)) if v is not None]   # plain tensors on self.flat
        self.mask = regressor.mask.detach().cpu().clone()
        d, p = regressor.mask.shape
        dev = x.device
        self.h_xi = torch.empty(d, p).pin_memory()
        self.d_xi = torch.empty(d, p, device=dev)
        self.n_out = 1 + d * p
        self.reversed_sym = reversed_sym                      # (gx, jgx) of the fused reversed regulariser, or None
        n_terms = 2 if reversed_sym is not None else 1
        self.d_out = torch.empty(n_terms * self.n_out, device=dev)
        self.h_out = torch.empty(n_terms * self.n_out).pin_memory()
        # private scratch: the closure's launches must not depend on which stream replays them
        eng = regressor.engine
        self.ws = None
        if hasattr(eng, 'new_workspace'):
            self.ws = eng.new_workspace(dev, eng.lib.symode_workspace_bytes(regressor.latent_dim, regressor.poly_order,
                                                                            regressor.flags, 1, x.shape[-2]))
        self._graph = None
        # Zero-copy closure: the kernel reads Xi from and writes [loss | grad] to pinned host memory, so one closure is
        # ONE launch + one stream sync (the last workgroup finalises inside the launch) -- no copy nodes, no graph.
        # Checked once against the copy path; any failure or difference leaves the copy path (+ HIP graph) in place.
        self.zero_copy = False
        self._bound = self._bound_fused = None
        self._stream = torch.cuda.current_stream(dev) if x.is_cuda else None
        if zero_copy and self.ws is not None:
            self.zero_copy = self._zero_copy_works()
        if self.zero_copy and hasattr(eng, 'bind_closure'):
            # all argument checks / conversions done once: the per-closure host cost is one ctypes call + one sync
            self._bound = eng.bind_closure(x, dx, self.h_xi, regressor.mask, regressor.poly_order, regressor.flags,
                                           (self.h_out[:1], self.h_out[1:self.n_out].view(d, p)), self.ws, self._stream)
        if not self.zero_copy and use_graph:
            self._capture()

    def _kw(self):
        return {'ws': self.ws} if self.ws is not None else {}

    def _launch(self, xi, out):
        """The closure's kernels on coefficients ``xi``, [loss | grad] of every term into ``out``: the pinned host pair
        (zero-copy) or the device pair of the copy path."""
        reg, (d, p), n = self.reg, self.mask.shape, self.n_out
        reg.engine.loss_grad(self.x, self.dx, xi, reg.mask, reg.poly_order, reg.flags,
                             out=(out[:1], out[1:n].view(d, p)), **self._kw())
        if self.reversed_sym is not None:
            gx, jgx = self.reversed_sym
            reg.engine.symreg_reversed(self.x, gx, jgx, xi, reg.mask, reg.poly_order, reg.flags,
                                       out=(out[n:n + 1], out[n + 1:].view(d, p)), **self._kw())

    def _launch_copy(self):
        """Upload coefficients, the fused kernels, download [loss | grad]: everything between the two host buffers."""
        self.d_xi.copy_(self.h_xi, non_blocking=True)
        self._launch(self.d_xi, self.d_out)
        self.h_out.copy_(self.d_out, non_blocking=True)

    def evaluate_fused(self, w_ratio):
        """Reversed-regulariser closure as ONE launch (symode_loss_grad_reversed): returns (Xi, mse, sym, d(mse + w_ratio sym)/dXi)
        through the pinned buffers; ``w_ratio`` = w_sym_reg / w_sindy_x."""
        reg, (d, p), n = self.reg, self.mask.shape, self.n_out
        Xi = self.get_Xi()
        self.h_xi.copy_(Xi.detach())
        gx, jgx = self.reversed_sym
        if self._bound_fused is None or self._bound_fused[0] != w_ratio:
            self._bound_fused = (w_ratio, reg.engine.bind_closure(
                self.x, self.dx, self.h_xi, reg.mask, reg.poly_order, reg.flags, (self.h_out[:2], self.h_out[2:2 + d * p].view(d, p)),
                self.ws, self._stream, reversed_sym=(gx, jgx), w_sym=w_ratio))
        self._bound_fused[1]()
        self._stream.synchronize()
        return Xi, self.h_out[0].clone(), self.h_out[1].clone(), self.h_out[2:2 + d * p].view(d, p).clone()

    def _zero_copy_works(self):
        try:
            self.h_xi.copy_(self.get_Xi().detach())
            self._launch_copy()
            torch.cuda.synchronize(self.x.device)
            want = self.h_out.clone()
            self.h_out.fill_(float('nan'))
            self._launch(self.h_xi, self.h_out)
            torch.cuda.synchronize(self.x.device)
            return bool(torch.equal(want, self.h_out))
        except Exception:                               # pragma: no cover - depends on the runtime
            return False

    def _capture(self):
        """Copy path: the closure's device work is launch-bound (a ~6 us kernel between two tiny copies): capture it once
        in a HIP graph and replay it per closure.  Any failure leaves the eager path in place."""
        try:
            self.h_xi.copy_(self.get_Xi().detach())
            side = torch.cuda.Stream(device=self.x.device)
            side.wait_stream(torch.cuda.current_stream(self.x.device))
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._launch_copy()                 # warm-up: lazy inits
            torch.cuda.current_stream(self.x.device).wait_stream(side)
            torch.cuda.synchronize(self.x.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch_copy()
            self._graph = g
        except Exception:                               # pragma: no cover - depends on the runtime
            self._graph = None

    def parameters(self):
        return self.params

    def get_Xi(self):                                                                   # sindy.py:169-176 on the host
        return self.coef.xi(*self.params)

    def set_threshold(self, threshold):                                                 # sindy.py:192-194
        with torch.no_grad():
            Xi = self.get_Xi()
            self.reg.note_near_threshold(Xi.numpy(), self.mask.numpy(), threshold, 'set_threshold (host L-BFGS variables)')
            self.mask = torch.logical_and(torch.abs(Xi) > threshold, self.mask).float()
        self.sync()

    def sync(self):
        flat = self.flat if self.flat is not None else torch.cat([p.detach().reshape(-1) for p in self.params])
        self.coef.adopt(self.reg, flat, self.mask)      # (the mask in place: the captured graph holds this pointer)

    def grad_to_flat(self, g_xi):
        """Chain rule of get_Xi: dL/d(flat parameters) from dL/dXi (d, p), as numpy float32."""
        return self.coef.grad(g_xi, flat=True)

    def evaluate(self):
        """Returns (Xi on host with graph, [mse, sym] values, [dmse/dXi, dsym/dXi]) -- one sync."""
        reg, d, p = self.reg, *self.mask.shape
        Xi = self.get_Xi()
        self.h_xi.copy_(Xi.detach())
        n = self.n_out
        if self._bound is not None and self.reversed_sym is None:
            self._bound()
            self._stream.synchronize()
        else:
            if self.zero_copy:
                self._launch(self.h_xi, self.h_out)
            elif self._graph is not None:
                self._graph.replay()
            else:
                self._launch_copy()
            torch.cuda.current_stream(self.x.device).synchronize()
        vals = [self.h_out[k * n].clone() for k in range(len(self.h_out) // n)]
        grads = [self.h_out[k * n + 1:(k + 1) * n].view(d, p).clone() for k in range(len(self.h_out) // n)]
        return Xi, vals, grads


class _HostParams:
    """Host-resident L-BFGS variables for closures that need device autograd (infinitesimal / finite symmetry
    regulariser through the stock autoencoder, latent branch): torch.optim.LBFGS runs its two-loop recursion and its
    dozens of tiny vector ops per iteration on host copies of the 12-42 parameters (microseconds each, against one
    kernel launch each on device tensors: 3.6 ms per closure measured in round 1), the closure itself runs on the
    device as before.  ``push`` writes the host values into the regressor's device parameters (one small copy per
    tensor), ``pull_grads`` brings the gradients back.  Same interface as _HostShadow for ``_lbfgs_phase``."""

    flat = None                                           # torch's own L-BFGS (no numpy variables here)

    def __init__(self, regressor):
        self.reg = regressor
        self.dev_params = list(regressor.parameters())
        self.params = [p.detach().cpu().clone().requires_grad_(True) for p in self.dev_params]

    def parameters(self):
        return self.params

    def push(self):
        with torch.no_grad():
            for dst, src in zip(self.dev_params, self.params):
                dst.copy_(src.detach(), non_blocking=True)

    def pull_grads(self):
        for host, dev in zip(self.params, self.dev_params):
            host.grad = None if dev.grad is None else dev.grad.detach().cpu()

    def wrap(self, closure):
        """closure(optimizer) evaluated on the device parameters, gradients handed to the host variables."""
        def host_closure(optimizer):
            self.push()
            for p in self.dev_params:
                p.grad = None
            loss = closure(_NoZeroGrad)
            self.pull_grads()
            return loss.detach().cpu()
        return host_closure

    def set_threshold(self, threshold):
        self.push()
        self.reg.set_threshold(threshold)                 # device threshold on the pushed values (sindy.py:192-194)

    def sync(self):
        self.push()


class _NoZeroGrad:
    """Stand-in for the optimiser inside a wrapped closure: the device gradients were cleared by the wrapper."""

    @staticmethod
    def zero_grad():
        pass


class _PlainLBFGS:
    """torch.optim.LBFGS (no line search) as the SAME sequence of torch tensor operations on the same parameter list --
    hence bit-identical iterates (tests/test_host_train.py) -- without deriving from torch.optim.Optimizer: constructing
    any torch optimiser imports torch._dynamo (0.55 s, a quarter of a one-seed process of the reference's run scripts).
    ``SYMODE_TORCH_OPTIM=1`` puts torch's own class back."""

    def __init__(self, params, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100):
        self.params = list(params)
        self.lr, self.max_iter = lr, max_iter
        self.max_eval = max_iter * 5 // 4 if max_eval is None else max_eval
        self.tol_g, self.tol_c, self.H = tolerance_grad, tolerance_change, history_size
        self.func_evals = self.n_iter = 0
        self.d = self.t = self.old_dirs = self.old_stps = self.ro = self.H_diag = self.prev_flat_grad = self.prev_loss = None
        self.al = None

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    def _flat_grad(self):
        return torch.cat([p.new(p.numel()).zero_() if p.grad is None else p.grad.view(-1) for p in self.params], 0)

    def _move(self, step_size, update):
        offset = 0
        for p in self.params:
            numel = p.numel()
            p.add_(update[offset:offset + numel].view_as(p), alpha=step_size)
            offset += numel

    @torch.no_grad()
    def step(self, closure):
        closure = torch.enable_grad()(closure)
        orig_loss = closure()
        loss = float(orig_loss)
        current_evals = 1
        self.func_evals += 1
        flat_grad = self._flat_grad()
        if flat_grad.abs().max() <= self.tol_g:
            return orig_loss
        d, t, old_dirs, old_stps, ro, H_diag = self.d, self.t, self.old_dirs, self.old_stps, self.ro, self.H_diag
        prev_flat_grad, prev_loss = self.prev_flat_grad, self.prev_loss
        n_iter = 0
        while n_iter < self.max_iter:
            n_iter += 1
            self.n_iter += 1
            if self.n_iter == 1:
                d = flat_grad.neg()
                old_dirs, old_stps, ro, H_diag = [], [], [], 1
            else:
                y = flat_grad.sub(prev_flat_grad)
                s = d.mul(t)
                ys = y.dot(s)
                if ys > 1e-10:
                    if len(old_dirs) == self.H:
                        old_dirs.pop(0)
                        old_stps.pop(0)
                        ro.pop(0)
                    old_dirs.append(y)
                    old_stps.append(s)
                    ro.append(1.0 / ys)
                    H_diag = ys / y.dot(y)
                num_old = len(old_dirs)
                if self.al is None:
                    self.al = [None] * self.H
                al = self.al
                q = flat_grad.neg()
                for i in range(num_old - 1, -1, -1):
                    al[i] = old_stps[i].dot(q) * ro[i]
                    q.add_(old_dirs[i], alpha=-al[i])
                d = r = torch.mul(q, H_diag)
                for i in range(num_old):
                    be_i = old_dirs[i].dot(r) * ro[i]
                    r.add_(old_stps[i], alpha=al[i] - be_i)
            if prev_flat_grad is None:
                prev_flat_grad = flat_grad.clone(memory_format=torch.contiguous_format)
            else:
                prev_flat_grad.copy_(flat_grad)
            prev_loss = loss
            t = min(1.0, 1.0 / flat_grad.abs().sum()) * self.lr if self.n_iter == 1 else self.lr
            gtd = flat_grad.dot(d)
            if gtd > -self.tol_c:
                break
            ls_func_evals = 0
            self._move(t, d)
            if n_iter != self.max_iter:
                with torch.enable_grad():
                    loss = closure()
                loss = float(loss)
                flat_grad = self._flat_grad()
                opt_cond = flat_grad.abs().max() <= self.tol_g
                ls_func_evals = 1
            current_evals += ls_func_evals
            self.func_evals += ls_func_evals
            if n_iter == self.max_iter:
                break
            if current_evals >= self.max_eval:
                break
            if opt_cond:
                break
            if d.mul(t).abs().max() <= self.tol_c:
                break
            if abs(loss - prev_loss) < self.tol_c:
                break
        self.d, self.t, self.old_dirs, self.old_stps, self.ro, self.H_diag = d, t, old_dirs, old_stps, ro, H_diag
        self.prev_flat_grad, self.prev_loss = prev_flat_grad, prev_loss
        return orig_loss


def _new_lbfgs(params, lr):
    """the L-BFGS of the trainers: torch's arithmetic without torch's Optimizer base (see _PlainLBFGS)"""
    if os.environ.get('SYMODE_TORCH_OPTIM', '0') == '1':
        return torch.optim.LBFGS(params, lr=lr)
    return _PlainLBFGS(params, lr=lr)


class _NumpyLBFGS:
    """torch.optim.LBFGS (no line search, default tolerances) on one flat float32 numpy vector.

    Same update rules, history handling and stopping tests as torch/optim/lbfgs.py, statement by
    statement (see also sweep.BatchedLBFGS); exists because at 12-42 parameters torch's tensor
    bookkeeping (~0.4 ms per inner iteration) costs 10x the fused closure itself.
    ``closure(x) -> (loss float, grad float32 array)``.
    """

    def __init__(self, x, lr, max_iter=20, tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100):
        self.x, self.lr, self.max_iter = x, np.float32(lr), max_iter
        self.tol_g, self.tol_c, self.H = tolerance_grad, tolerance_change, history_size
        self.n_iter = 0
        self.d = self.t = self.prev_g = self.prev_loss = None
        self.old_dirs, self.old_stps, self.ro, self.H_diag = [], [], [], np.float32(1.0)

    def step(self, closure):
        f32 = np.float32
        loss, g = closure(self.x)
        orig = loss
        if np.abs(g).max() <= self.tol_g:
            return orig
        n_iter = 0
        while n_iter < self.max_iter:
            n_iter += 1
            self.n_iter += 1
            if self.n_iter == 1:
                self.d = -g
                self.old_dirs, self.old_stps, self.ro, self.H_diag = [], [], [], f32(1.0)
            else:
                y = g - self.prev_g
                s = self.d * self.t
                ys = f32(np.dot(y, s))
                if ys > 1e-10:
                    if len(self.old_dirs) == self.H:
                        self.old_dirs.pop(0)
                        self.old_stps.pop(0)
                        self.ro.pop(0)
                    self.old_dirs.append(y)
                    self.old_stps.append(s)
                    self.ro.append(f32(1.0) / ys)
                    self.H_diag = ys / f32(np.dot(y, y))
                num_old = len(self.old_dirs)
                al = [None] * num_old
                q = -g
                for i in range(num_old - 1, -1, -1):
                    al[i] = f32(np.dot(self.old_stps[i], q)) * self.ro[i]
                    q = q - al[i] * self.old_dirs[i]
                r = q * self.H_diag
                for i in range(num_old):
                    be_i = f32(np.dot(self.old_dirs[i], r)) * self.ro[i]
                    r = r + self.old_stps[i] * (al[i] - be_i)
                self.d = r.astype(f32)
            self.prev_g = g.copy()
            self.prev_loss = loss
            if self.n_iter == 1:
                self.t = f32(min(1.0, 1.0 / float(np.abs(g).sum()))) * self.lr
            else:
                self.t = self.lr
            gtd = f32(np.dot(g, self.d))
            if gtd > -self.tol_c:
                break
            self.x += self.t * self.d
            if n_iter != self.max_iter:
                loss, g = closure(self.x)
                opt_cond = np.abs(g).max() <= self.tol_g
            else:
                break
            if opt_cond:
                break
            if np.abs(self.d * self.t).max() <= self.tol_c:
                break
            if abs(loss - self.prev_loss) < self.tol_c:
                break
        return orig


def _lbfgs_phase(regressor, closure, losses, num_epochs, lr_sindy, st_freq, threshold, log_interval, save_interval,
                 save_dir, print_eq, on_log=None, tol=1e-3, shadow=None):
    """L-BFGS epochs with convergence-triggered / periodic thresholding       (train.py:692-766, 805-852).
    ``shadow`` (optional _HostShadow) owns the optimisation variables instead of the regressor."""
    P = shadow if shadow is not None else regressor
    sync = shadow.sync if shadow is not None else (lambda: None)
    fast = shadow is not None and shadow.flat is not None          # numpy variables + numpy L-BFGS

    def new_optimizer():
        return _NumpyLBFGS(shadow.flat, lr_sindy) if fast else _new_lbfgs(P.parameters(), lr_sindy)

    optimizer = new_optimizer()
    prev_params = [p.detach().clone() for p in P.parameters()]
    pprev_params = [p.detach().clone() for p in P.parameters()]
    n_iters = 0
    for epoch in range(num_epochs):
        n_iters += 1
        optimizer.step(closure if fast else (lambda: closure(optimizer)))
        if any(torch.isnan(p).any() for p in P.parameters()):                         # train.py:697
            print(f'NaN encountered at iteration {epoch}; exit training.')
            break
        wandb_log = _as_float(losses)
        with torch.no_grad():
            param_update_norm = sum(torch.norm(p - q) for p, q in zip(P.parameters(), prev_params))
        if param_update_norm < tol:
            param_update_norm_2 = sum(torch.norm(p - q) for p, q in zip(P.parameters(), pprev_params))
            if param_update_norm_2 < tol:                                              # train.py:709-714
                print(f'Final convergence reached at iteration {epoch}; exit training.')
                sync()
                _save(regressor, save_dir, f'regressor_{epoch}.pt')
                break
            n_iters = 0
            P.set_threshold(threshold)
            optimizer = new_optimizer()
            pprev_params = [p.detach().clone() for p in P.parameters()]
            print(f'Convergence reached at iteration {epoch}; apply parameter thresholding and reset optimizer.')
        elif st_freq > 0 and n_iters % st_freq == 0:                                   # train.py:720-724
            n_iters = 0
            P.set_threshold(threshold)
            optimizer = new_optimizer()
            print('Max number of LBFGS iterations reached; apply parameter thresholding and reset optimizer.')
        prev_params = [p.detach().clone() for p in P.parameters()]

        if (epoch + 1) % log_interval == 0:
            sync()
            print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in _as_float(losses).items()]))
            if on_log is not None:
                wandb_log.update(on_log(epoch))
            if print_eq:
                regressor.print()
        wandb.log(wandb_log)
        if (epoch + 1) % save_interval == 0:
            sync()
            _save(regressor, save_dir, f'regressor_{epoch}.pt')
    sync()


def _train_on_device(regressor, x, dx, autoencoder, generator, num_epochs, lr_sindy, st_freq, threshold, w_sindy_x,
                     sindy_reg_type, w_sindy_reg, w_sym_reg, losses, save_dir, print_eq, log_interval=0, save_interval=0,
                     test_log=None, group=None, gram_closure=False):
    """The non-latent L-BFGS fit with NOTHING on the host between two epochs (device_lbfgs.DeviceTrainer): closure kernel +
    ONE optimiser launch per inner iteration, the per-epoch logic of train.py:697-725 as one more launch, and a record per
    epoch in pinned memory from which this function produces what the reference produces per epoch -- the convergence /
    thresholding / NaN messages, the loss line, the "test" line (train.py:739-751), the equations, the wandb record and the
    interval checkpoints -- in the reference's order.  The record holds the LAST closure evaluation's terms (what the
    reference's ``losses`` dict holds when the epoch ends) and, for the "test" line, the closure re-evaluated at the
    epoch's final coefficients and mask.  ``group``: x, dx are this rank's point shard.  ``gram_closure``: the closure is
    the quadratic form of the batch's fp64 Gram matrices (gram_closure.py), built in one pass and summed over the ranks in
    one all-reduce; the fit itself then needs no collective."""
    from .device_lbfgs import EVENT_FINAL, EVENT_NAN, EVENT_THRESHOLD_CONVERGED, EVENT_THRESHOLD_PERIOD, DeviceTrainer
    d = x.shape[-1]
    rev = None
    if w_sym_reg > 0.0:
        from .model_utils import precompute_symmreg_r
        gx, jgx = precompute_symmreg_r(x, autoencoder, generator, scale=0.01)
        gx, jgx = torch.stack(gx), torch.stack(jgx)
        rev = (gx.reshape(1, gx.shape[0], -1, d).contiguous(), jgx.reshape(1, jgx.shape[0], -1, d, d).contiguous(),
               w_sym_reg / w_sindy_x)
    xs, dxs = x.reshape(1, -1, d).contiguous(), dx.reshape(1, -1, d).contiguous()
    coef = regressor.coef
    with torch.no_grad():
        P0 = coef.pack(regressor).cpu()[None]
        mask_before = regressor.mask.detach().cpu().numpy().copy()
    tr = DeviceTrainer(xs, dxs, regressor.poly_order, regressor.flags, coef=coef, reversed_sym=rev, lr=lr_sindy,
                       threshold=threshold, st_freq=st_freq, w_x=w_sindy_x, w_reg=w_sindy_reg if sindy_reg_type == 'l1' else 0.0,
                       l1=sindy_reg_type == 'l1', engine=regressor.engine, detail=True, group=group,
                       closure='gram' if gram_closure else 'stream')

    state = {'mask_before': mask_before}

    def on_epoch(epoch, rec):
        code = int(rec['code'][0])
        if code == EVENT_NAN:                                                          # train.py:697-699
            print(f'NaN encountered at iteration {epoch}; exit training.')
            return True
        losses['loss_sindy_x'] = float(rec['mse'][0])
        if rev is not None:
            losses['loss_sym_reg'] = float(rec['sym'][0])
        if sindy_reg_type == 'l1':
            losses['loss_sindy_reg'] = float(rec['l1'][0])
        wandb_log = dict(losses)
        if code == EVENT_FINAL:                                                        # train.py:709-714
            print(f'Final convergence reached at iteration {epoch}; exit training.')
            coef.adopt(regressor, rec['params'][0], rec['mask'][0])    # a host state into the regressor
            _save(regressor, save_dir, f'regressor_{epoch}.pt')
            return True
        if code in (EVENT_THRESHOLD_CONVERGED, EVENT_THRESHOLD_PERIOD):
            regressor.note_near_threshold(rec['xi'][0], state['mask_before'], threshold, 'set_threshold (device trainer)')
            print('Convergence reached at iteration {}; apply parameter thresholding and reset optimizer.'.format(epoch)
                  if code == EVENT_THRESHOLD_CONVERGED else
                  'Max number of LBFGS iterations reached; apply parameter thresholding and reset optimizer.')
        state['mask_before'] = rec['mask'][0].copy()
        log = log_interval > 0 and (epoch + 1) % log_interval == 0
        save = save_interval > 0 and (epoch + 1) % save_interval == 0
        if log or save:
            coef.adopt(regressor, rec['params'][0], rec['mask'][0])    # a host state into the regressor
        if log:
            print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in losses.items()]))
            if test_log is not None:
                wandb_log.update(test_log(epoch, float(rec['test'][0])))
            if print_eq:
                regressor.print()
        wandb.log(wandb_log)
        if save:
            _save(regressor, save_dir, f'regressor_{epoch}.pt')
        return False

    out = tr.fit(P0, num_epochs, mask0=torch.from_numpy(mask_before)[None], on_epoch=on_epoch,
                 test_eval=test_log is not None and log_interval > 0)
    coef.adopt(regressor, out['params'][0], out['mask'][0])
    return out


def train_SIGED_lbfgs(
    train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir,  # global
    autoencoder, generator,  # symmetry discovery model
    regressor, regressor_dst, use_latent, distill_latent, lr_sindy, w_sindy_z, w_sindy_x,  # SINDy
    sindy_reg_type, w_sindy_reg, sym_reg_type, w_sym_reg, st_freq, threshold, int_t, int_dt,  # SINDy
    gram_closure=False, **kwargs
):
    if distill_latent and not use_latent:
        raise ValueError('Cannot distill without first learning latent space equation. Set use_latent=True.')
    train_data = next(iter(train_loader))                                              # ONE fixed batch (train.py:626)
    x, dx = train_data
    x, dx = x.to(device), dx.to(device)
    if sym_reg_type == 'i':
        symm_loss = make_symmreg_pttrain(autoencoder, generator)
    elif sym_reg_type == 'f':
        symm_loss = make_fsymmreg_pttrain(autoencoder, generator)
    elif sym_reg_type == 'r':
        symm_loss = make_rsymmreg_pttrain(autoencoder, generator)
    autoencoder.eval()
    generator.eval()
    losses = {}
    print_eq = kwargs.get('print_eq', False)
    group = kwargs.get('group')                # point shards: x, dx of train_loader are this rank's slice of the batch
    if group is not None and use_latent:
        raise ValueError('group=... (point shards) is implemented for the non-latent fit.')

    def reg_term(reg, loss):
        if sindy_reg_type == 'l1':                                                     # raw (unmasked) params, :680-683
            loss_sindy_reg = sum(torch.norm(p, 1) for p in reg.parameters())
            losses['loss_sindy_reg'] = loss_sindy_reg.detach()
            return loss + w_sindy_reg * loss_sindy_reg
        if sindy_reg_type == 'none':
            return loss
        raise ValueError(f'Unknown regularization type: {sindy_reg_type}')

    def closure(optimizer):                                                            # train.py:645-690
        optimizer.zero_grad()
        if use_latent:
            z, xhat = autoencoder(x)
            dz = autoencoder.compute_dz(x, dx)
            loss_sindy_z = regressor.mse_loss(z.detach(), dz.detach())                 # frozen AE: z, dz are data
            dz_pred = regressor(z)
            dx_pred = autoencoder.compute_dx(z, dz_pred)
            loss_sindy_x = torch.nn.functional.mse_loss(dx_pred, dx)
            losses['loss_sindy_z'] = loss_sindy_z.detach()
            losses['loss_sindy_x'] = loss_sindy_x.detach()
            loss = w_sindy_z * loss_sindy_z + w_sindy_x * loss_sindy_x
        else:
            loss_sindy_x = regressor.mse_loss(x, dx)                                   # fused HIP kernel
            loss_sym_reg = 0.0
            if group is not None:
                # x, dx are this rank's point shard: the residual's sum of squares, the point count and -- for the relative
                # regularisers, per generator -- numerator and denominator cross the ranks with their gradients in ONE
                # packed all-reduce; means and ratios are formed after it (model_utils.py:62, 118-121)
                n_loc = float(x.numel())
                also = [loss_sindy_x * n_loc, torch.tensor(n_loc, device=x.device)]
                if w_sym_reg > 0.0 and sym_reg_type in ['i', 'f']:
                    forward_step = _EulerFlow(regressor, int_t, int_dt)
                    x_fx = torch.stack([x, forward_step(x)], dim=1)
                    loss_sym_reg, red = symm_loss(x_fx, f=forward_step, x_const=x, group=group, also=also)
                else:
                    if w_sym_reg > 0.0:                                                # 'r': a plain batch mean per group element
                        also.append(symm_loss(x, h=regressor) * n_loc)
                    red = allreduce_sums(also, list(regressor.parameters()), group)
                    if w_sym_reg > 0.0:
                        loss_sym_reg = red[2] / red[1]
                loss_sindy_x = red[0] / red[1]
            elif w_sym_reg > 0.0:
                if sym_reg_type in ['i', 'f']:
                    forward_step = _EulerFlow(regressor, int_t, int_dt)
                    fx_pred = forward_step(x)
                    x_fx = torch.stack([x, fx_pred], dim=1)
                    loss_sym_reg = symm_loss(x_fx, f=forward_step, x_const=x)
                elif sym_reg_type == 'r':
                    loss_sym_reg = symm_loss(x, h=regressor)
            losses['loss_sindy_x'] = loss_sindy_x.detach()
            if w_sym_reg > 0.0:
                losses['loss_sym_reg'] = loss_sym_reg.detach()
            loss = w_sindy_x * loss_sindy_x + w_sym_reg * loss_sym_reg
        loss = reg_term(regressor, loss)
        loss.backward()
        return loss

    # numpy_lbfgs=True additionally swaps torch.optim.LBFGS for the numpy restatement (_NumpyLBFGS): 2.7x faster end
    # to end, same results on well-conditioned problems, but NOT the default: on ill-conditioned libraries (selkov,
    # cond 9e3, lr 1.0, no line search) the trajectory is chaotic in the last bits of every dot product and only
    # torch's own optimiser reproduces the reference's recorded run bit-for-bit in its mask.
    # Host-resident optimisation variables (see _HostShadow): whenever the closure is made only of fused
    # kernels -- plain / constrained SINDy, optionally with the reversed regulariser on a frozen autoencoder.
    shadow = None
    frozen = not any(p.requires_grad for m in (autoencoder, generator) for p in m.parameters())
    eligible = (x.is_cuda and not use_latent and kwargs.get('host_lbfgs', True)
                and (w_sym_reg <= 0.0 or (sym_reg_type == 'r' and frozen)))
    # DEFAULT for every closure made only of fused kernels: optimiser AND per-epoch logic on the device (_train_on_device).
    # torch's own optimiser on host-resident variables (the reference's torch.optim.LBFGS, operation for operation) stays
    # available: --torch_lbfgs / torch_lbfgs=True / SYMODE_TORCH_OPTIM=1.
    on_device = (eligible and not kwargs.get('torch_lbfgs', False) and not kwargs.get('numpy_lbfgs', False)
                 and os.environ.get('SYMODE_TORCH_OPTIM', '0') != '1' and w_sindy_x > 0 and sindy_reg_type in ('l1', 'none')
                 and hasattr(getattr(regressor.engine, 'lib', None), 'symode_trainer_run')
                 and regressor.mask.numel() <= 256)
    if eligible and not on_device and group is None:      # (the host-shadow closure is single-rank; shards take the generic closure)
        rev = None
        if w_sym_reg > 0.0:
            from .model_utils import precompute_symmreg_r
            gx, jgx = precompute_symmreg_r(x, autoencoder, generator, scale=0.01)
            rev = (torch.stack(gx).contiguous(), torch.stack(jgx).contiguous())
        shadow = _HostShadow(regressor, x, dx, reversed_sym=rev, numpy_vars=kwargs.get('numpy_lbfgs', False),
                             use_graph=kwargs.get('hip_graph', True), zero_copy=kwargs.get('zero_copy', True))

        def closure_np(flat):                                                          # numpy variables: (loss, flat gradient)
            with torch.no_grad():
                Xi, vals, grads = shadow.evaluate()
            losses['loss_sindy_x'] = vals[0]
            loss = w_sindy_x * float(vals[0])
            g_xi = w_sindy_x * grads[0].numpy()
            if rev is not None:
                losses['loss_sym_reg'] = vals[1]
                loss += w_sym_reg * float(vals[1])
                g_xi = g_xi + w_sym_reg * grads[1].numpy()
            g = shadow.grad_to_flat(g_xi.astype(np.float32))
            if sindy_reg_type == 'l1':
                l1 = float(np.abs(flat).sum())
                losses['loss_sindy_reg'] = l1
                loss += w_sindy_reg * l1
                g = g + np.float32(w_sindy_reg) * np.sign(flat)
            elif sindy_reg_type != 'none':
                raise ValueError(f'Unknown regularization type: {sindy_reg_type}')
            return loss, g.astype(np.float32)

        one_launch = (rev is not None and shadow.zero_copy and w_sindy_x > 0 and hasattr(regressor.engine, 'loss_grad_reversed'))

        def closure(optimizer):                                                        # same terms as train.py:645-690
            optimizer.zero_grad()
            lin = lambda v, g: v + (g * (Xi - Xi.detach())).sum()                      # value + exact first-order term  # noqa: E731
            if one_launch:                                                             # MSE + regulariser: one pass over the points
                Xi, mse, sym, g_tot = shadow.evaluate_fused(w_sym_reg / w_sindy_x)
                losses['loss_sindy_x'], losses['loss_sym_reg'] = mse, sym
                loss = lin(w_sindy_x * mse + w_sym_reg * sym, w_sindy_x * g_tot)
            else:
                Xi, vals, grads = shadow.evaluate()
                losses['loss_sindy_x'] = vals[0]
                loss = w_sindy_x * lin(vals[0], grads[0])
                if rev is not None:
                    losses['loss_sym_reg'] = vals[1]
                    loss = loss + w_sym_reg * lin(vals[1], grads[1])
            if sindy_reg_type == 'l1':
                loss_sindy_reg = sum(torch.norm(p, 1) for p in shadow.parameters())
                losses['loss_sindy_reg'] = loss_sindy_reg.detach()
                loss = loss + w_sindy_reg * loss_sindy_reg
            elif sindy_reg_type != 'none':
                raise ValueError(f'Unknown regularization type: {sindy_reg_type}')
            loss.backward()
            return loss

    def test_log(epoch, value=None):
        # ``value``: the closure at the epoch's final coefficients and mask, already evaluated by the device trainer.
        # The reference evaluates the TRAIN batch once per element of test_loader here (:739-751): the same number, n times
        # (lv: n = 780 at every logged epoch -- 45 % of the wall time of lv/noise99_eq_isymreg.cfg).  It is evaluated once
        # and accumulated n times in the reference's float arithmetic, so the logged mean is the reference's bit for bit.
        out = {'test_loss_sindy_z': 0.0, 'test_loss_sindy_x': 0.0}
        n = len(test_loader) if hasattr(test_loader, '__len__') else sum(1 for _ in test_loader)
        if n > 0:
            with torch.no_grad():
                if use_latent:
                    z, _ = autoencoder(x)
                    key, v = 'test_loss_sindy_z', regressor.mse_loss(z, autoencoder.compute_dz(x, dx)).item()
                elif value is not None:
                    key, v = 'test_loss_sindy_x', value
                elif group is not None:                                                # this rank's shard -> the batch mean
                    n_loc = float(x.numel())
                    red = allreduce_sums([regressor.mse_loss(x, dx) * n_loc, torch.tensor(n_loc, device=x.device)], [], group)
                    key, v = 'test_loss_sindy_x', (red[0] / red[1]).item()
                else:
                    key, v = 'test_loss_sindy_x', regressor.mse_loss(x, dx).item()
            for _ in range(n):
                out[key] += v
        out = {k: v / max(n, 1) for k, v in out.items()}
        print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in out.items()]))
        return out

    if shadow is not None and shadow.flat is not None:
        closure = closure_np
    if shadow is None and not on_device and x.is_cuda and kwargs.get('host_lbfgs', True):
        # autograd closures (i / f regulariser through the stock autoencoder, latent branch): the closure stays on the
        # device, the optimiser's variables move to the host
        shadow = _HostParams(regressor)
        closure = shadow.wrap(closure)
    if gram_closure and not on_device:
        raise ValueError('gram_closure=True needs the device trainer: the non-latent fit with MSE [+ L1] [+ the reversed '
                         'regulariser on a frozen autoencoder] on a GPU, without torch_lbfgs / numpy_lbfgs')
    if on_device:
        _train_on_device(regressor, x, dx, autoencoder, generator, num_epochs, lr_sindy, st_freq, threshold, w_sindy_x,
                         sindy_reg_type, w_sindy_reg, w_sym_reg, losses, save_dir, print_eq, log_interval, save_interval,
                         test_log=test_log, group=kwargs.get('group'), gram_closure=gram_closure)
    else:
        _lbfgs_phase(regressor, closure, losses, num_epochs, lr_sindy, st_freq, threshold, log_interval, save_interval,
                     save_dir, print_eq, on_log=test_log, shadow=shadow)

    # (Optional) Phase 2: distill equation from latent to data space                   # train.py:768-852
    if not distill_latent:
        return
    print('\n=== Phase 2: distill equation from latent to data space ===\n')
    x, _ = train_data
    x = x.to(device)
    with torch.no_grad():
        z, _ = autoencoder(x)
        dz_pred = regressor(z)
        dx = autoencoder.compute_dx(z, dz_pred)
    losses = {}

    def closure_dst(optimizer):
        optimizer.zero_grad()
        loss_sindy_x = regressor_dst.mse_loss(x, dx)
        losses['loss_sindy_x'] = loss_sindy_x.detach()
        loss = reg_term(regressor_dst, w_sindy_x * loss_sindy_x)
        loss.backward()
        return loss

    shadow_dst = None
    if x.is_cuda and kwargs.get('host_lbfgs', True):
        shadow_dst = _HostParams(regressor_dst)
        closure_dst = shadow_dst.wrap(closure_dst)
    _lbfgs_phase(regressor_dst, closure_dst, losses, num_epochs, lr_sindy, st_freq, threshold, log_interval,
                 save_interval, save_dir, print_eq, shadow=shadow_dst)


def _train_adam_on_device(train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir, regressor,
                          use_latent, lr_sindy, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg, st_freq, threshold,
                          print_eq, sym_reg_type=None, autoencoder=None, generator=None):
    """train_SIGED's plain branch on DeviceAdam: the same shuffles (one ``randperm`` per epoch from the global generator, as
    the loader draws them), prints, wandb records, test loss and checkpoints at the same epochs, produced from the
    launch's log and from the state adopted into the regressor at those epochs and at the end.  ``w_sym_reg > 0`` with
    ``sym_reg_type 'r'`` and a frozen autoencoder and generator adds ``w_sym_reg * symmreg_r`` to every minibatch loss:
    g(x), J_g(x) are computed once over the loader's rows."""
    from .dataset import DeviceBatches
    if use_latent:
        raise ValueError('device_adam covers the observed-space fit only: use_latent is set')
    if w_sym_reg < 0:
        raise ValueError(f'w_sym_reg is {w_sym_reg}: a weight is not negative')
    sym = w_sym_reg > 0
    if sym and sym_reg_type != 'r':
        raise ValueError(f"device_adam covers w_sym_reg > 0 (here {w_sym_reg}) with sym_reg_type 'r' only, not "
                         f"'{sym_reg_type}': the i / f regularisers run the autoencoder on Xi-dependent inputs")
    if sym and any(q.requires_grad for module in (autoencoder, generator) for q in module.parameters()):
        raise ValueError('device_adam with w_sym_reg > 0 needs a frozen autoencoder and generator (--fix_laligan: no parameter '
                         'requires grad): g(x), J_g(x) are computed once')
    if sindy_reg_type != 'l1':
        raise ValueError(f"device_adam covers sindy_reg_type 'l1', not '{sindy_reg_type}'")
    if not isinstance(train_loader, DeviceBatches):
        raise ValueError(f'device_adam needs train_loader to be a DeviceBatches, got {type(train_loader).__name__}')
    if train_loader.window != 0:
        raise ValueError(f'device_adam needs single-row items: train_loader.window is {train_loader.window}, not 0')
    x, dx = train_loader.arrays
    if not (x.is_cuda and dx.is_cuda):
        raise ValueError('device_adam needs the data set resident on the device (DeviceBatches kept it in host memory)')
    from .device_adam import DeviceAdam
    coef = regressor.coef
    rev = None
    if sym:                                                   # the weight as it stands: w_x * mse + w_sym_reg * regulariser
        from .model_utils import symmetry_operands
        _, gx, jgx, _, _ = symmetry_operands(x, torch.arange(x.shape[0], device=x.device)[None], autoencoder, generator)
        rev = (gx, jgx, w_sym_reg)
    trainer = DeviceAdam(x, dx, regressor.poly_order, regressor.include_sine, regressor.include_exp, coef, lr_sindy, w_sindy_x,
                         w_sindy_reg, threshold, st_freq, train_loader.bs, engine=regressor.engine, reversed_sym=rev)
    last_mask = [regressor.mask.detach().clone()]

    def at(epoch, every):
        return (epoch + 1) % every == 0

    def boundary(epoch):
        return at(epoch, log_interval) or at(epoch, save_interval) or (st_freq > 0 and at(epoch, st_freq))

    def on_epoch(epoch, rec):
        wandb_log = {'loss_sindy_x': float(rec['loss_sindy_x'][0]), 'loss_sindy_z': 0.0,
                     'loss_sindy_reg': float(rec['loss_sindy_reg'][0]),
                     'loss_sym_reg': float(rec['loss_sym_reg'][0]) if sym else 0.0}
        state = rec['state']
        if st_freq > 0 and at(epoch, st_freq) and not rec['nan'][0]:                   # train.py:545-546
            regressor.note_near_threshold(state['Xi'][0], last_mask[0], threshold, 'set_threshold (device Adam)')
            last_mask[0] = state['mask'][0].clone()
        if at(epoch, log_interval) or at(epoch, save_interval):
            coef.adopt(regressor, state['params'][0], state['mask'][0])
        if at(epoch, log_interval):
            print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in wandb_log.items()]))
            with torch.no_grad():
                tl = [regressor.mse_loss(xt.to(device), dxt.to(device)).item() for xt, dxt in test_loader]
            if tl:
                wandb_log['test_loss_sindy_x'] = float(np.mean(tl))
                print(f"Epoch {epoch}, test_loss_sindy_x: {wandb_log['test_loss_sindy_x']:.4f}")
            if print_eq:
                regressor.print()
        wandb.log(wandb_log)
        if at(epoch, save_interval):
            _save(regressor, save_dir, f'regressor_{epoch}.pt')

    regressor.train()
    out = trainer.fit(coef.pack(regressor)[None], num_epochs, (train_loader.epoch_order()[None] for _ in range(num_epochs)),
                      mask0=regressor.mask[None], on_epoch=on_epoch, boundary=boundary)
    coef.adopt(regressor, out['params'][0], out['mask'][0])


def train_SIGED(
    train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir,  # global
    autoencoder, discriminator, generator,  # symmetry discovery model
    lr_ae, lr_d, lr_g, w_recon, w_gan, w_reg_norm, w_reg_ortho, w_reg_closure,  # symmetry discovery parameters
    use_original_x, gan_st_freq, gan_st_thres, ae_arch,  # symmetry discovery parameters
    regressor, use_latent, lr_sindy, w_sindy_z, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg, st_freq, threshold,
    int_t, int_dt,  # SINDy
    **kwargs
):
    """Mini-batch Adam variant                                                       (train.py:382-614).
    ``device_adam=True`` (--device_adam): the plain branch runs whole epochs per launch on the device (device_adam.py),
    with ``sym_reg_type='r'`` and a frozen LaLiGAN also under the reversed symmetry regulariser; any other configuration is
    refused, not silently run the usual way."""
    if kwargs.get('device_adam'):
        return _train_adam_on_device(train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir,
                                     regressor, use_latent, lr_sindy, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg,
                                     st_freq, threshold, kwargs.get('print_eq'), sym_reg_type=kwargs.get('sym_reg_type'),
                                     autoencoder=autoencoder, generator=generator)
    optimizer_sindy = torch.optim.Adam(regressor.parameters(), lr=lr_sindy)
    symm_loss = make_symmreg_pttrain(autoencoder, generator)
    for epoch in range(num_epochs):
        running = {k: [] for k in ['loss_sindy_x', 'loss_sindy_z', 'loss_sindy_reg', 'loss_sym_reg']}
        regressor.train()
        for x, dx in train_loader:
            x, dx = x.to(device), dx.to(device)
            if use_latent:
                z, xhat = autoencoder(x)
                dz = autoencoder.compute_dz(x, dx)
                dz_pred = regressor(z)
                dx_pred = autoencoder.compute_dx(z, dz_pred)
                loss_sindy_z = w_sindy_z * torch.nn.functional.mse_loss(dz_pred, dz)
                loss_sindy_x = w_sindy_x * torch.nn.functional.mse_loss(dx_pred, dx)
                running['loss_sindy_z'].append(loss_sindy_z.item() / max(w_sindy_z, 1e-6))
                running['loss_sindy_x'].append(loss_sindy_x.item() / max(w_sindy_x, 1e-6))
                # linear-latent symmetry term, train.py:502-507 (with the [1] the shipped line forgets): fused kernel
                loss_sym_reg = symmreg_linear(z, regressor, generator.get_full_basis_list()) if w_sym_reg > 0 else 0.0
                running['loss_sym_reg'].append(float(loss_sym_reg))
                loss = loss_sindy_z + loss_sindy_x + w_sym_reg * loss_sym_reg
            else:
                loss_sindy_x = regressor.mse_loss(x, dx)
                running['loss_sindy_x'].append(loss_sindy_x.item())
                running['loss_sindy_z'].append(0.0)
                if w_sym_reg > 0:                          # the reference evaluates it even at weight 0 (logging only)
                    forward_step = _EulerFlow(regressor, int_t, int_dt)
                    x_fx = torch.stack([x, forward_step(x)], dim=1)
                    loss_sym_reg = symm_loss(x_fx, f=forward_step, x_const=x)
                    running['loss_sym_reg'].append(loss_sym_reg.item())
                else:
                    loss_sym_reg = 0.0
                    running['loss_sym_reg'].append(0.0)
                loss = w_sindy_x * loss_sindy_x + w_sym_reg * loss_sym_reg
            if sindy_reg_type == 'l1':
                loss_sindy_reg = sum(torch.norm(p, 1) for p in regressor.parameters())
                running['loss_sindy_reg'].append(loss_sindy_reg.item())
                loss = loss + w_sindy_reg * loss_sindy_reg
            else:
                raise ValueError(f'Unknown regularization type: {sindy_reg_type}')
            optimizer_sindy.zero_grad()
            loss.backward()
            optimizer_sindy.step()

        if st_freq > 0 and (epoch + 1) % st_freq == 0:                                 # train.py:545-546
            regressor.set_threshold(threshold)
        wandb_log = {k: float(np.mean(v)) for k, v in running.items()}
        if (epoch + 1) % log_interval == 0:
            print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in wandb_log.items()]))
            with torch.no_grad():
                tl = [regressor.mse_loss(xt.to(device), dxt.to(device)).item() for xt, dxt in test_loader] if not use_latent else []
            if tl:
                wandb_log['test_loss_sindy_x'] = float(np.mean(tl))
                print(f"Epoch {epoch}, test_loss_sindy_x: {wandb_log['test_loss_sindy_x']:.4f}")
            if kwargs.get('print_eq'):
                regressor.print()
        wandb.log(wandb_log)
        if (epoch + 1) % save_interval == 0:
            _save(regressor, save_dir, f'regressor_{epoch}.pt')


def train_WSINDy(wrapper, train_x, num_epochs, device, log_interval, save_interval, save_dir, w_sindy_reg, threshold,
                 **kwargs):
    """train.py:855-869"""
    train_x = train_x.to(device)
    for epoch in range(num_epochs):
        residual, completed = wrapper.solve(train_x, w_sindy_reg, threshold,
                                            **({'lstsq_driver': kwargs['lstsq_driver']} if kwargs.get('lstsq_driver') else {}))
        if (epoch + 1) % log_interval == 0:
            print(f'Iteration {epoch}, loss: {residual:.4f}')
            wrapper.regressor.print()
        if completed:
            print(f'Final convergence reached at iteration {epoch}; exit training.')
            break


def train_SINDy(regressor, x, dx, num_epochs, device, log_interval, save_interval, save_dir, w_sindy_reg, threshold,
                **kwargs):
    """Sequential-threshold least squares until the support stops changing   (train.py:872-887)."""
    x, dx = x.to(device), dx.to(device)
    for epoch in range(num_epochs):
        residual, completed = solve_SINDy_one_step(regressor, x, dx, w_sindy_reg, threshold,
                                                   **({'lstsq_driver': kwargs['lstsq_driver']} if kwargs.get('lstsq_driver') else {}))
        if (epoch + 1) % log_interval == 0:
            print(f'Iteration {epoch}, loss: {residual:.4f}')
            regressor.print()
        if completed:
            print(f'Final convergence reached at iteration {epoch}; exit training.')
            break
