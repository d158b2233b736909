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
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from .batched import allreduce_sums
from .host_closure import _HostParams, _HostShadow, _NoZeroGrad  # noqa: F401  (their old home: bench.py, tools/ and tests import them from here)
from .host_lbfgs import _new_lbfgs, _NumpyLBFGS, _PlainLBFGS  # noqa: F401
from .model_utils import (PRECOMPUTE_CHUNK, _EulerFlow, latent_operands, make_fsymmreg_pttrain, make_rsymmreg_pttrain,
                          make_symmreg_pttrain, odeint, reversed_operands, symmreg_linear)
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


def _at(epoch, every):
    return every > 0 and (epoch + 1) % every == 0


class _EpochReport:
    """What the reference does at the end of every epoch, in its order (train.py:727-766): at the log interval the loss
    line, the test line and the equations; the wandb record; at the save interval ``regressor_<epoch>.pt``.  The trainers
    differ in where the record comes from, in how the state reaches the regressor (``adopt``, called before the first
    thing that reads it) and in their test line (``test(epoch)``: prints it, returns what it adds to the record)."""

    def __init__(self, regressor, log_interval, save_interval, save_dir, print_eq):
        self.regressor, self.log_interval, self.save_interval = regressor, log_interval, save_interval
        self.save_dir, self.print_eq = save_dir, print_eq

    def __call__(self, epoch, record, adopt=None, test=None):
        log, save = _at(epoch, self.log_interval), _at(epoch, self.save_interval)
        if (log or save) and adopt is not None:
            adopt()
        if log:
            print(', '.join([f'Epoch {epoch}'] + [f'{k}: {v:.4f}' for k, v in record.items()]))
            if test is not None:
                record.update(test(epoch))
            if self.print_eq:
                self.regressor.print()
        wandb.log(record)
        if save:
            _save(self.regressor, self.save_dir, f'regressor_{epoch}.pt')


def _lbfgs_phase(regressor, closure, losses, num_epochs, lr_sindy, st_freq, threshold, report, on_log=None, tol=1e-3,
                 shadow=None):
    """L-BFGS epochs with convergence-triggered / periodic thresholding       (train.py:692-766, 805-852).
    ``shadow`` (optional _HostShadow / _HostParams) owns the optimisation variables instead of the regressor."""
    P = shadow if shadow is not None else regressor
    sync = shadow.sync if shadow is not None else None
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
                if sync is not None:
                    sync()
                _save(regressor, report.save_dir, f'regressor_{epoch}.pt')
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
        report(epoch, wandb_log, adopt=sync, test=on_log)
    if sync is not None:
        sync()


def _train_on_device(regressor, x, dx, autoencoder, generator, num_epochs, lr_sindy, st_freq, threshold, w_sindy_x,
                     sindy_reg_type, w_sindy_reg, w_sym_reg, losses, report, test_log=None, group=None, gram_closure=False):
    """The non-latent L-BFGS fit with NOTHING on the host between two epochs (device_lbfgs.DeviceTrainer): closure kernel +
    ONE optimiser launch per inner iteration, the per-epoch logic of train.py:697-725 as one more launch, and a record per
    epoch in pinned memory from which this function produces what the reference produces per epoch -- the convergence /
    thresholding / NaN messages and, through ``report``, the loss line, the "test" line (train.py:739-751), the equations,
    the wandb record and the interval checkpoints -- in the reference's order.  The record holds the LAST closure
    evaluation's terms (what the reference's ``losses`` dict holds when the epoch ends) and, for the "test" line, the
    closure re-evaluated at the epoch's final coefficients and mask.  ``group``: x, dx are this rank's point shard.
    ``gram_closure``: the closure is the quadratic form of the batch's fp64 Gram matrices (gram_closure.py), built in one
    pass and summed over the ranks in one all-reduce; the fit itself then needs no collective."""
    from .device_lbfgs import DeviceTrainer
    d = x.shape[-1]
    rev = None
    if w_sym_reg > 0.0:
        gx, jgx = reversed_operands(x, autoencoder, generator)
        # device trainer: a leading problem axis, and the weight relative to w_sindy_x (its closure is w_x * (mse + ratio * sym))
        rev = (gx.reshape(1, gx.shape[0], -1, d), jgx.reshape(1, jgx.shape[0], -1, d, d), w_sym_reg / w_sindy_x)
    xs, dxs = x.reshape(1, -1, d).contiguous(), dx.reshape(1, -1, d).contiguous()
    coef = regressor.coef
    with torch.no_grad():
        P0 = coef.pack(regressor).cpu()[None]
        mask_before = regressor.mask.detach().cpu().numpy().copy()
    tr = DeviceTrainer(xs, dxs, regressor.poly_order, regressor.flags, coef=coef, reversed_sym=rev, lr=lr_sindy,
                       threshold=threshold, st_freq=st_freq, w_x=w_sindy_x, w_reg=w_sindy_reg if sindy_reg_type == 'l1' else 0.0,
                       l1=sindy_reg_type == 'l1', engine=regressor.engine, detail=True, group=group,
                       closure='gram' if gram_closure else 'stream')

    def terms(rec):
        out = {'loss_sindy_x': float(rec['mse'][0])}
        if rev is not None:
            out['loss_sym_reg'] = float(rec['sym'][0])
        if sindy_reg_type == 'l1':
            out['loss_sindy_reg'] = float(rec['l1'][0])
        return out

    return _fit_on_device(tr, regressor, P0, mask_before, num_epochs, threshold, terms, losses, report, test_log)


def _fit_on_device(tr, regressor, P0, mask_before, num_epochs, threshold, terms, losses, report, test_log):
    """Run a DeviceTrainer and produce from its per-epoch records what the reference produces per epoch, in its order
    (shared by _train_on_device and _train_latent_on_device).  ``terms(record)``: the epoch's entries of ``losses``."""
    from .device_lbfgs import EVENT_FINAL, EVENT_NAN, EVENT_THRESHOLD_CONVERGED, EVENT_THRESHOLD_PERIOD
    coef = regressor.coef
    state = {'mask_before': mask_before}

    def on_epoch(epoch, rec):
        code = int(rec['code'][0])
        if code == EVENT_NAN:                                                          # train.py:697-699
            print(f'NaN encountered at iteration {epoch}; exit training.')
            return True
        losses.update(terms(rec))
        adopt = partial(coef.adopt, regressor, rec['params'][0], rec['mask'][0])      # a host state into the regressor
        if code == EVENT_FINAL:                                                        # train.py:709-714
            print(f'Final convergence reached at iteration {epoch}; exit training.')
            adopt()
            _save(regressor, report.save_dir, f'regressor_{epoch}.pt')
            return True
        if code in (EVENT_THRESHOLD_CONVERGED, EVENT_THRESHOLD_PERIOD):
            regressor.note_near_threshold(rec['xi'][0], state['mask_before'], threshold, 'set_threshold (device trainer)')
            print('Convergence reached at iteration {}; apply parameter thresholding and reset optimizer.'.format(epoch)
                  if code == EVENT_THRESHOLD_CONVERGED else
                  'Max number of LBFGS iterations reached; apply parameter thresholding and reset optimizer.')
        state['mask_before'] = rec['mask'][0].copy()
        report(epoch, dict(losses), adopt=adopt,
               test=None if test_log is None else partial(test_log, value=float(rec['test'][0])))
        return False

    out = tr.fit(P0, num_epochs, mask0=torch.from_numpy(mask_before)[None], on_epoch=on_epoch,
                 test_eval=test_log is not None and report.log_interval > 0)
    coef.adopt(regressor, out['params'][0], out['mask'][0])
    return out


def _train_latent_on_device(regressor, x, dx, autoencoder, num_epochs, lr_sindy, st_freq, threshold, w_sindy_z, w_sindy_x,
                            sindy_reg_type, w_sindy_reg, losses, report, test_log=None):
    """The latent L-BFGS fit (train.py:647-661) as _train_on_device runs the observed-space one: z, dz and the QR-reduced
    decoder Jacobian are computed once (model_utils.latent_operands -- the autoencoder is frozen data under this optimiser),
    every closure is one symode_loss_grad_latent launch, optimiser and epoch logic stay on the device.  Same messages, same
    ``report`` records (loss_sindy_z, loss_sindy_x [, loss_sindy_reg]), same "test" line (test_loss_sindy_z at the epoch's
    final coefficients and mask), same checkpoints as the host_params route."""
    from .device_lbfgs import DeviceTrainer
    z, dz, B, y, e0, D = latent_operands(x, dx, autoencoder)
    n, d = z.shape
    x_const = e0 / (n * D)                       # the part of loss_sindy_x no coefficient reaches: |dx - Q Q^T dx|^2
    coef = regressor.coef
    with torch.no_grad():
        P0 = coef.pack(regressor).cpu()[None]
        mask_before = regressor.mask.detach().cpu().numpy().copy()
    # the trainer's loss value is w_x * (loss2[0] + w_pair * loss2[1]) with both sums under 1 / (n d); like the reference's,
    # its gradient is the z-term's alone (compute_dx cuts the x-term from the graph: device_lbfgs.DeviceTrainer)
    tr = DeviceTrainer(z[None].float(), dz[None].float(), regressor.poly_order, regressor.flags, coef=coef, lr=lr_sindy,
                       threshold=threshold, st_freq=st_freq, w_x=w_sindy_z, w_reg=w_sindy_reg if sindy_reg_type == 'l1' else 0.0,
                       l1=sindy_reg_type == 'l1', engine=regressor.engine, detail=True, closure='latent',
                       latent=(B[None].float(), y[None].float(), (w_sindy_x / w_sindy_z) * (d / D)))

    def terms(rec):
        out = {'loss_sindy_z': float(rec['mse'][0]), 'loss_sindy_x': float(rec['sym'][0]) * d / D + x_const}
        if sindy_reg_type == 'l1':
            out['loss_sindy_reg'] = float(rec['l1'][0])
        return out

    return _fit_on_device(tr, regressor, P0, mask_before, num_epochs, threshold, terms, losses, report, test_log)


def _lbfgs_route(is_cuda, use_latent, w_sym_reg, sym_reg_type, w_sindy_x, sindy_reg_type, frozen, group, host_lbfgs,
                 torch_lbfgs, numpy_lbfgs, gram_closure, torch_optim_env, mask_numel, has_trainer, fused_latent=False,
                 w_sindy_z=1.0, has_latent=True):
    """Which of the five ways train_SIGED_lbfgs runs a fit ("The five routes"), from its arguments alone.
    ``fused``: the closure is made only of fused kernels.  'device': a fused fit on _train_on_device, the DEFAULT; 'shadow':
    a fused fit that asked for torch's / numpy's optimiser or that the device trainer does not cover, variables on a
    _HostShadow, one rank; 'host_params': an autograd closure on the GPU, variables on a _HostParams; 'plain': the
    regressor's own parameters (CPU, host_lbfgs=False).  ``torch_optim_env``: SYMODE_TORCH_OPTIM=1.
    'latent' (opt-in, ``fused_latent`` with ``use_latent``; ignored without it): the latent fit on _train_latent_on_device;
    what it does not cover is refused by name, never rerouted.  ``w_sindy_z`` and ``has_latent`` (the library exports
    symode_loss_grad_latent) are read on that route only."""
    if group is not None and use_latent:
        raise ValueError('group=... (point shards) is implemented for the non-latent fit.')
    if fused_latent and use_latent:
        needs = (('a GPU', is_cuda), ('host_lbfgs=True', host_lbfgs),
                 ('the device optimiser: no torch_lbfgs / numpy_lbfgs / SYMODE_TORCH_OPTIM=1',
                  not (torch_lbfgs or numpy_lbfgs or torch_optim_env)),
                 ('w_sindy_z > 0', w_sindy_z > 0), ("sindy_reg_type 'l1' or 'none'", sindy_reg_type in ('l1', 'none')),
                 ('at most 256 coefficients', mask_numel <= 256),
                 ('symode_loss_grad_latent and the device trainer in the library', has_latent and has_trainer),
                 ('gram_closure=False: the latent closure has no Gram form', not gram_closure))
        for what, ok in needs:
            if not ok:
                raise ValueError(f'fused_latent=True needs {what}')
        return 'latent'
    fused = is_cuda and not use_latent and host_lbfgs and (w_sym_reg <= 0.0 or (sym_reg_type == 'r' and frozen))
    if (fused and not (torch_lbfgs or numpy_lbfgs or torch_optim_env) and w_sindy_x > 0
            and sindy_reg_type in ('l1', 'none') and has_trainer and mask_numel <= 256):
        return 'device'
    if gram_closure:
        raise ValueError('gram_closure=True needs the device trainer: the non-latent fit with MSE [+ L1] [+ the reversed '
                         'regulariser on a frozen autoencoder] on a GPU, without torch_lbfgs / numpy_lbfgs')
    if fused and group is None:
        return 'shadow'
    return 'host_params' if is_cuda and host_lbfgs else 'plain'


_LossTerms = namedtuple('_LossTerms', 'w_sindy_z w_sindy_x sindy_reg_type w_sindy_reg sym_reg_type w_sym_reg int_t int_dt')


def _reg_term(reg, loss, losses, sindy_reg_type, w_sindy_reg):
    if sindy_reg_type == 'l1':                                                         # raw (unmasked) params, :680-683
        loss_sindy_reg = sum(torch.norm(p, 1) for p in reg.parameters())
        losses['loss_sindy_reg'] = loss_sindy_reg.detach()
        return loss + w_sindy_reg * loss_sindy_reg
    if sindy_reg_type == 'none':
        return loss
    raise ValueError(f'Unknown regularization type: {sindy_reg_type}')


def _autograd_closure(regressor, x, dx, autoencoder, symm_loss, terms, losses, use_latent, group):
    """The reference's closure (train.py:645-690) term by term: latent or observed-space fit, the i / f / r regulariser
    through ``symm_loss``, optionally over point shards (``group``)."""
    w_sindy_z, w_sindy_x, sindy_reg_type, w_sindy_reg, sym_reg_type, w_sym_reg, int_t, int_dt = terms

    def closure(optimizer):
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
        loss = _reg_term(regressor, loss, losses, sindy_reg_type, w_sindy_reg)
        loss.backward()
        return loss
    return closure


def _shadow_closure(shadow, engine, terms, losses):
    """The same terms as train.py:645-690 on a _HostShadow's torch variables: value and Xi-gradient of every fused term come
    from the device, autograd carries them through get_Xi on the host.  With the reversed regulariser on the zero-copy
    shadow, MSE and regulariser are ONE launch (one pass over the points)."""
    _, w_sindy_x, sindy_reg_type, w_sindy_reg, _, w_sym_reg, _, _ = terms
    rev = shadow.reversed_sym
    one_launch = (rev is not None and shadow.zero_copy and w_sindy_x > 0 and hasattr(engine, 'loss_grad_reversed'))

    def closure(optimizer):
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
    return closure


def _shadow_closure_numpy(shadow, terms, losses):
    """The fused terms on a _HostShadow's flat numpy variables, for _NumpyLBFGS: ``closure(flat) -> (loss, flat gradient)``."""
    _, w_sindy_x, sindy_reg_type, w_sindy_reg, _, w_sym_reg, _, _ = terms
    rev = shadow.reversed_sym

    def closure_np(flat):
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
    return closure_np


def _distill_closure(regressor_dst, x, dx, terms, losses):
    """Phase 2 (train.py:805-830): the data-space regressor on (x, decoded latent prediction)."""
    def closure_dst(optimizer):
        optimizer.zero_grad()
        loss_sindy_x = regressor_dst.mse_loss(x, dx)
        losses['loss_sindy_x'] = loss_sindy_x.detach()
        loss = _reg_term(regressor_dst, terms.w_sindy_x * loss_sindy_x, losses, terms.sindy_reg_type, terms.w_sindy_reg)
        loss.backward()
        return loss
    return closure_dst


def _test_log(epoch, value=None, *, regressor, x, dx, autoencoder, test_loader, use_latent, group):
    # ``value``: the closure at the epoch's final coefficients and mask, already evaluated by the device trainer.
    # The reference evaluates the TRAIN batch once per element of test_loader here (:739-751): the same number, n times
    # (lv: n = 780 at every logged epoch -- 45 % of the wall time of lv/noise99_eq_isymreg.cfg).  It is evaluated once
    # and accumulated n times in the reference's float arithmetic, so the logged mean is the reference's bit for bit.
    out = {'test_loss_sindy_z': 0.0, 'test_loss_sindy_x': 0.0}
    n = len(test_loader) if hasattr(test_loader, '__len__') else sum(1 for _ in test_loader)
    if n > 0:
        with torch.no_grad():
            if use_latent and value is None:
                z, _ = autoencoder(x)
                key, v = 'test_loss_sindy_z', regressor.mse_loss(z, autoencoder.compute_dz(x, dx)).item()
            elif value is not None:
                key, v = 'test_loss_sindy_z' if use_latent else 'test_loss_sindy_x', value
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


_SYMM_LOSS = {'i': make_symmreg_pttrain, 'f': make_fsymmreg_pttrain, 'r': make_rsymmreg_pttrain}


def train_SIGED_lbfgs(
    train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir,  # global
    autoencoder, generator,  # symmetry discovery model
    regressor, regressor_dst, use_latent, distill_latent, lr_sindy, w_sindy_z, w_sindy_x,  # SINDy
    sindy_reg_type, w_sindy_reg, sym_reg_type, w_sym_reg, st_freq, threshold, int_t, int_dt,  # SINDy
    gram_closure=False, fused_latent=False, **kwargs
):
    """Full-batch L-BFGS fit (train.py:617-852): read the one batch, pick the route (_lbfgs_route), build that route's
    closure, run phase 1, optionally distill the latent equation into data space (phase 2).

    numpy_lbfgs=True swaps torch.optim.LBFGS for the numpy restatement (_NumpyLBFGS): 2.7x faster end to end, same results
    on well-conditioned problems, but NOT the default: on ill-conditioned libraries (selkov, cond 9e3, lr 1.0, no line
    search) the trajectory is chaotic in the last bits of every dot product and only torch's own optimiser reproduces the
    reference's recorded run bit-for-bit in its mask.  torch's own optimiser on host-resident variables (the
    reference's torch.optim.LBFGS, operation for operation) stays available: --torch_lbfgs / torch_lbfgs=True /
    SYMODE_TORCH_OPTIM=1."""
    if distill_latent and not use_latent:
        raise ValueError('Cannot distill without first learning latent space equation. Set use_latent=True.')
    x, dx = next(iter(train_loader))                                                   # ONE fixed batch (train.py:626)
    x, dx = x.to(device), dx.to(device)
    symm_loss = _SYMM_LOSS[sym_reg_type](autoencoder, generator) if sym_reg_type in _SYMM_LOSS else None
    autoencoder.eval()
    generator.eval()
    losses = {}
    group = kwargs.get('group')                # point shards: x, dx of train_loader are this rank's slice of the batch
    host_lbfgs = kwargs.get('host_lbfgs', True)
    terms = _LossTerms(w_sindy_z, w_sindy_x, sindy_reg_type, w_sindy_reg, sym_reg_type, w_sym_reg, int_t, int_dt)
    route = _lbfgs_route(
        is_cuda=x.is_cuda, use_latent=use_latent, w_sym_reg=w_sym_reg, sym_reg_type=sym_reg_type, w_sindy_x=w_sindy_x,
        sindy_reg_type=sindy_reg_type, group=group, host_lbfgs=host_lbfgs, torch_lbfgs=kwargs.get('torch_lbfgs', False),
        numpy_lbfgs=kwargs.get('numpy_lbfgs', False), gram_closure=gram_closure,
        frozen=not any(p.requires_grad for m in (autoencoder, generator) for p in m.parameters()),
        torch_optim_env=os.environ.get('SYMODE_TORCH_OPTIM', '0') == '1', mask_numel=regressor.mask.numel(),
        has_trainer=hasattr(getattr(regressor.engine, 'lib', None), 'symode_trainer_run'), fused_latent=fused_latent,
        w_sindy_z=w_sindy_z, has_latent=hasattr(getattr(regressor.engine, 'lib', None), 'symode_loss_grad_latent'))
    report = _EpochReport(regressor, log_interval, save_interval, save_dir, kwargs.get('print_eq', False))
    test_log = partial(_test_log, regressor=regressor, x=x, dx=dx, autoencoder=autoencoder, test_loader=test_loader,
                       use_latent=use_latent, group=group)
    if route == 'device':
        _train_on_device(regressor, x, dx, autoencoder, generator, num_epochs, lr_sindy, st_freq, threshold, w_sindy_x,
                         sindy_reg_type, w_sindy_reg, w_sym_reg, losses, report, test_log=test_log, group=group,
                         gram_closure=gram_closure)
    elif route == 'latent':
        _train_latent_on_device(regressor, x, dx, autoencoder, num_epochs, lr_sindy, st_freq, threshold, w_sindy_z, w_sindy_x,
                                sindy_reg_type, w_sindy_reg, losses, report, test_log=test_log)
    else:
        if route == 'shadow':
            # host shadow: (n_g, N, d) / (n_g, N, d, d) as they come, the closure weighs the regulariser by w_sym_reg itself
            rev = reversed_operands(x, autoencoder, generator) if w_sym_reg > 0.0 else None
            shadow = _HostShadow(regressor, x, dx, reversed_sym=rev, numpy_vars=kwargs.get('numpy_lbfgs', False),
                                 use_graph=kwargs.get('hip_graph', True), zero_copy=kwargs.get('zero_copy', True))
            closure = (_shadow_closure_numpy(shadow, terms, losses) if shadow.flat is not None
                       else _shadow_closure(shadow, regressor.engine, terms, losses))
        else:
            shadow = None
            closure = _autograd_closure(regressor, x, dx, autoencoder, symm_loss, terms, losses, use_latent, group)
            if route == 'host_params':                 # the closure stays on the device, the optimiser's variables move to the host
                shadow = _HostParams(regressor)
                closure = shadow.wrap(closure)
        _lbfgs_phase(regressor, closure, losses, num_epochs, lr_sindy, st_freq, threshold, report, on_log=test_log,
                     shadow=shadow)

    # (Optional) Phase 2: distill equation from latent to data space                   # train.py:768-852
    if not distill_latent:
        return
    print('\n=== Phase 2: distill equation from latent to data space ===\n')
    with torch.no_grad():
        z, _ = autoencoder(x)
        dx = autoencoder.compute_dx(z, regressor(z))
    losses = {}
    closure_dst, shadow_dst = _distill_closure(regressor_dst, x, dx, terms, losses), None
    if x.is_cuda and host_lbfgs:
        shadow_dst = _HostParams(regressor_dst)
        closure_dst = shadow_dst.wrap(closure_dst)
    _lbfgs_phase(regressor_dst, closure_dst, losses, num_epochs, lr_sindy, st_freq, threshold,
                 _EpochReport(regressor_dst, log_interval, save_interval, save_dir, report.print_eq), shadow=shadow_dst)


def _test_loss_line(epoch, regressor, test_loader, device):
    """The Adam trainers' test line (train.py:560-570): the mean of the per-batch MSE over ``test_loader``, printed and
    returned for the record; nothing for an empty loader."""
    with torch.no_grad():
        tl = [regressor.mse_loss(xt.to(device), dxt.to(device)).item() for xt, dxt in test_loader]
    if not tl:
        return {}
    out = {'test_loss_sindy_x': float(np.mean(tl))}
    print(f"Epoch {epoch}, test_loss_sindy_x: {out['test_loss_sindy_x']:.4f}")
    return out


def _epoch_orders(train_loader, num_epochs, order_seed):
    """How DeviceAdam.fit gets its rows: the loader's own shuffles as one table per epoch, or the order seed alone."""
    if order_seed is not None:
        return dict(order_seeds=[int(order_seed)], shuffle=train_loader.shuffle)
    return dict(orders=(train_loader.epoch_order()[None] for _ in range(num_epochs)))


def _train_adam_on_device(train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir, regressor,
                          use_latent, lr_sindy, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg, st_freq, threshold,
                          print_eq, sym_reg_type=None, autoencoder=None, generator=None, w_sindy_z=0.0, order_seed=None):
    """train_SIGED's plain branch on DeviceAdam: the same shuffles (one ``randperm`` per epoch from the global generator, as
    the loader draws them; with ``order_seed`` -- --device_shuffle -- none is drawn: the launch computes epoch e's rows from
    (order_seed, e), device_adam.epoch_order, an equivalent draw with other rows per step, not a replay), prints, wandb records, test loss and checkpoints at the same epochs, produced from the
    launch's log and from the state adopted into the regressor at those epochs and at the end.  ``w_sym_reg > 0`` with
    ``sym_reg_type 'r'`` and a frozen autoencoder and generator adds ``w_sym_reg * symmreg_r`` to every minibatch loss:
    g(x), J_g(x) are computed once over the loader's rows.
    ``use_latent`` runs the latent branch (_train_adam_latent_on_device)."""
    from .dataset import DeviceBatches
    if use_latent:
        return _train_adam_latent_on_device(train_loader, num_epochs, log_interval, save_interval, save_dir, regressor, lr_sindy,
                                            w_sindy_z, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg, st_freq, threshold,
                                            print_eq, autoencoder, generator, order_seed)
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
    if sym:
        # device Adam: over the loader's rows in chunks, and the weight as it stands (w_x * mse + w_sym_reg * regulariser)
        rev = (*reversed_operands(x, autoencoder, generator, chunk=PRECOMPUTE_CHUNK), w_sym_reg)
    trainer = DeviceAdam(x, dx, regressor.poly_order, regressor.include_sine, regressor.include_exp, coef, lr_sindy, w_sindy_x,
                         w_sindy_reg, threshold, st_freq, train_loader.bs, engine=regressor.engine, reversed_sym=rev)
    last_mask = [regressor.mask.detach().clone()]
    report = _EpochReport(regressor, log_interval, save_interval, save_dir, print_eq)

    def on_epoch(epoch, rec):
        wandb_log = {'loss_sindy_x': float(rec['loss_sindy_x'][0]), 'loss_sindy_z': 0.0,
                     'loss_sindy_reg': float(rec['loss_sindy_reg'][0]),
                     'loss_sym_reg': float(rec['loss_sym_reg'][0]) if sym else 0.0}
        state = rec['state']
        if _at(epoch, st_freq) and not rec['nan'][0]:                                  # train.py:545-546
            regressor.note_near_threshold(state['Xi'][0], last_mask[0], threshold, 'set_threshold (device Adam)')
            last_mask[0] = state['mask'][0].clone()
        report(epoch, wandb_log, adopt=partial(coef.adopt, regressor, state['params'][0], state['mask'][0]),
               test=partial(_test_loss_line, regressor=regressor, test_loader=test_loader, device=device))

    regressor.train()
    out = trainer.fit(coef.pack(regressor)[None], num_epochs, **_epoch_orders(train_loader, num_epochs, order_seed),
                      mask0=regressor.mask[None], on_epoch=on_epoch,
                      boundary=lambda epoch: any(_at(epoch, every) for every in (log_interval, save_interval, st_freq)))
    coef.adopt(regressor, out['params'][0], out['mask'][0])


def _train_adam_latent_on_device(train_loader, num_epochs, log_interval, save_interval, save_dir, regressor, lr_sindy, w_sindy_z,
                                 w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg, st_freq, threshold, print_eq, autoencoder,
                                 generator, order_seed=None):
    """train_SIGED's ``use_latent`` branch on DeviceAdam(latent=...): the optimiser steps the SINDy coefficients alone, so the
    autoencoder is data -- z, dz, the QR-reduced decoder Jacobian and the per-row constant of loss_sindy_x are computed once
    over the loader's rows (model_utils.latent_operands), the generators are read once, and every epoch is part of one
    launch.  Same shuffles, prints, records and checkpoints as the tensor-op branch; no test line, as there.
    ``sym_reg_type`` is not read, as there: the regulariser of this branch is the linear-latent one whenever w_sym_reg > 0."""
    from .dataset import DeviceBatches
    if not w_sindy_z > 0:
        raise ValueError(f'device_adam with use_latent needs w_sindy_z > 0 (here {w_sindy_z}): loss_sindy_x has no gradient '
                         '(compute_dx cuts it from the graph), so without it no data term reaches the coefficients')
    # training mode matters where a layer depends on it: batch norm on batch statistics is not pointwise, and it moves
    mode_layers = (torch.nn.modules.batchnorm._BatchNorm, torch.nn.modules.dropout._DropoutNd)
    in_training = autoencoder.training and any(isinstance(layer, mode_layers) for layer in autoencoder.modules())
    if any(q.requires_grad for q in autoencoder.parameters()) or in_training:
        raise ValueError('device_adam with use_latent needs a frozen autoencoder in eval mode (no parameter requires grad, '
                         'batch norm pointwise): z, dz and the decoder Jacobian are computed once')
    arrays = getattr(train_loader, 'arrays', None)                   # (a loader without arrays is refused below, by its type)
    if arrays is not None and arrays[0].dim() != 2:
        raise ValueError(f'device_adam with use_latent needs one latent point per row: the items are {tuple(arrays[0].shape[1:])}, '
                         'not single (D,) points (n_comps > 1)')
    if sindy_reg_type != 'l1':
        raise ValueError(f"device_adam covers sindy_reg_type 'l1', not '{sindy_reg_type}'")
    if not isinstance(train_loader, DeviceBatches):
        raise ValueError(f'device_adam needs train_loader to be a DeviceBatches, got {type(train_loader).__name__}')
    if train_loader.window != 0:
        raise ValueError(f'device_adam needs single-row items: train_loader.window is {train_loader.window}, not 0')
    x, dx = train_loader.arrays
    if not (x.is_cuda and dx.is_cuda):
        raise ValueError('device_adam needs the data set resident on the device (DeviceBatches kept it in host memory)')
    was_training = autoencoder.training                      # (only without a layer that reads the flag, see above)
    autoencoder.eval()
    try:
        z, dz, B, y, e, D = latent_operands(x, dx, autoencoder, per_row=True)
    finally:
        autoencoder.train(was_training)
    if z.shape != (x.shape[0], regressor.latent_dim):
        raise ValueError(f'device_adam with use_latent needs one latent point per row: the {x.shape[0]} rows encode to z '
                         f'{tuple(z.shape)}, not ({x.shape[0]}, {regressor.latent_dim}) (n_comps > 1)')
    from .device_adam import DeviceAdam
    coef = regressor.coef
    d = z.shape[1]
    L = None
    if w_sym_reg > 0:
        L = torch.stack([v[:d, :d] for v in generator.get_full_basis_list()]).detach().to(z.device).float().contiguous()
    trainer = DeviceAdam(z.float(), dz.float(), regressor.poly_order, regressor.include_sine, regressor.include_exp, coef, lr_sindy,
                         w_sindy_x, w_sindy_reg, threshold, st_freq, train_loader.bs, engine=regressor.engine,
                         latent=(B.float(), y.float(), e.float() if D > d else None, D, L, w_sindy_z, w_sym_reg if L is not None else 0.0))
    last_mask = [regressor.mask.detach().clone()]
    report = _EpochReport(regressor, log_interval, save_interval, save_dir, print_eq)

    def on_epoch(epoch, rec):
        wandb_log = {k: float(rec[k][0]) for k in ('loss_sindy_x', 'loss_sindy_z', 'loss_sindy_reg', 'loss_sym_reg')}
        state = rec['state']
        if _at(epoch, st_freq) and not rec['nan'][0]:                                  # train.py:545-546
            regressor.note_near_threshold(state['Xi'][0], last_mask[0], threshold, 'set_threshold (device Adam)')
            last_mask[0] = state['mask'][0].clone()
        report(epoch, wandb_log, adopt=partial(coef.adopt, regressor, state['params'][0], state['mask'][0]), test=None)

    regressor.train()
    out = trainer.fit(coef.pack(regressor)[None], num_epochs, **_epoch_orders(train_loader, num_epochs, order_seed),
                      mask0=regressor.mask[None], on_epoch=on_epoch,
                      boundary=lambda epoch: any(_at(epoch, every) for every in (log_interval, save_interval, st_freq)))
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
    with ``sym_reg_type='r'`` and a frozen LaLiGAN also under the reversed symmetry regulariser; the ``use_latent`` branch
    runs there too under a frozen autoencoder in eval mode with ``w_sindy_z > 0`` (the linear-latent regulariser included);
    any other configuration is refused, not silently run the usual way.  ``device_shuffle=True`` (--device_shuffle, with
    device_adam only): the epoch launches compute their rows from (``seed``, epoch) instead of reading the loader's shuffles."""
    if kwargs.get('device_shuffle') and not kwargs.get('device_adam'):
        raise ValueError('device_shuffle is the epoch order of the device Adam fit: it needs device_adam (--device_adam)')
    if kwargs.get('device_adam'):
        return _train_adam_on_device(train_loader, test_loader, num_epochs, device, log_interval, save_interval, save_dir,
                                     regressor, use_latent, lr_sindy, w_sindy_x, sindy_reg_type, w_sindy_reg, w_sym_reg,
                                     st_freq, threshold, kwargs.get('print_eq'), sym_reg_type=kwargs.get('sym_reg_type'),
                                     autoencoder=autoencoder, generator=generator, w_sindy_z=w_sindy_z,
                                     order_seed=kwargs.get('seed', 0) if kwargs.get('device_shuffle') else None)
    optimizer_sindy = torch.optim.Adam(regressor.parameters(), lr=lr_sindy)
    symm_loss = make_symmreg_pttrain(autoencoder, generator)
    report = _EpochReport(regressor, log_interval, save_interval, save_dir, kwargs.get('print_eq'))
    test = None if use_latent else partial(_test_loss_line, regressor=regressor, test_loader=test_loader, device=device)
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
        report(epoch, {k: float(np.mean(v)) for k, v in running.items()}, test=test)


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
