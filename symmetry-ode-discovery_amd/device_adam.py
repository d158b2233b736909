"""Minibatch Adam fit of the SINDy coefficients with whole epochs per launch (symode_adam_epochs, csrc/adam.hpp): the plain
branch of ``train.train_SIGED`` -- per minibatch ``w_x * mse + w_reg * |params|_1``, backward, ``torch.optim.Adam.step``, and
``set_threshold`` every ``st_freq`` epochs -- for S independent problems (seeds) on ONE shared data set, one workgroup per
problem, nothing on the host inside a launch.

Covered: the observed-space fit, unconstrained or under the equivariance constraint (any ``CoefMap``), L1 regulariser, and
the reversed symmetry regulariser on operands g(x), J_g(x) computed once for the data set (``reversed_sym``,
symode_adam_epochs_reversed: ``+ w_sym * sum_g mean |J_g(x) h(x) - h(g x)|^2`` per minibatch).
The ``--use_latent`` branch under a frozen autoencoder (``latent``, symode_adam_epochs_latent): x, dx are then z, dz, and
every minibatch loss is ``w_z * mse_z + w_x * mse_x + w_sym * (linear-latent regulariser, not divided by the rows)`` on the
per-row operands of ``model_utils.latent_operands``; mse_x is logged and added but has no gradient, as in train_SIGED.
The rows of a step come from an index table built from the caller's shuffles, or -- ``fit(order_seeds=...)``, the device
shuffle -- from the launch itself, which computes them from (order seed, epoch, position) by ``epoch_order``'s function
(symode_adam_epochs*_keyed): no table, nothing between two launches, an equivalent draw of the shuffle rather than a replay.
``fit(hyper=...)`` gives every problem its own lr, w_reg, threshold and w_sym -- a hyper-parameter grid over common seeds in
one launch (symode_adam_run): problem s is, bit for bit, the fit of a trainer built with problem s's scalars.
Not covered (the callers refuse them): the i / f symmetry regularisers (they run the autoencoder on Xi-dependent inputs), a
latent fit whose autoencoder trains, several ranks.
"""
from __future__ import annotations

import numpy as np
import torch

from .engine import get_engine, library_flags
from .sindy import NEAR_THRESHOLD_BAND

# Bytes of index table handed to one launch: an epoch's table is 4 bytes per (problem, row) -- 0.5 MB for one problem on the
# 125 000-row sets, 32 MB for 64 seeds with their own shuffles -- and epochs_per_launch of them are stacked, next to the
# int64 permutations they are cut from.  Beyond this bound a launch takes fewer epochs.
TABLE_BYTES = 256 << 20

LOG_COLUMNS = ('loss_sindy_x', 'loss_sindy_reg', 'steps', 'near', 'nan', 'event', 'epoch')
# records of a trainer with ``reversed_sym``: column 7 is the epoch mean of the batch regulariser (unweighted)
LOG_COLUMNS_REVERSED = LOG_COLUMNS + ('loss_sym_reg',)
# records of a trainer with ``latent``: ten columns, the three loss terms unweighted
LOG_COLUMNS_LATENT = LOG_COLUMNS + ('loss_sym_reg', 'loss_sindy_z', 'unused')
# the columns of a problem's hyper-parameter row (SYMODE_ADAM_HYPER of include/symode.h), by the names ``fit(hyper=...)`` takes
HYPER_COLUMNS = ('lr', 'w_reg', 'threshold', 'w_sym')


ORDER_ROUNDS = 2          # ADAM_ORDER_ROUNDS of csrc/adam_order.hpp
_M32 = np.uint64(0xFFFFFFFF)


def _seed_words(seed):
    """``seed_words`` of csrc/adam_order.hpp: the 64-bit mix of a seed, as (low word, high word)."""
    m64 = (1 << 64) - 1
    z = ((int(seed) & m64) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & m64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & m64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & m64
    z ^= z >> 31
    return z & 0xFFFFFFFF, z >> 32


def _subsample_key(a, b, row):
    """``subsample_key``: fmix32((row ^ a) * 0x9E3779B1 + b) on Python integers."""
    m32 = 0xFFFFFFFF
    h = (((row ^ a) & m32) * 0x9E3779B1 + b) & m32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m32
    h ^= h >> 16
    return h


def _order_mix(k, half):
    """``adam_order_mix``: uint64 arrays that hold 32-bit words, every step reduced mod 2^32."""
    h = (np.uint64(k) + ((half + np.uint64(1)) & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779)) & _M32
    for down, up in ((15, 3), (11, 7), (13, 5)):
        h ^= h >> np.uint64(down)
        h = (h + (h << np.uint64(up))) & _M32
    h ^= h >> np.uint64(16)
    return h


def epoch_order(seed, epoch, n, rounds=ORDER_ROUNDS):
    """The row order of epoch ``epoch`` (the GLOBAL epoch number of the fit) under order seed ``seed``: a permutation of
    range(n) as int32, entry for entry what ``adam_order_row`` (csrc/adam_order.hpp) computes inside the keyed epoch
    launches.  A function of (seed, epoch, n) alone.  ``rounds`` is for the uniformity study only; the kernels use
    ORDER_ROUNDS.

    n == 1: the identity.  Otherwise bits = ceil(log2 n), and a position is a word (hi | lo) of ``bits`` bits whose low part
    has lb bits.  Round r = 0 .. ORDER_ROUNDS - 1 maps
        (hi | lo) -> (lo | (hi ^ F(k_r, lo)) mod 2^(bits - lb)),   lb <- bits - lb,
    starting from lb = bits - bits // 2 (an alternating unbalanced Feistel network, a bijection of [0, 2^bits), 2^bits < 2 n).
    Round key k_r = subsample_key(a, b, (epoch * ORDER_ROUNDS + r) mod 2^32), (a, b) the low and high word of
    seed_words(seed).  F(k, lo), all mod 2^32:
        h = k + (lo + 1) * 0x9E3779          (lo < 2^16: a 24-bit multiply)
        h ^= h >> 15;  h += h << 3;  h ^= h >> 11;  h += h << 7;  h ^= h >> 13;  h += h << 5;  h ^= h >> 16
    The network is applied again to every value that is still >= n (cycle walking): the walk follows the cycle of a
    permutation that started below n, so it ends."""
    n = int(n)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f'n must be in [1, 2^31), got {n}')
    if n == 1:
        return np.zeros(1, dtype=np.int32)
    a, b = _seed_words(seed)
    keys = [_subsample_key(a, b, (int(epoch) * rounds + r) & 0xFFFFFFFF) for r in range(rounds)]
    bits = (n - 1).bit_length()
    x = np.arange(n, dtype=np.uint64)
    walk = np.arange(n)                                   # the entries still on their walk
    while walk.size:
        y = x[walk]
        lb = bits - bits // 2
        for k in keys:
            hb = bits - lb
            lo, hi = y & np.uint64((1 << lb) - 1), y >> np.uint64(lb)
            y = (lo << np.uint64(hb)) | ((hi ^ _order_mix(k, lo)) & np.uint64((1 << hb) - 1))
            lb = hb
        x[walk] = y
        walk = walk[y >= n]
    return x.astype(np.int32)


class DeviceAdam:
    def __init__(self, x, dx, poly_order, include_sine, include_exp, coef, lr, w_sindy_x, w_sindy_reg, threshold, st_freq,
                 batch_size, betas=(0.9, 0.999), eps=1e-8, engine=None, reversed_sym=None, latent=None):
        """x, dx (n, d) fp32 on the device, shared by all problems; ``coef``: the CoefMap of the parametrisation;
        ``reversed_sym``: (gx (n_g, n, d), jgx (n_g, n, d, d), w_sym) on the device of x, or None;
        ``latent``: (B (n, d, d), y (n, d), e (n,) or None with D_obs == d, D_obs, L (n_gen, d, d) or None, w_z, w_sym) on the
        device of x, or None -- with it x, dx are z, dz and ``w_sindy_x`` weighs mse_x."""
        self.engine = engine or get_engine()
        self.x, self.dx = x.contiguous(), dx.contiguous()
        self.n, self.d = self.x.shape
        self.order, self.flags = int(poly_order), library_flags(include_sine, include_exp)
        self.coef = coef.to(self.x.device)
        if (self.coef.d, self.coef.p) != (self.d, self.engine.lib_size(self.d, self.order, self.flags)):
            raise ValueError(f'coefficient map is ({self.coef.d}, {self.coef.p}), the library of the data is '
                             f'({self.d}, {self.engine.lib_size(self.d, self.order, self.flags)})')
        self.q_eff = None
        if self.coef.Q is not None:
            self.q_eff = torch.from_numpy(self.coef.effective_Q()).to(self.x.device).contiguous()
        self.lr, self.w_x, self.w_reg = float(lr), float(w_sindy_x), float(w_sindy_reg)
        self.threshold, self.st_freq = float(threshold), int(st_freq)
        self.batch = int(batch_size)
        if self.batch < 1:
            raise ValueError(f'batch_size {batch_size} < 1')
        self.steps = (self.n + self.batch - 1) // self.batch
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.reversed_sym = None
        if reversed_sym is not None:
            gx, jgx, w_sym = reversed_sym
            for name, t, shape in (('gx', gx, (self.n, self.d)), ('jgx', jgx, (self.n, self.d, self.d))):
                if not isinstance(t, torch.Tensor) or t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
                    raise ValueError(f'reversed_sym {name} must be (n_g, {", ".join(map(str, shape))}) like x '
                                     f'{tuple(self.x.shape)}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
                if t.device != self.x.device or t.dtype != torch.float32:
                    raise ValueError(f'reversed_sym {name} must be fp32 on {self.x.device}, got {t.dtype} on {t.device}')
            if gx.shape[0] != jgx.shape[0]:
                raise ValueError(f'reversed_sym holds {gx.shape[0]} group elements in gx, {jgx.shape[0]} in jgx')
            if gx.shape[0] > 0 and not self.w_x > 0:
                raise ValueError(f'reversed_sym needs w_sindy_x > 0 (the regulariser is weighed against it), got {self.w_x}')
            self.reversed_sym = (gx.contiguous(), jgx.contiguous(), float(w_sym))
        self.latent = None
        if latent is not None:
            if reversed_sym is not None:
                raise ValueError('reversed_sym and latent are two different losses: give one of them')
            B, y, e, D_obs, L, w_z, w_sym = latent
            D_obs = int(D_obs)
            if D_obs < self.d:
                raise ValueError(f'latent D_obs is {D_obs}, below the latent dimension {self.d} of x {tuple(self.x.shape)}')
            if e is None and D_obs > self.d:
                raise ValueError(f'latent e must be (n,) with D_obs {D_obs} > d {self.d}, got None')
            for name, t, shape in (('B', B, (self.n, self.d, self.d)), ('y', y, (self.n, self.d)), ('e', e, (self.n,)),
                                   ('L', L, (self.d, self.d))):
                if t is None and name in 'eL':
                    continue
                lead = 1 if name == 'L' else 0
                if not isinstance(t, torch.Tensor) or t.dim() != len(shape) + lead or tuple(t.shape[lead:]) != shape:
                    raise ValueError(f'latent {name} must be ({"n_gen, " if lead else ""}{", ".join(map(str, shape))}) like x '
                                     f'{tuple(self.x.shape)}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
                if t.device != self.x.device or t.dtype != torch.float32:
                    raise ValueError(f'latent {name} must be fp32 on {self.x.device}, got {t.dtype} on {t.device}')
            if not float(w_z) > 0:
                raise ValueError(f'latent needs w_sindy_z > 0 (mse_x has no gradient and the regulariser is weighed against '
                                 f'mse_z), got {w_z}')
            cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
            self.latent = (B.contiguous(), y.contiguous(), cont(e), D_obs, cont(L), float(w_z), float(w_sym))
        self.log_columns = (LOG_COLUMNS_LATENT if self.latent is not None
                            else LOG_COLUMNS if self.reversed_sym is None else LOG_COLUMNS_REVERSED)

    def table(self, order):
        """One epoch's (S or 1, n) permutation cut into (S or 1, steps, batch) int32 row numbers, the short last batch
        padded with -1 (which the kernel neither reads nor counts)."""
        if order.dim() != 2 or order.shape[1] != self.n:
            raise ValueError(f'an epoch order must be (S or 1, {self.n}), got {tuple(order.shape)}')
        pad = self.steps * self.batch - self.n
        t = order.to(torch.int32)
        if pad:
            t = torch.cat([t, torch.full((t.shape[0], pad), -1, dtype=torch.int32, device=t.device)], dim=1)
        return t.view(t.shape[0], self.steps, self.batch)

    def hyper_table(self, hyper, S):
        """The (S, 4) fp32 device table [lr, w_reg, threshold, w_sym] of ``fit(hyper=...)``: every given key a length-S sequence
        or tensor, every missing column the trainer's own scalar."""
        if not isinstance(hyper, dict):
            raise ValueError(f'hyper must be a dict with keys among {HYPER_COLUMNS}, got {type(hyper).__name__}')
        unknown = sorted(set(hyper) - set(HYPER_COLUMNS))
        if unknown:
            raise ValueError(f'hyper has unknown keys {unknown}: the per-problem values are {HYPER_COLUMNS}')
        w_sym = self.latent[6] if self.latent is not None else self.reversed_sym[2] if self.reversed_sym is not None else 0.0
        if 'w_sym' in hyper and self.latent is None and self.reversed_sym is None:
            raise ValueError('hyper w_sym needs a trainer with reversed_sym or latent: the plain loss has no symmetry regulariser')
        table = torch.empty(S, len(HYPER_COLUMNS), dtype=torch.float32)
        for c, (name, scalar) in enumerate(zip(HYPER_COLUMNS, (self.lr, self.w_reg, self.threshold, w_sym))):
            if name not in hyper:
                table[:, c] = scalar
                continue
            col = torch.as_tensor(hyper[name]).detach().to('cpu', torch.float32)
            if col.shape != (S,):
                raise ValueError(f'hyper {name} must hold one value per problem ({S}), got shape {tuple(col.shape)}')
            table[:, c] = col
        return table.to(self.x.device).contiguous()

    def fit(self, params0, n_epochs, orders=None, mask0=None, on_epoch=None, epochs_per_launch=16, boundary=None, epoch0=0,
            state=None, order_seeds=None, shuffle=True, hyper=None):
        """``params0`` (S, n_params); ``orders`` yields one (S or 1, n) integer permutation on the device per epoch, drawn
        in epoch order.  ``order_seeds`` (1 or S integers, with ``orders`` None) is the device shuffle instead: no table is
        built and nothing is drawn, epoch e of problem s walks ``epoch_order(order_seeds[s or 0], e, n)`` -- e the global epoch
        number, so ``epoch0`` continues a fit and the cut into launches (``epochs_per_launch`` and ``boundary`` alone,
        TABLE_BYTES does not apply) changes no result -- computed inside the launch (symode_adam_epochs*_keyed);
        ``shuffle=False`` walks the rows in order.  It is an equivalent draw, not a replay of a torch generator.
        ``on_epoch(epoch, record)`` is called for every epoch after its launch was read back, with that
        epoch's own record: the LOG_COLUMNS (with ``reversed_sym``: LOG_COLUMNS_REVERSED, with ``latent``: LOG_COLUMNS_LATENT) as (S,) numpy arrays, and ``record['state']`` = {params, mask, Xi} (device
        tensors, valid until the next launch) when the epoch is the last of its launch, else None.  ``boundary(epoch)``
        true ends the launch after that epoch (a caller that needs the state there).  ``state``: (m, v, step) of an
        earlier fit to continue.  ``hyper``: a dict with any of the keys ``lr``, ``w_reg``, ``threshold``, ``w_sym`` (the last with
        ``reversed_sym`` or ``latent`` only), each a length-S sequence or tensor: problem s's own value in place of the
        trainer's scalar; missing keys are filled from the scalars.  The (S, 4) table is built once and read by every launch
        of the fit (symode_adam_run), under the epoch orders and under ``order_seeds`` alike.  Returns Xi, mask, params (device), log (n_epochs, S, 8; with ``latent`` 10) numpy, nan (S,) bool and m, v,
        step."""
        dev = self.x.device
        params = params0.detach().to(dev, torch.float32).clone().contiguous()
        S = params.shape[0]
        if params.shape != (S, self.coef.n_params):
            raise ValueError(f'params0 must be (S, {self.coef.n_params}), got {tuple(params0.shape)}')
        mask = (torch.ones(S, self.d, self.coef.p, device=dev) if mask0 is None
                else mask0.detach().to(dev, torch.float32).reshape(S, self.d, self.coef.p).clone().contiguous())
        if state is None:
            m, v, step = torch.zeros_like(params), torch.zeros_like(params), torch.zeros(S, dtype=torch.int32, device=dev)
        else:
            m, v, step = (t.detach().to(dev).clone().contiguous() for t in state)
        xi = self.coef.xi(*self.coef.split(params)).reshape(S, self.d, self.coef.p) if n_epochs == 0 else None
        per_problem = {} if hyper is None else {'hyper': self.hyper_table(hyper, S)}
        if (orders is None) == (order_seeds is None):
            raise ValueError('give the epoch orders or order_seeds (the device shuffle), one of them')
        if order_seeds is not None:
            order_seeds = self.engine._order_seeds(order_seeds, dev)
            if order_seeds.numel() not in (1, S):
                raise ValueError(f'order_seeds must hold 1 or {S} seeds, got {order_seeds.numel()}')
        else:
            orders = iter(orders)
        logs = []
        done = 0
        while done < n_epochs:
            tables = []
            while done + len(tables) < n_epochs:
                t = None if orders is None else self.table(next(orders))
                if t is not None and (t.shape[0] not in (1, S) or (tables and t.shape[0] != tables[0].shape[0])):
                    raise ValueError(f'an epoch order must have 1 or {S} rows, all epochs alike; got {t.shape[0]}')
                tables.append(t)
                epoch = epoch0 + done + len(tables) - 1
                full = len(tables) >= max(1, int(epochs_per_launch)) or (
                    t is not None and (len(tables) + 1) * t.numel() * 4 > TABLE_BYTES)
                if full or (boundary is not None and boundary(epoch)):
                    break
            if orders is None:
                idx, keyed = None, dict(_keyed=(order_seeds, len(tables), self.batch, shuffle))
            else:
                idx, keyed = torch.stack(tables).contiguous(), {}
            kw = dict(lr=self.lr, betas=self.betas, eps=self.eps, w_x=self.w_x, w_reg=self.w_reg, l1=True,
                      threshold=self.threshold, st_freq=self.st_freq, epoch0=epoch0 + done, near_band=NEAR_THRESHOLD_BAND,
                      q_eff=self.q_eff, allow_constant=self.coef.allow_constant, **keyed, **per_problem)
            if self.latent is not None:
                B, y, e, D_obs, L, w_z, w_sym = self.latent
                xi, log = self.engine.adam_epochs_latent(self.x, self.dx, B, y, e, D_obs, L, idx, params, m, v, step, mask,
                                                         self.order, self.flags, w_z=w_z, w_sym=w_sym, **kw)
            elif self.reversed_sym is None:
                xi, log = self.engine.adam_epochs(self.x, self.dx, idx, params, m, v, step, mask, self.order, self.flags, **kw)
            else:
                gx, jgx, w_sym = self.reversed_sym
                xi, log = self.engine.adam_epochs_reversed(self.x, self.dx, gx, jgx, idx, params, m, v, step, mask, self.order,
                                                           self.flags, w_sym=w_sym, **kw)
            log = log.cpu().numpy()
            logs.append(log)
            if on_epoch is not None:
                for k in range(len(tables)):
                    rec = {name: log[k, :, c] for c, name in enumerate(self.log_columns)}
                    rec['state'] = {'params': params, 'mask': mask, 'Xi': xi} if k == len(tables) - 1 else None
                    on_epoch(epoch0 + done + k, rec)
            done += len(tables)
        log = np.concatenate(logs) if logs else np.zeros((0, S, 8 if self.latent is None else 10), dtype=np.float32)
        return {'Xi': xi, 'mask': mask, 'params': params, 'log': log, 'nan': step < 0, 'm': m, 'v': v, 'step': step}
