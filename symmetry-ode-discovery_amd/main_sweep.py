"""Seed sweep of an equation-discovery config in ONE process per GPU (the reference runs
``for i in {0..49}; do python main.py --seed $i --config ...; done``, run_scripts/*.sh).

    python -m symode_amd.main_sweep --config dosc/noise20_sindy.cfg --seed 0 --n_seeds 50
    python -m symode_amd.main_sweep --config selkov/noise20_eq_sindy.cfg --n_seeds 64 --method stlsq
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m symode_amd.main_sweep \
        --config selkov/noise20_eq_sindy.cfg --n_seeds 64 --method stlsq          # BASELINE config 3: 8 x MI355X
    python -m symode_amd.main_sweep --config dosc/noise20_sindy.cfg --n_seeds 50 --eval_ltp --ltp_bound_rel 0.1
    python -m symode_amd.main_sweep --task dosc --sindy_optimizer adam --batch_size 256 --num_epochs 1000 --n_seeds 64

Every seed gets its own initial coefficients and its own ``--lbfgs_subsample`` draw of the data set
(main.py:36-38).  ``--method lbfgs`` (default): all seeds are optimised in lockstep by sweep.SeedSweepLBFGS on
the batched fused closure.  ``--method stlsq``: sequential-threshold least squares per seed (train.py:872-887) from
ONE gather-Gram launch over the (seed, point) index table (sweep.SeedSweepSTLSQ).  Under ``torch.distributed``
(one process per GPU, backend nccl = RCCL over xGMI) every rank holds a contiguous block of trajectories; the per-seed
``[loss | grad]`` vectors / Gram matrices are all-reduced and every rank takes identical decisions; rank 0 writes the
reference's ``eval_results/<save_dir>/seed{n}.npz`` so that ``evaluation.aggregate_results`` works unchanged.

The reversed symmetry regulariser (``--sym_reg_type r --w_sym_reg w``, EquivSINDy-r: lv/noise99_eq_rsymreg.cfg,
selkov/noise20_eq_symreg3.cfg) is swept too when the config loads a LaLiGAN and freezes it (``--load_laligan NAME
--fix_laligan``, no ``--use_latent``): autoencoder and generator are read from saved_models/NAME/ as main.py reads them,
and g(x), J_g(x) -- pointwise, independent of the seed and of Xi -- are computed ONCE (model_utils.precompute_symmreg_r, in
chunks of at most PRECOMPUTE_CHUNK rows) over the union of the rows this rank's seeds use, then gathered per seed.  The
regulariser enters with weight w_sym_reg / w_sindy_x as in the per-seed fit (train._train_on_device).  Default: the fused
stream closure on gathered (S, n_g, m_local, d) copies; ``--gram_closure``: per-seed [G | R] from one gather-Gram and one
gathered reversed-Gram launch on the shared arrays (GramStatistics.add_gathered), ONE all-reduce of [G | R | count] when
sharded.  The i / f regularisers (their closure runs the autoencoder on Xi-dependent inputs), a LaLiGAN that is not
loaded (each per-seed process would draw its own random network) or not frozen, and latent fits are refused with the
per-seed command to use instead.

``--eval_ltp`` scores the fitted models on the validation split without the true equation: after the fit rank 0 rolls ALL
seeds' models out over the validation trajectories in one launch (evaluation.eval_ltp_sweep; ``--ltp_bound_rel R`` sets
the horizon's error bound to R times the data's variance) and takes their held-out derivative MSE from one Gram matrix
(evaluation.val_mse_sweep); ``ltp_mean_error`` (n_ics,), ``ltp_horizon`` (n_ics,) and ``val_mse`` join each seed's npz and
the seeds are listed by median roll-out error.  Every rank holds the same final coefficients: no collective is added.

``--sindy_optimizer adam`` (the parser's default optimiser) sweeps the minibatch Adam fit of train_SIGED's plain branch --
no ``--use_latent``, ``w_sym_reg == 0``, with or without ``--eq_constraint`` -- on device_adam.DeviceAdam: one workgroup
per seed runs whole epochs per launch (symode_adam_epochs).  Every epoch of every seed is a pass over the WHOLE data set in
batches of ``--batch_size`` (``--lbfgs_subsample`` does not apply, as in main.py); seed s shuffles with its own device
generator seeded with s (one ``torch.rand(n)`` per epoch, stable argsort), so a seed's fit depends on the seed alone, not on
``--n_seeds`` or ``--seed``.  Adam with the latent branch or a symmetry regulariser is refused (for the reversed one use
``python -m symode_amd.main --device_adam`` per seed), and so is Adam on several
ranks (one process per seed block is the way to use several GPUs there).

A sweep's seed n does NOT reproduce ``python -m symode_amd.main --seed n`` row for row: the sweep draws each seed's
subsample with the counter hash (seeded_subsamples) -- under Adam each seed's shuffles from its own generator, where main
shuffles with the global one after drawing the model -- and its initial coefficients from its own torch.Generator(seed), as
the plain sweep always has; the success rate over seeds is what the two estimate alike.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from .autoencoder import AutoEncoder
from .batched import BatchedClosure
from .dataset import get_dataset
from .evaluation import aggregate_results, eval_ltp_sweep, sindy_truth, val_mse_sweep
from .lie import LieGenerator
from .model_utils import PRECOMPUTE_CHUNK, symmetry_operands  # noqa: F401  (their home: the device Adam trainer shares them)
from .parser_utils import get_args
from .sindy import SINDyRegression
from .sweep import GramClosure, SeedSweepLBFGS, SeedSweepSTLSQ, seeded_subsamples

def _pop(argv, flag, default, cast):
    if flag in argv:
        i = argv.index(flag)
        value = cast(argv[i + 1])
        del argv[i:i + 2]
        return value
    return default


def _pop_flag(argv, flag):
    if flag in argv:
        argv.remove(flag)
        return True
    return False


def _score_on_validation(val, Xi, mask, lib, task, bound_rel, dev, engine):
    """--eval_ltp: per-seed arrays for the npz files, from one roll-out launch and one validation Gram (rank 0)."""
    order, sine, exp = lib
    kw = dict(poly_order=order, include_sine=sine, include_exp=exp, **({'engine': engine} if engine is not None else {}))
    x = val.x.reshape(val.n_ics, val.n_steps, val.input_dim).to(dev)
    ltp = eval_ltp_sweep(Xi, mask, x, task=task, bound_rel=bound_rel, **kw)
    mse = val_mse_sweep(Xi, mask, val.x.to(dev), val.dx.to(dev), **kw)
    return {'ltp_mean_error': ltp['mean_error'], 'ltp_horizon': ltp['horizon'], 'val_mse': mse}


def _print_ltp_ranking(seeds, scores, forms):
    """Seeds by median roll-out error over the validation trajectories (NaN = diverged, last); with a truth table, how
    many of the best quarter have every equation's form right."""
    med = np.median(scores['ltp_mean_error'], axis=1)
    rank = np.argsort(np.where(np.isfinite(med), med, np.inf), kind='stable')
    print('seeds by median roll-out error on the validation trajectories (seed: median error, median horizon, val MSE):')
    for k in rank:
        print(f'  {seeds[k]}: {med[k]:.4e}, {int(np.median(scores["ltp_horizon"][k]))}, {scores["val_mse"][k]:.4e}')
    if forms is not None:
        q = max(1, len(seeds) // 4)
        print(f'correct form among the best {q} by roll-out error: {sum(forms[k] for k in rank[:q])}/{q}')


def _write_results(args, seeds, Xi, mask, truth, extra=None):
    """eval_results/<save_dir>/seed{n}.npz per seed (evaluation/eval_eq.py:7-34, main.py:128-138); ``extra``: further
    per-seed arrays (name -> array with the seeds on axis 0).  Returns correct_form_all per seed."""
    eval_dir = f'eval_results/{args["save_dir"]}'
    os.makedirs(eval_dir, exist_ok=True)
    tmask = truth != 0
    forms = []
    for k, s in enumerate(seeds):
        coef = np.where(mask[k], Xi[k], 0.0)
        cf = np.array([float(np.all(mask[k, i] == tmask[i])) for i in range(truth.shape[0])])
        mse = np.array([np.mean((coef[i, tmask[i]] - truth[i, tmask[i]]) ** 2) for i in range(truth.shape[0])])
        more = {} if extra is None else {name: v[k] for name, v in extra.items()}
        np.savez(f'{eval_dir}/seed{s}.npz', coefficients=coef, correct_form=cf, mse=mse, correct_form_all=np.all(cf),
                 mse_all=np.mean(mse), **more)
        forms.append(bool(np.all(cf)))
    return forms


def _refusal(args, method='lbfgs'):
    """None when main_sweep covers the config, else why not and the per-seed command to run instead.  ``--method stlsq`` is
    accepted with ``--sindy_optimizer lbfgs`` only, as before the Adam sweep existed; the Adam rules apply to the default method."""
    cfg = args.get('config')
    cmd = (f'python -m symode_amd.main --seed $i --config {cfg}' if cfg else 'python -m symode_amd.main --seed $i ...') + \
        ' for each seed (the per_seed loop of run_scripts/sweep.sh)'
    if method == 'stlsq' and args['sindy_optimizer'] != 'lbfgs':
        return f'main_sweep covers the L-BFGS fits (--sindy_optimizer lbfgs); run {cmd}'
    if args['sindy_optimizer'] not in ('lbfgs', 'adam'):
        return f'main_sweep covers the L-BFGS and Adam fits (--sindy_optimizer lbfgs | adam); run {cmd}'
    if args['use_latent']:
        return f'main_sweep does not cover latent fits (--use_latent); run {cmd}'
    if args['sindy_optimizer'] == 'adam':
        if args['w_sym_reg'] > 0:
            return f'main_sweep covers Adam fits without a symmetry regulariser (w_sym_reg 0) only; run {cmd}'
        if args.get('sindy_reg_type', 'l1') != 'l1':
            return f"main_sweep covers Adam fits with --sindy_reg_type l1 only; run {cmd}"
        return None
    if args['w_sym_reg'] > 0:
        if args['sym_reg_type'] != 'r':
            return (f"main_sweep covers the reversed symmetry regulariser only (--sym_reg_type r), not "
                    f"'{args['sym_reg_type']}': its closure runs the autoencoder on Xi-dependent inputs; run {cmd}")
        if args['load_laligan'] is None:
            return (f'main_sweep needs --load_laligan with the symmetry regulariser: without it every per-seed process '
                    f'fits against its own random autoencoder; run {cmd}')
        if not args['fix_laligan']:
            return f'main_sweep needs --fix_laligan with the symmetry regulariser (g(x), J_g(x) computed once); run {cmd}'
    return None


def _load_laligan(args, dev):
    """Frozen autoencoder and generator of saved_models/<load_laligan>/, as main._run loads them (main.py:45-63)."""
    autoencoder = AutoEncoder(**args).to(dev)
    generator = LieGenerator(**args).to(dev)
    path = args['load_laligan']
    autoencoder.load_state_dict(torch.load(f'saved_models/{path}/autoencoder.pt', weights_only=True, map_location=dev))
    saved = torch.load(f'saved_models/{path}/generator.pt', weights_only=True, map_location=dev)
    current = generator.state_dict()
    for name, param in current.items():                       # tolerate older generator files (main.py:52-60)
        saved.setdefault(name, param)
    generator.load_state_dict({k: v for k, v in saved.items() if k in current})
    masks = torch.load(f'saved_models/{path}/generator_mask.pt', weights_only=True, map_location=dev)
    generator.masks = [m.to(dev) if m is not None else None for m in masks]
    for module in (autoencoder, generator):
        module.eval()                                         # batch norm on its running statistics: g(x) is pointwise
        for param in module.parameters():
            param.requires_grad = False
    return autoencoder, generator


def _adam_sweep(args, seeds, template, coef, inits, x_all, dx_all, val_dataset, padded_truth, eval_ltp, ltp_bound_rel, dev,
                engine):
    """--sindy_optimizer adam: all seeds on DeviceAdam, every seed with its own shuffles of the whole data set."""
    from .device_adam import DeviceAdam
    n_all, n_seeds = x_all.shape[0], len(seeds)
    trainer = DeviceAdam(x_all, dx_all, template.poly_order, template.include_sine, template.include_exp, coef, args['lr_sindy'],
                         args['w_sindy_x'], args['w_sindy_reg'], args['threshold'], args['st_freq'], args['batch_size'],
                         engine=engine)
    gens = [torch.Generator(device=dev).manual_seed(s) for s in seeds]
    keys = torch.empty(n_seeds, n_all, device=dev)

    def orders():
        for _ in range(args['num_epochs']):
            for k, g in enumerate(gens):                            # row k is a function of seed k alone
                torch.rand(n_all, generator=g, out=keys[k])
            yield torch.argsort(keys, dim=1, stable=True)

    out = trainer.fit(torch.stack(inits).to(dev), args['num_epochs'], orders())
    scores = None
    if eval_ltp:
        scores = _score_on_validation(val_dataset, out['Xi'], out['mask'], (template.poly_order, template.include_sine, template.include_exp),
                                      args['task'], ltp_bound_rel, dev, engine)
    Xi, mask = out['Xi'].cpu().numpy(), out['mask'].cpu().numpy().astype(bool)
    forms = _write_results(args, seeds, Xi, mask, padded_truth(mask.shape[-1], template), scores)
    near = out['log'][:, :, 3].sum(axis=0) if len(out['log']) else np.zeros(n_seeds)
    print(f'{n_seeds} seeds, {args["num_epochs"]} epochs x {trainer.steps} Adam steps of {trainer.batch} rows, '
          f'NaN {int(out["nan"].sum())}, '
          f'seeds with near-threshold coefficients {[seeds[i] for i in np.nonzero(near)[0].tolist()] or "none"}')
    if eval_ltp:
        _print_ltp_ranking(seeds, scores, forms)
    return aggregate_results(args['save_dir'], min_seed=seeds[0], max_seed=seeds[-1] + 1)


def main(argv=None, engine=None, backend='nccl', one_gpu=False):
    """``engine`` / ``backend`` exist for the CPU rehearsal of the multi-rank path in tests (gloo + the test engine);
    ``one_gpu``: every rank uses cuda:0 (rehearsal of the HIP path with several ranks on a one-GPU box, gloo collectives)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    n_seeds = _pop(argv, '--n_seeds', 50, int)
    method = _pop(argv, '--method', 'lbfgs', str)
    if method not in ('lbfgs', 'stlsq'):
        raise SystemExit(f'--method {method}: lbfgs or stlsq')
    eval_ltp = _pop_flag(argv, '--eval_ltp')
    ltp_bound_rel = _pop(argv, '--ltp_bound_rel', None, float)
    args = vars(get_args(argv=argv))
    why = _refusal(args, method)
    if why is not None:
        raise SystemExit(why)
    sym = args['w_sym_reg'] > 0
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    adam = args['sindy_optimizer'] == 'adam'                                # (--method stlsq was refused above)
    if adam and world > 1:
        raise SystemExit('main_sweep runs the Adam fits in one process (no collective over seeds): give every GPU its own '
                         'block of seeds, python -m symode_amd.main_sweep --seed <first> --n_seeds <count> ... per process')
    if engine is None:
        if str(args['device']) == 'cpu':
            raise SystemExit('symode_amd runs the SINDy path on the GPU only (no CPU fallback): a HIP device is required')
        if world > 1:
            local = 0 if one_gpu else int(os.environ.get('LOCAL_RANK', '0'))
            torch.cuda.set_device(local)
            args['device'] = torch.device('cuda', local)
    dev = args['device']
    group = None
    if world > 1:
        if not dist.is_initialized():
            dist.init_process_group(backend, **({'device_id': dev} if backend == 'nccl' else {}))
        group = dist.group.WORLD
        if rank == 0:                                               # one rank makes the data files, the others read them
            train_dataset, val_dataset, args = get_dataset(args)
        dist.barrier()
        if rank != 0:
            train_dataset, val_dataset, args = get_dataset(args)
    else:
        train_dataset, val_dataset, args = get_dataset(args)
    # Every seed draws ONE subsample of the whole flattened data set (main.py:36-38: the first batch of a shuffled loader),
    # seeded by the seed alone; rank r works on rows [r m / W, (r+1) m / W) of that draw.  The union over the ranks is
    # the single-process subsample whatever the world size, so an N-rank run fits the same problems as a 1-rank run and
    # differs from it by summation order only.  (The data sets of the reference are a few MB: every rank keeps all of
    # x, dx resident and gathers its rows; the COMPUTE is what is sharded.)
    x_all, dx_all = train_dataset.x.to(dev), train_dataset.dx.to(dev)
    n_all = x_all.shape[0]
    m = int(n_all * args['lbfgs_subsample'])
    lo, hi = rank * m // world, (rank + 1) * m // world  # shards may differ by a row: counts are summed over the ranks
    seeds = list(range(args['seed'], args['seed'] + n_seeds))

    truth = sindy_truth[args['task']]

    def padded_truth(p, template):
        if truth.shape[1] < p and not (template.include_sine or template.include_exp):
            return np.concatenate([truth, np.zeros((truth.shape[0], p - truth.shape[1]))], axis=1)
        return truth

    if method == 'stlsq':
        if sym:
            raise SystemExit('--method stlsq sweeps the plain least-squares fit (use --method lbfgs with the symmetry regulariser)')
        if args['eq_constraint']:
            raise SystemExit('--method stlsq sweeps the unconstrained library (use --method lbfgs for EquivSINDy-c)')
        idx = seeded_subsamples(n_all, m, seeds, dev)[:, lo:hi]
        sw = SeedSweepSTLSQ(x_all, dx_all, args['poly_order'], args['include_sine'], args['include_exp'], n_seeds=n_seeds,
                            subsample=args['lbfgs_subsample'], seed0=args['seed'], group=group, engine=engine, idx=idx, idx_sorted=True)
        Xi, mask, passes = sw.solve(args['w_sindy_reg'], args['threshold'], max_iter=max(1, args['num_epochs']),
                                    lstsq_driver=args.get('lstsq_driver'))
        if rank == 0:
            class _T:                                               # library flags for the truth-table padding
                include_sine, include_exp = args['include_sine'], args['include_exp']
            scores = None
            if eval_ltp:
                scores = _score_on_validation(val_dataset, Xi.to(dev), mask.to(dev), (args['poly_order'], args['include_sine'], args['include_exp']),
                                              args['task'], ltp_bound_rel, dev, engine)
            forms = _write_results(args, seeds, Xi.numpy(), mask.numpy().astype(bool), padded_truth(mask.shape[-1], _T), scores)
            print(f'{n_seeds} seeds x {sw.n_points} points (over {world} rank(s)), STLSQ passes {int(passes.min())}-{int(passes.max())}')
            print(f'near-threshold coefficients (| |coef| - thr | < 1e-4): {sw.near_threshold if sw.near_threshold else "none"}')
            if eval_ltp:
                _print_ltp_ranking(seeds, scores, forms)
            return aggregate_results(args['save_dir'], min_seed=seeds[0], max_seed=seeds[-1] + 1)
        return None

    # one template regressor fixes the library / constraint; per-seed draws follow the constructor's order
    if sym:                                                         # loaded BEFORE the template (main.py's order)
        autoencoder, generator = _load_laligan(args, dev)
    if args['eq_constraint']:
        gen = generator if sym else LieGenerator(**args)
        L_list = gen.get_full_basis_list()
        rd = L_list[0].shape[-1] // args['n_comps']
        args['L_list'] = [L[:rd, :rd].detach().cpu() for L in L_list]
    template = SINDyRegression(**args, **({'engine': engine} if engine is not None else {})).to(dev)
    coef = template.coef
    inits = [coef.draw(torch.Generator().manual_seed(s)) for s in seeds]
    if adam:
        return _adam_sweep(args, seeds, template, coef, inits, x_all, dx_all, val_dataset, padded_truth, eval_ltp, ltp_bound_rel,
                           dev, engine)
    all_rows = seeded_subsamples(n_all, m, seeds, dev)[:, lo:hi]
    w_sym = args['w_sym_reg'] / args['w_sindy_x'] if sym else 0.0
    stats = None
    if sym:
        x_used, gx, jgx, table, used = symmetry_operands(x_all, all_rows, autoencoder, generator)
    if sym and args.get('gram_closure'):
        # [G | R] of every seed from the shared arrays and the index table: no per-seed copy of the points
        from .gram_closure import GramStatistics
        stats = GramStatistics(n_seeds, template.latent_dim, template.poly_order, template.flags, regulariser=True, device=dev,
                               **({'engine': engine} if engine is not None else {}))
        stats.add_gathered(x_used, dx_all[used].contiguous(), table, gx, jgx)
        clos = GramClosure(stats, w_sym=w_sym, coef=coef, group=group)
    else:
        X, DX = x_all[all_rows].contiguous(), dx_all[all_rows].contiguous()
        rev = None
        if sym:                                                     # (S, n_g, m_local, d) per-seed copies of g(x), J_g(x)
            rev = (gx[:, table.long()].transpose(0, 1).contiguous(), jgx[:, table.long()].transpose(0, 1).contiguous(), w_sym)
        clos = BatchedClosure(X, DX, template.poly_order, template.include_sine, template.include_exp, reversed_sym=rev,
                              coef=coef, group=group, **({'engine': engine} if engine is not None else {}))
    sweep = SeedSweepLBFGS(clos, args['lr_sindy'], args['threshold'], args['st_freq'], w_sindy_x=args['w_sindy_x'],
                           sindy_reg_type=args['sindy_reg_type'], w_sindy_reg=args['w_sindy_reg'],
                           gram_closure=bool(args.get('gram_closure')), statistics=stats)
    out = sweep.fit(torch.stack(inits).to(dev), args['num_epochs'])

    if rank != 0:
        return None
    scores = None
    if eval_ltp:
        scores = _score_on_validation(val_dataset, out['Xi'].to(dev), out['mask'].to(dev), (template.poly_order, template.include_sine, template.include_exp),
                                      args['task'], ltp_bound_rel, dev, engine)
    Xi, mask = out['Xi'].cpu().numpy(), out['mask'].cpu().numpy().astype(bool)
    forms = _write_results(args, seeds, Xi, mask, padded_truth(mask.shape[-1], template), scores)
    print(f'{n_seeds} seeds, epochs used {int(out["epochs"].min())}-{int(out["epochs"].max())}, '
          f'finished {int(out["finished"].sum())}, NaN {int(out["nan"].sum())}, '
          f'seeds with near-threshold coefficients {[seeds[i] for i in torch.nonzero(out["near_threshold"]).flatten().tolist()] or "none"}')
    if eval_ltp:
        _print_ltp_ranking(seeds, scores, forms)
    return aggregate_results(args['save_dir'], min_seed=seeds[0], max_seed=seeds[-1] + 1)


if __name__ == '__main__':
    main()
