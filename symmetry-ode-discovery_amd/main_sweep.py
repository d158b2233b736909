"""Seed sweep of an equation-discovery config in ONE process per GPU (the reference runs
``for i in {0..49}; do python main.py --seed $i --config ...; done``, run_scripts/*.sh).

    python -m symode_amd.main_sweep --config dosc/noise20_sindy.cfg --seed 0 --n_seeds 50
    python -m symode_amd.main_sweep --config selkov/noise20_eq_sindy.cfg --n_seeds 64 --method stlsq
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m symode_amd.main_sweep \
        --config selkov/noise20_eq_sindy.cfg --n_seeds 64 --method stlsq          # BASELINE config 3: 8 x MI355X
    python -m symode_amd.main_sweep --config dosc/noise20_sindy.cfg --n_seeds 50 --eval_ltp --ltp_bound_rel 0.1
    python -m symode_amd.main_sweep --config lv/noise99_eq_rsymreg.cfg --n_seeds 50 [--gram_closure]
    python -m symode_amd.main_sweep --task dosc --sindy_optimizer adam --batch_size 256 --num_epochs 1000 --n_seeds 64
    python -m symode_amd.main_sweep --task dosc --sindy_optimizer adam --device_shuffle --batch_size 256 --n_seeds 64
    python -m symode_amd.main_sweep --task dosc --sindy_optimizer adam --n_seeds 64 --eval_ltp \
        --grid threshold=0.01,0.05,0.075,0.15 --grid lr_sindy=0.1,1.0     # 8 grid points x 64 seeds in every epoch launch
    python -m symode_amd.main_sweep --config dosc/noise20_wsindy.cfg --wsindy --n_seeds 50 [--wsindy_grid threshold=0.1,0.2,0.3]
    python -m symode_amd.main_sweep --config lv/noise99_eq_rsymreg.cfg --n_seeds 64 --gram_closure --eval_ltp \
        --lbfgs_grid w_sym_reg=0.01,0.1,1 --lbfgs_grid threshold=0.05,0.1   # 6 grid points on the 64 seeds' Gram matrices

plan:   ``_refusal`` decides from the arguments alone whether the sweep runs, before a process group, a data file or a
        device is touched; what it refuses it answers with the per-seed command to run instead.
fit:    ``_fit_stlsq`` (--method stlsq), ``_fit_lbfgs`` (default; the reversed regulariser in stream or --gram_closure form),
        ``_fit_adam`` (--sindy_optimizer adam) or ``_fit_wsindy`` (--wsindy): every seed its own initial coefficients and its own subsample.
report: ``_report`` on rank 0: the reference's ``eval_results/<save_dir>/seed{n}.npz`` (``--eval_ltp`` adds roll-out error,
        horizon and held-out MSE per seed), the fit's summary, ``evaluation.aggregate_results``.

Under ``torch.distributed`` (one process per GPU, backend nccl = RCCL over xGMI) every rank works on a contiguous block of
each seed's rows; the per-seed ``[loss | grad]`` vectors / Gram matrices are all-reduced and every rank takes identical
decisions.

A sweep's seed n does NOT reproduce ``python -m symode_amd.main --seed n`` row for row: the sweep draws each seed's
subsample with the counter hash (seeded_subsamples) -- under Adam each seed's shuffles from its own generator, where main
shuffles with the global one after drawing the model -- and its initial coefficients from its own torch.Generator(seed), as
the plain sweep always has; the success rate over seeds is what the two estimate alike.  Under ``--device_shuffle`` the
Adam sweep draws no shuffle at all: every epoch launch computes its rows from (seed, epoch) (device_adam.epoch_order), so
the rows of a step differ from the tensor-op shuffle's as well -- an equivalent draw, not a replay -- and nothing runs on
the host or the device between two launches.

``--grid name=v1,v2,...`` (repeatable; names lr_sindy, w_sindy_reg, threshold; Adam only) fits the Cartesian product of the
value lists, the first axis given slowest, over COMMON seeds in the same launches: problem g * n_seeds + k is grid point g on
seed k, with seed k's initial coefficients and epoch orders at every point, so the fit of (g, k) is exactly the fit main_sweep
with that point's scalar flags gives seed k.  The results go to ``eval_results/<save_dir>/grid{g}/seed{n}.npz`` and
``eval_results/<save_dir>/grid.json``; ``main`` returns {g: aggregate}.

``--lbfgs_grid name=v1,v2,...`` (repeatable; names lr_sindy, w_sindy_reg, threshold, w_sym_reg; L-BFGS with --gram_closure only)
is the same grid for the L-BFGS sweep: the seeds' Gram matrices are built once, and the G x n_seeds problems of the device
trainer read them through ``SeedSweepLBFGS.fit(hyper=...)`` -- no copy of the points, no further data pass or collective.
Problem order, result files and table are ``--grid``'s; the files also hold the point's w_sym_reg.

``--device_stlsq`` (with --method stlsq) runs the threshold loop of the STLSQ sweep on the device as well
(``SeedSweepSTLSQ.solve(device=True)``: one launch for all seeds on the Gram matrices where the gather launch left them, the
full-rank driver only); outputs and summary lines are those of ``--method stlsq``.  ``--stlsq_grid name=v1,v2,...``
(repeatable; names threshold, w_sindy_reg; with --device_stlsq only) is the grid of that sweep: the G x n_seeds problems of the
one launch read the n_seeds matrices -- no further data pass, copy or collective.  Problem order, result files and table are
``--grid``'s.

``--equiv_stlsq`` (with --method stlsq --device_stlsq --eq_constraint) is that device fit under the equivariance constraint
Xi = Q beta (+ const), EquivSINDy-c: the template regressor of the L-BFGS sweep supplies Q (constraint_basis,
--constrain_constant), ``SeedSweepSTLSQ.solve(device=True, coef=...)`` solves per pass ONE joint system in the r' <= 64 free
parameters (symode_stlsq_sweep_constrained) -- one gather launch and one solve launch for the whole sweep, --stlsq_grid and
--eval_ltp as before.  Without the flag ``--method stlsq --eq_constraint`` is refused as it always was.

``--min_norm_stlsq`` (with --equiv_stlsq only; opt-in) runs that launch in its rank-revealing mode
(symode_stlsq_sweep_minnorm, ``solve(..., min_norm=True)``): a pass whose support leaves Q's columns collinear is solved by
the minimum-norm rule inside the launch instead of flagging the seed for the host loop.  The summary gains one line that
counts the problems with rank-truncated passes; without the flag every word printed is what it was.

``--symreg_stlsq`` (with --method stlsq --device_stlsq --w_sym_reg > 0 --sym_reg_type r --load_laligan ... --fix_laligan) is that
device fit with the reversed symmetry regulariser, EquivSINDy-r: on a fixed batch the regulariser is the quadratic form
v^T R v, so the minimiser of mse + w_sym * reg on a support is the solution of one linear system and the fit is sequential
thresholding without an optimiser.  [G | R | count] are built as under --gram_closure (one gather launch each, ONE all-reduce),
``SeedSweepSTLSQ.solve(device=True, rev=(R, w_sym))`` solves per pass ONE joint system in the d p <= 64 coefficients
(symode_stlsq_sweep_symreg); w_sym = w_sym_reg / w_sindy_x.  Under the flag --stlsq_grid also takes w_sym_reg=v1,v2,...
(values > 0).  Without the flag ``--method stlsq --w_sym_reg > 0`` is refused as it always was.

``--wsindy`` sweeps the weak-SINDy fit of ``main_wsindy`` (the `for i in {0..49}; do python main_wsindy.py --seed $i` loops):
sweep seed n reads the window main_wsindy --seed n reads (``sweep.weak_windows``), all windows are contracted and turned into
their normal matrices by ONE call (symode_weak_normal_windows) and fitted by ONE symode_stlsq_sweep launch
(``sweep.SeedSweepWSINDy``); --num_epochs is the pass limit, --num_test_funcs / --test_func_family are main_wsindy's.  The
parser's default --sindy_optimizer does not matter to it.  ``--wsindy_grid name=v1,v2,...`` (repeatable; names threshold,
w_sindy_reg; with --wsindy only) is its grid on the windows' shared matrices; problem order, result files and table are
``--grid``'s.

``--stlsq_path [--path_tol v]`` (with --method stlsq --device_stlsq) asks for no threshold: per seed and equation row the sparsity
path -- solve on the full library, drop the smallest coefficient, solve again, down to the empty model -- is walked in ONE launch
(symode_stlsq_path, ``SeedSweepSTLSQ.solve_path``), every model of the path is scored on the validation set's matrix, and the
sparsest model whose held-out error is within path_tol (default 0.02) of the best is kept.  Result files, --eval_ltp and the
aggregate are those of ``--method stlsq``; ``eval_results/<save_dir>/path.npz`` holds order, rss_train, rss_val and best of all
seeds.  --threshold is not used.  Not covered, and refused by name: the constrained and the regularised fits, --wsindy, the grids,
--lstsq_driver gelsy, --use_latent.

``--symreg_path [--path_tol v]`` (with --method stlsq --device_stlsq --w_sym_reg > 0 --sym_reg_type r --load_laligan ...
--fix_laligan) is that path for the fit with the reversed symmetry regulariser, EquivSINDy-r: [G | R | count] are built as under
--symreg_stlsq (ONE all-reduce), the validation set's matrix as under --stlsq_path, and ONE launch (symode_stlsq_path_symreg,
``SeedSweepSTLSQ.solve_path(rev=(R, w_sym))``) walks per seed ONE chain over the joint (d, p) support of d p <= 64 entries --
the regulariser couples the rows --, scores every model's mse on the validation matrix (the regulariser is scored on the
training set only) and keeps the sparsest model within path_tol of the best.  --stlsq_grid takes w_sym_reg=... and
w_sindy_reg=... under it (a threshold axis is refused: the path asks for no threshold).  ``eval_results/<save_dir>/path.npz``
holds order, mse_train, reg_train, mse_val, best and near of all problems.  It is a flag of its own: without it every argument
combination answers word for word what it answered before.

``--bagging B [--bag_chunks C] [--bag_inclusion v1,v2,...]`` (with --method stlsq --device_stlsq) is block-bootstrap bagging of
the threshold fit, ensemble SINDy (``SeedSweepSTLSQ.solve_bagged``): per seed B replicas, each a resample with replacement of the
C (default 128) chunks of the seed's time-ordered rows, are fit by the threshold loop (--threshold, --w_sindy_reg, --num_epochs
as ever), a term is kept when the share of replicas it survives in reaches the inclusion level, and the model is refit on that
support from the seed's own matrix.  Four launches whatever B: the chunk matrices (one gather), the replica matrices
(symode_gram_resample), the n_seeds x B replica fits (symode_stlsq_sweep), aggregation and refit (symode_stlsq_bag).  The levels
are multiples of 0.001 in [0, 1] (default BAG_INCLUSION; profiles/stlsq_bag.txt: how it was chosen, and where bagging loses);
several levels are a grid on the same replica fits -- problem order, result files and table are ``--grid``'s.
``eval_results/<save_dir>/bag.npz`` holds count, valid, mean, std and fell of all seeds.  Opt-in: without --bagging every argument
combination answers word for word what it answered before.  Not covered, and refused by name: the constrained and the
regularised fits, both paths, --wsindy, the other grids, --lstsq_driver gelsy, --use_latent, more than one rank.

``--fold_linear_action`` lets the closure of the reversed regulariser fold a linear group action g(x) = J x into its
coefficients where the data are found to be one (``BatchedClosure(linear_action=None)``): a faster kernel and the same
closure up to rounding, not bit for bit -- which is why it has to be asked for here.
"""
from __future__ import annotations

import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

from .autoencoder import AutoEncoder
from .batched import BatchedClosure
from .dataset import get_dataset, ode_dt_dict
from .evaluation import aggregate_results, eval_ltp_sweep, score_coefficients, truth_table, val_mse_sweep
from .lie import LieGenerator
from .model_utils import PRECOMPUTE_CHUNK, constraint_basis, load_laligan, symmetry_operands  # noqa: F401  (tests and tests/perf import the operands from here)
from .parser_utils import get_args, init_ranks
from .sindy import SINDyRegression
from .sweep import GramClosure, SeedSweepLBFGS, SeedSweepSTLSQ, SeedSweepWSINDy, seeded_subsamples


def _pop(argv, flag, default, cast):
    if flag in argv:
        i = argv.index(flag)
        value = cast(argv[i + 1])
        del argv[i:i + 2]
        return value
    return default


def _pop_all(argv, flag):
    """Every value of a repeatable flag, in the order given."""
    values = []
    while flag in argv:
        i = argv.index(flag)
        values.append(argv[i + 1] if i + 1 < len(argv) else '')
        del argv[i:i + 2]
    return values


def _pop_flag(argv, flag):
    if flag in argv:
        argv.remove(flag)
        return True
    return False


# ---- plan --------------------------------------------------------------------------------------------------------------------
GRID_NAMES = {'lr_sindy': 'lr', 'w_sindy_reg': 'w_reg', 'threshold': 'threshold'}      # --grid name -> DeviceAdam.fit(hyper=) key


# --lbfgs_grid name -> DeviceTrainer(hyper=) key
LBFGS_GRID_NAMES = {'lr_sindy': 'lr', 'w_sindy_reg': 'w_reg', 'threshold': 'threshold', 'w_sym_reg': 'w_sym'}
STLSQ_GRID_NAMES = {'threshold': 'threshold', 'w_sindy_reg': 'w_reg'}      # --stlsq_grid name -> SeedSweepSTLSQ.solve(hyper=) key
# ... under --symreg_stlsq: the weight of the reversed regulariser as a third axis
SYMREG_STLSQ_GRID_NAMES = {'threshold': 'threshold', 'w_sindy_reg': 'w_reg', 'w_sym_reg': 'w_sym'}
# ... under --symreg_path: SeedSweepSTLSQ.solve_path(hyper=) keys; the path asks for no threshold
SYMREG_PATH_GRID_NAMES = {'w_sindy_reg': 'w_reg', 'w_sym_reg': 'w_sym'}
WSINDY_GRID_NAMES = {'threshold': 'threshold', 'w_sindy_reg': 'w_reg'}     # --wsindy_grid name -> SeedSweepWSINDy.solve(hyper=) key
MAX_GRID_PROBLEMS = 65535                                  # problems of one device trainer


def _parse_grid(specs, names=GRID_NAMES, flag='--grid'):
    """``--grid name=v1,v2,...`` strings -> ([(name, [values])] in the order given, None), or (None, why not).  ``names``,
    ``flag``: the axes and the spelling of the flag that is being read (--lbfgs_grid: LBFGS_GRID_NAMES)."""
    axes = []
    for spec in specs:
        name, eq, values = str(spec).partition('=')
        if name not in names:
            return None, f"{flag} {spec}: unknown name '{name}', the grid axes are {', '.join(names)} (name=v1,v2,...)"
        if name in [a[0] for a in axes]:
            return None, f'{flag} {name} is given twice: one value list per name'
        try:
            axis = [float(v) for v in values.split(',')] if eq else []
        except ValueError:
            axis = []
        if not axis or not all(np.isfinite(axis)):
            return None, f"{flag} {spec}: the values of {name} must be a non-empty comma-separated list of numbers"
        axes.append((name, axis))
    return axes, None


def _grid_points(axes):
    """The Cartesian product of the axes, the first axis slowest: one {name: value} per grid point."""
    return [dict(zip([a[0] for a in axes], values)) for values in itertools.product(*[a[1] for a in axes])]


def _grid_problem(problem, n_seeds):
    """Problem ``g * n_seeds + k`` of a grid launch is grid point g on seed k: (g, k)."""
    return divmod(problem, n_seeds)


def _refusal(args, method='lbfgs', world=1, engine=None, grid=None, lbfgs_grid=None, n_seeds=None, device_stlsq=False,
             stlsq_grid=None, wsindy=False, wsindy_grid=None, equiv_stlsq=False, min_norm_stlsq=False, symreg_stlsq=False,
             stlsq_path=False, path_tol=None, symreg_path=False, bagging=None, bag_chunks=None, bag_inclusion=None):
    """None when main_sweep covers the run, else why not -- for a config it does not cover, with the per-seed command to run
    instead.  A pure function of its arguments: ``world`` the number of ranks, ``engine`` the injected test engine, if any.
    ``--method stlsq`` is accepted with ``--sindy_optimizer lbfgs`` only, as before the Adam sweep existed; the Adam rules
    apply to the default method.  ``grid``: the ``--grid`` strings, if any; their rules come after all others, and after
    them those of ``lbfgs_grid``, the ``--lbfgs_grid`` strings (``n_seeds``: for the size of its launch, if known).
    ``device_stlsq``, ``stlsq_grid``: the ``--device_stlsq`` flag and the ``--stlsq_grid`` strings; their rules stand before
    those of the two other grids, which say what they always said.  ``wsindy``, ``wsindy_grid``: the ``--wsindy`` flag and the
    ``--wsindy_grid`` strings; theirs is a fit of its own, so its rules (``_refusal_wsindy``) come before the optimiser rules
    and replace them -- the weak configs set no --sindy_optimizer, and the parser's default must not route them anywhere.
    ``equiv_stlsq``: the ``--equiv_stlsq`` flag; off, every answer is what it was.  On, its own rules (``_refusal_equiv_stlsq``)
    come first and the rule that keeps --eq_constraint out of --method stlsq does not apply.
    ``min_norm_stlsq``: the ``--min_norm_stlsq`` flag, a mode of --equiv_stlsq and refused by name without it.
    ``symreg_stlsq``: the ``--symreg_stlsq`` flag; off, every answer is what it was.  On, its own rules
    (``_refusal_symreg_stlsq``) come first, the rule that keeps the symmetry regulariser out of --method stlsq does not apply,
    and --stlsq_grid reads SYMREG_STLSQ_GRID_NAMES.
    ``stlsq_path``, ``path_tol``: the ``--stlsq_path`` flag and the ``--path_tol`` value (None: not given); off, every answer
    is what it was.  On, its own rules (``_refusal_stlsq_path``) come first; what they let through is a plain
    ``--method stlsq --device_stlsq`` run, which the rules below judge as they always did.
    ``symreg_path``: the ``--symreg_path`` flag; off (the default), every answer is what it was.  On, its own rules
    (``_refusal_symreg_path``) come first -- before those of --stlsq_path and --symreg_stlsq, which it refuses by name --,
    --path_tol is its tolerance, the rule that keeps the symmetry regulariser out of --method stlsq does not apply, and
    --stlsq_grid reads SYMREG_PATH_GRID_NAMES.
    ``bagging``, ``bag_chunks``, ``bag_inclusion``: the ``--bagging`` and ``--bag_chunks`` values and the ``--bag_inclusion``
    string (None: not given); without them every answer is what it was.  Given, their own rules (``_refusal_bagging``) come
    first and are all of them: what they let through is a plain ``--method stlsq --device_stlsq`` run on one rank."""
    if method not in ('lbfgs', 'stlsq'):
        return f'--method {method}: lbfgs or stlsq'
    if bagging is not None or bag_chunks is not None or bag_inclusion is not None:
        why = _refusal_bagging(args, method, world, engine, n_seeds, device_stlsq, bagging, bag_chunks, bag_inclusion,
                               equiv_stlsq or min_norm_stlsq, symreg_stlsq, stlsq_path or path_tol is not None, symreg_path,
                               wsindy or wsindy_grid, grid or lbfgs_grid or stlsq_grid)
        if why is not None:
            return why
    if symreg_path:
        why = _refusal_symreg_path(args, method, engine, device_stlsq, stlsq_path, symreg_stlsq, equiv_stlsq, min_norm_stlsq,
                                   wsindy or wsindy_grid, grid or lbfgs_grid, stlsq_grid, path_tol)
        if why is not None:
            return why
    if path_tol is not None and not stlsq_path and not symreg_path:
        return ('--path_tol needs --stlsq_path: it is the tolerance of the sparsity path (the sparsest model within path_tol of '
                'the best held-out error); the threshold loop takes --threshold')
    if stlsq_path:
        why = _refusal_stlsq_path(args, method, engine, device_stlsq, equiv_stlsq, min_norm_stlsq, symreg_stlsq,
                                  wsindy or wsindy_grid, grid or lbfgs_grid or stlsq_grid, path_tol)
        if why is not None:
            return why
    if symreg_stlsq:
        why = _refusal_symreg_stlsq(args, method, device_stlsq, wsindy or wsindy_grid, equiv_stlsq, min_norm_stlsq)
        if why is not None:
            return why
    if min_norm_stlsq and not equiv_stlsq:
        return _refusal_min_norm_stlsq()
    if equiv_stlsq:
        why = _refusal_equiv_stlsq(args, method, device_stlsq, wsindy or wsindy_grid)
        if why is not None:
            return why
    if wsindy or wsindy_grid:
        return _refusal_wsindy(args, method, world, engine, grid, lbfgs_grid, stlsq_grid, n_seeds, device_stlsq, wsindy, wsindy_grid)
    cfg = args.get('config')
    cmd = (f'python -m symode_amd.main --seed $i --config {cfg}' if cfg else 'python -m symode_amd.main --seed $i ...') + \
        ' for each seed (the per_seed loop of run_scripts/sweep.sh)'
    adam = args['sindy_optimizer'] == 'adam'
    if method == 'stlsq' and args['sindy_optimizer'] != 'lbfgs':
        return f'main_sweep covers the L-BFGS fits (--sindy_optimizer lbfgs); run {cmd}'
    if args['sindy_optimizer'] not in ('lbfgs', 'adam'):
        return f'main_sweep covers the L-BFGS and Adam fits (--sindy_optimizer lbfgs | adam); run {cmd}'
    if args['use_latent']:
        return f'main_sweep does not cover latent fits (--use_latent); run {cmd}'
    if adam:
        if args['w_sym_reg'] > 0:
            return f'main_sweep covers Adam fits without a symmetry regulariser (w_sym_reg 0) only; run {cmd}'
        if args.get('sindy_reg_type', 'l1') != 'l1':
            return f"main_sweep covers Adam fits with --sindy_reg_type l1 only; run {cmd}"
    elif args['w_sym_reg'] > 0:
        if args['sym_reg_type'] != 'r':
            return (f"main_sweep covers the reversed symmetry regulariser only (--sym_reg_type r), not "
                    f"'{args['sym_reg_type']}': its closure runs the autoencoder on Xi-dependent inputs; run {cmd}")
        if args['load_laligan'] is None:
            return (f'main_sweep needs --load_laligan with the symmetry regulariser: without it every per-seed process '
                    f'fits against its own random autoencoder; run {cmd}')
        if not args['fix_laligan']:
            return f'main_sweep needs --fix_laligan with the symmetry regulariser (g(x), J_g(x) computed once); run {cmd}'
    if adam and world > 1:
        return ('main_sweep runs the Adam fits in one process (no collective over seeds): give every GPU its own '
                'block of seeds, python -m symode_amd.main_sweep --seed <first> --n_seeds <count> ... per process')
    if engine is None and str(args.get('device')) == 'cpu':
        return 'symode_amd runs the SINDy path on the GPU only (no CPU fallback): a HIP device is required'
    if method == 'stlsq' and args['w_sym_reg'] > 0 and not symreg_stlsq and not symreg_path:
        return '--method stlsq sweeps the plain least-squares fit (use --method lbfgs with the symmetry regulariser)'
    if method == 'stlsq' and args.get('eq_constraint') and not equiv_stlsq:
        return '--method stlsq sweeps the unconstrained library (use --method lbfgs for EquivSINDy-c)'
    if args.get('device_shuffle') and (method == 'stlsq' or not adam):
        return ('--device_shuffle draws the epoch order of the minibatch Adam fit inside its launch: it needs '
                '--sindy_optimizer adam (with the default --method lbfgs), L-BFGS and STLSQ fits have no epoch order')
    if device_stlsq or stlsq_grid:
        why = _refusal_device_stlsq(args, method, grid, lbfgs_grid, n_seeds, device_stlsq, stlsq_grid,
                                    SYMREG_PATH_GRID_NAMES if symreg_path else
                                    SYMREG_STLSQ_GRID_NAMES if symreg_stlsq else STLSQ_GRID_NAMES,
                                    '--symreg_path' if symreg_path else '--symreg_stlsq')
        if why is not None:
            return why
    if grid and lbfgs_grid:
        return '--lbfgs_grid and --grid are the grids of two different sweeps (L-BFGS, Adam): give one of them'
    if grid:
        if method == 'stlsq' or not adam:
            return ('--grid gives every problem of the minibatch Adam launch its own hyper-parameters: it needs '
                    '--sindy_optimizer adam (with the default --method lbfgs); the L-BFGS and STLSQ sweeps take one value each')
        return _parse_grid(grid)[1]
    if lbfgs_grid:
        if method == 'stlsq' or adam:
            return ('--lbfgs_grid gives every problem of the device L-BFGS trainer its own hyper-parameters on shared Gram '
                    'matrices: it needs --sindy_optimizer lbfgs with the default --method lbfgs (the Adam sweep has --grid, the '
                    'STLSQ sweep takes one value each)')
        if not args.get('gram_closure'):
            return ('--lbfgs_grid needs --gram_closure: the grid points share the seeds\' Gram matrices, and the Gram route\'s '
                    'results differ from the streamed route\'s in the last bits -- a flag must not switch routes silently')
        axes, why = _parse_grid(lbfgs_grid, LBFGS_GRID_NAMES, '--lbfgs_grid')
        if why is not None:
            return why
        sym_axis = dict(axes).get('w_sym_reg')
        if sym_axis is not None and not args['w_sym_reg'] > 0:
            return ('--lbfgs_grid w_sym_reg needs the symmetry regulariser on the command line (--w_sym_reg > 0 with '
                    '--sym_reg_type r --load_laligan ... --fix_laligan): without it no regulariser matrices are built')
        if sym_axis is not None and not all(v > 0 for v in sym_axis):
            return (f'--lbfgs_grid w_sym_reg={",".join(f"{v:g}" for v in sym_axis)}: every value must be > 0 (a sweep without the '
                    'regulariser is another run, without --w_sym_reg)')
        n_points = int(np.prod([len(axis) for _, axis in axes]))
        if n_seeds is not None and n_points * n_seeds > MAX_GRID_PROBLEMS:
            return (f'--lbfgs_grid: {n_points} grid points x {n_seeds} seeds = {n_points * n_seeds} problems, one device trainer takes '
                    f'at most {MAX_GRID_PROBLEMS}')
    return None


SYMREG_STLSQ_MAX_COEFS = 64                                # d p of symode_stlsq_sweep_symreg: one lane per coefficient
EQUIV_STLSQ_MAX_PARAMS = 64                                # r' of symode_stlsq_sweep_constrained: one lane per free parameter


def _refusal_equiv_stlsq(args, method, device_stlsq, wsindy):
    """The rules of --equiv_stlsq that the arguments alone decide (r' <= 64 is known once Q exists: ``_fit_stlsq``)."""
    if wsindy:
        return ('--equiv_stlsq is the constrained fit of --method stlsq: the weak-SINDy sweep (--wsindy) fits the unconstrained '
                'library (drop one of them)')
    if method != 'stlsq':
        return '--equiv_stlsq is the constrained fit of the sequential-threshold least-squares sweep: it needs --method stlsq'
    if not device_stlsq:
        return ('--equiv_stlsq needs --device_stlsq: the constrained fit of the sweep runs on the device (the host route of '
                '--method stlsq sweeps the unconstrained library)')
    if not args.get('eq_constraint'):
        return ('--equiv_stlsq needs --eq_constraint: it fits under the equivariance constraint (drop --equiv_stlsq for the '
                'unconstrained library)')
    if args.get('lstsq_driver') == 'gelsy':
        return ('--equiv_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the '
                'host (python -m symode_amd.main_sindy per seed)')
    if args['w_sym_reg'] > 0:
        return ('--equiv_stlsq sweeps the constrained least-squares fit without a symmetry regulariser (w_sym_reg 0): use '
                '--method lbfgs with the regulariser')
    if args['use_latent']:
        return '--equiv_stlsq does not cover latent fits (--use_latent)'
    return None


def _refusal_min_norm_stlsq():
    """--min_norm_stlsq without --equiv_stlsq: what it is a mode of, and what that needs in turn."""
    return ('--min_norm_stlsq needs --equiv_stlsq: it is the rank-revealing mode of the constrained device fit (collinear '
            'columns of Q on the support are solved by the minimum-norm rule inside the launch), so it needs --method stlsq '
            '--device_stlsq --equiv_stlsq --eq_constraint; the unconstrained sweep meets no such systems')


def _refusal_symreg_stlsq(args, method, device_stlsq, wsindy, equiv_stlsq, min_norm_stlsq):
    """The rules of --symreg_stlsq that the arguments alone decide (d p <= 64 is known once the library is: ``_fit_stlsq``)."""
    if wsindy:
        return ('--symreg_stlsq is the regularised fit of --method stlsq: the weak-SINDy sweep (--wsindy) has no symmetry '
                'regulariser (drop one of them)')
    if method != 'stlsq':
        return ('--symreg_stlsq is the sequential-threshold least-squares sweep with the reversed symmetry regulariser: it '
                'needs --method stlsq')
    if not device_stlsq:
        return ('--symreg_stlsq needs --device_stlsq: the regularised fit of the sweep runs on the device (the host route of '
                '--method stlsq sweeps the plain least-squares fit)')
    if args.get('eq_constraint') or equiv_stlsq:
        return ('--symreg_stlsq does not go with --eq_constraint / --equiv_stlsq: the regularised fit under the equivariance '
                'constraint is not covered (use --method lbfgs)')
    if min_norm_stlsq:
        return ('--symreg_stlsq does not go with --min_norm_stlsq: the rank-revealing mode belongs to the constrained launch '
                '(--equiv_stlsq)')
    if not args['w_sym_reg'] > 0:
        return ('--symreg_stlsq needs --w_sym_reg > 0: it is the fit with the symmetry regulariser (drop --symreg_stlsq for the '
                'plain least-squares fit)')
    if args['sym_reg_type'] != 'r':
        return (f"--symreg_stlsq covers the reversed symmetry regulariser only (--sym_reg_type r), not '{args['sym_reg_type']}': "
                'the other regularisers are not quadratic in the coefficients')
    if args['load_laligan'] is None:
        return ('--symreg_stlsq needs --load_laligan: the regulariser\'s matrices are built from the group action of a saved '
                'LaLiGAN')
    if not args['fix_laligan']:
        return '--symreg_stlsq needs --fix_laligan: g(x), J_g(x) are computed once, from a frozen LaLiGAN'
    if args.get('lstsq_driver') == 'gelsy':
        return ('--symreg_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy has no '
                'regularised form')
    if args['use_latent']:
        return '--symreg_stlsq does not cover latent fits (--use_latent)'
    return None


BAG_CHUNKS = 128                                           # --bag_chunks' default
BAG_INCLUSION = 1.0                                        # --bag_inclusion's default (profiles/stlsq_bag.txt: how it was chosen)


def _parse_inclusion(text):
    """``--bag_inclusion v1,v2,...`` -> ([levels], None), or (None, why not): multiples of 0.001 in [0, 1], none twice."""
    from .sweep import inclusion_milli
    try:
        values = [float(v) for v in str(text).split(',')]
        milli = inclusion_milli(values)
    except ValueError:
        return None, (f'--bag_inclusion {text}: the inclusion levels must be a non-empty comma-separated list of multiples of 0.001 '
                      'in [0, 1] (the share of replicas a term has to survive in)')
    if len(set(milli)) != len(milli):
        return None, f'--bag_inclusion {text}: a level is given twice'
    return [t / 1000 for t in milli], None


def _refusal_bagging(args, method, world, engine, n_seeds, device_stlsq, bagging, bag_chunks, bag_inclusion, constrained, symreg_stlsq,
                     stlsq_path, symreg_path, wsindy, any_grid):
    """The rules of --bagging, --bag_chunks and --bag_inclusion, all decided by the arguments alone."""
    if bagging is None:
        given = ' and '.join(flag for flag, v in (('--bag_chunks', bag_chunks), ('--bag_inclusion', bag_inclusion)) if v is not None)
        return (f'{given} needs --bagging B: they are the chunk count and the inclusion levels of the bagged threshold fit (B '
                'bootstrap replicas per seed)')
    if wsindy:
        return ('--bagging is the bagged fit of --method stlsq: the weak-SINDy sweep (--wsindy) is not covered (drop one of them)')
    if method != 'stlsq':
        return ('--bagging is block-bootstrap bagging of the sequential-threshold least-squares sweep (ensemble SINDy): it needs '
                '--method stlsq')
    if not device_stlsq:
        return ('--bagging needs --device_stlsq: replicas, replica fits and refit are launches on the device (the host route of '
                '--method stlsq fits one subsample per seed)')
    if args.get('eq_constraint') or constrained:
        return ('--bagging does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: bagging under the equivariance '
                'constraint is not covered (drop them, or fit with --equiv_stlsq)')
    if args['w_sym_reg'] > 0 or symreg_stlsq or symreg_path:
        return ('--bagging does not go with --w_sym_reg > 0 / --symreg_stlsq / --symreg_path: bagging with the symmetry regulariser '
                'needs a joint refit over the rows and is not covered (drop them, or fit with --symreg_stlsq)')
    if stlsq_path:
        return ('--bagging does not go with --stlsq_path / --path_tol: the replicas are fit by the threshold loop, the path asks '
                'for no threshold (give one of them)')
    if any_grid:
        return ('--bagging does not go with --grid / --lbfgs_grid / --stlsq_grid / --wsindy_grid: its own grid is the list of '
                'inclusion levels, --bag_inclusion v1,v2,... (drop the grid)')
    if args.get('lstsq_driver') == 'gelsy':
        return ('--bagging fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the host '
                'route (drop one of them)')
    if args['use_latent']:
        return '--bagging does not cover latent fits (--use_latent)'
    if engine is None and str(args.get('device')) == 'cpu':
        return '--bagging runs on the GPU only (no CPU fallback): a HIP device is required'
    if world > 1:
        return ('--bagging runs in one process: the chunk matrices of the replicas are not all-reduced over ranks yet (give every '
                'GPU its own block of seeds, python -m symode_amd.main_sweep --seed <first> --n_seeds <count> ... per process)')
    if bagging < 1:
        return f'--bagging {bagging}: the number of bootstrap replicas per seed must be >= 1'
    if bag_chunks is not None and not 1 <= bag_chunks <= 1024:
        return f'--bag_chunks {bag_chunks}: a seed\'s rows are cut into 1 .. 1024 chunks'
    levels = [BAG_INCLUSION]
    if bag_inclusion is not None:
        levels, why = _parse_inclusion(bag_inclusion)
        if why is not None:
            return why
    if n_seeds is not None and n_seeds * bagging > MAX_GRID_PROBLEMS:
        return (f'--bagging: {n_seeds} seeds x {bagging} replicas = {n_seeds * bagging} replica problems, one launch takes at most '
                f'{MAX_GRID_PROBLEMS}')
    if n_seeds is not None and n_seeds * len(levels) > MAX_GRID_PROBLEMS:
        return (f'--bag_inclusion: {len(levels)} levels x {n_seeds} seeds = {n_seeds * len(levels)} problems, one launch takes at most '
                f'{MAX_GRID_PROBLEMS}')
    return None


PATH_TOL = 0.02                                            # --path_tol's default (profiles/stlsq_path.txt: how it was chosen)


def _refusal_stlsq_path(args, method, engine, device_stlsq, equiv_stlsq, min_norm_stlsq, symreg_stlsq, wsindy, any_grid, path_tol):
    """The rules of --stlsq_path, all decided by the arguments alone."""
    if method != 'stlsq':
        return ('--stlsq_path is the sparsity path of the sequential least-squares sweep (backward elimination scored on the '
                'validation set): it needs --method stlsq')
    if not device_stlsq:
        return ('--stlsq_path needs --device_stlsq: the path of every seed is one launch on the device (the host route of '
                '--method stlsq runs the threshold loop)')
    if args.get('eq_constraint') or equiv_stlsq or min_norm_stlsq:
        return ('--stlsq_path does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: the path under the equivariance '
                'constraint is a joint system over the rows and is not covered (drop them, or fit with --equiv_stlsq and a threshold)')
    if args['w_sym_reg'] > 0 or symreg_stlsq:
        return ('--stlsq_path does not go with --w_sym_reg > 0 / --symreg_stlsq: the path with the symmetry regulariser is a joint '
                'system over the rows and is not covered (drop them, or fit with --symreg_stlsq and a threshold)')
    if wsindy:
        return ('--stlsq_path is the path of --method stlsq: the weak-SINDy sweep (--wsindy) is not covered (drop one of them)')
    if any_grid:
        return ('--stlsq_path does not go with --grid / --lbfgs_grid / --stlsq_grid / --wsindy_grid: the path visits every '
                'support a threshold grid could reach and asks for no threshold (drop the grid)')
    if args.get('lstsq_driver') == 'gelsy':
        return ('--stlsq_path fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the '
                'host route (drop one of them)')
    if args['use_latent']:
        return '--stlsq_path does not cover latent fits (--use_latent)'
    if engine is None and str(args.get('device')) == 'cpu':
        return '--stlsq_path runs on the GPU only (no CPU fallback): a HIP device is required'
    if path_tol is not None and not (np.isfinite(path_tol) and path_tol >= 0):
        return f'--path_tol {path_tol:g}: the tolerance of the sparsity path must be a finite number >= 0'
    return None


def _refusal_symreg_path(args, method, engine, device_stlsq, stlsq_path, symreg_stlsq, equiv_stlsq, min_norm_stlsq, wsindy,
                         other_grid, stlsq_grid, path_tol):
    """The rules of --symreg_path that the arguments alone decide (d p <= 64 is known once the library is: ``_fit_stlsq``)."""
    if wsindy:
        return ('--symreg_path is the regularised sparsity path of --method stlsq: the weak-SINDy sweep (--wsindy) has no symmetry '
                'regulariser (drop one of them)')
    if method != 'stlsq':
        return ('--symreg_path is the sparsity path of the sequential least-squares sweep with the reversed symmetry regulariser: '
                'it needs --method stlsq')
    if not device_stlsq:
        return ('--symreg_path needs --device_stlsq: the path of every seed is one launch on the device (the host route of '
                '--method stlsq runs the threshold loop of the plain fit)')
    if stlsq_path:
        return ('--symreg_path does not go with --stlsq_path: they are two paths, the regularised joint one and the plain one per '
                'equation row (give one of them)')
    if symreg_stlsq:
        return ('--symreg_path does not go with --symreg_stlsq: the path asks for no threshold, the threshold loop for one (give '
                'one of them)')
    if args.get('eq_constraint') or equiv_stlsq or min_norm_stlsq:
        return ('--symreg_path does not go with --eq_constraint / --equiv_stlsq / --min_norm_stlsq: the path under the equivariance '
                'constraint goes rank deficient and is not covered (drop them, or fit with --equiv_stlsq and a threshold)')
    if not args['w_sym_reg'] > 0:
        return ('--symreg_path needs --w_sym_reg > 0: it is the path of the fit with the symmetry regulariser (--stlsq_path is the '
                'path of the plain least-squares fit)')
    if args['sym_reg_type'] != 'r':
        return (f"--symreg_path covers the reversed symmetry regulariser only (--sym_reg_type r), not '{args['sym_reg_type']}': "
                'the other regularisers are not quadratic in the coefficients')
    if args['load_laligan'] is None:
        return ('--symreg_path needs --load_laligan: the regulariser\'s matrices are built from the group action of a saved '
                'LaLiGAN')
    if not args['fix_laligan']:
        return '--symreg_path needs --fix_laligan: g(x), J_g(x) are computed once, from a frozen LaLiGAN'
    if other_grid:
        return ('--symreg_path does not go with --grid / --lbfgs_grid / --wsindy_grid: they are the grids of other sweeps (its own '
                'is --stlsq_grid w_sym_reg=... / w_sindy_reg=...)')
    if args.get('lstsq_driver') == 'gelsy':
        return ('--symreg_path fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy has no '
                'regularised form')
    if args['use_latent']:
        return '--symreg_path does not cover latent fits (--use_latent)'
    if engine is None and str(args.get('device')) == 'cpu':
        return '--symreg_path runs on the GPU only (no CPU fallback): a HIP device is required'
    if path_tol is not None and not (np.isfinite(path_tol) and path_tol >= 0):
        return f'--path_tol {path_tol:g}: the tolerance of the sparsity path must be a finite number >= 0'
    if any(str(spec).partition('=')[0] == 'threshold' for spec in stlsq_grid or ()):
        return ('--symreg_path does not take --stlsq_grid threshold=...: the path visits every support a threshold could reach and '
                'asks for no threshold (its axes are w_sym_reg and w_sindy_reg)')
    return None


def _refusal_device_stlsq(args, method, grid, lbfgs_grid, n_seeds, device_stlsq, stlsq_grid, names=STLSQ_GRID_NAMES,
                          sym_flag='--symreg_stlsq'):
    """The rules of --device_stlsq and --stlsq_grid (``_refusal``, which has applied the rules of --method stlsq itself).
    ``names``: the axes of the grid (SYMREG_STLSQ_GRID_NAMES under --symreg_stlsq, whose w_sym_reg values must be > 0;
    SYMREG_PATH_GRID_NAMES under --symreg_path, ``sym_flag`` then names that flag)."""
    given = ' and '.join(flag for flag, on in (('--device_stlsq', device_stlsq), ('--stlsq_grid', stlsq_grid)) if on)
    if method != 'stlsq':
        return (f'{given}: the device fit of the sequential-threshold least-squares sweep and its grid need --method stlsq '
                f'(the Adam sweep has --grid, the L-BFGS sweep --lbfgs_grid)')
    if stlsq_grid and (grid or lbfgs_grid):
        return ('--stlsq_grid, --grid and --lbfgs_grid are the grids of three different sweeps (STLSQ, Adam, L-BFGS): give '
                'one of them')
    if stlsq_grid and not device_stlsq:
        return ('--stlsq_grid needs --device_stlsq: the grid points share the seeds\' Gram matrices on the device, and the '
                'device fit is the full-rank driver\'s, whose results can differ from the host route\'s in the last bit -- a '
                'flag must not switch routes silently')
    if args.get('lstsq_driver') == 'gelsy':
        return ('--device_stlsq fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the '
                'host route (drop --device_stlsq)')
    if not stlsq_grid:
        return None
    axes, why = _parse_grid(stlsq_grid, names, '--stlsq_grid')
    if why is not None:
        return why
    for name, axis in axes:
        if name == 'w_sym_reg' and not all(v > 0 for v in axis):
            return (f'--stlsq_grid w_sym_reg={",".join(f"{v:g}" for v in axis)}: every value must be > 0 (a sweep without the '
                    f'regulariser is another run, without {sym_flag})')
        if not all(v >= 0 for v in axis):
            return f'--stlsq_grid {name}={",".join(f"{v:g}" for v in axis)}: every value must be >= 0'
    n_points = int(np.prod([len(axis) for _, axis in axes]))
    if n_seeds is not None and n_points * n_seeds > MAX_GRID_PROBLEMS:
        return (f'--stlsq_grid: {n_points} grid points x {n_seeds} seeds = {n_points * n_seeds} problems, one launch takes at most '
                f'{MAX_GRID_PROBLEMS}')
    return None


def _refusal_wsindy(args, method, world, engine, grid, lbfgs_grid, stlsq_grid, n_seeds, device_stlsq, wsindy, wsindy_grid):
    """The rules of --wsindy and --wsindy_grid, all of them: ``_refusal`` asks nothing else of such a run."""
    cfg = args.get('config')
    cmd = (f'python -m symode_amd.main_wsindy --seed $i --config {cfg}' if cfg else 'python -m symode_amd.main_wsindy --seed $i ...') + \
        ' for each seed (the per_seed loop of run_scripts/sweep.sh)'
    if not wsindy:
        return '--wsindy_grid needs --wsindy: it is the grid of the weak-SINDy sweep (the other sweeps have --grid, --lbfgs_grid, --stlsq_grid)'
    if method != 'lbfgs':
        return f'--wsindy is a fit of its own (weak form, sequential-threshold least squares on the device): drop --method {method}'
    if args['use_latent']:
        return f'--wsindy does not cover latent fits (--use_latent); run {cmd}'
    if args['w_sym_reg'] > 0:
        return f'--wsindy sweeps the plain weak-form least-squares fit (w_sym_reg 0), main_wsindy has no symmetry regulariser; run {cmd}'
    if args.get('eq_constraint'):
        return f'--wsindy sweeps the unconstrained library (no --eq_constraint); run {cmd}'
    if args.get('lstsq_driver') == 'gelsy':
        return f'--wsindy fits with the full-rank driver (gels) only: the rank rule of --lstsq_driver gelsy runs on the host; run {cmd}'
    if args.get('device_shuffle'):
        return '--device_shuffle draws the epoch order of the minibatch Adam fit: the weak-SINDy sweep has no epoch order (drop it)'
    if device_stlsq:
        return '--device_stlsq is the device fit of --method stlsq: the weak-SINDy sweep always fits on the device (drop it)'
    if grid or lbfgs_grid or stlsq_grid:
        return ('--grid, --lbfgs_grid and --stlsq_grid are the grids of three other sweeps (Adam, L-BFGS, STLSQ): the weak-SINDy sweep '
                'takes --wsindy_grid')
    if world > 1:
        return ('main_sweep runs the weak-SINDy fits in one process (no collective over seeds): give every GPU its own '
                'block of seeds, python -m symode_amd.main_sweep --wsindy --seed <first> --n_seeds <count> ... per process')
    if engine is None and str(args.get('device')) == 'cpu':
        return 'symode_amd runs the SINDy path on the GPU only (no CPU fallback): a HIP device is required'
    if n_seeds is not None and n_seeds > MAX_GRID_PROBLEMS:
        return f'--wsindy: {n_seeds} seeds = {n_seeds} problems, one launch takes at most {MAX_GRID_PROBLEMS}'
    if not wsindy_grid:
        return None
    axes, why = _parse_grid(wsindy_grid, WSINDY_GRID_NAMES, '--wsindy_grid')
    if why is not None:
        return why
    for name, axis in axes:
        if not all(v >= 0 for v in axis):
            return f'--wsindy_grid {name}={",".join(f"{v:g}" for v in axis)}: every value must be >= 0'
    n_points = int(np.prod([len(axis) for _, axis in axes]))
    if n_seeds is not None and n_points * n_seeds > MAX_GRID_PROBLEMS:
        return (f'--wsindy_grid: {n_points} grid points x {n_seeds} seeds = {n_points * n_seeds} problems, one launch takes at most '
                f'{MAX_GRID_PROBLEMS}')
    return None


# ---- fit: each takes the sweep's context (main) and returns Xi, mask (S, d, p), the library triple and its summary lines ------
def _rows(ctx):
    """This rank's columns lo:hi of every seed's subsample of the whole data set (see main)."""
    return seeded_subsamples(ctx.x_all.shape[0], ctx.m, ctx.seeds, ctx.dev)[:, ctx.lo:ctx.hi]


def _fit_stlsq(ctx):
    """--method stlsq: sequential-threshold least squares per seed (train.py:872-887) from ONE gather-Gram launch over the
    (seed, point) index table; the Gram matrices are all-reduced over the ranks."""
    args = ctx.args
    lib = (args['poly_order'], args['include_sine'], args['include_exp'])
    fit = {}
    if getattr(ctx, 'equiv_stlsq', False):
        # --equiv_stlsq: library and constraint are the template's, as the L-BFGS sweep builds it
        template = _template(ctx)[0]
        lib = (template.poly_order, template.include_sine, template.include_exp)
        coef = template.coef
        n_free = coef.r + (coef.d if coef.allow_constant else 0)
        if n_free > EQUIV_STLSQ_MAX_PARAMS:
            raise SystemExit(f"--equiv_stlsq: the constraint leaves r' = {n_free} free parameters ({coef.r} columns of Q"
                             f"{f' + {coef.d} constants' if coef.allow_constant else ''}), the device fit takes at most "
                             f'{EQUIV_STLSQ_MAX_PARAMS}; use --method lbfgs')
        fit = dict(coef=coef)
        if getattr(ctx, 'min_norm_stlsq', False):
            fit['min_norm'] = True
    names, column, laligan = STLSQ_GRID_NAMES, {}, None
    symreg_path = getattr(ctx, 'symreg_path', False)
    if getattr(ctx, 'symreg_stlsq', False) or symreg_path:
        # --symreg_stlsq / --symreg_path: library and LaLiGAN are the template's, as the L-BFGS sweep builds it
        template, _, laligan = _template(ctx)
        lib = (template.poly_order, template.include_sine, template.include_exp)
        n_coef = template.latent_dim * template.coef.p
        if n_coef > SYMREG_STLSQ_MAX_COEFS:
            flag = '--symreg_path' if symreg_path else '--symreg_stlsq'
            raise SystemExit(f'{flag}: the library has d p = {template.latent_dim} x {template.coef.p} = {n_coef} '
                             f'coefficients, the device fit takes at most {SYMREG_STLSQ_MAX_COEFS}; use --method lbfgs')
    rows = _rows(ctx)
    sw = SeedSweepSTLSQ(ctx.x_all, ctx.dx_all, *lib, n_seeds=len(ctx.seeds), subsample=args['lbfgs_subsample'], seed0=args['seed'],
                        group=ctx.group, engine=ctx.engine, idx=rows, idx_sorted=True)
    if getattr(ctx, 'stlsq_path', False):
        return _fit_stlsq_path(ctx, sw, lib)
    if getattr(ctx, 'bagging', None) is not None:
        return _fit_bagging(ctx, sw, lib)
    if laligan is not None:
        # [G | R | count] as _fit_lbfgs builds them under --gram_closure: no per-seed copy of the points, ONE all-reduce
        from .gram_closure import GramStatistics
        x_used, gx, jgx, table, used = symmetry_operands(ctx.x_all, rows, *laligan)
        stats = GramStatistics(len(ctx.seeds), template.latent_dim, template.poly_order, template.flags, regulariser=True,
                               device=ctx.dev, **ctx.kw)
        stats.add_gathered(x_used, ctx.dx_all[used].contiguous(), table, gx, jgx)
        if ctx.group is not None:
            stats.all_reduce(ctx.group)
        sw.set_grams(stats.G, stats.count)
        fit = dict(rev=(stats.R, args['w_sym_reg'] / args['w_sindy_x']))     # the weight relative to the MSE, as _fit_lbfgs
        names, column = SYMREG_STLSQ_GRID_NAMES, {'w_sym_reg': lambda v: v / args['w_sindy_x']}
    if symreg_path:
        return _fit_symreg_path(ctx, sw, lib, fit['rev'], column)
    n_seeds, points = len(ctx.seeds), getattr(ctx, 'grid', None)
    if points is not None:
        # --stlsq_grid: G points on common seeds, problem g * n_seeds + k = point g on seed k's matrices
        hyper = {names[name]: [column.get(name, float)(point[name]) for point in points for _ in ctx.seeds] for name in points[0]}
        Xi, mask, passes = sw.solve(args['w_sindy_reg'], args['threshold'], max_iter=max(1, args['num_epochs']),
                                    lstsq_driver=args.get('lstsq_driver'), device=True, hyper=hyper, **fit)
        lines = [f'{n_seeds} seeds x {sw.n_points} points (over {ctx.world} rank(s)), {len(points)} grid points on their Gram matrices']
        for g in range(len(points)):
            at = slice(g * n_seeds, (g + 1) * n_seeds)
            near = [rec for rec in sw.near_threshold if g * n_seeds <= rec[0] < (g + 1) * n_seeds]
            lines.append(f'grid {g}: STLSQ passes {int(passes[at].min())}-{int(passes[at].max())}, near-threshold coefficients '
                         f'(| |coef| - thr | < 1e-4): {near if near else "none"}')
        return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines + _min_norm_lines(sw, fit))
    route = dict(device=True) if getattr(ctx, 'device_stlsq', False) else {}
    Xi, mask, passes = sw.solve(args['w_sindy_reg'], args['threshold'], max_iter=max(1, args['num_epochs']),
                                lstsq_driver=args.get('lstsq_driver'), **route, **fit)
    lines = [f'{len(ctx.seeds)} seeds x {sw.n_points} points (over {ctx.world} rank(s)), STLSQ passes {int(passes.min())}-{int(passes.max())}',
             f'near-threshold coefficients (| |coef| - thr | < 1e-4): {sw.near_threshold if sw.near_threshold else "none"}']
    return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines + _min_norm_lines(sw, fit))


def _fit_stlsq_path(ctx, sw, lib):
    """--stlsq_path: the seeds' matrices as ``_fit_stlsq`` builds them, the validation set's matrix (every rank forms it from
    the whole set: no collective), ONE symode_stlsq_path launch (``SeedSweepSTLSQ.solve_path``).  Rank 0 also writes
    eval_results/<save_dir>/path.npz: order, rss_train, rss_val and best of all seeds."""
    args, val = ctx.args, ctx.val
    tol = PATH_TOL if ctx.path_tol is None else ctx.path_tol
    V = sw.val_grams(val.x.to(ctx.dev), val.dx.to(ctx.dev))
    Xi, mask, record = sw.solve_path(args['w_sindy_reg'], V, tol)
    if ctx.rank == 0:
        eval_dir = f'eval_results/{args["save_dir"]}'
        os.makedirs(eval_dir, exist_ok=True)
        np.savez(f'{eval_dir}/path.npz', seeds=np.asarray(ctx.seeds), path_tol=tol,
                 **{k: record[k] for k in ('order', 'rss_train', 'rss_val', 'best')})
    size = sw.p - record['best']                                          # (S, d): columns the chosen model keeps
    lines = [f'{len(ctx.seeds)} seeds x {sw.n_points} points (over {ctx.world} rank(s)), sparsity path of {sw.p + 1} models per row, '
             f'scored on {val.x.shape[0]} validation points, path_tol {tol:g}',
             'chosen support size per row: ' + ', '.join(f'row {j}: {int(size[:, j].min())}-{int(size[:, j].max())}'
                                                         for j in range(size.shape[1])),
             f'near-tie eliminations: {int((record["near"] > 0).sum())} of {len(ctx.seeds)} problems',
             f'--threshold ({args["threshold"]:g}) is not used by the path']
    return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines)


def _fit_bagging(ctx, sw, lib):
    """--bagging: the seeds' matrices as ``_fit_stlsq`` builds them and four launches (``SeedSweepSTLSQ.solve_bagged``); the
    levels of --bag_inclusion are ``ctx.grid`` (one level: no grid).  Rank 0 also writes eval_results/<save_dir>/bag.npz: count,
    valid, mean, std and fell of all seeds."""
    args = ctx.args
    B, C, levels = ctx.bagging, ctx.bag_chunks, ctx.bag_levels
    if C > sw.m_local:
        raise SystemExit(f'--bag_chunks {C}: a seed holds {sw.m_local} rows, every chunk needs at least one')
    Xi, mask, record = sw.solve_bagged(args['w_sindy_reg'], args['threshold'], B, n_chunks=C, inclusion=levels,
                                       max_iter=max(1, args['num_epochs']))
    n_seeds = len(ctx.seeds)
    if ctx.rank == 0:
        eval_dir = f'eval_results/{args["save_dir"]}'
        os.makedirs(eval_dir, exist_ok=True)
        np.savez(f'{eval_dir}/bag.npz', seeds=np.asarray(ctx.seeds), n_replicas=B, n_chunks=C, inclusion=np.asarray(levels),
                 **{k: record[k] for k in ('count', 'valid', 'mean', 'std', 'fell')})
    size = mask.sum(dim=(1, 2)).to(torch.int64).reshape(len(levels), n_seeds)
    valid = record['valid']
    lines = [f'{n_seeds} seeds x {sw.n_points} points (over {ctx.world} rank(s)), bagged: {B} replicas of {C} chunks x '
             f'{sw.m_local // C} rows per seed, valid replicas {int(valid.min())}-{int(valid.max())} of {B}, support size '
             + ', '.join(f'{int(size[g].min())}-{int(size[g].max())} at inclusion {level:g}' for g, level in enumerate(levels))
             + f', refits solved on the host: {int(record["fell"].sum())}']
    return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines)


def _fit_symreg_path(ctx, sw, lib, rev, column):
    """--symreg_path: [G | R | count] as ``_fit_stlsq`` builds them under --symreg_stlsq (``rev`` = (R, w_sym)), the validation
    set's matrix as ``_fit_stlsq_path`` forms it (every rank from the whole set: no collective), ONE symode_stlsq_path_symreg
    launch (``SeedSweepSTLSQ.solve_path(rev=...)``) -- under --stlsq_grid over G points x S seeds, ``column`` the map from an
    axis' values to the launch's.  Rank 0 also writes eval_results/<save_dir>/path.npz: the record's arrays of all problems."""
    args, val = ctx.args, ctx.val
    tol = PATH_TOL if ctx.path_tol is None else ctx.path_tol
    n_seeds, points = len(ctx.seeds), getattr(ctx, 'grid', None)
    hyper = None
    if points is not None:
        hyper = {SYMREG_PATH_GRID_NAMES[name]: [column.get(name, float)(point[name]) for point in points for _ in ctx.seeds]
                 for name in points[0]}
    V = sw.val_grams(val.x.to(ctx.dev), val.dx.to(ctx.dev))
    Xi, mask, record = sw.solve_path(args['w_sindy_reg'], V, tol, rev=rev, hyper=hyper)
    if ctx.rank == 0:
        eval_dir = f'eval_results/{args["save_dir"]}'
        os.makedirs(eval_dir, exist_ok=True)
        np.savez(f'{eval_dir}/path.npz', seeds=np.asarray(ctx.seeds), path_tol=tol,
                 **{k: record[k] for k in ('order', 'mse_train', 'reg_train', 'mse_val', 'best', 'near')})
    n0 = sw.d * sw.p
    size = n0 - record['best']                                            # (n_problems,): entries the chosen model keeps
    lines = [f'{n_seeds} seeds x {sw.n_points} points (over {ctx.world} rank(s)), regularised sparsity path of {n0 + 1} models per '
             f'problem (one chain over the {sw.d} rows), scored on {val.x.shape[0]} validation points, path_tol {tol:g}'
             + ('' if points is None else f', {len(points)} grid points on their Gram matrices')]
    if points is None:
        lines.append(f'chosen support size: {int(size.min())}-{int(size.max())} of {n0}')
    else:
        lines += [f'grid {g}: chosen support size: {int(size[g * n_seeds:(g + 1) * n_seeds].min())}-'
                  f'{int(size[g * n_seeds:(g + 1) * n_seeds].max())} of {n0}' for g in range(len(points))]
    lines += [f'near-tie eliminations: {int((record["near"] > 0).sum())} of {len(size)} problems',
              f'--threshold ({args["threshold"]:g}) is not used by the path']
    return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines)


def _min_norm_lines(sw, fit):
    """--min_norm_stlsq: one more summary line, the problems with passes the launch solved rank-truncated."""
    if not fit.get('min_norm'):
        return []
    hit = sw.rank_truncated
    return [f'rank-truncated passes (minimum-norm solution inside the launch): {int(hit.sum())} of {hit.size} problems']


def _fit_wsindy(ctx):
    """--wsindy: the weak-SINDy fit of main_wsindy per seed (main_wsindy.py:24-34, train.py:855-869) from ONE window
    contraction + normal-matrix call over the seeds' windows and ONE threshold-loop launch (sweep.SeedSweepWSINDy)."""
    args, train = ctx.args, ctx.train
    lib = (args['poly_order'], args['include_sine'], args['include_exp'])
    x3 = train.x.reshape(train.n_ics, train.n_steps, -1).to(ctx.dev)
    # (main_wsindy hands WSINDyWrapper the whole argument dict: the two keys where a caller sets them, else its defaults)
    tests = {k: args[k] for k in ('num_test_funcs', 'test_func_family') if k in args}
    sw = SeedSweepWSINDy(x3, *lib, dt=ode_dt_dict[args['task']], seeds=ctx.seeds, **tests, **ctx.kw)
    n_seeds, points = len(ctx.seeds), getattr(ctx, 'grid', None)
    head = f'{n_seeds} seeds x {sw.n_t} time points of one trajectory each, {sw.K} test functions'
    if points is not None:
        # --wsindy_grid: G points on common seeds, problem g * n_seeds + k = point g on seed k's matrices
        hyper = {WSINDY_GRID_NAMES[name]: [point[name] for point in points for _ in ctx.seeds] for name in points[0]}
        Xi, mask, passes = sw.solve(args['w_sindy_reg'], args['threshold'], max_iter=max(1, args['num_epochs']), hyper=hyper)
        lines = [f'{head}, {len(points)} grid points on their normal matrices']
        for g in range(len(points)):
            at = slice(g * n_seeds, (g + 1) * n_seeds)
            near = [rec for rec in sw.near_threshold if g * n_seeds <= rec[0] < (g + 1) * n_seeds]
            lines.append(f'grid {g}: STLSQ passes {int(passes[at].min())}-{int(passes[at].max())}, near-threshold coefficients '
                         f'(| |coef| - thr | < 1e-4): {near if near else "none"}')
        return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines)
    Xi, mask, passes = sw.solve(args['w_sindy_reg'], args['threshold'], max_iter=max(1, args['num_epochs']))
    lines = [f'{head}, STLSQ passes {int(passes.min())}-{int(passes.max())}',
             f'near-threshold coefficients (| |coef| - thr | < 1e-4): {sw.near_threshold if sw.near_threshold else "none"}']
    return SimpleNamespace(Xi=Xi, mask=mask, lib=lib, lines=lines)


def _load_laligan(args, dev):
    """Frozen autoencoder and generator of saved_models/<load_laligan>/, read as main._run reads them."""
    autoencoder = AutoEncoder(**args).to(dev)
    generator = LieGenerator(**args).to(dev)
    load_laligan(autoencoder, generator, args['load_laligan'], dev, map_location=dev)
    for module in (autoencoder, generator):
        module.eval()                                         # batch norm on its running statistics: g(x) is pointwise
        for param in module.parameters():
            param.requires_grad = False
    return autoencoder, generator


def _template(ctx):
    """What the L-BFGS and the Adam sweep start from: (template regressor -- it fixes library and constraint --, the seeds'
    initial parameters (S, n) in the constructor's draw order, the frozen LaLiGAN or None)."""
    args = ctx.args
    laligan = _load_laligan(args, ctx.dev) if args['w_sym_reg'] > 0 else None     # loaded BEFORE the template (main.py's order)
    if args['eq_constraint']:
        args['L_list'] = constraint_basis(laligan[1] if laligan else LieGenerator(**args), args['n_comps'])
    template = SINDyRegression(**args, **ctx.kw).to(ctx.dev)
    inits = [template.coef.draw(torch.Generator().manual_seed(s)) for s in ctx.seeds]
    return template, torch.stack(inits).to(ctx.dev), laligan


def _fit_lbfgs(ctx):
    """--method lbfgs: all seeds in lockstep on sweep.SeedSweepLBFGS.  With the reversed symmetry regulariser g(x), J_g(x) are
    computed once over the rows this rank's seeds use (weight w_sym_reg / w_sindy_x, as train._train_on_device) and enter
    either the fused stream closure as per-seed (S, n_g, m_local, d) copies or, under --gram_closure, per-seed [G | R] from
    the shared arrays and the index table: no per-seed copy of the points, ONE all-reduce of [G | R | count]."""
    args, dev = ctx.args, ctx.dev
    template, P0, laligan = _template(ctx)
    lib = (template.poly_order, template.include_sine, template.include_exp)
    rows = _rows(ctx)
    sym = laligan is not None
    w_sym = args['w_sym_reg'] / args['w_sindy_x'] if sym else 0.0
    stats = None
    if sym:
        x_used, gx, jgx, table, used = symmetry_operands(ctx.x_all, rows, *laligan)
    if sym and args.get('gram_closure'):
        from .gram_closure import GramStatistics
        stats = GramStatistics(len(ctx.seeds), template.latent_dim, template.poly_order, template.flags, regulariser=True,
                               device=dev, **ctx.kw)
        stats.add_gathered(x_used, ctx.dx_all[used].contiguous(), table, gx, jgx)
        clos = GramClosure(stats, w_sym=w_sym, coef=template.coef, group=ctx.group)
    else:
        X, DX = ctx.x_all[rows].contiguous(), ctx.dx_all[rows].contiguous()
        rev = None
        if sym:
            rev = (gx[:, table.long()].transpose(0, 1).contiguous(), jgx[:, table.long()].transpose(0, 1).contiguous(), w_sym)
        # (the fold kernel of a linear group action is the same closure up to rounding, not bit for bit: asked for by name)
        clos = BatchedClosure(X, DX, *lib, reversed_sym=rev, coef=template.coef, group=ctx.group,
                              linear_action=None if getattr(ctx, 'fold_linear_action', False) else False, **ctx.kw)
    sweep = SeedSweepLBFGS(clos, args['lr_sindy'], args['threshold'], args['st_freq'], w_sindy_x=args['w_sindy_x'],
                           sindy_reg_type=args['sindy_reg_type'], w_sindy_reg=args['w_sindy_reg'],
                           gram_closure=bool(args.get('gram_closure')), statistics=stats)
    points = getattr(ctx, 'grid', None)
    if points is None:
        out = sweep.fit(P0, args['num_epochs'])
        near = [ctx.seeds[i] for i in torch.nonzero(out["near_threshold"]).flatten().tolist()]
        lines = [f'{len(ctx.seeds)} seeds, epochs used {int(out["epochs"].min())}-{int(out["epochs"].max())}, '
                 f'finished {int(out["finished"].sum())}, NaN {int(out["nan"].sum())}, '
                 f'seeds with near-threshold coefficients {near or "none"}']
        return SimpleNamespace(Xi=out['Xi'], mask=out['mask'], lib=lib, lines=lines)
    # --lbfgs_grid: G points on common seeds, problem g * n_seeds + k = point g on seed k with seed k's matrices and start
    n_seeds = len(ctx.seeds)
    column = {'w_sym_reg': lambda v: v / args['w_sindy_x']}                  # the weight relative to the MSE, as w_sym above
    hyper = {LBFGS_GRID_NAMES[name]: [column.get(name, float)(point[name]) for point in points for _ in ctx.seeds]
             for name in points[0]}
    out = sweep.fit(P0.repeat(len(points), 1), args['num_epochs'], hyper=hyper)
    lines = []
    for g in range(len(points)):
        at = slice(g * n_seeds, (g + 1) * n_seeds)
        near = [ctx.seeds[i] for i in torch.nonzero(out["near_threshold"][at]).flatten().tolist()]
        lines.append(f'grid {g}: {n_seeds} seeds, epochs used {int(out["epochs"][at].min())}-{int(out["epochs"][at].max())}, '
                     f'finished {int(out["finished"][at].sum())}, NaN {int(out["nan"][at].sum())}, '
                     f'seeds with near-threshold coefficients {near or "none"}')
    return SimpleNamespace(Xi=out['Xi'], mask=out['mask'], lib=lib, lines=lines)


def _fit_adam(ctx):
    """--sindy_optimizer adam: the minibatch Adam fit of train_SIGED's plain branch on device_adam.DeviceAdam, one workgroup
    per seed, whole epochs per launch.  Every epoch of every seed is a pass over the WHOLE data set in batches of
    --batch_size (--lbfgs_subsample does not apply, as in main.py); seed s shuffles with its own device generator seeded
    with s, so a seed's fit depends on the seed alone, not on --n_seeds or --seed.  --device_shuffle: no generator, no keys
    and no argsort -- seed s is the order seed of problem s, the launch computes every row (DeviceAdam.fit(order_seeds=...));
    the fit is still a function of s alone, with other rows per step than the generator's shuffle gives.  --grid: the seeds'
    initial coefficients, order seeds or epoch orders repeated once per grid point, and the points' values as the per-problem
    table of DeviceAdam.fit(hyper=...); TABLE_BYTES then cuts the launches of the table path shorter."""
    from .device_adam import DeviceAdam
    args, dev, seeds = ctx.args, ctx.dev, ctx.seeds
    template, P0, _ = _template(ctx)
    lib = (template.poly_order, template.include_sine, template.include_exp)
    n_all, n_seeds = ctx.x_all.shape[0], len(seeds)
    trainer = DeviceAdam(ctx.x_all, ctx.dx_all, *lib, template.coef, args['lr_sindy'], args['w_sindy_x'], args['w_sindy_reg'],
                         args['threshold'], args['st_freq'], args['batch_size'], engine=ctx.engine)
    # --grid: G points on common seeds, problem g * n_seeds + k = point g on seed k with seed k's start and orders
    points = getattr(ctx, 'grid', None)
    G, grid = (1, {}) if points is None else (len(points), dict(hyper={
        GRID_NAMES[name]: [point[name] for point in points for _ in seeds] for name in points[0]}))
    if G > 1:
        P0 = P0.repeat(G, 1)
    if args.get('device_shuffle'):
        out = trainer.fit(P0, args['num_epochs'], order_seeds=seeds * G, **grid)
        return _adam_result(out, trainer, args, seeds, lib, points and G)
    gens = [torch.Generator(device=dev).manual_seed(s) for s in seeds]
    keys = torch.empty(n_seeds, n_all, device=dev)

    def orders():
        for _ in range(args['num_epochs']):
            for k, g in enumerate(gens):                            # row k is a function of seed k alone
                torch.rand(n_all, generator=g, out=keys[k])
            order = torch.argsort(keys, dim=1, stable=True)
            yield order if G == 1 else order.repeat(G, 1)           # the seeds' orders at every grid point

    return _adam_result(trainer.fit(P0, args['num_epochs'], orders(), **grid), trainer, args, seeds, lib, points and G)


def _adam_result(out, trainer, args, seeds, lib, G=None):
    """``G``: the number of grid points (problem g * n_seeds + k is point g on seed k), None without --grid."""
    n_seeds = len(seeds)
    near = out['log'][:, :, 3].sum(axis=0) if len(out['log']) else np.zeros((G or 1) * n_seeds)
    lines = []
    for g in range(G or 1):
        at = slice(g * n_seeds, (g + 1) * n_seeds)
        lines.append(('' if G is None else f'grid {g}: ') +
                     f'{n_seeds} seeds, {args["num_epochs"]} epochs x {trainer.steps} Adam steps of {trainer.batch} rows, '
                     f'NaN {int(out["nan"][at].sum())}, '
                     f'seeds with near-threshold coefficients {[seeds[i] for i in np.nonzero(near[at])[0].tolist()] or "none"}')
    return SimpleNamespace(Xi=out['Xi'], mask=out['mask'], lib=lib, lines=lines)


# ---- report ------------------------------------------------------------------------------------------------------------------
def _score_on_validation(val, Xi, mask, lib, task, bound_rel, dev, kw):
    """--eval_ltp: per-seed arrays for the npz files, from one roll-out launch over the validation trajectories
    (evaluation.eval_ltp_sweep; the horizon's bound is ``bound_rel`` times the data's variance) and one validation Gram
    (evaluation.val_mse_sweep).  Every rank holds the same final coefficients: rank 0 alone, no collective."""
    order, sine, exp = lib
    kw = dict(poly_order=order, include_sine=sine, include_exp=exp, **kw)
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
    forms = []
    for k, s in enumerate(seeds):
        coef, cf, mse, cf_all, mse_all = score_coefficients(Xi[k], mask[k], truth)
        more = {} if extra is None else {name: v[k] for name, v in extra.items()}
        np.savez(f'{eval_dir}/seed{s}.npz', coefficients=coef, correct_form=cf, mse=mse, correct_form_all=cf_all,
                 mse_all=mse_all, **more)
        forms.append(bool(cf_all))
    return forms


def _report(ctx, result, val_dataset, eval_ltp, ltp_bound_rel):
    """Rank 0: the per-seed result files, the fit's summary lines, the roll-out ranking, the aggregate (returned)."""
    if ctx.rank != 0:
        return None
    args, seeds = ctx.args, ctx.seeds
    scores = None
    if eval_ltp:
        scores = _score_on_validation(val_dataset, result.Xi.to(ctx.dev), result.mask.to(ctx.dev), result.lib, args['task'],
                                      ltp_bound_rel, ctx.dev, ctx.kw)
    Xi, mask = result.Xi.cpu().numpy(), result.mask.cpu().numpy().astype(bool)
    forms = _write_results(args, seeds, Xi, mask, truth_table(args['task'], mask.shape[-1], *result.lib[1:]), scores)
    for line in result.lines:
        print(line)
    if eval_ltp:
        _print_ltp_ranking(seeds, scores, forms)
    return aggregate_results(args['save_dir'], min_seed=seeds[0], max_seed=seeds[-1] + 1)


def _report_grid(ctx, result, val_dataset, eval_ltp, ltp_bound_rel):
    """--grid / --lbfgs_grid: ``_report`` per grid point into eval_results/<save_dir>/grid{g}/ (every seed file also holds the point's
    lr_sindy, w_sindy_reg and threshold -- under --lbfgs_grid its w_sym_reg too), the table of the points -- values, success rate = mean correct_form_all and, with
    --eval_ltp, the median over seeds of the per-seed median roll-out error and of val_mse -- on stdout and in
    eval_results/<save_dir>/grid.json, and {g: aggregate}."""
    if ctx.rank != 0:
        return None
    args, seeds, points = ctx.args, ctx.seeds, ctx.grid
    n_seeds = len(seeds)
    scores = None
    if eval_ltp:                                                     # all G x S models in the one roll-out launch
        scores = _score_on_validation(val_dataset, result.Xi.to(ctx.dev), result.mask.to(ctx.dev), result.lib, args['task'],
                                      ltp_bound_rel, ctx.dev, ctx.kw)
    Xi, mask = result.Xi.cpu().numpy(), result.mask.cpu().numpy().astype(bool)
    truth = truth_table(args['task'], mask.shape[-1], *result.lib[1:])
    for line in result.lines:
        print(line)
    table, out = [], {}
    for g, point in enumerate(points):
        at = slice(g * n_seeds, (g + 1) * n_seeds)
        values = {name: float(point.get(name, args[name])) for name in ctx.grid_names}
        extra = {name: np.full(n_seeds, v) for name, v in values.items()}
        if scores is not None:
            extra.update({name: np.asarray(v)[at] for name, v in scores.items()})
        sub = dict(args, save_dir=f'{args["save_dir"]}/grid{g}')
        forms = _write_results(sub, seeds, Xi[at], mask[at], truth, extra)
        row = dict(grid=g, **values, success_rate=float(np.mean(forms)))
        if scores is not None:
            med = np.median(extra['ltp_mean_error'], axis=1)
            row['ltp_median_error'] = float(np.median(np.where(np.isfinite(med), med, np.inf)))
            row['val_mse'] = float(np.median(extra['val_mse']))
        table.append(row)
        out[g] = aggregate_results(sub['save_dir'], min_seed=seeds[0], max_seed=seeds[-1] + 1)
    with open(f'eval_results/{args["save_dir"]}/grid.json', 'w') as f:                  # null: every seed diverged / NaN
        finite = [{k: v if not isinstance(v, float) or np.isfinite(v) else None for k, v in row.items()} for row in table]
        json.dump({'axes': [[name, axis] for name, axis in ctx.grid_axes], 'n_seeds': n_seeds, 'seed0': seeds[0], 'points': finite},
                  f, indent=1, allow_nan=False)
    print(f'grid of {len(points)} points x {n_seeds} seeds (' + ', '.join(table[0]) + '):')
    for row in table:
        print('  ' + ', '.join(f'{v:.6g}' if isinstance(v, float) else str(v) for v in row.values()))
    if scores is not None:
        best = min(table, key=lambda row: row['ltp_median_error'])          # the first of equals; inf = diverged
        print(f'best by validation roll-out error: grid {best["grid"]} (' +
              ' '.join(f'{name}={best[name]:g}' for name in ctx.grid_names) + ')')
    return out


def main(argv=None, engine=None, backend='nccl', one_gpu=False):
    """``engine`` / ``backend`` exist for the CPU rehearsal of the multi-rank path in tests (gloo + the test engine);
    ``one_gpu``: every rank uses cuda:0 (rehearsal of the HIP path with several ranks on a one-GPU box, gloo collectives)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    n_seeds = _pop(argv, '--n_seeds', 50, int)
    method = _pop(argv, '--method', 'lbfgs', str)
    eval_ltp = _pop_flag(argv, '--eval_ltp')
    ltp_bound_rel = _pop(argv, '--ltp_bound_rel', None, float)
    grid = _pop_all(argv, '--grid')
    lbfgs_grid = _pop_all(argv, '--lbfgs_grid')
    stlsq_grid = _pop_all(argv, '--stlsq_grid')
    device_stlsq = _pop_flag(argv, '--device_stlsq')
    wsindy_grid = _pop_all(argv, '--wsindy_grid')
    wsindy = _pop_flag(argv, '--wsindy')
    equiv_stlsq = _pop_flag(argv, '--equiv_stlsq')
    min_norm_stlsq = _pop_flag(argv, '--min_norm_stlsq')
    symreg_stlsq = _pop_flag(argv, '--symreg_stlsq')
    stlsq_path = _pop_flag(argv, '--stlsq_path')
    symreg_path = _pop_flag(argv, '--symreg_path')
    path_tol = _pop(argv, '--path_tol', None, float)
    bagging = _pop(argv, '--bagging', None, int)
    bag_chunks = _pop(argv, '--bag_chunks', None, int)
    bag_inclusion = _pop(argv, '--bag_inclusion', None, str)
    fold_linear_action = _pop_flag(argv, '--fold_linear_action')
    args = vars(get_args(argv=argv))
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    why = _refusal(args, method, world, engine, grid=grid or None, lbfgs_grid=lbfgs_grid or None, n_seeds=n_seeds,
                   device_stlsq=device_stlsq, stlsq_grid=stlsq_grid or None, wsindy=wsindy, wsindy_grid=wsindy_grid or None,
                   equiv_stlsq=equiv_stlsq, min_norm_stlsq=min_norm_stlsq, symreg_stlsq=symreg_stlsq, stlsq_path=stlsq_path,
                   path_tol=path_tol, symreg_path=symreg_path, bagging=bagging, bag_chunks=bag_chunks, bag_inclusion=bag_inclusion)
    if why is not None:
        raise SystemExit(why)
    group = init_ranks(args, world, one_gpu, backend, set_device=engine is None)
    if group is not None and rank != 0:                             # rank 0 makes the data files, the others read them
        dist.barrier()
    train_dataset, val_dataset, args = get_dataset(args)
    if group is not None and rank == 0:
        dist.barrier()
    # Every seed draws ONE subsample of the whole flattened data set (main.py:36-38: the first batch of a shuffled loader),
    # seeded by the seed alone; rank r works on rows [r m / W, (r+1) m / W) of that draw.  The union over the ranks is
    # the single-process subsample whatever the world size, so an N-rank run fits the same problems as a 1-rank run and
    # differs from it by summation order only.  (The data sets of the reference are a few MB: every rank keeps all of
    # x, dx resident and gathers its rows; the COMPUTE is what is sharded.)
    dev = args['device']
    x_all, dx_all = train_dataset.x.to(dev), train_dataset.dx.to(dev)
    m = int(x_all.shape[0] * args['lbfgs_subsample'])
    ctx = SimpleNamespace(args=args, seeds=list(range(args['seed'], args['seed'] + n_seeds)), dev=dev, group=group, rank=rank,
                          world=world, x_all=x_all, dx_all=dx_all, m=m, lo=rank * m // world, hi=(rank + 1) * m // world,
                          engine=engine, kw={} if engine is None else {'engine': engine}, grid=None,
                          device_stlsq=device_stlsq, fold_linear_action=fold_linear_action, train=train_dataset,
                          equiv_stlsq=equiv_stlsq, min_norm_stlsq=min_norm_stlsq, symreg_stlsq=symreg_stlsq,
                          stlsq_path=stlsq_path, path_tol=path_tol, val=val_dataset, symreg_path=symreg_path)
    if bagging is not None:
        ctx.bagging, ctx.bag_chunks = bagging, BAG_CHUNKS if bag_chunks is None else bag_chunks
        ctx.bag_levels = [BAG_INCLUSION] if bag_inclusion is None else _parse_inclusion(bag_inclusion)[0]
        if len(ctx.bag_levels) > 1:                                 # several levels: a grid on the same replica fits
            ctx.grid_names = {'bag_inclusion': 'inclusion'}
            ctx.grid_axes = [('bag_inclusion', ctx.bag_levels)]
            ctx.grid = _grid_points(ctx.grid_axes)
            args['bag_inclusion'] = ctx.bag_levels[0]               # (the report reads an axis' scalar from args)
    if wsindy_grid:
        ctx.grid_names = WSINDY_GRID_NAMES
        ctx.grid_axes = _parse_grid(wsindy_grid, WSINDY_GRID_NAMES, '--wsindy_grid')[0]
        ctx.grid = _grid_points(ctx.grid_axes)
    elif stlsq_grid:
        ctx.grid_names = SYMREG_PATH_GRID_NAMES if symreg_path else SYMREG_STLSQ_GRID_NAMES if symreg_stlsq else STLSQ_GRID_NAMES
        ctx.grid_axes = _parse_grid(stlsq_grid, ctx.grid_names, '--stlsq_grid')[0]
        ctx.grid = _grid_points(ctx.grid_axes)
    elif grid or lbfgs_grid:
        ctx.grid_names = GRID_NAMES if grid else LBFGS_GRID_NAMES
        ctx.grid_axes = _parse_grid(grid)[0] if grid else _parse_grid(lbfgs_grid, LBFGS_GRID_NAMES, '--lbfgs_grid')[0]
        ctx.grid = _grid_points(ctx.grid_axes)
    fit = {('stlsq', 'lbfgs'): _fit_stlsq, ('lbfgs', 'lbfgs'): _fit_lbfgs, ('lbfgs', 'adam'): _fit_adam}
    report = _report if ctx.grid is None else _report_grid
    fitter = _fit_wsindy if wsindy else fit[method, args['sindy_optimizer']]
    return report(ctx, fitter(ctx), val_dataset, eval_ltp, ltp_bound_rel)


if __name__ == '__main__':
    main()
