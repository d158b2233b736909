"""Seed sweep of the sequential-threshold least-squares fit, batched on the GPU.

The reference sweeps seeds with a shell loop, one process per seed (run_scripts/*.sh,
``for i in {0..49}``): every seed draws its own random subsample of the same data set
(``--lbfgs_subsample``, main.py:36-38) and fits it.  For the least-squares fit everything a seed
needs is its augmented Gram matrix, so the whole sweep is ONE gather kernel launch over the
(seed, point) index table (symode_aug_gram_gather, fp64 MFMA), an optional all-reduce of the
(S, (p+d)^2) fp64 matrices over the ranks' point shards (RCCL over xGMI), and S tiny host solves
per thresholding pass.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

from .coef_map import CoefMap
from .engine import LBFGS_ACCEPT, LBFGS_BEGIN, get_engine, library_flags
from . import lstsq as _lstsq
from .device_adam import _seed_words, _subsample_key
from .sindy import (NEAR_THRESHOLD_BAND, near_threshold_cases, stlsq_bag_from_gram, stlsq_constrained_from_gram,
                    stlsq_path_from_gram, stlsq_path_symreg_from_gram, stlsq_solve_from_gram, stlsq_symreg_from_gram,
                    weak_test_functions)


def seeded_subsamples(n, m, seeds, device, dtype=torch.int64):
    """(len(seeds), m) index table, rows ascending: for every seed an m-subset of range(n) that depends on THAT seed alone -- a
    seed's subsample (main.py:36-38: the first batch of a shuffled loader) does not depend on which other seeds run beside
    it, nor on the world size (every rank draws the same rows and takes its slice).
    On the GPU: ONE launch for all seeds (symode_seeded_subsamples: the m smallest of n counter-based keys per seed, radix
    select + ordered compaction, a workgroup per seed) -- the torch form below (a generator launch per seed, one batched
    top-k, one sort) took 1.1-1.2 ms for 64 seeds of 10^5 rows, three quarters of the STLSQ sweep.  On the CPU (tests of the
    host logic): uniform keys from a torch generator seeded by the seed, the m smallest kept."""
    device = torch.device(device)
    if m >= n:
        return torch.arange(n, device=device, dtype=dtype).expand(len(seeds), n).contiguous()
    if device.type == "cuda":
        return get_engine().seeded_subsamples(n, m, seeds, device).to(dtype)
    g = torch.Generator(device=device)
    keys = torch.empty(len(seeds), n, dtype=torch.float64, device=device)          # fp64 keys: ties are not a concern
    for row, seed in zip(keys, seeds):
        g.manual_seed(int(seed))
        row.uniform_(generator=g)
    idx = torch.topk(keys, m, dim=1, largest=False, sorted=False).indices
    return torch.sort(idx, dim=1).values.to(dtype)


BAG_MAX_CHUNKS = 1024                   # RESAMPLE_MAX_CHUNKS of csrc/gram_resample.hpp
BAG_MAX_REPLICA_PROBLEMS = 2 ** 31 - 1  # what symode_stlsq_sweep takes as a problem count


def resample_counts(seed, b, n_chunks):
    """How often each of ``n_chunks`` chunks is drawn for bootstrap replica ``b`` of ``seed``: the draw of symode_gram_resample
    (csrc/gram_resample.hpp) in Python integer arithmetic, constant for constant.  w = seed_words(seed_words(seed) + b) modulo
    2^64; draw t = 0 .. C-1 is u = subsample_key(low32(w), high32(w), t) and lands on chunk (u * C) >> 32.  Returns (C,) int32,
    which sums to C."""
    C = int(n_chunks)
    lo, hi = _seed_words(int(seed))
    lo, hi = _seed_words(((hi << 32) | lo) + int(b))
    counts = np.zeros(C, dtype=np.int32)
    for t in range(C):
        counts[(_subsample_key(lo, hi, t) * C) >> 32] += 1
    return counts


def resample_grams(chunk, seeds, n_replicas):
    """symode_gram_resample in numpy: chunk (S, C, n, n) fp64 -> ((S B, n, n) fp64, counts (S B, C) int32), replica b of seed k at
    k B + b, each the sum from 0.0 over c ascending of count[c] * chunk[k, c], chunks that were not drawn skipped."""
    chunk = np.asarray(chunk, dtype=np.float64)
    S, C = chunk.shape[:2]
    B = int(n_replicas)
    out, counts = np.zeros((S * B,) + chunk.shape[2:]), np.zeros((S * B, C), dtype=np.int32)
    for k in range(S):
        for b in range(B):
            counts[k * B + b] = resample_counts(seeds[k], b, C)
            for c in np.nonzero(counts[k * B + b])[0]:
                out[k * B + b] = out[k * B + b] + float(counts[k * B + b, c]) * chunk[k, c]
    return out, counts


def inclusion_milli(inclusion):
    """The inclusion levels of a bagged fit in thousandths: a value or a list of values in [0, 1], each a multiple of 0.001."""
    values = [inclusion] if np.isscalar(inclusion) else list(inclusion)
    if not values:
        raise ValueError('inclusion: at least one level is needed')
    milli = []
    for v in values:
        t = int(round(float(v) * 1000)) if np.isfinite(float(v)) else -1
        if not 0 <= t <= 1000 or abs(float(v) * 1000 - t) > 1e-6:
            raise ValueError(f'inclusion: every level must be a multiple of 0.001 in [0, 1], got {v!r}')
        milli.append(t)
    return milli


SINGULAR_WORDS = 'singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead'


def _hyper_columns(hyper, defaults, S, prefix, named, named_empty):
    """A ``hyper`` dict of per-problem columns read against ``defaults`` {column: the scalar argument it stands in for}:
    (n_problems, {column: one value per problem}), a column left out filled from its scalar; without a table one problem per
    seed.  ``prefix`` and ``named`` / ``named_empty`` (the table names a column that is not allowed / no column at all) word
    the refusals as each caller has them."""
    n_problems = S
    if hyper is not None:
        if set(hyper) - set(defaults) or not hyper:
            raise ValueError(f"{prefix}hyper: the per-problem columns of {named if hyper else named_empty}, got {sorted(hyper)}")
        lengths = {len(v) for v in hyper.values()}
        n_problems = lengths.pop()
        if lengths or n_problems < S or n_problems % S != 0:
            raise ValueError(f'{prefix}hyper: every column needs one value per problem, a multiple of the {S} seeds (problem s '
                             f'on seed s % {S}); got lengths {sorted({len(v) for v in hyper.values()})}')
    return n_problems, {k: (hyper or {}).get(k, [v] * n_problems) for k, v in defaults.items()}


def _in_fp32(values):
    """per-problem values as a launch holds them: rounded to fp32 (kept in fp64 for the host twins)"""
    return np.array([float(np.float32(v)) for v in values], dtype=np.float64)


class _HostSets:
    """Host copies of single sets of device matrices, made when first asked for: at most one device-to-host copy per
    (matrix, set), and only for the sets touched."""

    def __init__(self, **matrices):
        self.matrices, self.held = matrices, {}

    def __call__(self, name, k):
        if (name, k) not in self.held:
            self.held[name, k] = self.matrices[name][k].cpu().numpy()
        return self.held[name, k]


def _flagged_to_host(fell, solve_on_host, also=False):
    """The problems a launch flagged go to the host, ``solve_on_host(s)`` each; where there was one (or ``also``), the
    RuntimeWarning of the full-rank driver that names the minimum-norm answer."""
    flagged = np.nonzero(fell)[0].tolist()
    for s in flagged:
        solve_on_host(s)
    if flagged or also:
        import warnings
        warnings.warn(SINGULAR_WORDS, RuntimeWarning)


class _DeviceSTLSQ:
    """The device fit of a sweep whose problems are (p+d, p+d) fp64 matrices on the device: what SeedSweepSTLSQ and
    SeedSweepWSINDy share.  The class supplies engine, S, d, p, n_points and ``grams(device=True)``."""

    _fetch_with_fit = None                 # an int32 device tensor to bring back in the fit's one copy (SeedSweepWSINDy)

    def _replay(self, s, G_s, w_reg, threshold, max_iter, lstsq_driver, Xi, mask, passes, coef=None, rev=None):
        """Problem s again in numpy, pass by pass from the full mask, for the detailed near-threshold record.  ``coef`` (a
        CoefMap with Q): the constrained fit's pass (sindy.stlsq_constrained_from_gram), whose drivers ``lstsq_driver`` names.
        ``rev`` (problem s's R (d p, d p), its w_sym): the pass with the reversed regulariser (sindy.stlsq_symreg_from_gram)."""
        mask[s] = True
        for it in range(max_iter):
            if rev is not None:
                xi32 = stlsq_symreg_from_gram(G_s, rev[0], self.n_points, mask[s], float(w_reg), float(rev[1]), self.d, lstsq_driver)[0]
            elif coef is not None:
                xi32 = stlsq_constrained_from_gram(G_s, self.n_points, mask[s], float(w_reg), self.d, coef, lstsq_driver)[0]
            else:
                xi, _ = stlsq_solve_from_gram(G_s, self.n_points, mask[s], float(w_reg), self.d, lstsq_driver)
                xi32 = xi.astype(np.float32)
            self.near_threshold += [(s, it, i, k, v) for i, k, v in near_threshold_cases(xi32, mask[s], threshold)]
            new_mask = np.logical_and(np.abs(xi32) > np.float32(threshold), mask[s])   # strict >, monotone (sindy.py:194)
            converged = np.array_equal(new_mask, mask[s])
            Xi[s], mask[s], passes[s] = xi32, new_mask, it + 1
            if converged:
                break

    def _solve_device(self, w_sindy_reg, threshold, max_iter, hyper, coef=None, min_norm=False, rev=None):
        """``solve(device=True)``: one symode_stlsq_sweep launch on the matrices where the gather launch left them; only
        Xi, mask, passes, near and fell come back.  The launch takes ridge weight and threshold in fp32, as its per-problem
        table holds them, with or without a table -- so problem (g, k) of a grid is bit for bit seed k of the scalar device
        solve with point g's values -- and what is replayed or solved on the host here uses the same rounded values.
        Every rank holds the same all-reduced matrices and takes the same decisions.
        ``coef`` (a CoefMap with Q): the launch is symode_stlsq_sweep_constrained, the fit under Xi = Q beta (+ const); a
        problem it flags (a pivot under SINGULAR_RCOND^2 of the first: possibly rank deficient) is solved by the host loop
        with the minimum-norm rule on every pass.
        ``min_norm`` (with ``coef``): the launch is symode_stlsq_sweep_minnorm, which performs that rule on every pass itself
        (rcond = SINGULAR_RCOND).  A problem whose passes were rank-truncated then costs no host work and no copy of its
        matrix; what is left to the host is a problem the launch flags (the factor of Wm Wm^T not positive definite) and the
        replay for the near-threshold record, with the rule the launch applied ('min_norm' where a pass was truncated).
        ``rev`` ((S, d p, d p) fp64 matrices R of the reversed regulariser, w_sym): the launch is symode_stlsq_sweep_symreg,
        per pass the minimiser of mse + w_sym * reg; ``hyper`` then also takes a ``w_sym`` column, and the launch holds that
        value in fp32 as well.  A problem it flags is solved by the host loop with the minimum-norm rule on every pass."""
        S, d, p = self.S, self.d, self.p
        defaults = {'w_reg': w_sindy_reg, 'threshold': threshold}
        named = 'the STLSQ sweep are w_reg and threshold'
        if rev is not None:
            defaults['w_sym'] = rev[1]
        n_problems, col = _hyper_columns(hyper, defaults, S, '', named if rev is None else 'the STLSQ sweep with the reversed '
                                         'regulariser are w_reg, threshold and w_sym', named)
        w, thr = _in_fp32(col['w_reg']), _in_fp32(col['threshold'])
        if not (np.all(np.isfinite(w)) and np.all(np.isfinite(thr)) and np.all(w >= 0) and np.all(thr >= 0)):
            raise ValueError('the ridge weight and the threshold of every problem must be finite and >= 0')
        if rev is not None:
            wsym = _in_fp32(col['w_sym'])
            if not (np.all(np.isfinite(wsym)) and np.all(wsym >= 0)):
                raise ValueError('the weight w_sym of the reversed regulariser must be finite and >= 0 for every problem')
        G, R = self.grams(device=True), None
        # the launch: (engine method, its operands, its own keywords, how many items it returns, where ``trunc`` is among them)
        floor = _lstsq.SINGULAR_RCOND ** 2
        if rev is not None:
            R = torch.as_tensor(rev[0]).to(device=G.device, dtype=torch.float64).reshape(S, d * p, d * p).contiguous()
            rows = [w, thr, wsym]
            launch, args, own, n_out, at_trunc = ('stlsq_sweep_symreg', (G, R, self.n_points, w[0], thr[0], wsym[0], max_iter),
                                                  {'pivot_floor': floor}, 5, None)
        else:
            rows = [w, thr]
            launch, args, own, n_out, at_trunc = 'stlsq_sweep', (G, self.n_points, w[0], thr[0], max_iter), {}, 5, None
            if coef is not None:
                q_solve, q_xi = (torch.from_numpy(q).to(G.device) for q in (coef.solve_matrix(), coef.xi_matrix()))
                args += (q_solve, q_xi, coef.allow_constant)
                launch, own, n_out, at_trunc = (('stlsq_sweep_minnorm', {'rcond': _lstsq.SINGULAR_RCOND}, 8, 6) if min_norm
                                                else ('stlsq_sweep_constrained', {'pivot_floor': floor}, 6, None))
        table = None if hyper is None else torch.from_numpy(np.stack(rows, axis=1).astype(np.float32)).to(G.device)
        out = getattr(self.engine, launch)(*args, hyper=table, d=d, near_band=NEAR_THRESHOLD_BAND, to_host=True,           # one copy back
                                           tail=self._fetch_with_fit, **own)
        if len(out) > n_out:
            self._fetched(out[n_out])
        Xi, mask, passes = np.array(out[0]), np.asarray(out[1]).astype(bool), np.asarray(out[2]).astype(np.int64)
        near, fell = np.array(out[3]), out[4]
        trunc = np.zeros(n_problems, dtype=np.int32) if at_trunc is None else out[at_trunc]
        self.near_threshold = []
        held = _HostSets(G=G, R=R)
        on_host = lambda s: held('G', s % S)                                              # noqa: E731
        rev_on_host = lambda s: None if rev is None else (held('R', s % S), wsym[s])      # noqa: E731
        self.rank_truncated = np.array(trunc) > 0                       # (n_problems,): a pass solved with rank < n on the device

        def flagged(s):
            if rev is not None or coef is not None:
                # possibly rank deficient: the host loop from the full mask, the minimum-norm rule on every pass
                self._replay(s, on_host(s), w[s], thr[s], max_iter, 'min_norm', Xi, mask, passes, coef, rev_on_host(s))
                near[s] = 0                                              # (its near-threshold record is the loop's)
                return
            # a pivot that was not positive: the problem is the host loop's, rank-revealing fallback included
            Gs = np.ascontiguousarray(on_host(s), dtype=np.float64)[None]
            xi1, m1 = np.zeros((1, d, p), dtype=np.float32), np.ones((1, d, p), dtype=np.uint8)
            p1, n1, f1 = (np.zeros(1, dtype=np.int32) for _ in range(3))
            rc = _lstsq._native().symode_host_stlsq_sweep(Gs.ctypes.data, 1, d, p, int(self.n_points), float(w[s]), float(thr[s]),
                                                          int(max_iter), 1, float(NEAR_THRESHOLD_BAND), xi1.ctypes.data, m1.ctypes.data,
                                                          p1.ctypes.data, n1.ctypes.data, f1.ctypes.data)
            if rc != 0:
                raise RuntimeError(f'symode_host_stlsq_sweep failed with code {rc}')
            Xi[s], mask[s], passes[s], near[s] = xi1[0], m1[0].astype(bool), p1[0], n1[0]

        # (the constrained fit names the minimum-norm answer also where the launch itself gave it: a rank-truncated pass)
        _flagged_to_host(fell, flagged, also=coef is not None and self.rank_truncated.any())
        for s in np.nonzero(near)[0].tolist():
            self._replay(s, on_host(s), w[s], thr[s], max_iter, 'min_norm' if trunc[s] > 0 else 'gels', Xi, mask, passes, coef,
                         rev_on_host(s))
        return torch.from_numpy(Xi), torch.from_numpy(mask.astype(np.float32)), passes


class SeedSweepSTLSQ(_DeviceSTLSQ):
    def __init__(self, x, dx, poly_order, include_sine=False, include_exp=False, n_seeds=64, subsample=0.5, seed0=0,
                 group=None, engine=None, idx=None, idx_sorted=False):
        """x, dx: (N_local, d) rows of the flattened data set (dataset.py:193-194) this rank gathers from.
        ``idx`` (S, m_local) int32: the rows of x this rank contributes to each seed's subsample; by default every
        (seed, rank) draws its own seeded permutation of the rank's shard."""
        assert x.dim() == 2 and x.shape == dx.shape
        self.engine = engine or get_engine()
        self.x, self.dx = x.contiguous(), dx.contiguous()
        self.n_local, self.d = x.shape
        self.order, self.flags = poly_order, library_flags(include_sine, include_exp)
        self.p = self.engine.lib_size(self.d, poly_order, self.flags)
        self.S = n_seeds
        self.group = group
        if idx is not None:
            assert idx.dim() == 2 and idx.shape[0] == n_seeds
            self.idx = idx.to(torch.int32).to(x.device).contiguous()
            self.m_local = idx.shape[1]
            # a seed's Gram is a sum over its rows: visit them in ascending order (near-sequential reads of x, dx)
            if not idx_sorted:                               # (seeded_subsamples' tables already are)
                self.idx = torch.sort(self.idx, dim=1).values.contiguous()
        else:
            rank = dist.get_rank(group) if group is not None else 0
            m = max(1, int(self.n_local * subsample))
            # seeded subset per (seed, rank): reproducible
            self.idx = seeded_subsamples(self.n_local, m, [1_000_003 * (seed0 + s) + rank for s in range(n_seeds)],
                                         x.device, dtype=torch.int32)
            self.m_local = m
        # what the bootstrap replicas of ``solve_bagged`` are keyed by: the seed of each problem, the rank left out
        self.seeds = [1_000_003 * (seed0 + s) for s in range(n_seeds)]
        self._gram, self._gram_dev = None, None

    def grams(self, device=False):
        """(S, p+d, p+d) fp64 on the host, summed over the ranks' shards.  ``device=True``: the same all-reduced matrices
        as the tensor the gather launch (and the all-reduce) left on the device, without the copy."""
        if not device and self._gram is not None:
            return self._gram
        if self._gram_dev is None and self._gram is not None:          # matrices that were handed in on the host
            self._gram_dev = torch.from_numpy(np.ascontiguousarray(self._gram, dtype=np.float64)).to(self.x.device)
        if self._gram_dev is None:
            G = self.engine.aug_gram_gather(self.x, self.dx, self.idx, self.order, self.flags)
            if self.group is not None:
                n = torch.tensor([float(self.m_local)], dtype=torch.float64, device=G.device)
                dist.all_reduce(G, op=dist.ReduceOp.SUM, group=self.group)
                dist.all_reduce(n, op=dist.ReduceOp.SUM, group=self.group)
                self.n_points = int(n.item())
            else:
                self.n_points = int(self.m_local)
            self._gram_dev = G
        if device:
            return self._gram_dev
        if self._gram is None:
            self._gram = self._gram_dev.cpu().numpy()
        return self._gram

    def set_grams(self, G, n_points):
        """Hand in the seeds' (S, p+d, p+d) fp64 matrices on the device, already summed over the ranks, and the points behind
        each (a caller that built them beside other statistics, in one collective): ``grams`` then gathers nothing."""
        self._gram_dev, self._gram, self.n_points = G, None, int(n_points)

    def val_grams(self, x_val, dx_val):
        """(1, p+d, p+d) fp64 on the device: the augmented Gram matrix of the held-out rows x_val, dx_val (N_val, d), one dense
        symode_aug_gram launch -- ``solve_path``'s ``val_gram``, shared by all seeds (n_val_sets = 1).  Under several ranks
        every rank hands in the WHOLE validation set and forms the same matrix, so there is no collective."""
        assert x_val.dim() == 2 and x_val.shape == dx_val.shape and x_val.shape[1] == self.d
        dev = self.x.device
        return self.engine.aug_gram(x_val.to(dev).contiguous()[None], dx_val.to(dev).contiguous()[None], self.order, self.flags)

    def solve_path(self, w_sindy_reg, val_gram, tol, floor_rel=1e-10, device=True, keep_path=False, rev=None, hyper=None):
        """The sparsity path for every seed: backward elimination from the full library to the empty model (solve, drop the
        smallest coefficient, solve again), every model scored on the held-out matrix ``val_gram`` ((n_val, p+d, p+d) fp64 raw
        sums, host or device, n_val = 1 or S: ``val_grams``), and per equation row the sparsest model kept whose held-out
        error is <= (1 + tol) max(best, 0) + floor_rel Vyy.  No threshold is asked for.
        ``floor_rel`` = 1e-10 keeps the rule meaningful where the best error is rounding noise around 0 (an exact fit): it is
        two decades above the (p + 1)^2 2^-53 ~ 5e-13 rounding level of the quadratic forms, relative to Vyy, at p = 64.
        ``device=True``: ONE symode_stlsq_path launch on the matrices where ``grams(device=True)`` left them and one copy
        back of the small outputs; a problem the launch flags (a pivot that is not positive) goes to the host twin
        (sindy.stlsq_path_from_gram) with the RuntimeWarning of the full-rank driver, and only those problems' matrices are
        copied.  ``device=False``: the host twin for every seed.
        Returns (Xi (S, d, p) float32, mask (S, d, p) float32, record) with record = dict(order (S, d, p), rss_train, rss_val
        (S, d, p+1), best (S, d), near (S,)) and, with ``keep_path=True``, path_xi (S, d, p+1, p).
        ``rev=(R, w_sym)``: the path of the fit with the reversed symmetry regulariser, EquivSINDy-r (R as ``solve`` takes
        it).  R couples the equation rows, so there is ONE chain per PROBLEM over the joint (d, p) support of n0 = d p <= 64
        entries, not one per row: record = dict(order (n_problems, n0) flat indices j p + k, mse_train, reg_train, mse_val
        (n_problems, n0+1) -- raw sums over the rows; the regulariser is scored on the training set only --, best, near
        (n_problems,)) and, with ``keep_path=True``, path_xi (n_problems, n0+1, d, p).  ``device=True`` is ONE
        symode_stlsq_path_symreg launch, a flagged problem goes to sindy.stlsq_path_symreg_from_gram; the ridge weight and
        w_sym are held in fp32 on both routes, as the launch holds them.  ``hyper={"w_reg": [...], "w_sym": [...]}`` (with
        ``rev`` and ``device=True``): one value per PROBLEM as in ``solve``, problem s on seed s % S; a column left out takes
        the scalar argument."""
        if rev is not None:
            return self._solve_path_symreg(w_sindy_reg, val_gram, tol, floor_rel, device, keep_path, rev, hyper)
        if hyper is not None:
            raise ValueError('solve_path: hyper (a per-problem table of w_reg / w_sym) needs rev=(R, w_sym): the table is the '
                             "regularised path's")
        S, d, p = self.S, self.d, self.p
        for name, v in (('w_sindy_reg', w_sindy_reg), ('tol', tol), ('floor_rel', floor_rel)):
            if not (np.isfinite(float(v)) and float(v) >= 0):
                raise ValueError(f'solve_path: {name} must be finite and >= 0, got {v}')
        shape = tuple(val_gram.shape)
        if len(shape) != 3 or shape[1:] != (p + d, p + d) or shape[0] not in (1, S):
            raise ValueError(f'solve_path: val_gram must be (n_val, p + d, p + d) = (1 or {S}, {p + d}, {p + d}), got {shape}')
        gamma = float(np.sqrt(float(w_sindy_reg)))

        def twin(s, Gs, Vs, Rs):
            return stlsq_path_from_gram(Gs, Vs, gamma, float(tol), float(floor_rel), NEAR_THRESHOLD_BAND, d, self.n_points)

        def launch(G, V, R):
            return self.engine.stlsq_path(G, V, self.n_points, gamma, float(tol), float(floor_rel), d=d, near_band=NEAR_THRESHOLD_BAND,
                                          to_host=True, keep_path=keep_path)

        return self._path_fit(device, keep_path, ('order', 'rss_train', 'rss_val', 'best', 'near'), twin, launch, val_gram)

    def _path_fit(self, device, keep_path, keys, twin, launch, val_gram, R=None):
        """The two routes of a sparsity path, whatever the fit.  ``device=False``: every seed through ``twin(s, G_s, V_s, R_s)``
        -> (Xi, mask, record), stacked.  ``device=True``: ``launch(G, V, R)`` on the device matrices, one fetch, and the
        problems it flagged patched from the twin (with the full-rank driver's warning), only their matrices copied.
        ``keys``: what the record keeps."""
        S, n_val = self.S, val_gram.shape[0]
        keys += ('path_xi',) if keep_path else ()
        if not device:
            G = self.grams()
            Rh = R if R is None else R.detach().cpu().numpy() if torch.is_tensor(R) else np.asarray(R)
            Vh = val_gram.detach().cpu().numpy() if torch.is_tensor(val_gram) else np.asarray(val_gram, dtype=np.float64)
            out = [twin(s, G[s], Vh[s % n_val], None if R is None else Rh[s]) for s in range(S)]
            record = {k: np.stack([np.asarray(o[2][k]) for o in out]) for k in keys}
            record['near'] = record['near'].astype(np.int32)              # (the launch's type)
            return (torch.from_numpy(np.stack([o[0] for o in out])),
                    torch.from_numpy(np.stack([o[1] for o in out]).astype(np.float32)), record)
        G = self.grams(device=True)
        if R is not None:
            R = torch.as_tensor(R).to(device=G.device, dtype=torch.float64).reshape(S, self.d * self.p, self.d * self.p).contiguous()
        V = torch.as_tensor(val_gram).to(device=G.device, dtype=torch.float64).contiguous()
        o = launch(G, V, R)
        Xi, mask = np.array(o['Xi']), np.asarray(o['mask']).astype(bool)
        record = {k: np.array(o[k]) for k in keys}
        held = _HostSets(G=G, V=V, R=R)

        def flagged(s):
            # possibly rank deficient: the problem is the host twin's, minimum-norm fallback included
            Xi[s], mask[s], rec = twin(s, held('G', s % S), held('V', s % n_val), None if R is None else held('R', s % S))
            for k in keys:
                record[k][s] = rec[k]

        _flagged_to_host(o['fell'], flagged)
        return torch.from_numpy(Xi), torch.from_numpy(mask.astype(np.float32)), record

    def _solve_path_symreg(self, w_sindy_reg, val_gram, tol, floor_rel, device, keep_path, rev, hyper):
        """``solve_path(rev=...)``: see there."""
        S, d, p = self.S, self.d, self.p
        n0 = d * p
        if n0 > 64:
            raise ValueError(f'solve_path: rev (the reversed symmetry regulariser): d p = {d} x {p} = {n0} unknowns, the joint '
                             'system of a step takes at most 64')
        if len(rev) != 2 or tuple(rev[0].shape) != (S, n0, n0):
            raise ValueError(f'solve_path: rev must be (R, w_sym) with R (S, d p, d p) = ({S}, {n0}, {n0})')
        for name, v in (('w_sindy_reg', w_sindy_reg), ('w_sym', rev[1]), ('tol', tol), ('floor_rel', floor_rel)):
            if not (np.isfinite(float(v)) and float(v) >= 0):
                raise ValueError(f'solve_path: {name} must be finite and >= 0, got {v}')
        shape = tuple(val_gram.shape)
        if len(shape) != 3 or shape[1:] != (p + d, p + d) or shape[0] not in (1, S):
            raise ValueError(f'solve_path: val_gram must be (n_val, p + d, p + d) = (1 or {S}, {p + d}, {p + d}), got {shape}')
        if hyper is not None and not device:
            raise ValueError('solve_path: hyper (a per-problem table of w_reg / w_sym) needs device=True: the host route takes '
                             'one value each')
        named = 'the regularised path are w_reg and w_sym'
        _, col = _hyper_columns(hyper, {'w_reg': w_sindy_reg, 'w_sym': rev[1]}, S, 'solve_path: ', named, named)
        w, wsym = np.array([float(v) for v in col['w_reg']], dtype=np.float64), _in_fp32(col['w_sym'])
        if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(np.isfinite(wsym)) and np.all(wsym >= 0)):
            raise ValueError('solve_path: the ridge weight and w_sym of every problem must be finite and >= 0')
        gamma = _in_fp32(np.sqrt(w))                                           # as the launch holds it

        def twin(s, Gs, Vs, Rs):
            return stlsq_path_symreg_from_gram(Gs, Rs, Vs, gamma[s], wsym[s], float(tol), float(floor_rel), NEAR_THRESHOLD_BAND, d,
                                               self.n_points)

        def launch(G, V, R):
            table = None if hyper is None else torch.from_numpy(np.stack([gamma, wsym], axis=1).astype(np.float32)).to(G.device)
            return self.engine.stlsq_path_symreg(G, R, V, self.n_points, gamma[0], wsym[0], float(tol), float(floor_rel), hyper=table,
                                                 d=d, pivot_floor=_lstsq.SINGULAR_RCOND ** 2, near_band=NEAR_THRESHOLD_BAND,
                                                 to_host=True, keep_path=keep_path)

        return self._path_fit(device, keep_path, ('order', 'mse_train', 'reg_train', 'mse_val', 'best', 'near'), twin, launch,
                              val_gram, rev[0])

    def chunk_grams(self, n_chunks):
        """(S, C, p+d, p+d) fp64 on the device: for every seed the augmented Gram matrices of C = ``n_chunks`` chunks of its
        rows, ONE symode_aug_gram_gather launch.  Seed k's ascending rows idx[k, :C L], L = m // C, are viewed as an (S C, L)
        table: chunk c holds rows c L .. (c + 1) L - 1 of the seed's subsample, neighbours in time.  The rows beyond C L --
        fewer than C of them -- are in no chunk: they take part in the seed's own matrix (``grams``), on which the bagged
        model is refit, and in no replica."""
        C = int(n_chunks)
        if not 1 <= C <= BAG_MAX_CHUNKS:
            raise ValueError(f'n_chunks = {C}: the chunk counts of a replica take 1 .. {BAG_MAX_CHUNKS} chunks')
        if C > self.m_local:
            raise ValueError(f'n_chunks = {C} chunks need at least one row each: a seed holds m = {self.m_local} rows')
        if self.group is not None and dist.get_world_size(self.group) > 1:
            raise ValueError('chunk_grams: more than one rank is not covered (the chunk matrices would need their own all-reduce)')
        L = self.m_local // C
        table = self.idx[:, :C * L].reshape(self.S * C, L).contiguous()
        G = self.engine.aug_gram_gather(self.x, self.dx, table, self.order, self.flags)
        return G.reshape(self.S, C, self.p + self.d, self.p + self.d)

    def solve_bagged(self, w_sindy_reg, threshold, n_replicas, n_chunks=128, inclusion=1.0, max_iter=10, device=True):
        """Block-bootstrap bagging of the threshold fit (ensemble SINDy) for every seed: B = ``n_replicas`` replicas of a seed's
        data, each a resample with replacement of the seed's C = ``n_chunks`` chunks of rows (``chunk_grams``), are fit by the
        threshold loop; a term is kept when the share of replicas it survives in reaches ``inclusion``; the model is refit
        on that support from the seed's own matrix.  Four launches whatever B and the number of levels: the chunk matrices
        (symode_aug_gram_gather), the replica matrices (symode_gram_resample), the S B replica fits (symode_stlsq_sweep with
        this ridge weight, threshold and ``max_iter``), aggregation and refit (symode_stlsq_bag).  ``inclusion``: a value, or a
        list of G values -- the grid, problem (g, k) = g S + k is seed k at level g; multiples of 0.001 in [0, 1].
        Returns (Xi (G S, d, p) float32, mask (G S, d, p) float32, record) with record = dict(count (S, d, p) int32, valid (S,)
        int32, mean, std (S, d, p) float64 -- per term the replicas that keep it, and mean and standard deviation of its
        coefficient over those -- fell (G S,) bool: the refits the launch handed to the host; all False with ``device=False``).  A replica whose fit met a pivot
        that is not positive is left out (``valid`` counts the rest); a refit that did is solved by the host twin
        (sindy.stlsq_bag_from_gram: the minimum-norm answer, with the full-rank driver's RuntimeWarning).  The launches take
        ridge weight and threshold in fp32, as ``solve(device=True)`` does.
        ``device=False``: resample, replica fits (symode_host_stlsq_sweep, full-rank driver), aggregation and refit in numpy on
        the chunk matrices of the one gather launch."""
        S, d, p = self.S, self.d, self.p
        B = int(n_replicas)
        if B < 1:
            raise ValueError(f'n_replicas = {B}: a bagged fit needs at least one replica')
        if S * B > BAG_MAX_REPLICA_PROBLEMS:
            raise ValueError(f'{S} seeds x {B} replicas are more than the {BAG_MAX_REPLICA_PROBLEMS} problems of one launch')
        milli = inclusion_milli(inclusion)
        w, thr = _in_fp32([w_sindy_reg])[0], _in_fp32([threshold])[0]
        if not (np.isfinite(w) and np.isfinite(thr) and w >= 0 and thr >= 0):
            raise ValueError('the ridge weight and the threshold must be finite and >= 0')
        max_iter = max(1, int(max_iter))
        chunk = self.chunk_grams(n_chunks)
        G = self.grams(device=True)
        tau = [t for t in milli for _ in range(S)]
        if device:
            rep = self.engine.gram_resample(chunk, self.seeds, B)
            rxi, rmask, _, _, rfell = self.engine.stlsq_sweep(rep, self.n_points, w, thr, max_iter, d=d,
                                                              near_band=NEAR_THRESHOLD_BAND)
            out = self.engine.stlsq_bag(G, rxi, rmask, rfell, B, w, tau_table=tau, d=d, to_host=True)          # one copy back
            Xi, mask, fell = np.array(out[0]), np.asarray(out[1]).astype(bool), np.array(out[2])
            record = dict(count=np.array(out[3]), valid=np.array(out[4]), mean=np.array(out[5]), std=np.array(out[6]))
            held = _HostSets(G=G)
            replicas = None

            def on_host(s):
                nonlocal replicas
                if replicas is None:                                # the replica fits come to the host only when a refit fell
                    replicas = tuple(t.cpu().numpy() for t in (rxi, rmask, rfell))
                k = s % S
                return held('G', k), tuple(t[k * B:(k + 1) * B] for t in replicas)
        else:
            rep, _ = resample_grams(chunk.cpu().numpy(), self.seeds, B)
            rxi, rm8 = np.zeros((S * B, d, p), dtype=np.float32), np.ones((S * B, d, p), dtype=np.uint8)
            rp, rn, rfell = (np.zeros(S * B, dtype=np.int32) for _ in range(3))
            rep = np.ascontiguousarray(rep)
            lib = _lstsq._native()
            if not lib:
                raise RuntimeError('solve_bagged(device=False) fits the replicas with symode_host_stlsq_sweep: build the library')
            rc = lib.symode_host_stlsq_sweep(rep.ctypes.data, S * B, d, p, int(self.n_points), float(w), float(thr), max_iter, 1,
                                             float(NEAR_THRESHOLD_BAND), rxi.ctypes.data, rm8.ctypes.data, rp.ctypes.data,
                                             rn.ctypes.data, rfell.ctypes.data)
            if rc != 0:
                raise RuntimeError(f'symode_host_stlsq_sweep failed with code {rc}')
            Gh = self.grams()
            Xi, mask = np.zeros((len(tau), d, p), dtype=np.float32), np.zeros((len(tau), d, p), dtype=bool)
            record = None
            on_host = lambda s: (Gh[s % S], tuple(t[(s % S) * B:(s % S + 1) * B] for t in (rxi, rm8, rfell)))      # noqa: E731

        def twin(s):
            Gs, (xi_b, mask_b, fell_b) = on_host(s)
            Xi[s], mask[s], rec = stlsq_bag_from_gram(Gs, xi_b, mask_b, fell_b, tau[s], float(w), d, self.n_points)
            return rec

        if device:
            _flagged_to_host(fell, twin)
        else:
            recs = [twin(s) for s in range(len(tau))]
            record = {k: np.stack([np.asarray(r[k]) for r in recs[:S]]) for k in ('count', 'valid', 'mean', 'std')}
            record['valid'] = record['valid'].astype(np.int32)
            fell = np.zeros(len(tau), dtype=np.int32)               # (nothing is handed over: the twin's own fallback answers)
        record['fell'] = np.asarray(fell) != 0
        return torch.from_numpy(Xi), torch.from_numpy(mask.astype(np.float32)), record

    def solve(self, w_sindy_reg, threshold, max_iter=10, lstsq_driver=None, device=False, hyper=None, coef=None, min_norm=False,
              rev=None):
        """STLSQ to convergence for every seed (train.py:872-887 per seed).
        Returns (Xi (S, d, p) float32, mask (S, d, p) float32, passes (S,)).
        ``device=True``: the fit runs on the device (``_solve_device``; the full-rank driver only), the host route stays the
        default.  ``hyper={"w_reg": [...], "threshold": [...]}`` (with ``device=True``): one value per PROBLEM, n_problems = G x S
        for a grid of G points on the S seeds' shared matrices, problem s on seed s % S; the arrays returned are then
        (G S, d, p) and (G S,), and a column left out takes the scalar argument.
        ``coef`` (a CoefMap with Q): the fit under the equivariance constraint Xi = Q beta (+ const), EquivSINDy-c
        (solve_SINDy_one_step's constrained branch per seed); Xi is then ``get_Xi`` of the last solve, unmasked.  On the host
        it is the numpy loop (sindy.stlsq_constrained_from_gram) with the driver given; ``device=True`` as above.
        ``min_norm=True`` (with ``device=True`` and a ``coef`` that holds Q; opt-in): the rank-revealing mode of the constrained
        launch (symode_stlsq_sweep_minnorm).  A pass whose support leaves Q's columns collinear is solved inside the launch
        by the minimum-norm rule the host loop would apply (``lstsq_normal(Gq, cq, m, 'gelsy', SINGULAR_RCOND)``), so such
        problems are not handed to the host; the RuntimeWarning that names the minimum-norm answer is raised all the same,
        and ``self.rank_truncated`` (n_problems,) bool says which problems it concerns.
        ``rev=(R, w_sym)``: the fit with the reversed symmetry regulariser, EquivSINDy-r -- per pass the minimiser of
        mse + w_sym * reg on the support, one linear system (sindy.stlsq_symreg_system).  R (S, d p, d p) fp64, host or device,
        raw sums over each seed's points (``symreg_reversed_gram_gather`` on the rows behind ``grams``).  On the host it is the
        numpy loop (sindy.stlsq_symreg_from_gram), the full-rank driver by default; ``device=True`` is ONE
        symode_stlsq_sweep_symreg launch, ``hyper`` then also takes a ``w_sym`` column.  d p <= 64."""
        if rev is not None:
            if coef is not None and coef.Q is not None:
                raise ValueError('rev (the reversed symmetry regulariser) does not go with coef (the equivariance constraint): '
                                 'the combined system Qe^T (Gm + w_sym R) Qe is not covered')
            if min_norm:
                raise ValueError('rev (the reversed symmetry regulariser) does not go with min_norm=True: the rank-revealing mode '
                                 'is the constrained launch\'s')
            if lstsq_driver == 'gelsy':
                raise ValueError("rev (the reversed symmetry regulariser) does not go with lstsq_driver='gelsy': the regularised "
                                 'system is solved with the full-rank driver (gels)')
            if self.d * self.p > 64:
                raise ValueError(f'rev (the reversed symmetry regulariser): d p = {self.d} x {self.p} = {self.d * self.p} unknowns, '
                                 'the joint system of a pass takes at most 64')
            if len(rev) != 2 or tuple(rev[0].shape) != (self.S, self.d * self.p, self.d * self.p):
                raise ValueError(f'rev must be (R, w_sym) with R (S, d p, d p) = ({self.S}, {self.d * self.p}, {self.d * self.p})')
            if not (np.isfinite(float(rev[1])) and float(rev[1]) >= 0 and np.isfinite(float(w_sindy_reg)) and float(w_sindy_reg) >= 0
                    and np.isfinite(float(threshold)) and float(threshold) >= 0):
                raise ValueError('rev (the reversed symmetry regulariser): w_sym, the ridge weight and the threshold must be finite '
                                 'and >= 0')
            if lstsq_driver is None:
                lstsq_driver = 'gels'
        elif hyper is not None and 'w_sym' in hyper:
            raise ValueError('hyper: a w_sym column needs rev=(R, w_sym): without the regulariser\'s matrices there is nothing to weigh')
        if min_norm:
            if not device:
                raise ValueError('min_norm=True needs device=True: it is a mode of the device launch (on the host route '
                                 "lstsq_driver='gelsy' is the rank-revealing fit)")
            if coef is None or coef.Q is None:
                raise ValueError('min_norm=True needs coef=<a CoefMap that holds Q>: it is the rank-revealing mode of the '
                                 'constrained fit Xi = Q beta (+ const); the unconstrained launch meets no collinear columns')
            if lstsq_driver == 'gelsy':
                raise ValueError("min_norm=True does not go with lstsq_driver='gelsy': the launch cuts the rank at SINGULAR_RCOND "
                                 "on the triangular factor (the full-rank driver's fallback), gelsy's default rule "
                                 'eps32 * max(m, n) runs on the host route')
        if coef is not None and coef.Q is None:
            coef = None                                    # a map without Q: the variables are Xi, the unconstrained fit
        if hyper is not None and not device:
            raise ValueError('hyper (a per-problem table of w_reg / threshold) needs device=True: the host route takes one value each')
        if lstsq_driver is None:                   # torch.linalg.lstsq's default on the device the data lives on (sindy.py)
            lstsq_driver = "gels" if self.x.is_cuda else "gelsy"
        if device:
            if lstsq_driver != 'gels':
                raise ValueError(f"device=True fits with the full-rank driver (gels) only, not lstsq_driver='{lstsq_driver}': the "
                                 'rank rule of gelsy runs on the host route')
            return self._solve_device(w_sindy_reg, threshold, max(1, int(max_iter)), hyper, coef, min_norm, rev)
        G = self.grams()
        S, d, p = self.S, self.d, self.p
        Xi = np.zeros((S, d, p), dtype=np.float32)
        mask = np.ones((S, d, p), dtype=bool)
        passes = np.zeros(S, dtype=np.int64)
        self.near_threshold = []              # (seed index, pass, row, col, |coef|): BASELINE.md section 3
        todo = range(S)
        lib = _lstsq._native() if os.environ.get('SYMODE_STLSQ_NATIVE', '1') != '0' else None
        if rev is not None:
            R = rev[0].detach().cpu().numpy() if torch.is_tensor(rev[0]) else np.asarray(rev[0])
            for s in todo:
                self._replay(s, G[s], w_sindy_reg, threshold, max_iter, lstsq_driver, Xi, mask, passes, rev=(R[s], float(rev[1])))
            return torch.from_numpy(Xi), torch.from_numpy(mask.astype(np.float32)), passes
        if lib and lstsq_driver in ('gels', 'gelsy') and coef is None:
            # the whole loop below for all seeds in ONE native call (host_lstsq.cpp::symode_host_stlsq_sweep: same solver, same
            # inputs, same arithmetic); seeds that met a near-threshold coefficient are replayed here for the detailed record
            Gc = np.ascontiguousarray(G, dtype=np.float64)
            m8 = np.ones((S, d, p), dtype=np.uint8)
            p32, near, fell = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
            rc = lib.symode_host_stlsq_sweep(Gc.ctypes.data, S, d, p, int(self.n_points), float(w_sindy_reg), float(threshold),
                                             int(max_iter), 0 if lstsq_driver == 'gelsy' else 1, float(NEAR_THRESHOLD_BAND),
                                             Xi.ctypes.data, m8.ctypes.data, p32.ctypes.data, near.ctypes.data, fell.ctypes.data)
            if rc != 0:
                raise RuntimeError(f'symode_host_stlsq_sweep failed with code {rc}')
            if fell.any():
                import warnings
                warnings.warn(SINGULAR_WORDS, RuntimeWarning)
            mask, passes = m8.astype(bool), p32.astype(np.int64)
            todo = [int(s) for s in np.nonzero(near)[0]]
        for s in todo:
            self._replay(s, G[s], w_sindy_reg, threshold, max_iter, lstsq_driver, Xi, mask, passes, coef)
        return torch.from_numpy(Xi), torch.from_numpy(mask.astype(np.float32)), passes


# =================================================================================================
# Seed sweep of the weak-SINDy fit (main_wsindy for S seeds at once)
# =================================================================================================
def weak_windows(seeds, n_ics, n_steps, n_t):
    """(len(seeds), 2) int64 rows [trajectory, start]: for seed n the window ``main_wsindy --seed n`` fits
    (main_wsindy.py:26-27 after its ``np.random.seed(n)``: first ``start = randint(0, n_steps - n_t)``, then
    ``traj = randint(0, n_ics)``; ``np.random.RandomState(n)`` is the generator np.random.seed(n) leaves).
    The two agree whenever ``get_dataset`` draws nothing from numpy's global generator between the seeding and the two
    draws.  That holds for the four ODE tasks (lv, selkov, dosc, growth) with their data files on disk AND when they are
    generated: data.py draws initial conditions and noise from torch generators of its own, seeded from the data's seed.
    It does not hold for rd / mt_rd, whose loader adds noise from numpy's global generator -- tasks with no trajectories
    to take a window of, which the weak-SINDy drivers do not cover."""
    if not 1 <= n_t < n_steps:
        raise ValueError(f'n_t = {n_t} must lie in 1 .. n_steps - 1 = {n_steps - 1}: the window start is drawn from [0, n_steps - n_t)')
    out = np.zeros((len(seeds), 2), dtype=np.int64)
    for row, seed in zip(out, seeds):
        rs = np.random.RandomState(int(seed))
        row[1] = rs.randint(0, n_steps - n_t)
        row[0] = rs.randint(0, n_ics)
    return out


class SeedSweepWSINDy(_DeviceSTLSQ):
    """``main_wsindy`` for S seeds in three launches.  A seed differs from the next only in the window of the shared data
    it reads; time grid, test functions and M = V V^T are common.  The weak fit on a window is an STLSQ fit on the
    (p+d, p+d) matrix N = Z^T M Z, Z = [G | b], with ridge gamma = sqrt(w_sindy_reg) (WSINDyWrapper.solve adds
    w_sindy_reg I to G^T M G, the STLSQ entries gamma^2 I), so: ONE symode_weak_normal_windows call (window contraction,
    normal matrices) and ONE symode_stlsq_sweep launch, the matrices never leaving the device."""

    def __init__(self, x3, poly_order, include_sine=False, include_exp=False, dt=None, seeds=None, windows=None, n_t=None,
                 num_test_funcs=50, test_func_family='trig', engine=None):
        """x3 (n_ics, n_steps, d) on the device, ``dt`` its time step.  ``seeds``: the windows are ``weak_windows``' (sweep
        seed n reads the window main_wsindy --seed n reads); or ``windows`` (S, 2) [trajectory, start] rows given outright.
        ``n_t`` points per window, int(0.8 n_steps) by default (main_wsindy.py:26)."""
        assert x3.dim() == 3 and dt is not None and (seeds is None) != (windows is None)
        self.engine = engine or get_engine()
        self.x = x3.contiguous()
        self.n_ics, self.n_steps, self.d = x3.shape
        self.order, self.flags = poly_order, library_flags(include_sine, include_exp)
        self.p = self.engine.lib_size(self.d, poly_order, self.flags)
        self.n_t = int(0.8 * self.n_steps) if n_t is None else int(n_t)
        self.n_points = self.n_t
        self.windows = weak_windows(list(seeds), self.n_ics, self.n_steps, self.n_t) if windows is None else np.asarray(windows)
        self.S = len(self.windows)
        t = torch.arange(self.n_t) * dt                                         # main_wsindy.py:31-33
        _, _, self.V, self.V_drv, self._VVt = weak_test_functions(t, self.n_t * dt, num_test_funcs, test_func_family, x3.device)
        self.K = self.V.shape[0]
        self._normal_dev, self._normal, self.bad = None, None, None

    def normals(self, device=False):
        """(S, p+d, p+d) fp64: every window's N.  ``device=True``: the tensor the one call of the entry left on the device."""
        if self._normal_dev is None:
            M = torch.from_numpy(np.ascontiguousarray(self._VVt)).to(self.x.device)
            self._normal_dev, self._fetch_with_fit = self.engine.weak_normal_windows(self.x, self.windows, self.n_t, self.V,
                                                                                     self.V_drv, M, self.order, self.flags)
        if device:
            return self._normal_dev
        if self._normal is None:
            self._normal = self._normal_dev.cpu().numpy()
        return self._normal

    grams = normals                        # the name _DeviceSTLSQ reads its matrices by

    def _fetched(self, bad):
        """The kernel's range flags, read in the copy that fetched the fit's results."""
        self.bad = np.array(bad)
        if self.bad.any():
            s = int(np.argmax(self.bad))
            raise RuntimeError(f'symode_weak_normal_windows flagged windows[{s}] = {self.windows[s].tolist()} as out of range')

    def solve(self, w_sindy_reg, threshold, max_iter=10, hyper=None):
        """The threshold loop of train_WSINDy (train.py:855-869) for every seed on the device, the full-rank driver (gels).
        Returns (Xi (S, d, p) float32, mask (S, d, p) float32, passes (S,)); ``near_threshold`` is kept as by
        SeedSweepSTLSQ.  ``hyper={"w_reg": [...], "threshold": [...]}``: one value per PROBLEM, w_reg in units of
        w_sindy_reg, problem s on seed s % S (a grid of G points on the S windows' shared matrices)."""
        gamma = lambda w: float(np.sqrt(w)) if np.isfinite(w) and w >= 0 else float('nan')     # noqa: E731  (refused by name below)
        if hyper is not None and 'w_reg' in hyper:
            hyper = dict(hyper, w_reg=[gamma(float(w)) for w in hyper['w_reg']])
        return self._solve_device(gamma(float(w_sindy_reg)), threshold, max(1, int(max_iter)), hyper)


# =================================================================================================
# Seed sweep of the L-BFGS fit (train_SIGED_lbfgs for S seeds at once)
# =================================================================================================
class BatchedLBFGS:
    """torch.optim.LBFGS (no line search), restated for S independent problems stepped in lockstep.

    Every problem keeps its own state (iteration count, direction, step, curvature history, scale of the
    initial Hessian) in (S, ...) tensors; one ``step`` evaluates the closure of all problems with one
    fused kernel launch per inner iteration and applies, per problem, exactly the update rules and
    stopping tests of torch/optim/lbfgs.py (defaults: max_iter 20, tolerance_grad 1e-7, tolerance_change
    1e-9, history 100).  Problems that stop early simply stop changing.

    Everything is mask arithmetic -- no host synchronisation inside ``step``.  Two forms.  The kernel form (variables
    on the GPU, ``fused``): a step is the device trainer's sequence, closure then ONE optimiser launch per inner
    iteration (symode_lbfgs_step, a wavefront per problem: BEGIN -- optimality test, first iteration up to the move --
    then ACCEPT -- take the re-evaluated loss / gradient, stopping tests, next iteration: curvature memory in ring buffers
    with per-problem head / count, two-loop recursion, step length, move).  It is the launch of symode_trainer_update,
    which tests/trainer_model.py checks against fp64 (tests/test_gpu_trainer_steps.py ties the two bit for bit).  The
    tensor-op form is the same arithmetic statement by statement (CPU / gloo runs, ``SYMODE_LBFGS_FUSED=0``) with only
    the two-loop recursion as a kernel (symode_lbfgs_direction).

    Where the kernel form's bits differ from the tensor-op statement of a step's first iteration: with an L1 weight
    (``data_term``) the objective value sums |params| by the kernel's wave reduction, as every later iteration does,
    not by torch's sum (the gradient and the move are the same bits); and a ``frozen`` problem's ``_loss`` / ``_g``
    are left as they were instead of being refreshed (SeedSweepLBFGS reads neither).
    """

    def __init__(self, params, lr, max_iter=20, tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100, engine=None,
                 use_graph=False):
        self.P = params                                   # (S, n), updated in place
        S, n = params.shape
        self.lr, self.max_iter, self.tol_g, self.tol_c, self.H = lr, max_iter, tolerance_grad, tolerance_change, history_size
        dev, dt = params.device, params.dtype
        self.engine = engine if (engine is not None and params.is_cuda and n <= 256 and history_size <= 128) else None
        self.n_iter = torch.zeros(S, dtype=torch.long, device=dev)
        self.d = torch.zeros(S, n, device=dev, dtype=dt)
        self.t = torch.zeros(S, device=dev, dtype=dt)
        self.old_dirs = torch.zeros(S, history_size, n, device=dev, dtype=dt)
        self.old_stps = torch.zeros(S, history_size, n, device=dev, dtype=dt)
        self.ro = torch.zeros(S, history_size, device=dev, dtype=dt)
        self.head = torch.zeros(S, dtype=torch.long, device=dev)       # oldest stored pair
        self.hist = torch.zeros(S, dtype=torch.long, device=dev)       # number of stored pairs
        self.H_diag = torch.ones(S, device=dev, dtype=dt)
        self.prev_g = torch.zeros(S, n, device=dev, dtype=dt)
        self.prev_loss = torch.zeros(S, device=dev, dtype=dt)
        self._rows = torch.arange(S, device=dev)
        self._loss = torch.zeros(S, device=dev, dtype=dt)              # closure values / gradients / live flags of the running step
        self._g = torch.zeros(S, n, device=dev, dtype=dt)
        self._act = torch.zeros(S, dtype=torch.bool, device=dev)
        # HIP-graph replay of the inner iteration: GPU variables + the direction kernel (no host sync inside) only
        self.use_graph = bool(use_graph and params.is_cuda and self.engine is not None)
        # the kernel form: the whole optimiser side of an iteration as one launch (symode_lbfgs_step), a wave per problem
        self.data_term = None          # (closure of the bare data term, w_x, w_reg): objective = w_x * data + w_reg * |P|_1
        self.fused = bool(self.engine is not None and hasattr(self.engine, 'lbfgs_step') and dt == torch.float32
                          and params.is_contiguous() and os.environ.get('SYMODE_LBFGS_FUSED', '1') != '0')
        self._graph, self._graph_closure, self._warm = None, None, 0

    def reset(self, which):
        """Fresh optimiser for the selected problems (the reference re-creates LBFGS after thresholding).  In place:
        a captured iteration graph holds these buffers."""
        self.n_iter.masked_fill_(which, 0)
        self.hist.masked_fill_(which, 0)
        self.head.masked_fill_(which, 0)
        self.H_diag.masked_fill_(which, 1.0)

    def _direction(self, g):
        if self.engine is not None:
            return self.engine.lbfgs_direction(g, self.old_dirs, self.old_stps, self.ro, self.head, self.hist, self.H_diag)
        S = g.shape[0]
        num_old = int(self.hist.max().item())
        q = -g
        al = torch.zeros(S, max(num_old, 1), device=g.device, dtype=g.dtype)
        for k in range(num_old - 1, -1, -1):                               # logical slot k of every problem
            live = (k < self.hist).to(g.dtype)
            slot = (self.head + k) % self.H
            a = (self.old_stps[self._rows, slot] * q).sum(1) * self.ro[self._rows, slot] * live
            al[:, k] = a
            q = q - a[:, None] * self.old_dirs[self._rows, slot]
        r = q * self.H_diag[:, None]
        for k in range(num_old):
            live = (k < self.hist).to(g.dtype)
            slot = (self.head + k) % self.H
            be = (self.old_dirs[self._rows, slot] * r).sum(1) * self.ro[self._rows, slot] * live
            r = r + self.old_stps[self._rows, slot] * ((al[:, k] - be) * live)[:, None]
        return r

    def _iteration(self, closure, evaluate=True):
        """One inner iteration of every problem in tensor ops on the persistent buffers (self.P, _loss, _g, _act and the
        optimiser state): everything is updated in place, so the sequence of launches can be captured once and replayed."""
        P, g, loss, act = self.P, self._g, self._loss, self._act
        self.n_iter.add_(act.long())
        first = act & (self.n_iter == 1)
        upd = act & ~first
        # ---- curvature memory (torch: "do lbfgs update (update memory)") -------------------
        self.hist.masked_fill_(first, 0)
        self.head.masked_fill_(first, 0)
        self.H_diag.masked_fill_(first, 1.0)
        y = g - self.prev_g
        s = self.d * self.t[:, None]
        ys = (y * s).sum(1)
        mem = upd & (ys > 1e-10)
        full = mem & (self.hist == self.H)
        pos = torch.where(full, self.head, (self.head + self.hist) % self.H)      # overwrite the oldest when full
        m3 = mem[:, None]
        self.old_dirs[self._rows, pos] = torch.where(m3, y, self.old_dirs[self._rows, pos])
        self.old_stps[self._rows, pos] = torch.where(m3, s, self.old_stps[self._rows, pos])
        safe_ys = torch.where(mem, ys, torch.ones_like(ys))
        self.ro[self._rows, pos] = torch.where(mem, 1.0 / safe_ys, self.ro[self._rows, pos])
        self.head.copy_(torch.where(full, (self.head + 1) % self.H, self.head))
        self.hist.copy_(torch.where(mem & ~full, self.hist + 1, self.hist))
        yy = (y * y).sum(1)
        self.H_diag.copy_(torch.where(mem, ys / torch.where(mem, yy, torch.ones_like(yy)), self.H_diag))
        # ---- direction: empty history gives d = -g, as torch's first iteration -----------------
        d_new = self._direction(g)
        self.d.copy_(torch.where(act[:, None], d_new, self.d))
        self.prev_g.copy_(torch.where(act[:, None], g, self.prev_g))
        self.prev_loss.copy_(torch.where(act, loss, self.prev_loss))
        # ---- step length ---------------------------------------------------------------------
        t_first = torch.clamp(1.0 / g.abs().sum(1), max=1.0) * self.lr
        t_new = torch.where(self.n_iter == 1, t_first, torch.full_like(t_first, self.lr))
        self.t.copy_(torch.where(act, t_new, self.t))
        gtd = (g * self.d).sum(1)
        live = act & ~(gtd > -self.tol_c)                                  # directional derivative below tolerance
        P.add_(torch.where(live, self.t, torch.zeros_like(self.t))[:, None] * self.d)
        if evaluate:                                                       # (no re-evaluation on the last iteration)
            nl, ng = closure(P)
            loss.copy_(torch.where(live, nl, loss))
            g.copy_(torch.where(live[:, None], ng, g))
            stop = (g.abs().amax(1) <= self.tol_g) | ((self.d * self.t[:, None]).abs().amax(1) <= self.tol_c) \
                | ((loss - self.prev_loss).abs() < self.tol_c)
            live = live & ~stop
        act.copy_(live)

    def _evaluate_step(self, closure, mode=LBFGS_ACCEPT, frozen=None):
        """The kernel form's iteration: closure at the current parameters (the bare data term when ``data_term`` is set:
        scale and L1 term are formed by the launch), then ONE optimiser launch -- BEGIN opens the step, ACCEPT finishes
        the running iteration and starts the next one for the problems still active."""
        if self.data_term is not None:
            raw, w_x, w_reg = self.data_term
            nl, ng = raw(self.P)
            l1 = (w_x, w_reg)
        else:
            nl, ng = closure(self.P)
            l1 = None
        self.engine.lbfgs_step(mode, nl, ng, self.P, self._g, self._loss, self._act, self, self.lr, self.tol_g, self.tol_c, l1=l1,
                               frozen=frozen)

    def _replayed(self, body, closure):
        """``body(closure)`` is a handful of launches on persistent buffers: after a few eager runs (lazy initialisations
        done) it is captured ONCE in a HIP graph and replayed -- same kernels, same buffers."""
        if self._graph is None or self._graph_closure is not closure:
            if self._warm < 3 or (self._graph is not None and self._graph_closure is not closure):
                self._warm += 1
                return body(closure)
            try:
                torch.cuda.synchronize(self.P.device)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    body(closure)
                self._graph, self._graph_closure = graph, closure
            except Exception:                                              # pragma: no cover - depends on the runtime
                self.use_graph = False
                return body(closure)
        self._graph.replay()

    @torch.no_grad()
    def step(self, closure, frozen=None):
        """closure(P) -> (loss (S,), grad (S, n)).  ``frozen`` (S,) bool: problems that must not move.  Returns the
        objective (S,) at the last evaluation of each problem; in the kernel form a frozen problem's entry is the value
        from before it froze (0 if it never took a step), in the tensor-op form the value at its resting parameters."""
        if self.fused:
            # (closure, BEGIN), then (closure, ACCEPT) max_iter - 1 times -- symode_trainer_run's sequence: the last launch's
            # move is the one torch performs without re-evaluating (n_iter == max_iter)
            for it in range(self.max_iter):
                if it == 0:
                    self._evaluate_step(closure, LBFGS_BEGIN, frozen)
                elif self.use_graph:
                    self._replayed(self._evaluate_step, closure)
                else:
                    self._evaluate_step(closure)
                if it > 0 and it % 5 == 0 and not bool(self._act.any()):    # the only host sync, every 5th iteration
                    break
            return self._loss.clone()
        loss, g = closure(self.P)
        self._loss.copy_(loss)
        self._g.copy_(g)
        # optimality test in torch's sense (`if flat_grad.abs().max() <= tolerance_grad: return`): a NaN gradient does NOT
        # stop the step -- the parameters go to NaN and the trainer's NaN guard ends the run (train.py:697)
        act = ~(g.abs().amax(dim=1) <= self.tol_g)
        if frozen is not None:
            act = act & ~frozen
        self._act.copy_(act)
        for it in range(1, self.max_iter + 1):
            if it == self.max_iter:
                self._iteration(closure, False)
                break
            if self.use_graph:                                              # ~60 small launches around one closure kernel
                self._replayed(self._iteration, closure)
            else:
                self._iteration(closure, True)
            if it % 5 == 0 and not bool(self._act.any()):                   # the only host sync, every 5th iteration
                break
        return self._loss.clone()


class GramClosure:
    """The closure surface of batched.BatchedClosure (S, d, p, coef, xi_from, grads_to, evaluate) over prebuilt
    gram_closure.GramStatistics: the closure of a Gram-form sweep that never holds per-seed copies of the points.
    ``evaluate`` reads the statistics as they stand (summed over the ranks once the device trainer has all-reduced them)."""

    def __init__(self, statistics, Q=None, use_kron_product=True, allow_constant=True, w_sym=0.0, group=None, coef=None):
        self.statistics = statistics
        self.engine = statistics.engine
        self.S, self.d, self.p = statistics.S, statistics.d, statistics.p
        self.order, self.flags = statistics.order, statistics.flags
        self.coef = coef if coef is not None else CoefMap(self.d, self.p, Q, use_kron_product, allow_constant)
        self.w_sym = float(w_sym)
        self.group = group
        self.distributed = group is not None

    def xi_from(self, beta, const=None):
        return self.coef.xi(beta, const)

    def grads_to(self, grad_xi):
        return self.coef.grad(grad_xi)

    def evaluate(self, beta, const=None, mask=None):
        """(loss (S,) = mse [+ w_sym * regulariser], d/dbeta [or d/dXi], d/dconst), as BatchedClosure.evaluate."""
        Xi = self.xi_from(beta, const)
        loss, grad, _ = self.statistics.evaluate(Xi, mask, self.w_sym)
        g_beta, g_const = self.grads_to(grad)
        return loss, g_beta, g_const


class SeedSweepLBFGS:
    """``train_SIGED_lbfgs`` (non-latent, MSE [+ L1]) for S seeds in lockstep: the per-epoch logic of
    train.py:692-725 -- NaN guard, update-norm convergence test, threshold + optimiser reset, final
    convergence -- evaluated per problem on (S, ...) tensors; the closure of all seeds is ONE launch of the
    fused Theta + residual + gradient kernel (BatchedClosure), all-reduced over point shards if sharded."""

    def __init__(self, closure, lr_sindy, threshold, st_freq, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=0.0, tol=1e-3,
                 gram_closure=False, statistics=None):
        """``gram_closure``: the device trainer evaluates every closure as the quadratic form of the seeds' fp64 Gram
        matrices (gram_closure.py), built once from the closure's data (and summed over the point shards in one
        all-reduce) instead of streaming the points per evaluation.  ``statistics``: a prebuilt GramStatistics of this
        rank's points (e.g. from ``add_gathered``), all-reduced by the trainer; implies the Gram closure, and ``closure``
        then only supplies the coefficient plumbing (a GramClosure, which holds no points)."""
        self.c = closure
        self.coef = getattr(closure, 'coef', None) or CoefMap(closure.d, closure.p, closure.Q, getattr(closure, 'use_kron', True),
                                                              getattr(closure, 'allow_constant', True))   # (a duck-typed closure)
        self.statistics = statistics
        self.gram_closure = bool(gram_closure) or statistics is not None
        self.lr, self.threshold, self.st_freq, self.tol = lr_sindy, threshold, st_freq, tol
        self.w_x, self.reg_type, self.w_reg = w_sindy_x, sindy_reg_type, w_sindy_reg
        if sindy_reg_type not in ("l1", "none"):
            raise ValueError(f"Unknown regularization type: {sindy_reg_type}")

    def _data_term(self, P, alias=True):
        """loss, gradient of the bare MSE (+ regulariser the closure carries) w.r.t. the flat parameters.  ``alias``:
        the results may be views of the closure's output buffer (they are consumed before the next evaluation)."""
        a, b = self.coef.split(P)
        loss, ga, gb = self.c.evaluate(a.contiguous(), b, mask=self.mask, **({'alias': True} if alias and self._can_alias else {}))
        return loss, self.coef.join(ga, gb)

    def _closure(self, P):
        loss, g = self._data_term(P, alias=False)
        if self.w_x != 1.0:
            loss, g = self.w_x * loss, self.w_x * g
        if self.reg_type == "l1" and self.w_reg != 0.0:                     # over the raw parameters (train.py:681)
            loss = loss + self.w_reg * P.abs().sum(1)
            g = g + self.w_reg * torch.sign(P)
        return loss, g

    def _xi(self, P):
        a, b = self.coef.split(P)
        return self.c.xi_from(a.contiguous(), b)

    def _native_ok(self, P0):
        """The device-resident trainer (device_lbfgs.DeviceTrainer: optimiser AND epoch logic as kernels of the library, no
        stock torch op between the epochs) serves every GPU fit; the tensor-op form below is its restatement for CPU /
        gloo test doubles and ``SYMODE_LBFGS_FUSED=0``."""
        c = self.c
        eng = getattr(c, 'engine', None)
        if self.statistics is not None:
            return bool(P0.is_cuda and P0.shape[1] <= 256 and c.d * c.p <= 256)
        return bool(P0.is_cuda and eng is not None and hasattr(getattr(eng, 'lib', None), 'symode_trainer_run')
                    and os.environ.get('SYMODE_LBFGS_FUSED', '1') == '1'
                    and P0.shape[1] <= 256 and c.d * c.p <= 256 and getattr(c, 'n_chunks', 1) == 1)

    def _fit_native(self, P0, num_epochs, mask0, on_epoch, hyper=None):
        from .device_lbfgs import DeviceTrainer
        c = self.c
        stats, rev = None, c.sym if self.statistics is None else None
        if self.statistics is not None:
            stats = self.statistics
            if stats.regulariser:
                rev = (None, None, c.w_sym)
        elif self.gram_closure:
            from .gram_closure import GramStatistics
            stats = GramStatistics(c.S, c.d, c.order, c.flags, regulariser=c.sym is not None, device=c.x.device, engine=c.engine)
            stats.add(c.x, c.dx, *(c.sym[:2] if c.sym is not None else ()))
        x, dx = (None, None) if stats is not None else (c.x, c.dx)          # the Gram form holds no reference to the points
        tr = DeviceTrainer(x, dx, c.order, c.flags, coef=self.coef, reversed_sym=rev, lr=self.lr, threshold=self.threshold,
                           st_freq=self.st_freq, w_x=self.w_x,
                           w_reg=self.w_reg if self.reg_type == 'l1' else 0.0, l1=True, tol=self.tol,
                           inv_count=None if self.statistics is not None else c.inv_count,
                           engine=c.engine, group=(c.group or dist.group.WORLD) if c.distributed else None,
                           detail=on_epoch is not None and c.S <= 64, closure='stream' if stats is None else 'gram',
                           statistics=stats, hyper=hyper)
        self.trainer = tr
        cb = None
        if on_epoch is not None:
            dev = P0.device

            def cb(epoch, rec):                              # the tensor-op form's callback signature
                done = torch.from_numpy((rec['code'] == 3) | (rec['code'] == 4) | (rec['code'] == -1))
                return on_epoch(epoch, tr.field('params'), tr.field('mask').view(tr.S, c.d, c.p), done.to(dev))
        out = tr.fit(P0, num_epochs, mask0=mask0, on_epoch=cb)
        self.mask = out['mask'].to(P0.device)
        return {k: v.to(P0.device) for k, v in out.items()}

    @torch.no_grad()
    def fit(self, P0, num_epochs, mask0=None, on_epoch=None, hyper=None):
        """P0 (S, n): initial flat parameters per seed ([Xi] or [beta | const]).
        ``hyper``: the per-problem table of ``DeviceTrainer(hyper=...)`` (keys lr, w_reg, threshold, w_sym, one value per
        problem) -- a hyper-parameter grid on the seeds' shared Gram matrices: P0 then has one row per PROBLEM (a multiple
        of the closure's S seeds, problem s on seed s % S).  Gram form on the device trainer only.
        ``on_epoch(epoch, P, mask, done)`` (optional) is called after the epoch's logic with the live device tensors (a
        caller that reads them synchronises; returning True ends the fit) -- per-epoch logs / interval checkpoints.
        Returns dict(Xi, mask, params, epochs (S,), finished (S,), nan (S,))."""
        c = self.c
        if hyper is not None and not self.gram_closure:
            raise ValueError('hyper (a per-problem table) needs the Gram form (gram_closure=True or statistics): the streamed '
                             'closure reads one set of points per problem')
        if self._native_ok(P0):
            return self._fit_native(P0, num_epochs, mask0, on_epoch, hyper)
        if hyper is not None:
            raise ValueError('hyper (a per-problem table) needs the device trainer (a GPU closure of one chunk, d p <= 256, '
                             'SYMODE_LBFGS_FUSED=1): the tensor-op form takes one value each')
        if self.gram_closure:
            raise ValueError('gram_closure=True needs the device trainer (a GPU closure of one chunk, d p <= 256)')
        P = P0.clone().contiguous()
        S = P.shape[0]
        self.mask = torch.ones(S, c.d, c.p, device=P.device) if mask0 is None else mask0.clone()
        graph_ok = P.is_cuda and not getattr(c, 'distributed', False) and os.environ.get('SYMODE_SWEEP_GRAPH', '1') != '0'
        opt = BatchedLBFGS(P, self.lr, engine=getattr(c, 'engine', None) if P.is_cuda else None, use_graph=graph_ok)
        closure = self._closure                               # ONE bound-method object: the captured graph is tied to it
        self._can_alias = 'alias' in getattr(getattr(c.evaluate, '__code__', None), 'co_varnames', ())
        if opt.fused:
            opt.data_term = (self._data_term, self.w_x, self.w_reg if self.reg_type == "l1" else 0.0)
        prev, pprev = P.clone(), P.clone()
        n_iters = torch.zeros(S, dtype=torch.long, device=P.device)
        done = torch.zeros(S, dtype=torch.bool, device=P.device)
        nan = torch.zeros(S, dtype=torch.bool, device=P.device)
        epochs = torch.zeros(S, dtype=torch.long, device=P.device)
        near = torch.zeros(S, dtype=torch.long, device=P.device)         # near-threshold coefficients met per seed
        for epoch in range(num_epochs):
            if epoch % 4 == 0 and bool(done.all()):                        # host sync every 4th epoch only
                break
            live = ~done
            n_iters = n_iters + live.long()
            epochs = torch.where(live, torch.full_like(epochs, epoch + 1), epochs)
            opt.step(closure, frozen=done)
            bad = live & torch.isnan(P).any(dim=1)                         # train.py:697-699
            nan |= bad
            done |= bad
            live = ~done
            upd = self.coef.update_norm(P, prev)
            conv = live & (upd < self.tol)
            final = conv & (self.coef.update_norm(P, pprev) < self.tol)             # train.py:709-714
            done |= final
            thr_conv = conv & ~final
            thr_freq = (live & ~conv & (n_iters % self.st_freq == 0)) if self.st_freq > 0 else torch.zeros_like(done)
            ev = thr_conv | thr_freq
            Xi = self._xi(P)
            new_mask = torch.logical_and(Xi.abs() > self.threshold, self.mask > 0).float()
            close = ((Xi.abs() - self.threshold).abs() < NEAR_THRESHOLD_BAND) & (self.mask > 0)
            near = near + torch.where(ev, close.sum(dim=(1, 2)), torch.zeros_like(near))
            self.mask.copy_(torch.where(ev[:, None, None], new_mask, self.mask))   # strict >, monotone (sindy.py:194); in place:
            #                                                                       the captured iteration reads this buffer
            opt.reset(ev)
            n_iters = torch.where(ev, torch.zeros_like(n_iters), n_iters)
            pprev = torch.where(thr_conv[:, None], P, pprev)               # only on convergence-triggered events (:718)
            prev = torch.where((live & ~final)[:, None], P, prev)
            if on_epoch is not None and on_epoch(epoch, P, self.mask, done):
                break
        return {"Xi": self._xi(P), "mask": self.mask, "params": P, "epochs": epochs, "finished": done & ~nan, "nan": nan,
                "near_threshold": near}
