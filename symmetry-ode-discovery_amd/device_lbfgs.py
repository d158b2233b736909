"""``train_SIGED_lbfgs`` (reference train.py:617-766; its latent branch on precomputed operands) for S problems with the
optimiser AND the per-epoch logic resident on the GPU: the host enqueues whole epochs (``symode_trainer_run``: closure,
optimiser launch, ... , epoch-end launch -- 2 * max_iter + 1 launches, include/symode.h) and reads one small record per
epoch from pinned memory.  No stock torch GPU op runs between the first and the last epoch, so a one-seed process pays no
code-object loading beyond this library's own kernels.

The arithmetic is torch.optim.LBFGS's (no line search) statement by statement, as in ``sweep.BatchedLBFGS`` (the
tensor-op form of the same iteration, kept for CPU / gloo runs and as the test double of these kernels).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.distributed as dist

from .coef_map import CoefMap
from .engine import (CLOSURE_GRAM, CLOSURE_LATENT, CLOSURE_STREAM, LBFGS_ACCEPT, LBFGS_BEGIN, TRAINER_FIELDS, SymodeError, TrainerDesc,
                     TrainerGrid, get_engine)
from .gram_closure import GramStatistics

NEAR_THRESHOLD_BAND = 1e-4            # sindy.NEAR_THRESHOLD_BAND; repeated here to keep imports light

EVENT_NONE, EVENT_THRESHOLD_CONVERGED, EVENT_THRESHOLD_PERIOD, EVENT_FINAL, EVENT_NAN, EVENT_IDLE = 0, 1, 2, 3, 4, -1
HYPER_COLUMNS = ('lr', 'w_reg', 'threshold', 'w_sym')     # a row of the per-problem table (SYMODE_TRAINER_HYPER), by hyper's keys
MAX_PROBLEMS = 65535                                      # of one trainer (symode_trainer: n_problems)
_FIELD_DTYPES = {"act": torch.uint8, "n_iter": torch.int64, "head": torch.int64, "count": torch.int64, "n_iters": torch.int32,
                 "done": torch.uint8, "nan": torch.uint8, "finished": torch.uint8, "epochs": torch.int32, "near": torch.int32}


class DeviceTrainer:
    LOG_RING = 8                      # epochs of records kept; the host runs at most two epochs ahead of its reading

    def __init__(self, x, dx, poly_order, flags=0, Q=None, use_kron_product=True, allow_constant=True, reversed_sym=None,
                 lr=1.0, threshold=0.1, st_freq=0, w_x=1.0, w_reg=0.0, l1=True, tol=1e-3, max_iter=20, history=100,
                 tol_grad=1e-7, tol_change=1e-9, inv_count=None, engine=None, detail=None, group=None, closure="stream",
                 statistics=None, coef=None, latent=None, hyper=None):
        """x, dx (S, N_local, d) device tensors; ``coef``: the variables <-> Xi map (coef_map.CoefMap; default: built from
        Q / use_kron_product / allow_constant); ``reversed_sym = (gx (S, n_g, N, d), jgx (S, n_g, N, d, d), weight)`` as
        batched.BatchedClosure; ``group``: point shards, [loss | grad] summed over the ranks between closure and update;
        ``detail``: keep coefficients and mask of every epoch in the record (default: for S <= 64).
        ``closure="gram"``: every closure is the quadratic form of the fixed fp64 matrices [G | R] (gram_closure.py), built
        here in one pass over x, dx (, gx, jgx) -- or taken from ``statistics``, a GramStatistics of this rank's points, when
        x, dx, gx, jgx may be None -- and, with ``group``, summed over the ranks in ONE all-reduce at set-up; the fit then
        runs without any collective and holds no reference to the point data.
        ``closure="latent"``: the latent fit (train.py:647-661) on the operands of ``model_utils.latent_operands``: x := z,
        dx := dz, ``latent = (B (S, N, d, d), y (S, N, d), w_pair)``, w_x := w_sindy_z; every closure is one
        symode_loss_grad_latent launch (mse = loss_sindy_z, sym = mean |B h - y|^2).  The x-term enters the loss VALUE with
        w_pair and the GRADIENT not at all, as in the reference (SYMODE_CLOSURE_LATENT, include/symode.h).  One rank, streamed
        points only: ``group`` and ``statistics`` are refused.
        ``hyper`` (with ``closure="gram"``): a dict with any of the keys ``lr``, ``w_reg``, ``threshold``, ``w_sym`` (the last
        with the regulariser's matrices only), each one value per PROBLEM -- a hyper-parameter grid on shared matrices
        (symode_trainer_grid): the trainer has as many problems as the columns have rows, a multiple of the statistics' S
        sets, problem s fits on set s % S at row s's values, bit for bit the scalar trainer on that set alone; missing
        columns are filled from the scalar arguments.  Without ``hyper``: the scalar descriptor and entries, as ever."""
        self.engine = engine or get_engine()
        kinds = {"stream": CLOSURE_STREAM, "gram": CLOSURE_GRAM, "latent": CLOSURE_LATENT}
        if closure not in kinds:
            raise SymodeError(f"closure must be 'stream', 'gram' or 'latent', got {closure!r}")
        self.kind = kinds[closure]
        self.gram, self.latent = self.kind == CLOSURE_GRAM, self.kind == CLOSURE_LATENT
        self.order, self.flags = int(poly_order), int(flags)
        # --- the closure kind and its operands: the only per-kind part of the set-up (with _descriptor's branch)
        self.stats = self.sym = self.latent_ops = self.x = self.dx = self.hyper = None
        self.pair = self.latent or reversed_sym is not None
        self.w_sym = float(reversed_sym[2]) if reversed_sym is not None else 0.0
        if self.latent:
            B, y, self.w_sym = self._latent_operands(x, latent, reversed_sym, group, statistics, w_x)
            self.latent_ops = (B.contiguous(), y.contiguous())
        elif latent is not None:
            raise SymodeError("latent operands are for closure='latent'")
        if self.gram:
            self.stats = self._gram_statistics(x, dx, reversed_sym, statistics, group)
            self.S, self.d, dev = self.stats.S, self.stats.d, self.stats.device
            if hyper is not None:                             # the grid: more problems than sets of matrices
                self.hyper = self._hyper_table(hyper, (lr, w_reg, threshold, self.w_sym), dev)
                self.S = self.hyper.shape[0]
            self.n_points = self.stats.count
            if inv_count is None:
                inv_count = self.stats.inv_count()
            group = None                                      # the fit itself needs no collective
        else:
            if hyper is not None:
                raise SymodeError(f"hyper (a per-problem table) is for closure='gram', got closure={closure!r}: the streamed and "
                                  "latent closures read one set of points per problem")
            if statistics is not None:
                raise SymodeError("statistics are for closure='gram'")
            if not (x.is_cuda and x.dim() == 3 and x.shape == dx.shape and x.dtype == torch.float32):
                raise SymodeError("DeviceTrainer expects x, dx as (S, N, d) fp32 device tensors; there is no CPU fallback")
            self.x, self.dx = x.contiguous(), dx.contiguous()
            self.S, self.n_points, self.d = x.shape
            dev = x.device
            if reversed_sym is not None:
                gx, jgx, weight = reversed_sym
                if gx.dim() != 4 or gx.shape[0] != self.S or tuple(gx.shape[2:]) != tuple(x.shape[1:]) or tuple(jgx.shape) != tuple(gx.shape) + (self.d,):
                    raise SymodeError("reversed_sym operands do not match x")
                self.sym = (gx.contiguous(), jgx.contiguous(), float(weight))
        self.device = dev
        self.p = self.engine.lib_size(self.d, self.order, self.flags)
        self.dp = self.d * self.p
        self.group = group
        world = dist.get_world_size(group) if group is not None else 1
        self.coef = coef if coef is not None else CoefMap(self.d, self.p, Q, use_kron_product, allow_constant)
        self.r, self.n = self.coef.r, self.coef.n_params
        self.q_eff = None
        if self.coef.Q is not None:
            if self.coef.Q.shape[0] != self.dp:
                raise SymodeError(f"Q has {self.coef.Q.shape[0]} rows, expected d*p = {self.dp}")
            self.q_eff = torch.from_numpy(self.coef.effective_Q()).to(dev)
        if self.n > 256 or self.dp > 256 or history > 128:
            raise SymodeError("DeviceTrainer handles at most 256 parameters / coefficients and 128 curvature pairs")
        self.detail = (self.S <= 64) if detail is None else bool(detail)
        self.distributed = group is not None
        # --- state block: ONE allocation, laid out by the library
        offs = (ctypes.c_size_t * len(TRAINER_FIELDS))()
        nbytes = self.engine.lib.symode_trainer_layout(self.S, self.n, self.dp, history, 1 if self.q_eff is not None else 0, offs)
        if nbytes == 0:
            raise SymodeError("symode_trainer_layout refused the problem sizes")
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._off = dict(zip(TRAINER_FIELDS, [int(o) for o in offs]))
        self._shape = {"params": (self.S, self.n), "xi": (self.S, self.d, self.p), "mask": (self.S, self.d, self.p),
                       "cl_loss": (self.S, 2), "cl_grad": (self.S, self.dp), "g": (self.S, self.n), "loss": (self.S,),
                       "d": (self.S, self.n), "prev_g": (self.S, self.n), "prev": (self.S, self.n), "pprev": (self.S, self.n),
                       "old_dirs": (self.S, int(history), self.n), "old_stps": (self.S, int(history), self.n),
                       "ro": (self.S, int(history)), "test_grad": (self.S, self.dp)}   # every other array: (S,)
        # --- per-epoch records: pinned host memory the kernels write directly (sharded runs: device memory, copied)
        R = self.LOG_RING
        mk = (lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)) if self.distributed else \
             (lambda *s: torch.zeros(*s, dtype=torch.float32).pin_memory())
        self.log = mk(R, self.S, 8)
        self.log_test = mk(R, self.S, 2)
        self.log_xi = mk(R, self.S, self.dp) if self.detail else None
        self.log_mask = mk(R, self.S, self.dp) if self.detail else None
        self.log_params = mk(R, self.S, self.n) if self.detail else None
        n_global = self.n_points * world
        if group is not None and inv_count is None:          # shards need not be equal: the count is summed once, at set-up
            cnt = torch.tensor([float(self.n_points)], dtype=torch.float64, device=dev)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
            n_global = int(cnt.item())
        self.T = self._descriptor(float(inv_count) if inv_count is not None else 1.0 / (n_global * self.d), w_x, w_reg, l1, lr,
                                  tol_grad, tol_change, max_iter, history, threshold, tol, st_freq)
        self._Tp = ctypes.byref(self.T)
        # --- the epochs' entry and what it is called with: the grid's takes the descriptor that wraps T and carries the table
        # (a Gram fit has no collective inside, so the grid never meets _epoch_sharded)
        self._run_fn, self._Gp = self.engine.lib.symode_trainer_run, self._Tp
        if self.hyper is not None:
            self.G = TrainerGrid(self.T, self.hyper.data_ptr(), self.stats.S)
            self.T = self.G.base                              # (ctypes copied it: this is the one the launches read)
            self._Tp, self._Gp = ctypes.byref(self.G.base), ctypes.byref(self.G)
            self._run_fn = self.engine.lib.symode_trainer_grid_run
        self.max_iter = int(max_iter)
        self.threshold = float(threshold)

    def _descriptor(self, inv_count, w_x, w_reg, l1, lr, tol_grad, tol_change, max_iter, history, threshold, tol, st_freq):
        """The symode_trainer of this fit: the closure kind with the operands it names (what it does not name stays NULL / 0),
        then what every kind shares.  The streamed kinds get their reduction scratch here."""
        T = TrainerDesc()
        T.closure, T.w_sym = self.kind, self.w_sym
        self.ws = None
        if self.gram:
            T.aug_gram = self.stats.G.data_ptr()
            T.rev_gram = self.stats.R.data_ptr() if self.pair else None
        else:
            T.x, T.dx = self.x.data_ptr(), self.dx.data_ptr()
            ws_bytes = self.engine.lib.symode_workspace_bytes(self.d, self.order, self.flags, self.S, self.n_points)
            self.ws = self.engine.new_workspace(self.device, ws_bytes)
            T.workspace, T.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * 8
            if self.latent:
                T.latent_B, T.latent_y = (t.data_ptr() for t in self.latent_ops)
            elif self.sym is not None:
                T.gx, T.jgx, T.n_g = self.sym[0].data_ptr(), self.sym[1].data_ptr(), self.sym[0].shape[1]
        T.n_problems, T.n_points, T.d, T.order, T.flags, T.inv_count = self.S, self.n_points, self.d, self.order, self.flags, inv_count
        T.q_eff = self.q_eff.data_ptr() if self.q_eff is not None else None
        T.r, T.allow_constant, T.n_params = self.r, int(self.coef.allow_constant), self.n
        T.w_x, T.w_reg, T.l1 = float(w_x), float(w_reg), int(bool(l1))
        T.lr, T.tol_grad, T.tol_change, T.max_iter, T.history = float(lr), float(tol_grad), float(tol_change), int(max_iter), int(history)
        T.threshold, T.tol_update, T.near_band, T.st_freq = float(threshold), float(tol), NEAR_THRESHOLD_BAND, int(st_freq)
        T.state, T.state_bytes = self.state.data_ptr(), self.state.numel()
        T.log, T.log_test = self.log.data_ptr(), self.log_test.data_ptr()
        if self.detail:
            T.log_xi, T.log_mask, T.log_params = self.log_xi.data_ptr(), self.log_mask.data_ptr(), self.log_params.data_ptr()
        T.log_epochs = self.LOG_RING
        return T

    # -- plumbing -----------------------------------------------------------------------------------------------------
    def _gram_statistics(self, x, dx, reversed_sym, statistics, group):
        """[G | R | count] of this rank's points, summed over ``group`` in one collective."""
        if statistics is None:
            if not (x is not None and x.is_cuda and x.dim() == 3 and x.shape == dx.shape and x.dtype == torch.float32):
                raise SymodeError("DeviceTrainer expects x, dx as (S, N, d) fp32 device tensors; there is no CPU fallback")
            statistics = GramStatistics(x.shape[0], x.shape[2], self.order, self.flags, regulariser=reversed_sym is not None,
                                        device=x.device, engine=self.engine)
            gx, jgx = (reversed_sym[0], reversed_sym[1]) if reversed_sym is not None else (None, None)
            statistics.add(x, dx, gx, jgx)
        elif (statistics.order, statistics.flags) != (self.order, self.flags) or statistics.regulariser != (reversed_sym is not None):
            raise SymodeError("statistics were built for another library or without / with the regulariser")
        if group is not None:
            statistics.all_reduce(group)
        return statistics

    def _hyper_table(self, hyper, scalars, dev):
        """The (n_problems, 4) fp32 device table [lr, w_reg, threshold, w_sym]: every given key one value per problem, every
        missing column the scalar argument."""
        if not isinstance(hyper, dict):
            raise SymodeError(f"hyper must be a dict with keys among {HYPER_COLUMNS}, got {type(hyper).__name__}")
        unknown = sorted(set(hyper) - set(HYPER_COLUMNS))
        if unknown:
            raise SymodeError(f"hyper has unknown keys {unknown}: the per-problem values are {HYPER_COLUMNS}")
        if not hyper:
            raise SymodeError(f"hyper is empty: give at least one of {HYPER_COLUMNS}, one value per problem")
        if 'w_sym' in hyper and not self.stats.regulariser:
            raise SymodeError("hyper w_sym needs the regulariser's matrices (statistics with R / reversed_sym): the plain closure has "
                              "no symmetry regulariser")
        cols = {name: torch.as_tensor(v).detach().to('cpu', torch.float32).reshape(-1) for name, v in hyper.items()}
        rows = {int(c.numel()) for c in cols.values()}
        if len(rows) != 1:
            raise SymodeError(f"hyper columns must hold one value per problem each, got lengths {sorted(rows)}")
        n = rows.pop()
        if n < 1 or n % self.stats.S != 0:
            raise SymodeError(f"hyper has {n} rows, not a multiple of the statistics' {self.stats.S} sets of matrices (problem s "
                              "fits on set s % S)")
        if n > MAX_PROBLEMS:
            raise SymodeError(f"hyper has {n} rows: one trainer takes at most {MAX_PROBLEMS} problems")
        table = torch.empty(n, len(HYPER_COLUMNS), dtype=torch.float32)
        for c, (name, scalar) in enumerate(zip(HYPER_COLUMNS, scalars)):
            table[:, c] = cols[name] if name in cols else float(scalar)
        return table.to(dev).contiguous()

    @staticmethod
    def _latent_operands(z, latent, reversed_sym, group, statistics, w_sindy_z):
        """What the latent kind refuses, and its operands (B, y, w_pair) once they match z."""
        if group is not None:
            raise SymodeError("closure='latent' does not take group=... (point shards): the multi-rank latent fit is not implemented")
        if statistics is not None:
            raise SymodeError("closure='latent' does not take statistics: there is no Gram form of the latent closure")
        if reversed_sym is not None:
            raise SymodeError("closure='latent' does not take reversed_sym: the latent fit has no symmetry regulariser")
        if not w_sindy_z > 0:
            raise SymodeError(f"closure='latent' needs w_sindy_z > 0 (w_x), got {w_sindy_z}: the x-term is weighed against it")
        if latent is None or len(latent) != 3:
            raise SymodeError("closure='latent' needs latent=(B, y, w_pair)")
        B, y, w_pair = latent
        ok = torch.is_tensor(z) and z.dim() == 3 and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in (B, y))
        if not ok or tuple(y.shape) != tuple(z.shape) or tuple(B.shape) != tuple(z.shape) + (z.shape[-1],):
            raise SymodeError("latent operands do not match z: B (S, N, d, d) and y (S, N, d) as fp32 device tensors")
        return B, y, float(w_pair)

    def _check(self, rc, what):
        if rc != 0:
            # a launch that failed half-way may have left tickets of the one-launch reductions behind: start them afresh
            if self.ws is not None:
                self.engine.lib.symode_workspace_init(self.ws.data_ptr(), self.ws.numel() * 8, self._st())
            self.engine._check(rc, what)

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def field(self, name):
        """A device view of one array of the state block."""
        dt = _FIELD_DTYPES.get(name, torch.float32)
        shape = self._shape.get(name, (self.S,))
        n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        off = self._off[name]
        return self.state[off:off + n].view(dt).view(*shape)

    def _record(self, slot):
        log = self.log[slot].cpu().numpy() if self.distributed else self.log[slot].numpy().copy()
        test = self.log_test[slot].cpu().numpy() if self.distributed else self.log_test[slot].numpy().copy()
        rec = {"code": log[:, 0].astype(np.int64), "mse": log[:, 1], "sym": log[:, 2], "l1": log[:, 3], "update_norm": log[:, 4],
               "update_norm_2": log[:, 5], "near": log[:, 6].astype(np.int64), "epoch": log[:, 7].astype(np.int64),
               "test": test[:, 0] if self.pair else test.reshape(-1)[:self.S], "xi": None, "mask": None, "params": None}
        if self.detail:
            get = (lambda a: a[slot].cpu().numpy()) if self.distributed else (lambda a: a[slot].numpy().copy())
            rec["xi"] = get(self.log_xi).reshape(self.S, self.d, self.p)
            rec["mask"] = get(self.log_mask).reshape(self.S, self.d, self.p)
            rec["params"] = get(self.log_params)
        return rec

    def _epoch_sharded(self, epoch, test_eval):
        """One epoch with the ranks' partial [loss | grad] summed between closure and update (RCCL / gloo)."""
        # mirrors symode_trainer_run (the one other statement of the epoch sequence) with a collective between closure and update
        lib, st = self.engine.lib, self._st()
        width = (2 if self.pair else 1) * self.S
        cl = self.state[self._off["cl_loss"]:self._off["cl_grad"] + self.S * self.dp * 4].view(torch.float32)
        # (cl_loss is (S, 2) floats with cl_grad right behind it; the plain closure fills the first S floats only)
        for it in range(self.max_iter):
            self._check(lib.symode_trainer_closure(self._Tp, None, None, st), "symode_trainer_closure")
            if width < 2 * self.S:
                dist.all_reduce(cl[:width], group=self.group)
                dist.all_reduce(cl[2 * self.S:], group=self.group)
            else:
                dist.all_reduce(cl, group=self.group)
            self._check(lib.symode_trainer_update(self._Tp, LBFGS_BEGIN if it == 0 else LBFGS_ACCEPT, st), "symode_trainer_update")
        self._check(lib.symode_trainer_epoch_end(self._Tp, epoch, st), "symode_trainer_epoch_end")
        if test_eval:
            slot = epoch % self.LOG_RING
            tg = self.field("test_grad")
            self._check(lib.symode_trainer_closure(self._Tp, ctypes.c_void_p(self.log_test[slot].data_ptr()),
                                                   ctypes.c_void_p(tg.data_ptr()), st), "symode_trainer_closure")
            dist.all_reduce(self.log_test[slot], group=self.group)

    # -- the fit --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def fit(self, P0, num_epochs, mask0=None, on_epoch=None, test_eval=False):
        """P0 (S, n) start parameters ([Xi] or [beta | const]), host or device.  ``on_epoch(epoch, record)`` is called once
        per epoch, in order, with the epoch's record (numpy arrays over the problems: code, mse, sym, l1, update_norm,
        near, test, and with ``detail`` xi / mask after the epoch's events); returning True ends the fit.
        Returns dict(Xi, mask, params, epochs, finished, nan, near_threshold) of host tensors."""
        lib, dev = self.engine.lib, self.device
        P0 = P0.detach().to(torch.float32).contiguous()
        if tuple(P0.shape) != (self.S, self.n):
            raise SymodeError(f"P0 must be ({self.S}, {self.n}), got {tuple(P0.shape)}")
        m0 = None
        if mask0 is not None:
            m0 = mask0.detach().to(torch.float32).contiguous()
            if m0.numel() != self.S * self.dp:
                raise SymodeError("mask0 does not match the coefficient shape")
        stream = torch.cuda.current_stream(dev)
        self._check(lib.symode_trainer_init(self._Tp, ctypes.c_void_p(P0.data_ptr()),
                                            None if m0 is None else ctypes.c_void_p(m0.data_ptr()), self._st()),
                    "symode_trainer_init")
        if not P0.is_cuda or (m0 is not None and not m0.is_cuda):
            stream.synchronize()                            # pageable host sources: the copies must finish before they go away
        done = np.zeros(self.S, dtype=bool)

        def enqueue(e):
            if self.distributed:
                self._epoch_sharded(e, test_eval)
            else:
                self._check(self._run_fn(self._Gp, e, 1, 1 if test_eval else 0, self._st()), "symode_trainer_run")
            ev = torch.cuda.Event()
            ev.record(stream)
            return ev

        pending = [enqueue(0)] if num_epochs > 0 else []
        for e in range(num_epochs):
            if e + 1 < num_epochs:
                pending.append(enqueue(e + 1))              # the next epoch is in flight while this one's record is read
            pending.pop(0).synchronize()
            rec = self._record(e % self.LOG_RING)
            stop = bool(on_epoch(e, rec)) if on_epoch is not None else False
            done |= (rec["code"] == EVENT_FINAL) | (rec["code"] == EVENT_NAN) | (rec["code"] == EVENT_IDLE)
            if stop or done.all():
                break
        stream.synchronize()
        out = {k: self.field(k).cpu() for k in ("params", "xi", "mask", "epochs", "finished", "nan", "near")}
        return {"Xi": out["xi"].reshape(self.S, self.d, self.p), "mask": out["mask"].reshape(self.S, self.d, self.p),
                "params": out["params"], "epochs": out["epochs"].long(), "finished": out["finished"].bool(),
                "nan": out["nan"].bool(), "near_threshold": out["near"].long()}
