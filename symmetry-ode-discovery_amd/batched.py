"""Batched / sharded evaluation of the SINDy closure over independent (trajectory, seed) problems.

One process per GPU.  Every rank keeps, resident in HBM, its shard of the points of each of S
problems: x, dx (S, N_local, d).  One call evaluates loss and gradient of all S problems with
the fused Theta + residual + gradient kernel and, when a process group is given, sums the
per-rank partials with ONE all-reduce per chunk of problems (RCCL over xGMI when the backend
is "nccl"); chunks are pipelined so the collective of chunk c overlaps the kernel of chunk
c+1.  The message is S*(1 + d*p) floats -- latency-bound, hence few, fused collectives.

The reference runs one process per seed and has no distributed code (run_scripts/*.sh loop
over seeds); this is the new design SURVEY section 8(e) calls point-sharding.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .coef_map import CoefMap
from .engine import STEP_SLOW, STEP_STALE, get_engine, library_flags, step_key


def allreduce_sums(sums, params, group):
    """Point-sharded scalar sums and their parameter gradients through ONE collective.

    ``sums``: scalar tensors, each a sum over THIS rank's points (with or without an autograd graph); ``params``: the
    leaf tensors they are differentiated by.  Every sum is differentiated locally, the values and gradients of all of
    them travel in one packed fp64 buffer (n * (1 + |params|) numbers -- a few hundred bytes) through one all-reduce,
    and what comes back is, per sum, a scalar tensor whose VALUE is the global sum and whose first derivative with
    respect to ``params`` is the global gradient (value + g . (p - p.detach())).  Whatever the caller builds from them
    -- a mean, a ratio of two batch means (the relative regularisers, model_utils.py:62, 118-121: numerator and
    denominator must be summed over the ranks SEPARATELY before the division) -- autograd differentiates on that
    handful of scalars: the quotient rule is applied after the collective, on global numbers, on every rank alike."""
    params = list(params)
    sizes = [p.numel() for p in params]
    P = sum(sizes)
    dev = sums[0].device
    buf = torch.zeros(len(sums), 1 + P, dtype=torch.float64, device=dev)
    for i, s in enumerate(sums):
        buf[i, 0] = s.detach()
        if s.requires_grad:
            gs = torch.autograd.grad(s, params, retain_graph=True, allow_unused=True)
            o = 1
            for g, n in zip(gs, sizes):
                if g is not None:
                    buf[i, o:o + n] = g.reshape(-1)
                o += n
    if group is not None:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    out = []
    for i in range(len(sums)):
        v = buf[i, 0].to(sums[i].dtype)
        o = 1
        for p, n in zip(params, sizes):
            g = buf[i, o:o + n].to(p.dtype).view_as(p)
            v = v + (g * (p - p.detach())).sum()
            o += n
        out.append(v)
    return out


class BatchedClosure:
    def __init__(self, x, dx, poly_order, include_sine=False, include_exp=False, Q=None, use_kron_product=True,
                 allow_constant=True, group=None, world_size=None, n_chunks=1, engine=None, reversed_sym=None, fuse_sym=True, coef=None,
                 const_jacobian=None, live_columns=True, linear_action=None, regulariser_gram=None, residual_gram=None, reduced=None):
        """``coef``: the variables <-> Xi map (coef_map.CoefMap; default: built from Q / use_kron_product / allow_constant).
        ``reversed_sym = (gx (S, n_g, N_local, d), jgx (S, n_g, N_local, d, d), weight)`` adds  weight * the reversed
        symmetry regulariser (model_utils.py:126-170 on precomputed (g(x), J_g(x))) to every problem's loss and gradient:
        by default residual and regulariser run as ONE launch per chunk (symode_loss_grad_reversed: Theta(x) shared, x read
        once); ``fuse_sym=False`` keeps them as two launches summed into the same packed buffer before the collective.
        ``const_jacobian``: None (default) -- one detection pass over jgx at set-up (engine.jacobian_constant) asks whether
        J_g is the same matrix at every point of each (problem, group element), as it is for a linear or affine action or a
        frozen linear autoencoder; if so the closures get the compact (S, n_g, d, d) table and stream nothing of J_g
        (bit-identical results); False -- always the materialised (S, n_g, N, d, d) form (A/B, tests).
        The verdict is remembered with jgx's in-place version counter and data pointer and the pass runs again when either
        differs at the next evaluation.  What that cannot see: jgx refilled through a raw pointer or another view of its
        storage made outside torch's version tracking (a foreign kernel writing into it) -- rebuild the closure then.
        ``live_columns``: True (default) -- ``evaluate``, where Xi is known to come from the map, tells the compact-table
        closures which library columns the map can fill (``CoefMap.live_mask``, read once here): the columns the
        constraint keeps at zero up to the round-off of Q count as exactly zero and cost nothing per point where the
        library has a kernel for the set; False -- the dense launch (A/B, tests).  ``loss_grad_xi`` called directly is
        dense unless it is given a set.
        ``linear_action``: None (default) -- where the constant-J verdict is yes (d = 2 plain polynomial library, one group
        element, fused launch), a second pass (engine.linear_action) asks whether g(x) is the linear image J x of x to within
        4 * 2^-24 per component; if so the fused closure takes the kernel that folds the action into the coefficients: it reads
        x and dx alone and evaluates the library once per point.  Same closure up to rounding, NOT bit for bit (g(x) is
        replaced by J x); SYMODE_CLOSURE_FOLD=0 or False keep the streamed kernels.  The verdict is remembered with the
        version counters and data pointers of x and gx, as jgx's is.
        ``regulariser_gram``: None (default) -- where the linear verdict is yes, the library Gram G = sum_n Theta Theta^T of this
        rank's shard of every problem is built once (engine.aug_gram, its top-left p x p block) and handed to the fold closure:
        the regulariser and its gradient become a d p p fp64 product per problem and the point loop carries the residual alone
        (engine.loss_grad_reversed, ``gram=``).  The term is linear in G, so the [loss | grad] all-reduce stays what it is.
        The matrix is remembered with the version counters and data pointers of x and dx and rebuilt when any of them moves
        (``gram_builds`` counts); SYMODE_FOLD_GRAM=0 or False keep the plain fold kernel.
        ``residual_gram``: None (default) -- with ``regulariser_gram``, the WHOLE augmented matrix [Theta | dx]^T [Theta | dx] is
        kept and the closure has no point loop at all (engine.loss_grad_reversed, ``aug=``): the residual is the quadratic form
        of the rows and columns the regulariser leaves out, a call reads 8 KB per problem instead of x and dx, and the one
        pass over the points is the set-up's.  ``evaluate`` on one chunk without point shards hands the launch the coefficient
        map as well (``coef=``): Xi from (beta, const) and the gradient by them come out of the same kernel.  Linear in the
        matrix like the regulariser, so the all-reduce stays what it is.  SYMODE_FOLD_RESID_GRAM=0 or False give the step
        with the point loop, bit for bit.
        ``reduced``: None (default) -- where ``evaluate`` takes that one-launch step and is called without a mask, the closure
        is reduced once to its quadratic form in the variables, loss = v^T B v with v = [beta; const; 1] and B (K+1, K+1) fp64
        per problem, K = r + d (engine.quad_reduce), and a step reads B alone (engine.quad_step_plan: one allocation, one
        call).  Taken when K + 1 <= 16 and (K+1)^2 < (p+d)^2 + p^2, i.e. when B is the smaller table.  The form is exact for
        the fp64 closure; it differs from the one-launch step, which rounds Xi to fp32 once, by less than one fp32 rounding of
        the outputs.  B is remembered with the version counters and data pointers of x, dx, gx, jgx and Q, the weight and
        the column set, and built again when any of them moves (``reduced_builds`` counts).  On this route the loss pair and
        the gradient by Xi are not formed: ``sym_buffers`` and ``buffers[0][n:]`` keep what the last other launch left there.
        A call WITH a mask keeps the one-launch kernel: SeedSweepLBFGS mutates its mask in place, also inside a captured
        iteration, and a replayed graph runs no Python, so no version key could follow it.  A call made while the current
        stream is capturing builds nothing: without a valid B it takes the one-launch kernel.  SYMODE_QUAD_REDUCED=0 or False
        give the one-launch step, bit for bit."""
        assert x.dim() == 3 and x.shape == dx.shape, "x, dx must be (S, N_local, d)"
        self.engine = engine or get_engine()
        self.x, self.dx = x.contiguous(), dx.contiguous()
        self.S, self.n_local, self.d = x.shape
        self.order = poly_order
        self.flags = library_flags(include_sine, include_exp)
        self.p = self.engine.lib_size(self.d, poly_order, self.flags)
        self.coef = coef if coef is not None else CoefMap(self.d, self.p, Q, use_kron_product, allow_constant)
        self.group = group
        self.distributed = group is not None or (world_size or 1) > 1
        # world_size without a group and without a process group at all: the caller adds the shards' packed outputs itself
        self._collective = self.distributed and (group is not None or dist.is_initialized())
        self.world = world_size if world_size is not None else (dist.get_world_size(group) if self.distributed else 1)
        self.n_global = self.n_local * self.world
        if group is not None:                                # shards need not be equal: the count is summed once, at set-up
            cnt = torch.tensor([float(self.n_local)], dtype=torch.float64, device=x.device)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
            self.n_global = int(cnt.item())
        self.inv_count = 1.0 / (self.n_global * self.d)
        self.n_chunks = max(1, min(n_chunks, self.S))
        nacc = 1 + self.d * self.p
        # packed [loss | grad] per chunk so that one collective carries both
        bounds = torch.linspace(0, self.S, self.n_chunks + 1).long().tolist()
        self.chunks = [(a, b) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
        self.buffers = [torch.empty((b - a) * nacc, dtype=torch.float32, device=x.device) for a, b in self.chunks]
        # private scratch: a captured HIP graph (sweep.BatchedLBFGS) replays these launches from its own stream
        self._ws_kw = {}
        if x.is_cuda and hasattr(self.engine, 'new_workspace'):
            self._ws_kw = {'ws': self.engine.new_workspace(x.device, self.engine.lib.symode_workspace_bytes(
                self.d, poly_order, self.flags, max(b - a for a, b in self.chunks), self.n_local))}
        self.sym = None
        if reversed_sym is not None:
            gx, jgx, weight = reversed_sym
            assert gx.dim() == 4 and gx.shape[0] == self.S and gx.shape[2:] == x.shape[1:] and jgx.shape == gx.shape + (self.d,)
            self.sym = (gx.contiguous(), jgx.contiguous(), float(weight))
            self.sym_buffers = [torch.empty_like(b) for b in self.buffers]
        self.fuse_sym = fuse_sym
        self._cj_detect = (const_jacobian is None or bool(const_jacobian)) and self.sym is not None and x.is_cuda \
            and hasattr(self.engine, 'jacobian_constant')
        self._cj_seen, self._cj_table = None, None
        if self._cj_detect:
            self._jacobian_for_launch()
        self._lin_detect = linear_action is None or bool(linear_action)
        self._lin_detect = self._lin_detect and self._cj_detect and fuse_sym and self.d == 2 and self.flags == 0 \
            and 1 <= poly_order <= 5 and self.sym[0].shape[1] == 1 and hasattr(self.engine, 'linear_action')
        self._lin_seen, self._lin_m, self.linear_detections = None, None, 0
        if self._lin_detect:
            self._linear_for_launch()
        self._gram_on = (regulariser_gram is None or bool(regulariser_gram)) and self._lin_detect and hasattr(self.engine, 'aug_gram')
        self._gram_seen, self._gram, self._aug, self.gram_builds = None, None, None, 0
        self._resid_on = (residual_gram is None or bool(residual_gram)) and self._gram_on and hasattr(self.engine, 'closure_quad_enabled')
        if self._gram_on:
            self._gram_for_launch()
        self._alias_out = None                               # g_beta / g_const of an ``alias=True`` evaluation with the map in the launch
        self._live = None                                    # the map's column set, where it names a dead column at all
        if live_columns and self._cj_detect:
            live = self.coef.live_mask()
            self._live = None if live == 0xFFFFFFFFFFFFFFFF else live
        K = self.coef.r + (self.d if self.coef.allow_constant else 0)
        self._reduced_on = (reduced is None or bool(reduced)) and self._resid_on and self.coef.Q is not None and self.coef.r > 0 \
            and not self.distributed and len(self.chunks) == 1 and self.fuse_sym and hasattr(self.engine, 'quad_step_plan') \
            and K + 1 <= 16 and (K + 1) ** 2 < (self.p + self.d) ** 2 + self.p ** 2
        self._reduced_seen, self._reduced_step, self.reduced_builds = None, None, 0

    def _reduced_key(self):
        """What the reduced form was built from: the keys of ``_gram_for_launch`` and ``_linear_for_launch``, the weight, the
        column set and Q"""
        return step_key(*self._reduced_operands())

    def _reduced_operands(self):
        """The five arguments the key is read from, by ``step_key`` here and by the prepared step in every call"""
        return self.x, self.dx, self.sym, self.coef.Q, self._live

    def _reduced_for_launch(self):
        """The prepared step on the reduced form B of the closure ``evaluate`` would launch, built once per ``_reduced_key``
        (``reduced_builds`` counts); None where that closure is not the one without a point loop, where the library's
        switches refuse the form, and -- nothing is built inside a capture -- while the current stream is capturing."""
        self._reduced_seen, self._reduced_step = None, None
        if torch.cuda.is_current_stream_capturing():
            return None
        lin = self._linear_for_launch()
        aug = self._quad_for_launch() if lin is not None else None
        if aug is None or not self.engine.closure_reduced_enabled():
            return None
        key = self._reduced_key()
        B = self.engine.quad_reduce(aug, lin, self._cj_table, self.order, self.coef, self.sym[2], self.inv_count, self._live)
        self._reduced_step = self.engine.quad_step_plan(B, self.order, self._live, self.coef.r,
                                                        self.d if self.coef.allow_constant else 0, self._ws_kw['ws'],
                                                        key=self._reduced_operands())
        self._reduced_seen = key
        self.reduced_builds += 1
        return self._reduced_step

    def _reduced_off_the_straight_path(self, code, step, beta, const, alias):
        """What ``evaluate`` does with an answer of the prepared step that is neither its result nor None.  STEP_STALE: the
        form is built again and the step tried once more.  STEP_SLOW (the native plan alone): the operands go through the
        plan's ``ReducedStep``, which makes them dense or raises; with ``alias`` it writes the plan's buffers.  Any other number
        is an error code of the launch (``engine._check`` raises).  None: take the one-launch kernel."""
        door = self.engine.loss_grad_reversed
        if code == STEP_STALE:
            step = self._reduced_for_launch()
            if step is None:
                return None
            code = door(None, None, None, None, None, None, self.order, reduced=(step, beta, const, alias) + self._reduced_operands())
            if code is None or type(code) is tuple:
                return code
            if code == STEP_STALE:                           # a key that does not equal itself (a NaN weight)
                return None
        if code == STEP_SLOW:
            slow = step.slow
            if alias:
                slow._alias = step.alias_buffers()
            return door(None, None, None, None, None, None, self.order, reduced=(slow, beta, const, alias))
        self.engine._check(code, "symode_quad_step")

    def _jacobian_for_launch(self):
        """What the closures get as J_g: the compact table when the detection pass found every slab constant, else the
        materialised tensor.  The pass runs once per (version, pointer) of jgx."""
        jgx = self.sym[1]
        if not self._cj_detect:
            return jgx
        seen = (jgx._version, jgx.data_ptr())
        if seen != self._cj_seen:
            table, const = self.engine.jacobian_constant(jgx)
            self._cj_seen, self._cj_table = seen, (table if const else None)
        return jgx if self._cj_table is None else self._cj_table

    def _linear_for_launch(self):
        """The fp64 (S, 1, p, p) substitution matrices where g(x) = J x was detected (and J_g is a compact table), else None.
        The pass runs once per (version, pointer) of x, gx and jgx; ``linear_detections`` counts its runs."""
        if not self._lin_detect:
            return None
        table = self._jacobian_for_launch()
        if self._cj_table is None:
            return None
        gx = self.sym[0]
        seen = (self.x._version, self.x.data_ptr(), gx._version, gx.data_ptr(), self._cj_seen)
        if seen != self._lin_seen:
            m, linear = self.engine.linear_action(self.x, gx, table, self.order, self.flags)
            self._lin_seen, self._lin_m = seen, (m if linear else None)
            self.linear_detections += 1
        return self._lin_m

    def _gram_for_launch(self):
        """The fp64 (S, 1, p, p) raw library Gram sums of x where the fold closure is taken, else None; ``self._aug`` is the
        whole (S, p+d, p+d) augmented matrix they are the top-left block of.  Built once per (version, pointer) of x and dx;
        ``gram_builds`` counts."""
        if not self._gram_on or self._linear_for_launch() is None:
            return None
        seen = (self.x._version, self.x.data_ptr(), self.dx._version, self.dx.data_ptr())
        if seen != self._gram_seen:
            G = self.engine.aug_gram(self.x, self.dx, self.order, self.flags)
            self._gram_seen, self._aug, self._gram = seen, G, G[:, None, :self.p, :self.p].contiguous()
            self.gram_builds += 1
        return self._gram

    def _quad_for_launch(self):
        """The augmented matrices where the closure without a point loop is taken (``residual_gram``), else None."""
        if not self._resid_on or self._gram_for_launch() is None or not self.engine.closure_quad_enabled():
            return None
        return self._aug

    # -- coefficient plumbing (batched get_Xi, sindy.py:169-176) ----------------------------
    def xi_from(self, beta, const=None):
        return self.coef.xi(beta, const)

    def grads_to(self, grad_xi):
        return self.coef.grad(grad_xi)

    # -- the hot path -------------------------------------------------------------------------
    def loss_grad_xi(self, Xi, mask=None, alias=False, live_columns=None, coef=None):
        """loss (S,), dloss/dXi (S, d, p) summed over all ranks' shards.  ``alias=True``: with a single chunk the results
        are returned as views of the packed buffer the kernel wrote (no copies; overwritten by the next evaluation).
        ``live_columns``: the library columns Xi can be non-zero in (an int, bit k = column k), for the symmetry launches
        (engine.loss_grad_reversed); None: every column.
        ``coef`` = (beta, const) in the place of Xi (``evaluate``: one chunk, no point shards, the closure without a point
        loop): the launch forms Xi itself and the call returns (loss, g_beta, g_const) instead."""
        works = []
        live_kw = {} if live_columns is None else {'live_columns': live_columns}
        fused = self.sym is not None and self.fuse_sym and hasattr(self.engine, 'loss_grad_reversed')
        jg = self._jacobian_for_launch() if self.sym is not None else None      # (S, n_g, d, d) table or the (S, n_g, N, d, d) tensor
        lin = self._linear_for_launch() if fused else None                      # M of a detected linear action: the fold kernel
        gram = self._gram_for_launch() if lin is not None else None             # G of x: the fold kernel's Gram form
        aug = self._quad_for_launch() if gram is not None else None             # [Theta | dx]^T [Theta | dx]: no point loop
        if coef is not None:
            # ONE launch for the step: Xi from the variables, the closure, the gradient by the variables; what is returned is
            # written where it is returned from -- fresh tensors, or with ``alias`` buffers of this object
            (a, b), buf = self.chunks[0], self.buffers[0]
            n, dev = self.S, self.x.device
            beta, const = coef
            gx, jgx, weight = self.sym
            if alias:
                if self._alias_out is None:
                    self._alias_out = (torch.empty(n, self.coef.r, dtype=torch.float32, device=dev),
                                       torch.empty(n, self.d, 1, dtype=torch.float32, device=dev) if self.coef.allow_constant else None)
                loss, (g_beta, g_const) = buf[:n], self._alias_out
            else:
                loss = torch.empty(n, dtype=torch.float32, device=dev)
                g_beta = torch.empty(n, self.coef.r, dtype=torch.float32, device=dev)
                g_const = torch.empty(n, self.d, 1, dtype=torch.float32, device=dev) if self.coef.allow_constant else None
            self.engine.loss_grad_reversed(self.x, self.dx, gx, jg, None, mask, self.order, self.flags, w_sym=weight,
                                           inv_count=self.inv_count, out=(self.sym_buffers[0][:2 * n], buf[n:], loss), **live_kw,
                                           **self._ws_kw, linear_m=lin, aug=aug, coef=(self.coef, beta, const),
                                           coef_out=(None, g_beta, g_const))
            return loss, g_beta, g_const
        for ci, ((a, b), buf) in enumerate(zip(self.chunks, self.buffers)):
            n = b - a
            loss = buf[:n]
            grad = buf[n:].view(n, self.d, self.p)
            if fused:
                # ONE launch per chunk: residual and regulariser share Theta(x), x is read once; the kernel leaves
                # (mse, regulariser) per problem and the gradient of mse + weight * regulariser
                gx, jgx, weight = self.sym
                sb = self.sym_buffers[ci]
                l2 = sb[:2 * n].view(n, 2)
                if aug is not None:
                    # ... or reads no point at all, and leaves mse + weight * regulariser in the loss slot itself
                    self.engine.loss_grad_reversed(self.x[a:b], self.dx[a:b], gx[a:b], jg[a:b], Xi[a:b],
                                                   None if mask is None else mask[a:b], self.order, self.flags, w_sym=weight,
                                                   inv_count=self.inv_count, out=(l2, grad, loss), **live_kw, **self._ws_kw,
                                                   linear_m=lin[a:b], aug=aug[a:b])
                else:
                    self.engine.loss_grad_reversed(self.x[a:b], self.dx[a:b], gx[a:b], jg[a:b], Xi[a:b],
                                                   None if mask is None else mask[a:b], self.order, self.flags, w_sym=weight,
                                                   inv_count=self.inv_count, out=(l2, grad), **live_kw, **self._ws_kw,
                                                   **({} if lin is None else {'linear_m': lin[a:b]}),
                                                   **({} if gram is None else {'gram': gram[a:b]}))
                    torch.add(l2[:, 0], l2[:, 1], alpha=weight, out=loss)
                if self._collective:
                    works.append(dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                continue
            l, g = self.engine.loss_grad(self.x[a:b], self.dx[a:b], Xi[a:b], None if mask is None else mask[a:b],
                                         self.order, self.flags, inv_count=self.inv_count, out=(loss, grad), **self._ws_kw)
            if l.data_ptr() != loss.data_ptr():          # an engine that does not write in place
                loss.copy_(l)
                grad.copy_(g)
            if self.sym is not None:
                gx, jgx, weight = self.sym
                sb = self.sym_buffers[ci]
                sl, sg = sb[:n], sb[n:].view(n, self.d, self.p)
                l2, g2 = self.engine.symreg_reversed(self.x[a:b], gx[a:b], jg[a:b], Xi[a:b], None if mask is None else mask[a:b],
                                                     self.order, self.flags, out=(sl, sg), inv_count=self.inv_count, **live_kw,
                                                     **self._ws_kw)
                if l2.data_ptr() != sl.data_ptr():
                    sl.copy_(l2)
                    sg.copy_(g2)
                buf.add_(sb, alpha=weight)
            if self._collective:
                works.append(dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        for w in works:
            w.wait()
        if alias and len(self.chunks) == 1:
            n = self.S
            return self.buffers[0][:n], self.buffers[0][n:].view(n, self.d, self.p)
        loss = torch.cat([buf[:b - a] for (a, b), buf in zip(self.chunks, self.buffers)])
        grad = torch.cat([buf[b - a:].view(b - a, self.d, self.p) for (a, b), buf in zip(self.chunks, self.buffers)])
        return loss, grad

    def evaluate(self, beta, const=None, mask=None, alias=False):
        """Closure of all S problems: (loss (S,), d/dbeta [or d/dXi when unconstrained], d/dconst).
        Without a mask, where the constructor's ``reduced`` route holds, the call is the step on the reduced form: the three
        results are views of one packed buffer (fresh per call unless ``alias``), and the loss pair and d/dXi are not formed --
        ``sym_buffers`` and ``buffers[0][n:]`` keep their last contents.  A call with a mask, and a call under stream capture
        that finds no valid form, take the one-launch kernel."""
        if self._reduced_on and mask is None and (const is not None or not self.coef.allow_constant):
            # the step on the reduced form: one call through the engine's door; the prepared step (engine.quad_step_plan) compares
            # the key of the five operands named here, allocates, launches and returns the views
            step = self._reduced_step
            if step is None:
                step = self._reduced_for_launch()
            if step is not None:
                out = self.engine.loss_grad_reversed(None, None, None, None, None, None, self.order,
                                                     reduced=(step, beta, const, alias, self.x, self.dx, self.sym, self.coef.Q, self._live))
                if type(out) is tuple:
                    return out
                if out is not None:
                    out = self._reduced_off_the_straight_path(out, step, beta, const, alias)
                    if out is not None:
                        return out
        if self.coef.Q is not None and self.coef.r > 0 and not self.distributed and len(self.chunks) == 1 and self.sym is not None \
                and self.fuse_sym and self._resid_on and self._linear_for_launch() is not None and self._quad_for_launch() is not None:
            return self.loss_grad_xi(None, mask, alias=alias, live_columns=self._live, coef=(beta, const))
        Xi = self.xi_from(beta, const)
        loss, grad = self.loss_grad_xi(Xi, mask, alias=alias, live_columns=self._live)
        g_beta, g_const = self.grads_to(grad)
        return loss, g_beta, g_const

    def aug_gram(self):
        """fp64 (S, p+d, p+d) augmented Gram matrices, all-reduced over the point shards."""
        G = self.engine.aug_gram(self.x, self.dx, self.order, self.flags)
        if self.distributed:
            dist.all_reduce(G, op=dist.ReduceOp.SUM, group=self.group)
        return G
