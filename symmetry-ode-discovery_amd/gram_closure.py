"""Gram-form closure of the non-latent L-BFGS fit: the data enter the closure only through fixed fp64 matrices.

On a fixed batch (reference train.py:626-629) the closure MSE + w_sym * reversed regulariser (train.py:663-679) is a
quadratic form in the coefficients:
    mse = inv (tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy)),   G = [Theta | dx]^T [Theta | dx]          (symode_aug_gram)
    reg = inv v^T R v,                                    R = sum_g sum_n B^T B                   (symode_symreg_reversed_gram)
with W = Xi * M, v = vec(W), inv = 1 / (N d).  G and R are sums over points, so they are accumulated in ONE pass over the data
(in chunks if need be), point shards are combined by ONE all-reduce of [G | R | count], and every closure afterwards
(symode_quad_closure) costs O((d p)^2) per problem whatever N is.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .engine import SymodeError, get_engine


class GramStatistics:
    """[G | R | count] of one problem set (S problems, state dimension d, library (order, flags)), with or without the
    reversed regulariser's R.  ``add`` may be called once per chunk of points; the sums are raw (no 1/(N d))."""

    def __init__(self, S, d, order, flags=0, regulariser=False, device="cuda", engine=None):
        self.engine = engine or get_engine()
        self.S, self.d, self.order, self.flags = int(S), int(d), int(order), int(flags)
        self.p = self.engine.lib_size(self.d, self.order, self.flags)
        self.dp = self.d * self.p
        self.F = self.p + self.d
        self.regulariser = bool(regulariser)
        self.device = torch.device(device)
        nG = self.S * self.F * self.F
        nR = self.S * self.dp * self.dp if self.regulariser else 0
        # ONE fp64 buffer: [G | R | count] -- the sharded fit all-reduces it as one collective
        self.buffer = torch.zeros(nG + nR + 1, dtype=torch.float64, device=self.device)
        self.G = self.buffer[:nG].view(self.S, self.F, self.F)
        self.R = self.buffer[nG:nG + nR].view(self.S, self.dp, self.dp) if self.regulariser else None
        self._count = self.buffer[nG + nR:]

    @property
    def count(self) -> int:
        """Points accumulated per problem (over all ranks after ``all_reduce``)."""
        return int(round(self._count.item()))

    @torch.no_grad()
    def add(self, x, dx, gx=None, jgx=None):
        """Accumulate a chunk: x, dx (S, n, d); gx (S, n_g, n, d), jgx (S, n_g, n, d, d) when the statistics carry R."""
        if x.dim() == 2:
            x, dx = x[None], dx[None]
            gx = None if gx is None else gx[None]
            jgx = None if jgx is None else jgx[None]
        if x.shape[0] != self.S or x.shape[2] != self.d or x.shape != dx.shape:
            raise SymodeError(f"chunk x {tuple(x.shape)} / dx {tuple(dx.shape)} does not match S={self.S}, d={self.d}")
        if self.regulariser and (gx is None or jgx is None):
            raise SymodeError("these statistics carry the reversed regulariser: add() needs gx and jgx")
        if x.shape[1] == 0:
            return self
        self.G += self.engine.aug_gram(x, dx, self.order, self.flags)
        if self.regulariser:
            self.R += self.engine.symreg_reversed_gram(x, gx, jgx, self.order, self.flags)
        self._count += float(x.shape[1])
        return self

    @torch.no_grad()
    def add_gathered(self, x, dx, idx, gx=None, jgx=None):
        """Accumulate S index subsets of ONE shared data set without materialising them: x, dx (N, d), idx (S, m) int32
        rows (problem s adds the points x[idx[s]]); gx (n_g, N, d), jgx (n_g, N, d, d) when the statistics carry R.
        G from ONE gather-Gram launch, R from ONE gathered reversed-Gram launch; the count grows by m."""
        if x.dim() != 2 or x.shape != dx.shape or x.shape[1] != self.d or idx.dim() != 2 or idx.shape[0] != self.S:
            raise SymodeError(f"x {tuple(x.shape)} / dx {tuple(dx.shape)} / idx {tuple(idx.shape)} do not match S={self.S}, "
                              f"d={self.d}")
        if self.regulariser and (gx is None or jgx is None):
            raise SymodeError("these statistics carry the reversed regulariser: add_gathered() needs gx and jgx")
        if idx.shape[1] == 0:
            return self
        self.G += self.engine.aug_gram_gather(x, dx, idx, self.order, self.flags)
        if self.regulariser:
            self.R += self.engine.symreg_reversed_gram_gather(x, gx, jgx, idx, self.order, self.flags)
        self._count += float(idx.shape[1])
        return self

    @torch.no_grad()
    def add_gram(self, G, n_points):
        """Accumulate prebuilt augmented Gram matrices (S, p+d, p+d) of ``n_points`` points each (e.g. from
        ``aug_gram_gather``); only for statistics without R."""
        if self.regulariser:
            raise SymodeError("add_gram cannot supply the regulariser's R")
        self.G += G.reshape(self.G.shape).to(torch.float64)
        self._count += float(n_points)
        return self

    @torch.no_grad()
    def all_reduce(self, group=None):
        """Sum [G | R | count] over the ranks of ``group``: ONE fp64 collective."""
        dist.all_reduce(self.buffer, op=dist.ReduceOp.SUM, group=group)
        return self

    def inv_count(self) -> float:
        n = self.count
        if n < 1:
            raise SymodeError("no points accumulated")
        return 1.0 / (n * self.d)

    @torch.no_grad()
    def loss_grad(self, xi, mask=None, w_sym=1.0, inv_count=None):
        """The kernel's outputs: (loss (S,) or (S, 2) = (mse, regulariser), grad (S, d, p) of mse + w_sym * regulariser)."""
        inv = self.inv_count() if inv_count is None else float(inv_count)
        xi = xi.reshape(self.S, self.d, self.p)
        mask = None if mask is None else mask.reshape(self.S, self.d, self.p)
        return self.engine.quad_closure(self.G, self.R, xi, mask, inv, w_sym)

    def evaluate(self, xi, mask=None, w_sym=1.0):
        """As ``BatchedClosure.evaluate`` for unconstrained problems: (loss (S,), dloss/dXi (S, d, p), None), the loss being
        mse (+ w_sym * regulariser when the statistics carry R)."""
        loss, grad = self.loss_grad(xi, mask, w_sym)
        if self.regulariser:
            loss = loss[:, 0] + float(w_sym) * loss[:, 1]
        return loss, grad, None
