"""The map between the optimiser's variables and the coefficient matrix Xi (the reference's ``get_Xi``, sindy.py:169-176:
``Xi``, or ``Q @ beta`` viewed Kronecker-wise / transposed, plus ``const`` in the constant column), its transpose and the
layout of the flat vector ``[beta | const]`` -- the one place that spells them out.  Torch and numpy only, no engine.

The forms do NOT share arithmetic, on purpose: one problem is ``Q @ beta`` then ``+ cat([const, 0])``, S problems are
``beta @ Q.T`` then an in-place add into the constant column, the numpy forms stay in fp32 on the host.  L-BFGS on an
ill-conditioned library is chaotic in the last bit of every dot product (train.train_SIGED_lbfgs), so each caller keeps
its operations, operand order and dtype."""
from __future__ import annotations

import numpy as np
import torch


class CoefMap:
    def __init__(self, d, p, Q=None, use_kron_product=True, allow_constant=True):
        """Q (d p, r), or None: the variables ARE Xi.  ``allow_constant=False`` (--constrain_constant): ``const`` stays a
        variable that the model does not read (sindy.py:60, 173-175)."""
        self.d, self.p, self.Q = int(d), int(p), Q
        self.use_kron, self.allow_constant = bool(use_kron_product), bool(allow_constant)
        self.r = 0 if Q is None else int(Q.shape[1])
        self.sizes = (self.d * self.p,) if Q is None else (self.r, self.d)      # of the parameter tensors, in their order
        self.n_params = sum(self.sizes)
        self._Qnp = self._Qc = None

    @classmethod
    def from_regressor(cls, reg):
        args = (reg.Q, reg.use_kron_product, reg.allow_constant) if reg.constraint else ()
        return cls(reg.latent_dim, reg.get_term_num(), *args)

    def to(self, device):
        return self if self.Q is None else CoefMap(self.d, self.p, self.Q.detach().to(device), self.use_kron, self.allow_constant)

    def _numpy_Q(self):
        if self._Qnp is None:                       # strides as they come: the fp32 gradient product is taken on this array
            self._Qnp = self.Q.detach().cpu().numpy() if torch.is_tensor(self.Q) else np.asarray(self.Q)
        return self._Qnp

    def device_Q(self, device):
        """Q as a launch reads it (engine.loss_grad_reversed, ``coef=``): fp32, contiguous (d p, r), on ``device``, rows in Q's
        own order (the launch is told ``use_kron``).  Kept while Q's version counter and data pointer stay what they were."""
        Q = self.Q
        key = (torch.device(device), Q._version, Q.data_ptr())
        seen = getattr(self, "_Qdev", None)
        if seen is None or seen[0] != key:
            seen = (key, Q.detach().to(device=device, dtype=torch.float32).contiguous())
            self._Qdev = seen
        return seen[1]

    def split(self, P):
        """(beta, const) views of a flat (n,) or (S, n) tensor; (Xi, None) when unconstrained."""
        lead = P.shape[:-1]
        if self.Q is None:
            return P.view(*lead, self.d, self.p), None
        return P[..., :self.r], P[..., self.r:].reshape(*lead, self.d, 1)

    def join(self, a, b=None):
        """The flat vector(s) of the pieces; a missing ``const`` piece (a constant the model does not read) is a zero block."""
        if isinstance(a, np.ndarray):               # one problem, fp32 on the host
            if self.Q is None:
                return a.reshape(-1)
            return np.concatenate([a, np.zeros(self.d, dtype=np.float32) if b is None else b]).astype(np.float32)
        S = a.shape[0]
        if self.Q is None:
            return a.reshape(S, -1)
        if b is None:
            b = torch.zeros(S, self.d, 1, device=a.device, dtype=a.dtype)
        return torch.cat([a, b.reshape(S, -1)], dim=1)

    def draw(self, generator):
        """Initial flat variables in the order ``SINDyRegression`` draws them (beta, then const)."""
        return torch.cat([torch.randn(n, generator=generator) for n in self.sizes])

    def update_norm(self, A, B):
        """sum over the parameter tensors of ||A - B||, per problem (train.py:702-704)."""
        if self.Q is None:
            return (A - B).norm(dim=1)
        r = self.r
        return (A[:, :r] - B[:, :r]).norm(dim=1) + (A[:, r:] - B[:, r:]).norm(dim=1)

    def xi(self, beta, const=None):
        """Xi of one problem (beta (r,), const (d, 1): differentiable torch; or fp32 numpy with const (d,)) or of S problems
        (beta (S, r), const (S, d, 1) or None).  Unconstrained: ``beta`` is Xi."""
        if self.Q is None:
            return beta
        d, p = self.d, self.p
        if isinstance(beta, np.ndarray):
            if self._Qc is None:
                self._Qc = np.ascontiguousarray(self._numpy_Q(), dtype=np.float32)
            flat = self._Qc @ beta
            Xi = flat.reshape(d, p).copy() if self.use_kron else flat.reshape(p, d).T.copy()
            if self.allow_constant:
                Xi[:, 0] += const
            return Xi
        if beta.dim() == 1:
            flat = self.Q @ beta
            Xi = flat.view(d, -1) if self.use_kron else flat.view(-1, d).transpose(0, 1)
            if self.allow_constant:
                Xi = Xi + torch.cat([const, torch.zeros((Xi.shape[0], Xi.shape[1] - 1), device=Xi.device)], dim=1)
            return Xi
        flat = beta @ self.Q.T                                  # (S, d*p)
        Xi = flat.view(-1, d, p) if self.use_kron else flat.view(-1, p, d).transpose(1, 2)
        if self.allow_constant and const is not None:
            Xi = Xi.clone()
            Xi[:, :, 0:1] += const
        return Xi.contiguous()

    def grad(self, g_xi, flat=False):
        """(g_beta, g_const) from dL/dXi -- (S, d, p) torch or (d, p) fp32 numpy; g_const is None for a constant the model
        does not read.  ``flat=True``: the flat gradient instead (``join`` of the pieces)."""
        if self.Q is None:
            g_beta, g_const = g_xi, None
        elif isinstance(g_xi, np.ndarray):
            G = g_xi if self.use_kron else g_xi.T
            g_beta = self._numpy_Q().T @ G.reshape(-1)
            g_const = g_xi[:, 0] if self.allow_constant else None
        else:
            g = g_xi if self.use_kron else g_xi.transpose(1, 2)
            g_beta = g.reshape(g_xi.shape[0], -1) @ self.Q
            g_const = g_xi[:, :, 0:1].clone() if self.allow_constant else None
        return self.join(g_beta, g_const) if flat else (g_beta, g_const)

    def pack(self, reg):
        """The regressor's variables as one flat (n,) tensor on their device."""
        return torch.cat([q.detach().reshape(-1) for q in reg.parameters()])

    def adopt(self, reg, params, mask=None):
        """A flat (n,) state (tensor or numpy, host or device) into the regressor's variables and, in place, its mask."""
        with torch.no_grad():
            for dst, src in zip(reg.parameters(), self.split(torch.as_tensor(params))):
                dst.data.copy_(src)
            if mask is not None:
                reg.mask.copy_(torch.as_tensor(mask).view_as(reg.mask))

    def effective_Q(self):
        """Q as fp32 numpy with its rows in Xi's (d, p) row-major order, so that Xi = (q_eff @ beta).reshape(d, p) on either
        branch (the transposed view reads Xi[i, t] = flat[t * d + i]): what the device trainer's XiMap reads."""
        Q = np.ascontiguousarray(self._numpy_Q(), dtype=np.float32)
        if self.use_kron:
            return Q
        rows = (np.arange(self.p)[None, :] * self.d + np.arange(self.d)[:, None]).reshape(-1)
        return np.ascontiguousarray(Q[rows])

    def solve_matrix(self):
        """The matrix the constrained least-squares fit solves in (sindy.py:277-282), fp64 numpy (d p, r'), with
        r' = r + (d if allow_constant else 0): row j p + k is Q's row for equation j, library column k in the reference's
        equation-major indexing -- ``Q[mask.flatten()]``, taken as it stands also when ``use_kron_product`` is false, where
        Xi reads Q's rows in the other order (``xi_matrix``); the reference's quirk is kept -- and, with ``allow_constant``,
        d unit columns behind it: column r + j holds its 1 in row j p, the constant term of equation j."""
        Q = np.asarray(self._numpy_Q(), dtype=np.float64)
        if self.allow_constant:
            Q = np.concatenate([Q, np.zeros((Q.shape[0], self.d))], axis=1)
            for j in range(self.d):
                Q[j * self.p, self.r + j] = 1.0
        return np.ascontiguousarray(Q)

    def xi_matrix(self):
        """The matrix that forms Xi from beta, fp32 numpy (d p, r) with rows in Xi's (d, p) row-major order:
        ``effective_Q``, under the name the constrained fit reads it by next to ``solve_matrix``."""
        return self.effective_Q()

    def live_columns(self):
        """(d, p) bool: the entries of Xi the map can make non-zero.  The constraint keeps whole entries of Xi at zero (for
        the planar rotations every even degree), but the rows of Q that say so are not zero: its basis comes out of an SVD
        and all but one of them carry round-off, 1e-7 against 0.2-0.4 in the live rows -- a test for ``== 0`` finds
        nothing.  An entry counts as live when its row of ``effective_Q`` has max |.| above 64 eps_fp32 max|Q| (7.6e-6
        max|Q|: ten times the largest dead row seen, four orders under the smallest live one); whatever lies between
        counts as live, the threshold may only err towards doing the work.  Column 0 is live in every row when the model
        reads ``const``; without Q everything is."""
        if self.Q is None or self.r == 0:
            return np.ones((self.d, self.p), dtype=bool)
        rows =np.abs(self.effective_Q()).max(axis=1)
        live = (rows > 64.0 * np.finfo(np.float32).eps * rows.max()).reshape(self.d, self.p)
        if self.allow_constant:
            live[:, 0] = True
        return live

    def live_mask(self):
        """``live_columns`` as the launches take it: an int with bit k set when column k is live in any row -- all 64 bits
        when nothing is dead or the library has more than 64 columns."""
        cols = self.live_columns().any(axis=0)
        if self.p > 64 or cols.all():
            return 0xFFFFFFFFFFFFFFFF
        return sum(1 << k for k in np.flatnonzero(cols).tolist())
