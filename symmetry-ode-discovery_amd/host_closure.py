"""Host-resident L-BFGS variables of a regressor whose data lives in HBM: ``_HostShadow`` for closures made only of
fused kernels, ``_HostParams`` for closures that need device autograd."""
from __future__ import annotations

import numpy as np
import torch


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
