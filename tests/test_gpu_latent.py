"""The latent L-BFGS fit on the fused path, on the GPU: symode_loss_grad_latent against an fp64 CPU evaluation of its
formula, the closure and the whole fit against the existing host_params route, and what the device trainer refuses."""
import numpy as np
import pytest
import torch

from tests.helpers import only_compiled
from tests.latent_cases import (FIT, closure_from_operands, events, random_points, run_fit, seeded_autoencoder)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5                       # the fused pair closure's figure (f6 / reversed-closure tests): of the largest gradient entry, of the loss
LIBS = only_compiled([(1, 3, 0), (2, 1, 0), (2, 3, 0), (2, 2, 3), (2, 5, 0), (3, 3, 0)])
# 1, around one wave, one workgroup + 1, and one point past one workgroup's slab of 256 chunks (d = 2: 513; d = 1, 3: 1025)
SIZES = (1, 63, 64, 65, 257, 513, 1025)


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd


def _problem(d, order, flags, n_problems, n, seed):
    """Operands of n_problems problems (fp32, CPU): B with singular values in [0.5, 2], a mask with zeros in every row and
    one all-zero row (d = 1 has one row: all-zero in problem 1 of a batch, zeros elsewhere)."""
    from oracle import sindy_oracle as O
    g = torch.Generator().manual_seed(seed)
    p = O.term_count(d, order, bool(flags & 1), bool(flags & 2))
    z = 0.8 * torch.randn(n_problems, n, d, generator=g)
    dz, y = torch.randn(n_problems, n, d, generator=g), torch.randn(n_problems, n, d, generator=g)
    U, _ = torch.linalg.qr(torch.randn(n_problems, n, d, d, generator=g))
    V, _ = torch.linalg.qr(torch.randn(n_problems, n, d, d, generator=g))
    sv = 0.5 + 1.5 * torch.rand(n_problems, n, d, generator=g)
    B = (U * sv[..., None, :]) @ V.transpose(-1, -2)
    xi = 0.5 * torch.randn(n_problems, d, p, generator=g)
    mask = (torch.rand(n_problems, d, p, generator=g) > 0.3).float()
    mask[..., 0] = 0.0
    mask[..., 1] = 1.0
    if d > 1:
        mask[:, -1] = 0.0
    elif n_problems > 1:
        mask[1] = 0.0
    return z, dz, B.contiguous(), y, xi, mask


def _want(z, dz, B, y, xi, mask, order, flags, w_pair):
    out = [closure_from_operands(z[s].double(), dz[s].double(), B[s].double(), y[s].double(), xi[s].double(), mask[s].double(),
                                 order, w_pair, bool(flags & 1), bool(flags & 2)) for s in range(z.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


@pytest.mark.parametrize("n_problems", [1, 3])
@pytest.mark.parametrize("d, order, flags", LIBS)
def test_kernel_matches_the_fp64_formula(S, d, order, flags, n_problems):
    eng = S.get_engine()
    worst = 0.0
    for n in SIZES:
        ops = _problem(d, order, flags, n_problems, n, seed=1000 * d + 10 * order + n)
        dev = [t.to(DEV) for t in ops]
        for w_pair in (0.0, 0.37):
            want_l, want_g = _want(*ops, order, flags, w_pair)
            if n_problems == 1:
                l2, g = eng.loss_grad_latent(*(t[0] for t in dev), order, flags, w_pair=w_pair)
                l2, g = l2[None], g[None]
            else:
                l2, g = eng.loss_grad_latent(*dev, order, flags, w_pair=w_pair)
            l2, g = l2.double().cpu(), g.double().cpu()
            assert l2.shape == (n_problems, 2) and g.shape == want_g.shape
            for s in range(n_problems):
                el = float(((l2[s] - want_l[s]).abs() / want_l[s].abs()).max())
                scale = float(want_g[s].abs().max())
                eg = float((g[s] - want_g[s]).abs().max()) / scale if scale > 0 else float(g[s].abs().max())
                worst = max(worst, el, eg)
                assert el <= TOL, (n, w_pair, s, "loss", el)
                assert eg <= TOL, (n, w_pair, s, "grad", eg)
                assert torch.equal(g[s][ops[5][s] == 0], torch.zeros_like(g[s][ops[5][s] == 0]))      # masked entries: exactly 0
    print(f"latent kernel d={d} order={order} flags={flags} S={n_problems}: worst relative error {worst:.2e} (bound {TOL:.0e})")


@pytest.mark.parametrize("d, order, flags", LIBS)
def test_identity_B_is_twice_the_plain_closure_and_launches_repeat_bitwise(S, d, order, flags):
    eng = S.get_engine()
    for n in (65, 1025):
        z, dz, B, y, xi, mask = [t.to(DEV) for t in _problem(d, order, flags, 3, n, seed=7 + n)]
        eye = torch.eye(d, device=DEV).expand(3, n, d, d).contiguous()
        l2, g = eng.loss_grad_latent(z, dz, eye, dz, xi, mask, order, flags, w_pair=1.0)
        l1, g1 = eng.loss_grad(z, dz, xi, mask, order, flags)
        for s in range(3):
            assert float((l2[s] - l1[s]).abs().max()) <= TOL * float(l1[s].abs())
            scale = float(g1[s].abs().max())
            assert float((g[s] - 2.0 * g1[s]).abs().max()) <= TOL * 2.0 * scale
        a = eng.loss_grad_latent(z, dz, B, y, xi, mask, order, flags, w_pair=0.37)
        a = (a[0].clone(), a[1].clone())
        b = eng.loss_grad_latent(z, dz, B, y, xi, mask, order, flags, w_pair=0.37)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("D", [2, 6])
def test_closure_matches_the_existing_route(S, D):
    """loss_sindy_z, loss_sindy_x and the Xi-gradient of one closure evaluation: fused (latent_operands +
    symode_loss_grad_latent) against train._autograd_closure(use_latent=True) on the GPU, both against the same closure in
    fp64 on the CPU.  The existing route's gradient is the z-term's (compute_dx cuts the x-term from the graph), hence the
    launch with w_pair = 0."""
    from symode_amd import train as T
    from symode_amd.model_utils import latent_operands
    from tests.oracle_engine import OracleEngine
    d, order, n, w_z, w_x = 2, 3, 500, 0.7, 0.3
    terms = T._LossTerms(w_z, w_x, "none", 0.0, "i", 0.0, 0.1, 0.01)
    x, dx = random_points(n, 1, D, seed=D)
    torch.manual_seed(2)
    Xi0 = 0.5 * torch.randn(d, 10)
    mask = (torch.rand(d, 10) > 0.3).float()

    def existing(device, dtype, engine=None):
        ae = seeded_autoencoder(D, d, 1, seed=40 + D, dtype=dtype, device=device)
        kw = {} if engine is None else {"engine": engine}
        reg = S.SINDyRegression(d, order, False, False, threshold=0.1, device=device, **kw).to(dtype)
        reg.Xi.data, reg.mask = Xi0.to(device, dtype), mask.to(device, dtype)
        losses = {}
        closure = T._autograd_closure(reg, x.to(device, dtype), dx.to(device, dtype), ae, None, terms, losses, True, None)
        closure(torch.optim.SGD(reg.parameters(), lr=0.0))
        return float(losses["loss_sindy_z"]), float(losses["loss_sindy_x"]), reg.Xi.grad.double().cpu(), ae, reg

    tz, tx, tg, _, _ = existing("cpu", torch.float64, OracleEngine())
    ez, ex, eg, ae, reg = existing(DEV, torch.float32)
    z, dz, B, y, e0, D_out = latent_operands(x.to(DEV), dx.to(DEV), ae)
    l2, g = S.get_engine().loss_grad_latent(z, dz, B, y, reg.Xi.detach(), reg.mask, order, 0, w_pair=0.0)
    fz, fx = float(l2[0]), float(l2[1]) * d / D_out + e0 / (n * D_out)
    fg = (w_z * g).double().cpu()
    gs = float(tg.abs().max())
    err = lambda a, b, s: abs(a - b) / s  # noqa: E731
    figs = {"loss_sindy_z": (err(fz, ez, tz), err(fz, tz, tz), err(ez, tz, tz)),
            "loss_sindy_x": (err(fx, ex, tx), err(fx, tx, tx), err(ex, tx, tx)),
            "grad": (float((fg - eg).abs().max()) / gs, float((fg - tg).abs().max()) / gs, float((eg - tg).abs().max()) / gs)}
    for k, (fe, ft, et) in figs.items():
        print(f"latent closure D={D} {k}: fused vs existing {fe:.2e}, fused vs fp64 {ft:.2e}, existing vs fp64 {et:.2e}")
    for k, (fe, ft, et) in figs.items():
        assert fe <= TOL, (k, fe)
        assert ft <= et + TOL, (k, ft, et)


def test_fit_matches_the_host_params_route(S, tmp_path, monkeypatch, capsys):
    """30 epochs on the damped oscillator through a near-identity autoencoder: the fused route against host_params --
    identical masks, Xi within the L-BFGS trainer figure of 1e-3, the same convergence / thresholding messages.  The case is
    admissible: the plain route on the CPU records no near-threshold coefficient on it and repeats its mask (checked when
    the seed and noise were chosen); no run here may record one either."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(S.train.wandb, "log", lambda *a, **k: None, raising=False)
    routes = []
    real = S.train._lbfgs_route
    monkeypatch.setattr(S.train, "_lbfgs_route", lambda **kw: routes.append(real(**kw)) or routes[-1])
    capsys.readouterr()
    r_host = run_fit(S, DEV, fused_latent=False)
    out_host = capsys.readouterr().out
    r_fused = run_fit(S, DEV, fused_latent=True)
    out_fused = capsys.readouterr().out
    assert routes == ["host_params", "latent"]
    assert r_host.near_threshold == [] and r_fused.near_threshold == []
    dxi = float((r_fused.Xi.detach() - r_host.Xi.detach()).abs().max())
    print(f"latent fit: max |Xi_fused - Xi_host| = {dxi:.2e}; events {events(out_fused)}")
    print("Xi host ", r_host.Xi.detach().cpu().numpy().round(5).tolist(), "\nXi fused", r_fused.Xi.detach().cpu().numpy().round(5).tolist())
    assert torch.equal(r_fused.mask.cpu(), r_host.mask.cpu())
    assert dxi <= 1e-3
    assert events(out_fused) == events(out_host) and len(events(out_host)) >= 1
    # the same transcript shape: the same lines with the same keys, epoch by epoch
    keys = lambda out: [[part.split(":")[0] for part in line.split(", ")] for line in out.splitlines() if line.startswith("Epoch")]  # noqa: E731
    assert keys(out_fused) == keys(out_host)
    assert any("test_loss_sindy_z" in line for line in out_fused.splitlines())
    assert int(r_fused.mask.sum()) < r_fused.mask.numel()                       # thresholding did happen


def test_device_trainer_refuses_what_the_latent_closure_does_not_cover(S):
    from symode_amd.device_lbfgs import DeviceTrainer
    from symode_amd.engine import CLOSURE_LATENT, SymodeError
    z, dz, B, y, _, _ = [t.to(DEV) for t in _problem(2, 2, 0, 1, 64, seed=0)]
    ok = dict(poly_order=2, closure="latent", latent=(B, y, 0.5), w_x=1.0)
    with pytest.raises(SymodeError, match="closure='latent' does not take group"):
        DeviceTrainer(z, dz, **dict(ok, group=object()))
    with pytest.raises(SymodeError, match="closure='latent' does not take statistics"):
        DeviceTrainer(z, dz, **dict(ok, statistics=object()))
    with pytest.raises(SymodeError, match="w_sindy_z > 0"):
        DeviceTrainer(z, dz, **dict(ok, w_x=0.0))
    with pytest.raises(SymodeError, match="latent operands are for closure='latent'"):
        DeviceTrainer(z, dz, 2, latent=(B, y, 0.5))
    tr = DeviceTrainer(z, dz, **ok)                                              # and the covered case is accepted
    assert tr.latent and tr.pair and tr.T.closure == CLOSURE_LATENT and tr.T.n_g == 0 and not tr.T.gx


def _enqueue_epoch_by_hand(tr, epoch):
    """The epoch of symode_trainer_run stated entry by entry, with symode_loss_grad_latent called by name on the LATENT
    descriptor's operands -- the double of the dispatch in symode_trainer_closure: closure (w_pair = 0), BEGIN update,
    (closure, ACCEPT update) x (max_iter - 1), epoch end, the closure at the epoch's final state into the test line."""
    import ctypes
    lib, st, T = tr.engine.lib, tr._st(), tr.T
    xi, mask = tr.field("xi").data_ptr(), tr.field("mask").data_ptr()

    def closure(loss, grad):
        rc = lib.symode_loss_grad_latent(T.x, T.dx, T.latent_B, T.latent_y, T.n_problems, T.n_points, T.d, T.order, T.flags, xi, mask,
                                         T.inv_count, 0.0, ctypes.c_void_p(loss), ctypes.c_void_p(grad), T.workspace,
                                         T.workspace_bytes, st)
        assert rc == 0, rc

    for it in range(T.max_iter):
        closure(tr.field("cl_loss").data_ptr(), tr.field("cl_grad").data_ptr())
        assert lib.symode_trainer_update(tr._Tp, 2 if it == 0 else 1, st) == 0
    assert lib.symode_trainer_epoch_end(tr._Tp, epoch, st) == 0
    closure(tr.log_test[epoch % tr.LOG_RING].data_ptr(), tr.field("test_grad").data_ptr())


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("n", [513, 65])
@pytest.mark.parametrize("d, order, flags", only_compiled([(2, 3, 0), (1, 3, 0)]))
def test_trainer_run_equals_the_hand_enqueued_epoch_bit_for_bit(S, d, order, flags, n, constrained):
    """symode_trainer_run on a SYMODE_CLOSURE_LATENT descriptor against the same epochs enqueued by hand on a second trainer
    built from the same inputs: the same kernels with the same arguments in the same order, so the whole state block and
    every record agree as bytes.  3 problems, max_iter 4 over a ring of 3 curvature pairs (it wraps), st_freq 2 (a
    period-triggered thresholding with optimiser reset by epoch 2), 5 epochs."""
    import ctypes
    from symode_amd.device_lbfgs import EVENT_NAN, EVENT_THRESHOLD_PERIOD, DeviceTrainer
    from symode_amd.engine import CLOSURE_LATENT
    epochs, n_problems = 5, 3
    z, dz, B, y, xi0, mask0 = [t.to(DEV) for t in _problem(d, order, flags, n_problems, n, seed=11)]
    if d > 1:                                       # _problem zeroes the last row everywhere: keep ONE all-zero row, in problem 1
        mask0[0, -1], mask0[2, -1] = mask0[0, 0], mask0[2, 0]
    g = torch.Generator().manual_seed(5)
    dp = xi0[0].numel()
    Q = None
    if constrained:                                 # (d p, 5) with orthonormal columns (d = 1: d p = 4 < 5, orthonormal rows)
        Q = torch.linalg.qr(torch.randn(max(dp, 5), min(dp, 5), generator=g))[0]
        Q = (Q if dp >= 5 else Q.T).contiguous()
    P0 = (0.5 * torch.randn(n_problems, 5 + d, generator=g)).to(DEV) if constrained else xi0.reshape(n_problems, dp).clone()
    make = lambda: DeviceTrainer(z, dz, order, flags, Q=Q, allow_constant=True, closure="latent", latent=(B, y, 0.37), lr=0.05,  # noqa: E731
                                 st_freq=2, max_iter=4, history=3, detail=True)
    a, b = make(), make()
    assert a.T.closure == CLOSURE_LATENT and (a.q_eff is not None) == constrained
    a.fit(P0, epochs, mask0=mask0, test_eval=True)
    assert b.engine.lib.symode_trainer_init(b._Tp, ctypes.c_void_p(P0.data_ptr()), ctypes.c_void_p(mask0.data_ptr()), b._st()) == 0
    for e in range(epochs):
        _enqueue_epoch_by_hand(b, e)
    torch.cuda.synchronize()
    codes = a.log[:epochs, :, 0]
    print(f"latent trainer d={d} n={n} constrained={constrained}: event codes per epoch {codes.long().tolist()}")
    assert torch.equal(a.state, b.state)            # symode_trainer_init zeroes the block: padding compares too
    for name in ("log", "log_test", "log_xi", "log_mask", "log_params"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # (checked when the seeds were chosen: every case thresholds on the period and none runs into NaN)
    assert bool((codes == EVENT_THRESHOLD_PERIOD).any()) and not bool((codes == EVENT_NAN).any())
    # the dispatch itself, once, with explicit outputs: the LATENT closure at the trainer's coefficients and mask, w_pair = 0
    xi, mask = a.field("xi").clone(), a.field("mask").clone()
    loss, grad = torch.zeros(n_problems, 2, device=DEV), torch.zeros(n_problems, d, dp // d, device=DEV)
    assert a.engine.lib.symode_trainer_closure(a._Tp, ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(grad.data_ptr()), a._st()) == 0
    want_l, want_g = a.engine.loss_grad_latent(z, dz, B, y, xi, mask, order, flags, w_pair=0.0, inv_count=a.T.inv_count)
    assert torch.equal(loss, want_l) and torch.equal(grad, want_g)


def test_fused_latent_without_use_latent_is_ignored(S, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(S.train.wandb, "log", lambda *a, **k: None, raising=False)
    from tests.latent_cases import fit_data
    x, dx, Xi0 = fit_data()
    routes, masks = [], []
    real = S.train._lbfgs_route
    monkeypatch.setattr(S.train, "_lbfgs_route", lambda **kw: routes.append(real(**kw)) or routes[-1])
    ident = torch.nn.Identity()
    for fused in (False, True):
        r = S.SINDyRegression(2, FIT["order"], False, False, threshold=FIT["threshold"], device=DEV)
        r.Xi.data = Xi0.to(DEV)
        S.train.train_SIGED_lbfgs(
            train_loader=[(x.to(DEV), dx.to(DEV))], test_loader=[], num_epochs=3, device=DEV, log_interval=10 ** 9,
            save_interval=10 ** 9, save_dir="t", autoencoder=ident, generator=ident, regressor=r, regressor_dst=None,
            use_latent=False, distill_latent=False, lr_sindy=0.1, w_sindy_z=0.0, w_sindy_x=1.0, sindy_reg_type="l1",
            w_sindy_reg=0.0, sym_reg_type="i", w_sym_reg=0.0, st_freq=10, threshold=FIT["threshold"], int_t=0.1, int_dt=0.01,
            print_eq=False, fused_latent=fused)
        masks.append((r.Xi.detach().cpu().clone(), r.mask.cpu().clone()))
    assert routes == ["device", "device"]
    assert torch.equal(masks[0][0], masks[1][0]) and torch.equal(masks[0][1], masks[1][1])     # bit for bit what it was
    assert np.isfinite(masks[0][0].numpy()).all()
