"""GPU parity of the training-loop layer: L-BFGS trainer, symmetry regularisers (S1-S4) and the
integrator, through the HIP engine, against the reference's recorded outputs."""
import os

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.helpers import load_fixture_autoencoder, load_fixture_generator, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd


def _regressor(S, g, tag, d, order, thr):
    if f"{tag}_init_Xi" in g.files:
        r = S.SINDyRegression(d, order, False, False, threshold=thr, device=DEV)
        r.Xi.data = t(g[f"{tag}_init_Xi"]).to(DEV)
    else:
        r = S.SINDyRegression(d, order, False, False, L_list=[torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], threshold=thr,
                              device=DEV, constrain_constant=False)
        r.Q = t(g[f"{tag}_Q"]).to(DEV)
        r.beta.data, r.const.data = t(g[f"{tag}_init_beta"]).to(DEV), t(g[f"{tag}_init_const"]).to(DEV)
    return r


@pytest.mark.parametrize("mode", ["host_numpy", "host_torch", "device", "device_kernels"])
@pytest.mark.parametrize("tag", ["dosc_sindy", "dosc_esindy", "selkov_sindy"])
def test_lbfgs_trainer_on_gpu_matches_reference_run(S, golden, tag, mode, tmp_path, monkeypatch):
    """The reference's three recorded runs through every optimiser placement: the DEFAULT (optimiser + epoch logic as
    device kernels: one launch per inner iteration beside the closure kernel, one per epoch), torch.optim.LBFGS's own
    operations on host variables (``torch_lbfgs=True``) / on device tensors, and the numpy restatement."""
    host_lbfgs, numpy_lbfgs = mode != "device", mode == "host_numpy"
    if numpy_lbfgs and tag == "selkov_sindy":
        pytest.skip("opt-in numpy L-BFGS: chaotic trajectory on the ill-conditioned selkov library (see train.py)")
    monkeypatch.chdir(tmp_path)
    g = golden("f4_lbfgs")
    d, order = [int(v) for v in g[f"{tag}_cfg"]]
    lr, st_freq, thr, epochs = g[f"{tag}_hp"]
    x, dx = t(g[f"{tag}_x"]), t(g[f"{tag}_dx"])
    r = _regressor(S, g, tag, d, order, float(thr))
    ident = torch.nn.Identity()
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], test_loader=[], num_epochs=int(epochs), device=DEV,
                              log_interval=10 ** 9, save_interval=10 ** 9, save_dir="t", autoencoder=ident, generator=ident,
                              regressor=r, regressor_dst=None, use_latent=False, distill_latent=False, lr_sindy=float(lr),
                              w_sindy_z=0.0, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=0.0, sym_reg_type="i",
                              w_sym_reg=0.0, st_freq=int(st_freq), threshold=float(thr), int_t=0.1, int_dt=0.01, print_eq=False,
                              host_lbfgs=host_lbfgs, numpy_lbfgs=numpy_lbfgs, torch_lbfgs=mode != "device_kernels")
    assert np.array_equal(r.mask.cpu().numpy(), g[f"{tag}_mask_final"])            # identical sparsity mask
    if mode == "device_kernels":                # the reference saves on final convergence (train.py:709-714)
        import os
        assert any(f.startswith("regressor_") for f in os.listdir("saved_models/t"))
    want = g[f"{tag}_Xi_final"]
    got = r.get_Xi().detach().cpu().numpy()
    # the iteration ends on "parameter update < 1e-3" (train.py:643): both runs sit within that ball of the minimiser
    # (the restated optimiser on the ill-conditioned selkov library, cond 9e3: same mask, coefficients 7e-4 apart inside it)
    atol = 1e-3 if (mode == "device_kernels" and tag == "selkov_sindy") else 1e-4
    assert np.allclose(got * g[f"{tag}_mask_final"], want * g[f"{tag}_mask_final"], rtol=1e-3, atol=atol), np.abs(got - want).max()
    if f"{tag}_eval_cf" in g.files:
        coef, cf, mse, cf_all, mse_all = S.evaluation.eval_sindy_regressor(r, S.evaluation.sindy_truth[tag.split("_")[0]])
        assert np.array_equal(cf, g[f"{tag}_eval_cf"]) and bool(cf_all) == bool(g[f"{tag}_eval_cf_all"])


@pytest.mark.parametrize("tag,act,rep", [("relu_sim2", "ReLU", "(2,sim2)"), ("tanh_learn", "Tanh", "(2,1,2)")])
def test_symmetry_regularisers_match_reference(S, golden, tag, act, rep):
    from symode_amd import model_utils as MU
    g = golden("f6_symreg")
    ae = load_fixture_autoencoder(g, tag, act, DEV)
    gen = load_fixture_generator(g, tag, rep, DEV)
    d, order, sine, exp = [int(v) for v in g[f"{tag}_cfg"]]
    r = S.SINDyRegression(d, order, bool(sine), bool(exp), threshold=0.1, device=DEV)
    r.Xi.data = t(g[f"{tag}_Xi"]).to(DEV)
    r.mask = t(g[f"{tag}_mask"]).to(DEV)
    x = t(g[f"{tag}_x"]).to(DEV)
    K, dt = int(g[f"{tag}_K"]), float(g[f"{tag}_dt"])
    flow = MU._EulerFlow(r, K * dt + 1e-9, dt)

    # integrator: fused kernel (no grad) and autograd-chained route agree with the reference
    with torch.no_grad():
        assert np.allclose(flow(x).cpu().numpy(), g[f"{tag}_euler"], rtol=1e-5, atol=1e-6)
        assert np.allclose(MU.odeint(r, x, K * dt + 1e-9, dt, full_traj=True).cpu().numpy(), g[f"{tag}_euler_traj"], rtol=1e-5, atol=1e-6)
        assert np.allclose(MU.odeint(r, x, K * dt + 1e-9, dt, method="rk4").cpu().numpy(), g[f"{tag}_rk4"], rtol=1e-5, atol=1e-6)
    assert np.allclose(flow(x).detach().cpu().numpy(), g[f"{tag}_euler"], rtol=1e-5, atol=1e-6)     # grad-enabled route

    def run(fn):
        r.Xi.grad = None
        loss = fn()
        loss.backward()
        return loss.item(), r.Xi.grad.detach().cpu().numpy()

    def check(name, loss, grad, rl=1e-5, rg=2e-5):          # measured on MI355X: <= 1.0e-6 / 1.1e-6 over both fixtures
        wl, wg = float(g[f"{tag}_{name}_loss"]), g[f"{tag}_{name}_grad"]
        print(f"{tag} {name}: loss rel err {abs(loss - wl) / abs(wl):.2e}, grad scaled err {np.abs(grad - wg).max() / np.abs(wg).max():.2e}")
        assert np.isclose(loss, wl, rtol=rl), (name, loss, wl)
        assert np.abs(grad - wg).max() <= rg * np.abs(wg).max(), (name, np.abs(grad - wg).max() / np.abs(wg).max())

    s2 = MU.make_symmreg_pttrain(ae, gen)
    check("s2", *run(lambda: s2(torch.stack([x, flow(x)], dim=1), f=flow)))
    check("s2abs", *run(lambda: s2(torch.stack([x, flow(x)], dim=1), f=flow, relative=False)))
    s3 = MU.make_fsymmreg_pttrain(ae, gen)
    check("s3", *run(lambda: s3(torch.stack([x, flow(x)], dim=1), f=flow)))
    s4 = MU.make_rsymmreg_pttrain(ae, gen)
    check("s4", *run(lambda: s4(x, h=r)))                                    # fused kernel on precomputed (g(x), J_g)
    basis = gen.get_full_basis_list()
    check("s1", *run(lambda: MU.symmreg_linear(x, r, basis)))


def test_forward_and_jvp_gradients_vs_fp64_double_backward(S):
    """The hand-written reverse of the forward-mode kernel (second-order term included) against
    torch's create_graph=True jvp on the fp64 oracle."""
    torch.manual_seed(2)
    for d, order, sine, exp in [(2, 3, False, False), (2, 5, False, False), (3, 2, True, True), (1, 4, False, True)]:
        r = S.SINDyRegression(d, order, sine, exp, threshold=0.1, device=DEV)
        r.mask = (torch.rand_like(r.mask) > 0.2).float()
        x, v = torch.randn(300, d) * 0.6, torch.randn(300, d)
        c1, c2 = torch.randn(300, d), torch.randn(300, d)
        xg, vg = x.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        out, jv = r.forward_and_jvp(xg, vg)
        ((out * c1.to(DEV)).sum() + (jv * c2.to(DEV)).sum()).backward()
        Xi = r.Xi.detach().cpu().double().requires_grad_(True)
        xo, vo = x.double().requires_grad_(True), v.double().requires_grad_(True)
        f = lambda a: O.forward(a, Xi, r.mask.cpu().double(), order, sine, exp)  # noqa: E731
        oo, jo = torch.autograd.functional.jvp(f, xo, vo, create_graph=True)
        ((oo * c1.double()).sum() + (jo * c2.double()).sum()).backward()
        for got, want, nm in [(xg.grad, xo.grad, "x"), (vg.grad, vo.grad, "v"), (r.Xi.grad, Xi.grad, "Xi")]:
            err = (got.cpu().double() - want).abs().max().item() / want.abs().max().item()
            assert err < 2e-5, (d, order, nm, err)


def test_train_sindy_and_wsindy_on_gpu(S, golden):
    g = golden("f3_stlsq")
    x, dx = t(g["selkov_ridge_x"]), t(g["selkov_ridge_dx"])
    r = S.SINDyRegression(2, 3, False, False, threshold=0.075, device=DEV, lstsq_driver="gelsy")   # CPU-made goldens
    S.train.train_SINDy(r, x, dx, num_epochs=8, device=DEV, log_interval=100, save_interval=100, save_dir="t", w_sindy_reg=0.1, threshold=0.075)
    assert np.array_equal(r.mask.cpu().numpy(), g["selkov_ridge_masks"][-1])
    w = golden("f7_wsindy")
    xw = t(w["x"]).to(DEV)
    n = xw.shape[0]
    r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV, lstsq_driver="gelsy")
    wr = S.WSINDyWrapper(r, torch.arange(n) * 0.02, float(w["tmax"]), device=DEV)
    assert np.allclose(wr.V[:, :48].cpu().numpy(), w["V_head"], rtol=1e-5, atol=1e-7)
    assert np.allclose(wr.V_drv[:, :48].cpu().numpy(), w["V_drv_head"], rtol=1e-5, atol=1e-7)
    for wm, wx, wc in zip(w["masks"], w["xis"], w["conv"]):
        res, c = wr.solve(xw, 0.0, 0.05)
        assert np.array_equal(r.mask.cpu().numpy(), wm) and bool(c) == bool(wc)
        # fused fp64 contraction (symode_weak_gram): the reference's own fp32 GEMMs are the remaining difference
        assert np.allclose(r.Xi.detach().cpu().numpy(), wx, rtol=1e-5, atol=1e-5 * np.abs(wx).max()), np.abs(r.Xi.detach().cpu().numpy() - wx).max() / np.abs(wx).max()


def _train_kwargs(**over):
    kw = dict(test_loader=[], num_epochs=6, device=DEV, log_interval=10 ** 9, save_interval=10 ** 9, save_dir="t",
              regressor_dst=None, use_latent=False, distill_latent=False, lr_sindy=0.1, w_sindy_z=0.0, w_sindy_x=1.0,
              sindy_reg_type="l1", w_sindy_reg=0.0, sym_reg_type="i", w_sym_reg=0.0, st_freq=50, threshold=0.05,
              int_t=0.03, int_dt=0.01, print_eq=False)
    kw.update(over)
    return kw


@pytest.mark.parametrize("sym", ["i", "f", "r"])
def test_trainer_with_symmetry_regulariser_runs_and_matches_oracle_closure(S, golden, sym, tmp_path, monkeypatch):
    """EquivSINDy-r style closure (MSE + w * sym-reg) through train_SIGED_lbfgs with a frozen tiny
    autoencoder: first-closure loss equals the oracle's value for the same terms, training lowers it."""
    monkeypatch.chdir(tmp_path)
    g = golden("f6_symreg")
    tag, act, rep = "relu_sim2", "ReLU", "(2,sim2)"
    ae = load_fixture_autoencoder(g, tag, act, DEV)
    gen = load_fixture_generator(g, tag, rep, DEV)
    d, order, sine, exp = [int(v) for v in g[f"{tag}_cfg"]]
    x = t(g[f"{tag}_x"])
    Xi0 = t(g[f"{tag}_Xi"])
    dx = O.forward(x, Xi0 * 0.5, torch.ones_like(Xi0), order, bool(sine), bool(exp)).detach()
    r = S.SINDyRegression(d, order, bool(sine), bool(exp), threshold=0.05, device=DEV)
    r.Xi.data = Xi0.to(DEV)
    logged = []
    monkeypatch.setattr(S.train.wandb, "log", lambda dct, *a, **k: logged.append(dict(dct)), raising=False)
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ae, generator=gen, regressor=r,
                              **_train_kwargs(sym_reg_type=sym, w_sym_reg=0.1, num_epochs=4))
    assert len(logged) >= 1 and all(np.isfinite(list(l.values())).all() for l in logged)
    first, last = logged[0], logged[-1]
    assert last["loss_sindy_x"] < first["loss_sindy_x"] * 1.01
    assert "loss_sym_reg" in first and first["loss_sym_reg"] >= 0


def test_device_lbfgs_path_writes_logs_and_interval_checkpoints(S, golden, tmp_path, monkeypatch, capsys):
    """The default path (optimiser + epoch logic on the device) with the reference configs' log / save intervals produces
    what the reference produces per epoch, from its per-epoch records: an 'Epoch k, loss_sindy_x' line and a "test" line
    (train.py:739-751) per logged epoch, one wandb record per epoch with the reference's keys, ``regressor_<epoch>.pt`` at the
    save interval and on final convergence (train.py:709-714) -- and nothing after a run that only ran out of epochs;
    the same final mask with and without the logging; the same records as torch's own optimiser writes on the same
    problem (first epoch: 20 iterations from the same start)."""
    monkeypatch.chdir(tmp_path)
    g = golden("f4_lbfgs")
    x, dx = t(g["dosc_sindy_x"]), t(g["dosc_sindy_dx"])
    ident = torch.nn.Identity()
    masks, records = [], {}
    for name, log, save, torch_opt in (("dl1", 1, 2, False), ("quiet", 10 ** 9, 10 ** 9, False), ("torch", 1, 2, True)):
        r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
        r.Xi.data = t(g["dosc_sindy_init_Xi"]).to(DEV)
        logged = []
        monkeypatch.setattr(S.train.wandb, "log", lambda dct, *a, _l=logged, **k: _l.append(dict(dct)), raising=False)
        S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ident, generator=ident, regressor=r,
                                  **_train_kwargs(num_epochs=60, lr_sindy=0.1, threshold=0.05, st_freq=50, torch_lbfgs=torch_opt,
                                                  log_interval=log, save_interval=save, save_dir=name, test_loader=[(x, dx)] * 3))
        masks.append(r.mask.cpu().numpy())
        records[name] = logged
        if name == "dl1":
            out = capsys.readouterr().out
    assert "Epoch 0, loss_sindy_x:" in out and "Epoch 1, loss_sindy_x:" in out and "Final convergence reached" in out
    assert out.count("test_loss_sindy_x") == len(records["dl1"])
    files = sorted(os.listdir("saved_models/dl1"))
    assert "regressor_1.pt" in files and "regressor_3.pt" in files and len(files) >= 3
    assert sorted(os.listdir("saved_models/torch")) == files                       # the same checkpoints as the host path
    state = torch.load(f"saved_models/dl1/{files[-1]}", weights_only=True)
    assert set(state) == {"Xi"}
    assert all(np.array_equal(m, g["dosc_sindy_mask_final"]) for m in masks)
    dev, ref = records["dl1"], records["torch"]
    assert len(dev) == len(ref) == len(records["quiet"]) == len(g["dosc_sindy_loss_hist"])
    assert set(dev[0]) == set(ref[0]) == {"loss_sindy_x", "loss_sindy_reg", "test_loss_sindy_x", "test_loss_sindy_z"}
    assert np.isclose(dev[0]["loss_sindy_x"], ref[0]["loss_sindy_x"], rtol=1e-5)
    assert np.isclose(dev[0]["test_loss_sindy_x"], ref[0]["test_loss_sindy_x"], rtol=1e-5)
    assert np.isclose(dev[0]["loss_sindy_reg"], ref[0]["loss_sindy_reg"], rtol=1e-5)
    # a run that runs out of epochs writes no final checkpoint (the reference saves on final convergence / at the interval)
    r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
    r.Xi.data = t(g["dosc_sindy_init_Xi"]).to(DEV)
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ident, generator=ident, regressor=r,
                              **_train_kwargs(num_epochs=2, lr_sindy=0.1, threshold=0.05, st_freq=50, save_dir="short"))
    assert not os.path.exists("saved_models/short")


@pytest.mark.parametrize("torch_opt", [False, True], ids=["device_trainer", "torch_lbfgs"])
def test_nan_gradient_ends_the_fit_with_the_reference_message(S, golden, tmp_path, monkeypatch, capsys, torch_opt):
    """A NaN in the data makes loss and gradient NaN at the finite start: torch.optim.LBFGS does not stop on a NaN gradient
    (`<=` test), the parameters go to NaN and train.py:697-699 ends the run -- on the device trainer as on torch's optimiser."""
    monkeypatch.chdir(tmp_path)
    g = golden("f4_lbfgs")
    x, dx = t(g["dosc_sindy_x"]), t(g["dosc_sindy_dx"]).clone()
    dx[17, 1] = float("nan")
    r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
    r.Xi.data = t(g["dosc_sindy_init_Xi"]).to(DEV)
    ident = torch.nn.Identity()
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ident, generator=ident, regressor=r,
                              **_train_kwargs(num_epochs=5, lr_sindy=0.1, torch_lbfgs=torch_opt, save_dir="nan"))
    out = capsys.readouterr().out
    assert "NaN encountered at iteration 0; exit training." in out and "Final convergence" not in out
    assert torch.isnan(r.Xi).any() and not os.path.exists("saved_models/nan")


def test_reversed_regulariser_host_and_device_lbfgs_agree(S, golden, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    g = golden("f6_symreg")
    tag, act, rep = "tanh_learn", "Tanh", "(2,1,2)"
    ae = load_fixture_autoencoder(g, tag, act, DEV)
    gen = load_fixture_generator(g, tag, rep, DEV)
    d, order, sine, exp = [int(v) for v in g[f"{tag}_cfg"]]
    x = t(g[f"{tag}_x"])
    Xi0 = t(g[f"{tag}_Xi"])
    dx = O.forward(x, Xi0 * 0.5, torch.ones_like(Xi0), order, bool(sine), bool(exp)).detach()
    out = []
    for host, kernels in ((True, False), (False, False), (True, True)):     # last: the default (optimiser as device kernels)
        r = S.SINDyRegression(d, order, bool(sine), bool(exp), threshold=0.01, device=DEV)
        r.Xi.data = Xi0.to(DEV)
        S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ae, generator=gen, regressor=r,
                                  **_train_kwargs(sym_reg_type="r", w_sym_reg=0.1, num_epochs=3, host_lbfgs=host, threshold=0.01,
                                                  torch_lbfgs=not kernels))
        out.append((r.Xi.detach().cpu().numpy(), r.mask.cpu().numpy()))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][1], out[2][1])
    # un-converged L-BFGS trajectories (fp32 host vs device arithmetic) after 3 epochs
    assert np.allclose(out[0][0], out[1][0], rtol=2e-2, atol=2e-3)
    assert np.allclose(out[0][0], out[2][0], rtol=2e-2, atol=2e-3)


def test_latent_branch_and_distillation_with_identity_autoencoder(S, golden, tmp_path, monkeypatch):
    """use_latent + distill_latent (train.py:647-661, 768-852) with ae_arch='none': z = x, dz = dx."""
    monkeypatch.chdir(tmp_path)
    g = golden("f4_lbfgs")
    x, dx = t(g["dosc_sindy_x"]), t(g["dosc_sindy_dx"])
    ae = S.autoencoder.AutoEncoder(ae_arch="none").to(DEV)
    gen = S.lie.LieGenerator(repr="(1,so2)", group_idx="0", device=DEV).to(DEV)
    r = S.SINDyRegression(2, 2, False, False, threshold=0.05, device=DEV)
    r_dst = S.SINDyRegression(2, 2, False, False, threshold=0.05, device=DEV)
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ae, generator=gen, regressor=r,
                              **_train_kwargs(use_latent=True, distill_latent=True, regressor_dst=r_dst, w_sindy_z=1.0,
                                              w_sindy_x=1.0, num_epochs=40, lr_sindy=0.1))
    want = torch.tensor(O.SINDY_TRUTH["dosc"] != 0)
    assert torch.equal(r.mask.cpu().bool(), want)
    assert torch.equal(r_dst.mask.cpu().bool(), want)
    assert np.allclose((r_dst.Xi * r_dst.mask).detach().cpu().numpy(), O.SINDY_TRUTH["dosc"], atol=5e-3)


def test_lbfgs_seed_sweep_on_gpu_matches_sequential_trainer(S, golden, tmp_path, monkeypatch):
    """S seeds optimised in lockstep on the batched closure == S sequential train_SIGED_lbfgs runs.
    (Equality is asserted on the well-conditioned damped-oscillator problem; on selkov -- cond 9e3, lr 1.0,
    no line search -- un-converged L-BFGS trajectories are chaotic in the last bits, so only the
    reference's own recorded run is pinned there.)"""
    monkeypatch.chdir(tmp_path)
    from symode_amd.batched import BatchedClosure
    from symode_amd.sweep import SeedSweepLBFGS
    g = golden("f4_lbfgs")
    ident = torch.nn.Identity()
    # selkov: seed 0 is the recorded reference run
    x, dx = t(g["selkov_sindy_x"]).to(DEV), t(g["selkov_sindy_dx"]).to(DEV)
    init = t(g["selkov_sindy_init_Xi"]).reshape(1, -1).to(DEV)
    out = SeedSweepLBFGS(BatchedClosure(x[None].contiguous(), dx[None].contiguous(), 3), 1.0, 0.075, 50).fit(init, 60)
    assert np.array_equal(out["mask"][0].cpu().numpy(), g["selkov_sindy_mask_final"])
    # dosc: six seeds against six sequential runs
    x, dx = t(g["dosc_sindy_x"]).to(DEV), t(g["dosc_sindy_dx"]).to(DEV)
    n_seeds = 6
    torch.manual_seed(5)
    inits = torch.cat([t(g["dosc_sindy_init_Xi"]).reshape(1, -1), torch.randn(n_seeds - 1, 20)]).to(DEV)
    X, DX = x[None].expand(n_seeds, -1, -1).contiguous(), dx[None].expand(n_seeds, -1, -1).contiguous()
    out = SeedSweepLBFGS(BatchedClosure(X, DX, 3), 0.1, 0.05, 50).fit(inits, 60)
    assert np.array_equal(out["mask"][0].cpu().numpy(), g["dosc_sindy_mask_final"])
    for s in range(n_seeds):
        r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
        r.Xi.data = inits[s].view(2, 10).clone()
        S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ident, generator=ident, regressor=r,
                                  **_train_kwargs(num_epochs=60, lr_sindy=0.1, threshold=0.05, st_freq=50))
        assert torch.equal(out["mask"][s], r.mask), s
        want = (r.Xi * r.mask).detach().cpu().numpy()
        assert np.allclose((out["Xi"][s] * out["mask"][s]).cpu().numpy(), want, rtol=5e-3, atol=5e-4), s


def test_lbfgs_direction_kernel_matches_torch_recursion(S):
    """Wave-per-problem two-loop recursion vs the masked torch loops, ring buffers wrapped, ragged history."""
    from symode_amd.sweep import BatchedLBFGS
    torch.manual_seed(0)
    for n, H in [(20, 100), (42, 100), (7, 16), (200, 8)]:
        Sn = 37
        P = torch.zeros(Sn, n, device=DEV)
        a = BatchedLBFGS(P, 1.0, history_size=H, engine=S.get_engine())
        a.old_dirs.normal_().mul_(0.5 / n ** 0.5)            # keep the 2H-step recursion well inside fp32 range
        a.old_stps.normal_().mul_(0.5 / n ** 0.5)
        a.ro.uniform_(0.1, 1.0)
        a.hist = torch.randint(0, H + 1, (Sn,), device=DEV)
        a.head = torch.randint(0, H, (Sn,), device=DEV)
        a.H_diag.uniform_(0.5, 2.0)
        g = torch.randn(Sn, n, device=DEV)
        got = a._direction(g)
        a.engine = None
        want = a._direction(g)
        assert torch.isfinite(want).all()
        assert torch.allclose(got, want, rtol=2e-4, atol=2e-4 * want.abs().max().item()), (n, H)


def test_fused_lbfgs_iteration_matches_the_tensor_op_form_and_torch(S, monkeypatch):
    """symode_lbfgs_step (the optimiser side of an inner iteration as one launch, a wave per problem) vs the
    same arithmetic in tensor ops (SYMODE_LBFGS_FUSED=0) and vs torch.optim.LBFGS per problem on the CPU, on convex
    quadratics: sizes that wrap the ring buffer (history 4), leave lanes idle (n = 7), use several components per lane
    (n = 150), problems that stop early (one starts at its optimum, one has a zero gradient direction)."""
    from symode_amd.sweep import BatchedLBFGS
    eng = S.get_engine()
    # (n, history): components per lane 1 (n <= 64), 2, 3, 4 of the LDS-staged recursion, and the unstaged form (150, 100)
    for n, H, Sn, lr, steps in [(7, 100, 6, 0.3, 4), (20, 4, 9, 0.2, 3), (150, 100, 5, 0.05, 2), (100, 20, 4, 0.05, 2),
                                (150, 8, 3, 0.05, 2), (256, 6, 3, 0.03, 2)]:
        torch.manual_seed(n)
        A = torch.randn(Sn, n, n) / n ** 0.5
        A = A @ A.transpose(1, 2) + 0.5 * torch.eye(n)
        b = torch.randn(Sn, n)
        P0 = torch.randn(Sn, n)
        P0[1] = torch.linalg.solve(A[1], b[1])                   # starts (numerically) at its optimum
        Ad, bd = A.to(DEV), b.to(DEV)

        def batched(Pm):
            AP = torch.einsum("sij,sj->si", Ad, Pm)
            return 0.5 * (Pm * AP).sum(1) - (bd * Pm).sum(1), AP - bd

        runs = {}
        for mode, fused in (("kernels", "1"), ("ops", "0")):
            monkeypatch.setenv("SYMODE_LBFGS_FUSED", fused)
            P = P0.to(DEV).clone()
            opt = BatchedLBFGS(P, lr, history_size=H, engine=eng)
            assert opt.fused == (fused == "1")
            losses = [opt.step(batched).cpu() for _ in range(steps)]
            runs[mode] = (P.cpu(), torch.stack(losses), opt.n_iter.cpu(), opt.hist.cpu(), opt.head.cpu())
        Pf, Lf, nf, hf, hdf = runs["kernels"]
        Pt, Lt, nt, ht, hdt = runs["ops"]
        # (where a problem converges to the last bit the stopping tests fire an iteration or two apart: only the problem
        # that starts at its optimum is pinned on its count)
        assert int(nf[1]) == int(nt[1]) and int(nf[1]) < 20 * steps, (n, nf, nt)
        assert (hf <= H).all() and (hdf < H).all() and (hf == torch.clamp(hf, 0, H)).all()
        assert torch.allclose(Lf, Lt, rtol=1e-4, atol=1e-5), n
        assert torch.allclose(Pf, Pt, rtol=2e-3, atol=2e-4), (n, (Pf - Pt).abs().max())
        ref = [P0[s].clone().requires_grad_(True) for s in range(Sn)]
        for s in range(Sn):
            o = torch.optim.LBFGS([ref[s]], lr=lr, history_size=H)

            def cl():
                o.zero_grad()
                l = 0.5 * ref[s] @ A[s] @ ref[s] - b[s] @ ref[s]
                l.backward()
                return l
            for _ in range(steps):
                o.step(cl)
        want = torch.stack([r.detach() for r in ref])
        assert torch.allclose(Pf, want, rtol=2e-3, atol=3e-4), (n, (Pf - want).abs().max())


def test_seed_sweep_with_fused_optimiser_kernels_equals_the_tensor_op_sweep(S, golden, monkeypatch):
    """SeedSweepLBFGS end to end, optimiser side as kernels (scale and L1 term formed by the optimiser launch, closure
    output consumed in place) vs SYMODE_LBFGS_FUSED=0: same masks, epochs and finished flags, coefficients
    to 2e-3 -- unconstrained with a scaled data term + L1 term, unconstrained unweighted, and the so(2)-constrained recorded run
    (beta | const layout).  Arm "1" is the default route, the device trainer (symode_trainer_run); arms "step graph" /
    "step eager" force the sweep's own kernel form (_native_ok -> False: BatchedLBFGS.step on symode_lbfgs_step with the
    bare data term, ``frozen`` = the seeds that finished earlier, the (closure, ACCEPT) body replayed from a HIP graph or
    not) and must give the trainer's bits; arm "0" is the tensor-op form."""
    from symode_amd.batched import BatchedClosure
    from symode_amd.sweep import SeedSweepLBFGS
    g = golden("f4_lbfgs")
    x, dx = t(g["dosc_sindy_x"]).to(DEV), t(g["dosc_sindy_dx"]).to(DEV)
    torch.manual_seed(3)
    inits = torch.cat([t(g["dosc_sindy_init_Xi"]).reshape(1, -1), torch.randn(5, 20)]).to(DEV)
    xe, dxe = t(g["dosc_esindy_x"]).to(DEV), t(g["dosc_esindy_dx"]).to(DEV)
    Q = t(g["dosc_esindy_Q"]).to(DEV)
    first = torch.cat([t(g["dosc_esindy_init_beta"]), t(g["dosc_esindy_init_const"]).reshape(-1)])[None]
    inits_e = torch.cat([first, torch.randn(3, Q.shape[1] + 2)]).to(DEV)

    def rep(v, n):
        return v[None].expand(n, -1, -1).contiguous()

    cases = [
        # the parser's default weights make lr 0.1 overshoot (the loss climbs from the second epoch on, either form): two
        # epochs pin the arithmetic of the L1 term, the long run uses a weight the iteration is stable with
        ("default weights", lambda: SeedSweepLBFGS(BatchedClosure(rep(x, 6), rep(dx, 6), 3), 0.1, 0.05, 50, w_sindy_x=0.1,
                                                    sindy_reg_type="l1", w_sindy_reg=0.1), inits, 2),
        ("weighted", lambda: SeedSweepLBFGS(BatchedClosure(rep(x, 6), rep(dx, 6), 3), 0.05, 0.05, 50, w_sindy_x=2.0,
                                             sindy_reg_type="l1", w_sindy_reg=1e-3), inits, 60),
        ("plain", lambda: SeedSweepLBFGS(BatchedClosure(rep(x, 6), rep(dx, 6), 3), 0.1, 0.05, 50), inits, 60),
        ("so2", lambda: SeedSweepLBFGS(BatchedClosure(rep(xe, 4), rep(dxe, 4), 2, Q=Q, use_kron_product=True, allow_constant=True),
                                       1.0, 0.01, 100), inits_e, 40),
    ]
    for name, make, P0, epochs in cases:
        out = {}
        for arm, fused, forced, graph in (("1", "1", False, "1"), ("step graph", "1", True, "1"), ("step eager", "1", True, "0"),
                                          ("0", "0", False, "1")):
            with monkeypatch.context() as mp:
                mp.setenv("SYMODE_LBFGS_FUSED", fused)
                mp.setenv("SYMODE_SWEEP_GRAPH", graph)
                if forced:
                    mp.setattr(SeedSweepLBFGS, "_native_ok", lambda self, P0: False)
                sw = make()
                out[arm] = sw.fit(P0, epochs)
                assert hasattr(sw, "trainer") == (arm == "1"), arm
        for arm in ("step graph", "step eager"):
            for k in ("mask", "params", "Xi", "epochs", "finished", "nan"):
                assert torch.equal(out["1"][k], out[arm][k]), (name, arm, k)
        if name in ("weighted", "plain"):    # seeds finish epochs apart: the later steps of the forced arms ran with frozen problems
            assert int(out["1"]["epochs"].min()) < int(out["1"]["epochs"].max()), (name, out["1"]["epochs"])
        a, b = out["1"], out["0"]
        assert torch.equal(a["mask"], b["mask"]), name
        assert torch.equal(a["finished"], b["finished"]) and torch.equal(a["nan"], b["nan"]), name
        if name != "weighted":               # (with the non-smooth L1 term the convergence test fires a few epochs apart)
            assert (a["epochs"] - b["epochs"]).abs().max() <= 1, (name, a["epochs"], b["epochs"])
        atol = 5e-3 if name == "weighted" else 2e-4       # (L1: coefficients jitter around the kink, |step| ~ lr * w_reg)
        assert torch.allclose(a["Xi"] * a["mask"], b["Xi"] * b["mask"], rtol=2e-3, atol=atol), (name, (a["Xi"] - b["Xi"]).abs().max())
    assert np.array_equal(out["1"]["mask"][0].cpu().numpy(), g["dosc_esindy_mask_final"])       # the reference's recorded run


def test_fused_euler_flow_matches_stepwise_tangent_flow_and_its_gradients(S):
    """symode_euler_jvp / _vjp (K steps in one launch) vs the step-by-step route (forward_and_jvp per step)."""
    from symode_amd import model_utils as MU
    torch.manual_seed(9)
    for d, order, sine, exp, K in [(2, 3, False, False, 10), (2, 2, False, True, 3), (3, 2, True, False, 5), (2, 5, False, False, 4)]:
        r = S.SINDyRegression(d, order, sine, exp, threshold=0.1, device=DEV)
        r.Xi.data *= 0.3
        r.mask = (torch.rand_like(r.mask) > 0.2).float()
        x, v = (torch.randn(400, d) * 0.5).to(DEV), torch.randn(400, d).to(DEV)
        c1, c2 = torch.randn(400, d).to(DEV), torch.randn(400, d).to(DEV)
        dt = 0.01
        flow = MU._EulerFlow(r, K * dt + 1e-9, dt)
        out = []
        for fused in (True, False):
            xg, vg = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
            r.Xi.grad = None
            if fused:
                fx, tv = flow.tangent(xg, vg)
            else:
                fx, tv = xg, vg
                for _ in range(K):
                    h, jv = r.forward_and_jvp(fx, tv)
                    fx, tv = fx + dt * h, tv + dt * jv
            ((fx * c1).sum() + (tv * c2).sum()).backward()
            out.append([t_.detach().cpu() for t_ in (fx, tv, xg.grad, vg.grad, r.Xi.grad)])
        for a, b, nm in zip(out[0], out[1], ["f(x)", "J_f v", "dx", "dv", "dXi"]):
            assert torch.allclose(a, b, rtol=2e-4, atol=2e-5 * max(b.abs().max().item(), 1e-6)), (d, order, nm)
        with torch.no_grad():
            assert torch.allclose(flow(x), out[0][0].to(DEV), rtol=1e-5, atol=1e-6)     # odeint kernel == fused flow


def test_caches_follow_the_tensor_object_not_its_address(S, golden):
    """Every epoch draws a new subsample (main.py:36-38) and the allocator hands the freed batch's address to the next one:
    the (g(x), J_g(x)) cache of the reversed regulariser and the Gram cache must key on the live tensor, not on data_ptr."""
    g = golden("f6_symreg")
    ae = load_fixture_autoencoder(g, "tanh_learn", "Tanh", DEV)
    gen = load_fixture_generator(g, "tanh_learn", "(2,1,2)", DEV)
    for p in list(ae.parameters()) + list(gen.parameters()):
        p.requires_grad = False
    r = S.SINDyRegression(2, 2, False, False, threshold=0.05, device=DEV)
    from torch.utils.dlpack import from_dlpack, to_dlpack
    torch.manual_seed(0)
    buf = (torch.randn(4096, 2) * 0.5).to(DEV)
    y1 = torch.randn(4096, 2).to(DEV)
    x1 = from_dlpack(to_dlpack(buf))                                # a tensor object of its own (fresh version counter) on buf's memory
    l1 = S.model_utils.symmreg_r(x1, ae, gen, h=r).item()
    G1 = r.aug_gram(x1, y1).copy()
    addr = x1.data_ptr()
    del x1
    buf.copy_((torch.randn(4096, 2) * 0.5 + 0.3).to(DEV))           # "the next epoch's subsample" lands at the same address
    x2 = from_dlpack(to_dlpack(buf))
    assert x2.data_ptr() == addr and x2._version == 0
    l2 = S.model_utils.symmreg_r(x2, ae, gen, h=r).item()
    S.model_utils._R_CACHE.clear()
    fresh = S.model_utils.symmreg_r(x2, ae, gen, h=r).item()
    assert l2 == fresh and l2 != l1
    G2 = r.aug_gram(x2, y1)
    assert not np.allclose(G1, G2) and np.allclose(G2, S.get_engine().aug_gram(x2, y1, 2, 0).cpu().numpy())


@pytest.mark.parametrize("tag,act,rep", [("relu_sim2", "ReLU", "(2,sim2)"), ("tanh_learn", "Tanh", "(2,1,2)")])
def test_constant_half_of_the_symmetry_regularisers_with_gradients(S, golden, tag, act, rep):
    """S2 / S3 closures with the x component of the autoencoder work cached per batch (x_const) against the all-at-once form:
    same loss, same dloss/dXi through the fused Euler tangent kernels."""
    MU = S.model_utils
    g = golden("f6_symreg")
    ae = load_fixture_autoencoder(g, tag, act, DEV)
    gen = load_fixture_generator(g, tag, rep, DEV)
    for p in list(ae.parameters()) + list(gen.parameters()):
        p.requires_grad = False
    d, order, sine, exp = [int(v) for v in g[f"{tag}_cfg"]]
    x = t(g[f"{tag}_x"]).to(DEV)[:256].contiguous()
    for kind, fn in (("i", MU.symmreg_i), ("f", MU.symmreg_f)):
        out = []
        for split in (False, True):
            r = S.SINDyRegression(d, order, bool(sine), bool(exp), threshold=0.05, device=DEV)
            r.Xi.data = t(g[f"{tag}_Xi"]).to(DEV)
            flow = MU._EulerFlow(r, 0.05, 0.01)
            x_fx = torch.stack([x, flow(x)], dim=1)
            loss = fn(x_fx, ae, gen, f=flow, require_grad=True, **({"x_const": x} if split else {}))
            loss.backward()
            out.append((loss.item(), r.Xi.grad.detach().cpu().clone()))
        assert out[1][0] == pytest.approx(out[0][0], rel=2e-5), kind
        assert (out[1][1] - out[0][1]).abs().max() <= 2e-4 * out[0][1].abs().max(), kind


@pytest.mark.parametrize("sym", ["i", "f"])
def test_host_resident_variables_for_autograd_closures(S, golden, sym, tmp_path, monkeypatch):
    """train_SIGED_lbfgs with the infinitesimal / finite regulariser: L-BFGS variables on the host (closure on the device,
    train._HostParams) vs on the device -- the same algorithm on the same closure: identical masks, close coefficients."""
    monkeypatch.chdir(tmp_path)
    g = golden("f6_symreg")
    tag, act, rep = "relu_sim2", "ReLU", "(2,sim2)"
    ae = load_fixture_autoencoder(g, tag, act, DEV)
    gen = load_fixture_generator(g, tag, rep, DEV)
    d, order, sine, exp = [int(v) for v in g[f"{tag}_cfg"]]
    x, Xi0 = t(g[f"{tag}_x"]), t(g[f"{tag}_Xi"])
    dx = O.forward(x, Xi0 * 0.5, torch.ones_like(Xi0), order, bool(sine), bool(exp)).detach()
    out = []
    for host in (True, False):
        r = S.SINDyRegression(d, order, bool(sine), bool(exp), threshold=0.05, device=DEV)
        r.Xi.data = Xi0.to(DEV)
        S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], autoencoder=ae, generator=gen, regressor=r,
                                  **_train_kwargs(sym_reg_type=sym, w_sym_reg=0.1, num_epochs=3, host_lbfgs=host))
        out.append((r.Xi.detach().cpu().numpy(), r.mask.cpu().numpy()))
    assert np.array_equal(out[0][1], out[1][1])
    assert np.allclose(out[0][0], out[1][0], rtol=2e-2, atol=2e-3)      # two un-converged fp32 L-BFGS trajectories (host vs device arithmetic)
