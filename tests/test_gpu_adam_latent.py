"""train_SIGED(use_latent=True, device_adam=True) against train_SIGED(use_latent=True) -- the tensor-op loop, one Python
iteration per minibatch -- at the same commit, on the same ``randperm`` draws: a seeded small autoencoder in eval mode
(mlp, hidden 16, 2 layers, batch norm), frozen; one so2 generator; 600 rows in batches of 256 (two full batches and one of
88), 4 epochs with a thresholding event after the second and the fourth.

The yardstick is the fp64 model of tests/adam_latent_model.py run over the whole trajectory on the fp32 operands the
device route reads: the tensor-op route's distance from that trajectory is the reference figure, the device route may be
at most 4 x that far and never needs to be closer than the step tolerance on ``params`` (tests/adam_latent_cases.py)."""
import os

import numpy as np
import pytest
import torch

from tests import adam_cases
from tests import adam_latent_cases as C
from tests import adam_latent_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, BATCH, EPOCHS, ST_FREQ, SAVE = 600, 256, 4, 2, 2
LR, W_Z, W_X, W_SYM, W_REG, THR = 1e-2, 0.7, 0.4, 2e-3, 1e-3, 0.1
SEED = 77


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd


class _So2(torch.nn.Module):
    """The generator as train_SIGED's latent branch reads it: a basis list with the one so(2) element."""

    def get_full_basis_list(self):
        return [torch.tensor([[0.0, -1.0], [1.0, 0.0]], device=DEV)]


def _setup(D):
    from symode_amd.autoencoder import AutoEncoder
    g = torch.Generator().manual_seed(40 + D)
    f = adam_cases.field(2)
    mix = torch.randn(2, D, generator=g) if D > 2 else torch.eye(2)
    x = (f["x"] @ mix + (0.1 * torch.sin(f["x"] @ mix) if D > 2 else 0.0)).contiguous().to(DEV)
    dx = (f["dx"] @ mix).contiguous().to(DEV)
    torch.manual_seed(11 + D)
    ae = AutoEncoder(ae_arch="mlp", input_dim=D, latent_dim=2, hidden_dim=16, n_layers=2, n_comps=1, batch_norm=True,
                     activation="ReLU").to(DEV)
    ae.train()
    with torch.no_grad():                                     # batch-norm statistics warmed on the data
        for k in range(4):
            ae(x[k::4])
    ae.eval()
    for q in ae.parameters():
        q.requires_grad = False
    return x, dx, ae


def _regressor(S):
    torch.manual_seed(123)
    reg = S.SINDyRegression(2, 3, False, False, threshold=THR, device=DEV)
    with torch.no_grad():
        reg.Xi.mul_(0.3)
    return reg


def _run(S, x, dx, ae, capsys, save_dir, **kw):
    from symode_amd.dataset import DeviceBatches
    reg = _regressor(S)
    loader = DeviceBatches([x, dx], N, BATCH, True, DEV)
    ident = torch.nn.Identity()
    torch.manual_seed(SEED)
    capsys.readouterr()
    S.train.train_SIGED(train_loader=loader, test_loader=[], num_epochs=EPOCHS, device=DEV, log_interval=1, save_interval=SAVE,
                        save_dir=save_dir, autoencoder=ae, discriminator=ident, generator=_So2(), lr_ae=0, lr_d=0, lr_g=0, w_recon=0,
                        w_gan=0, w_reg_norm=0, w_reg_ortho=0, w_reg_closure=0, use_original_x=False, gan_st_freq=0, gan_st_thres=0.0,
                        ae_arch="mlp", regressor=reg, use_latent=True, lr_sindy=LR, w_sindy_z=W_Z, w_sindy_x=W_X, sindy_reg_type="l1",
                        w_sindy_reg=W_REG, w_sym_reg=W_SYM, sym_reg_type="i", st_freq=ST_FREQ, threshold=THR, int_t=0.1, int_dt=0.01,
                        print_eq=False, **kw)
    out = capsys.readouterr().out
    rng = torch.rand(1, device=DEV).item()                    # where the generator stands after the run
    lines = [l for l in out.splitlines() if l.startswith("Epoch") and "loss_sindy_z" in l]
    assert not [l for l in out.splitlines() if "test_loss" in l]
    return reg, lines, rng, sorted(os.listdir(f"saved_models/{save_dir}"))


def _numbers(line):
    return {k.strip(): float(v) for k, v in (part.split(": ") for part in line.split(", ")[1:])}


def _model_trajectory(S, x, dx, ae, D):
    """The fp64 model over the four epochs on the operands of the device route, with the loader's own shuffles.  Returns the
    final state, per event (|Xi| of the live coefficients before it, mask after it), the epoch means and the generator's place."""
    from symode_amd.dataset import DeviceBatches
    from symode_amd.model_utils import latent_operands
    from symode_amd.sindy import NEAR_THRESHOLD_BAND
    z, dz, B, y, e, _ = latent_operands(x, dx, ae, per_row=True)
    data = dict(z=z.cpu(), dz=dz.cpu(), B=B.cpu(), y=y.cpu(), e=e.cpu() if D > 2 else None, L=_So2().get_full_basis_list()[0].cpu()[None])
    cfg = M.make_cfg(2, 3, 0, w_z=W_Z, D_obs=D, n_gen=1, lr=LR, w_x=W_X, w_reg=W_REG, w_sym=W_SYM, threshold=THR, st_freq=ST_FREQ,
                     near_band=NEAR_THRESHOLD_BAND)
    reg = _regressor(S)
    st = dict(params=reg.Xi.detach().cpu().double().reshape(-1), m=torch.zeros(20, dtype=torch.float64), v=torch.zeros(20, dtype=torch.float64),
              mask=reg.mask.detach().cpu().double().reshape(-1), step=0)
    loader = DeviceBatches([x, dx], N, BATCH, True, DEV)
    torch.manual_seed(SEED)
    orders = [loader.epoch_order().cpu() for _ in range(EPOCHS)]
    rng = torch.rand(1, device=DEV).item()
    events, means = [], []
    for epoch, order in enumerate(orders):
        recs = []
        for lo in range(0, N, BATCH):
            st, rec = M.step(st, order[lo:lo + BATCH], data, cfg)
            recs.append(rec)
        live = st["params"].abs()[st["mask"] > 0].clone()   # a coefficient that is already off stays off wherever it drifts
        st, ev, _ = M.epoch_end(st, st["params"], cfg, epoch)
        if ev["event"]:
            events.append((live, st["mask"].clone()))
        means.append({k: float(np.mean([float(r[k]) for r in recs])) for k in ("mse_z", "mse_x", "sym", "l1")})
    return st, events, means, rng


def _dist(reg, st):
    want = st["params"] * st["mask"]
    got = (reg.Xi.detach() * reg.mask).cpu().double().reshape(-1)
    return float((got - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("D", [2, 4])
def test_train_SIGED_use_latent_on_the_device_against_the_tensor_op_loop(S, D, capsys, tmp_path, monkeypatch):
    from symode_amd.sindy import NEAR_THRESHOLD_BAND
    monkeypatch.chdir(tmp_path)
    x, dx, ae = _setup(D)
    st, events, means, rng64 = _model_trajectory(S, x, dx, ae, D)
    # the fp64 trajectory alone decides both events away from the threshold, and they remove some coefficients, not all
    assert len(events) == 2
    for before, mask_after in events:
        assert float((before - THR).abs().min()) >= NEAR_THRESHOLD_BAND, (before - THR).abs().min()
    assert 0 < int((st["mask"] == 0).sum()) < st["mask"].numel()
    ref, ref_lines, ref_rng, ref_saved = _run(S, x, dx, ae, capsys, "ref")
    got, got_lines, got_rng, got_saved = _run(S, x, dx, ae, capsys, "dev", device_adam=True)
    assert ref_rng == got_rng == rng64                                           # the same shuffles, three times
    want_mask = st["mask"].reshape(2, 10)
    assert torch.equal(ref.mask.cpu().double(), want_mask) and torch.equal(got.mask.cpu().double(), want_mask)
    d_ref, d_got = _dist(ref, st), _dist(got, st)
    print(f"D={D}: distance from the fp64 trajectory, tensor-op route {d_ref:.3e}, device route {d_got:.3e} "
          f"(bound max(4 x {d_ref:.3e}, {C.TOL['params']:.1e}))")
    assert d_got <= max(4.0 * d_ref, C.TOL["params"]), (d_got, d_ref)
    # the printed epoch lines: the same keys in the same order, every number to the four printed decimals
    assert len(ref_lines) == len(got_lines) == EPOCHS
    for epoch, (a, b, m) in enumerate(zip(ref_lines, got_lines, means)):
        na, nb = _numbers(a), _numbers(b)
        assert list(na) == list(nb) == ["loss_sindy_x", "loss_sindy_z", "loss_sindy_reg", "loss_sym_reg"] and a.split(",")[0] == b.split(",")[0]
        print(f"  epoch {epoch}: tensor-op {a} | device {b}")
        for k, mk in (("loss_sindy_x", "mse_x"), ("loss_sindy_z", "mse_z"), ("loss_sindy_reg", "l1"), ("loss_sym_reg", "sym")):
            assert abs(na[k] - nb[k]) <= 1.0001e-4, (epoch, k, na[k], nb[k])           # one unit of the last printed place
            assert abs(nb[k] - m[mk]) <= 1.5e-4, (epoch, k, nb[k], m[mk])
        assert nb["loss_sym_reg"] > 0 and nb["loss_sindy_x"] > 0
    assert ref_saved == got_saved == [f"regressor_{e}.pt" for e in range(EPOCHS) if (e + 1) % SAVE == 0]
