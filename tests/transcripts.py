"""Transcripts of trainer runs (test infrastructure, not product code): what a fit prints, the keys of every
``wandb.log`` payload, the checkpoint names it writes and the coefficients it ends on.

The recordings under tests/golden/train_*_transcript.json are THIS project's own output, made at the commit before
train_SIGED_lbfgs was split into routes and builders -- not the reference's.  They pin the order and the text of the
per-epoch report across every route of the trainer."""
import contextlib
import io
import json
import os

import torch

from tests.helpers import load_fixture_autoencoder, load_fixture_generator, t

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPU_CASES = ("plain", "plain_i")
GPU_CASES = ("device", "device_r", "shadow_torch", "shadow_numpy", "host_params_f", "adam_r")


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _record(train, regressor, workdir, run):
    logged, buf, cwd, old = [], io.StringIO(), os.getcwd(), train.wandb.log
    train.wandb.log = lambda payload, *a, **k: logged.append(list(payload))
    os.chdir(workdir)
    try:
        with contextlib.redirect_stdout(buf):
            run()
    finally:
        os.chdir(cwd)
        train.wandb.log = old
    saved = os.path.join(workdir, "saved_models", "t")
    return {"stdout": buf.getvalue().splitlines(), "wandb_keys": logged,
            "files": sorted(os.listdir(saved)) if os.path.isdir(saved) else [],
            "params": [p.detach().cpu().tolist() for p in regressor.parameters()], "mask": regressor.mask.cpu().tolist()}


def _symmetry_fixture(golden, tag, dev):
    act, rep = {"relu_sim2": ("ReLU", "(2,sim2)"), "tanh_learn": ("Tanh", "(2,1,2)")}[tag]
    g = golden("f6_symreg")
    return load_fixture_autoencoder(g, tag, act, dev), load_fixture_generator(g, tag, rep, dev)


def run_case(S, golden, case, workdir, dev="cpu", engine=None):
    """One recorded configuration: the damped oscillator of f4_lbfgs (d = 2, order 3; every row on the CPU, the first 512
    on the GPU) with log, save and threshold intervals that all fall inside the run."""
    g = golden("f4_lbfgs")
    n = None if dev == "cpu" else 512
    x, dx = t(g["dosc_sindy_x"])[:n].contiguous(), t(g["dosc_sindy_dx"])[:n].contiguous()
    r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=dev, **({"engine": engine} if engine is not None else {}))
    r.Xi.data = t(g["dosc_sindy_init_Xi"]).to(dev)
    ae = gen = torch.nn.Identity()
    sym, w_sym, extra = "i", 0.0, {}
    if case in ("plain_i", "host_params_f"):
        ae, gen = _symmetry_fixture(golden, "relu_sim2", dev)
        sym, w_sym = case[-1], 0.1
    elif case in ("device_r", "adam_r"):
        ae, gen = _symmetry_fixture(golden, "tanh_learn", dev)
        sym, w_sym = "r", 0.1
    if case == "shadow_torch":
        extra = {"torch_lbfgs": True}
    elif case == "shadow_numpy":
        extra = {"numpy_lbfgs": True}
    common = dict(device=dev, save_dir="t", autoencoder=ae, generator=gen, regressor=r, use_latent=False, w_sindy_z=0.0,
                  w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=1e-3, sym_reg_type=sym, w_sym_reg=w_sym, st_freq=2,
                  threshold=0.05, int_t=0.03, int_dt=0.01, print_eq=True)
    if case == "adam_r":
        from symode_amd.dataset import DeviceBatches
        torch.manual_seed(0)                                     # the loader's shuffles
        train = DeviceBatches([x, dx], x.shape[0], 128, True, dev)
        test = DeviceBatches([x[:100], dx[:100]], 100, 64, False, dev)
        ident = torch.nn.Identity()

        def run():
            S.train.train_SIGED(train_loader=train, test_loader=test, num_epochs=2, log_interval=1, save_interval=2,
                                discriminator=ident, lr_ae=0, lr_d=0, lr_g=0, w_recon=0, w_gan=0, w_reg_norm=0, w_reg_ortho=0,
                                w_reg_closure=0, use_original_x=False, gan_st_freq=0, gan_st_thres=0.0, ae_arch="mlp",
                                lr_sindy=1e-2, device_adam=True, **common)
    else:
        def run():
            S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], test_loader=[(x, dx)] * 3, num_epochs=6, log_interval=2,
                                      save_interval=3, regressor_dst=None, distill_latent=False, lr_sindy=0.1, **extra, **common)
    return _record(S.train, r, str(workdir), run)
