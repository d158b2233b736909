"""Transcripts of trainer runs (test infrastructure, not product code): what a fit prints, the keys of every
``wandb.log`` payload, the checkpoint names it writes and the coefficients it ends on.

The recordings under tests/golden/train_*_transcript.json are THIS project's own output, made at the commit before
train_SIGED_lbfgs was split into routes and builders -- not the reference's.  They pin the order and the text of the
per-epoch report across every route of the trainer.  tests/golden/main_sweep_*transcript.json are the same for the sweep
driver: main_sweep's own output at the commit before it was split into plan / fit / report."""
import contextlib
import io
import json
import os
import re

import numpy as np
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


# ---- main_sweep ------------------------------------------------------------------------------------------------------------
SWEEP_CPU_CASES = ("lbfgs", "lbfgs_ltp", "stlsq", "stlsq_ltp")
SWEEP_GPU_CASES = ("adam", "lv_stream", "lv_gram", "selkov_stream", "selkov_gram")
# integer, decimal and exponent forms: recorded on one machine and checked on another, the digits may differ; text, order and
# count of the lines may not (a sign after a digit is text: 'passes 1-2')
NUMBER = re.compile(r"(?:(?<!\d)[-+])?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")
DOSC_SMALL = (6, 3, 600, 3, 0.01)                            # 6 + 3 trajectories x 200 samples (test_host_ltp_sweep.py)


def mask_numbers(lines):
    return [NUMBER.sub("#", line) for line in lines]


def record_sweep(main_sweep, argv, workdir, save_dir, coefficients=False, **main_kw):
    """One ``main_sweep.main`` call in ``workdir``: masked stdout, the files under eval_results/<save_dir>/, every npz key with
    dtype and shape, correct_form per seed file (and the coefficients, for the GPU cases' tolerance)."""
    buf, cwd = io.StringIO(), os.getcwd()
    os.chdir(workdir)
    try:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        with contextlib.redirect_stdout(buf):
            main_sweep.main(list(argv) + ["--save_dir", save_dir], **main_kw)
    finally:
        os.chdir(cwd)
    out = os.path.join(workdir, "eval_results", save_dir)
    rec = {"stdout": mask_numbers(buf.getvalue().splitlines()), "files": sorted(os.listdir(out)), "npz": {}, "correct_form": {}}
    if coefficients:
        rec["coefficients"] = {}
    for name in rec["files"]:
        with np.load(os.path.join(out, name)) as z:
            rec["npz"][name] = {k: [str(z[k].dtype), list(z[k].shape)] for k in sorted(z.files)}
            rec["correct_form"][name] = z["correct_form"].tolist()
            if coefficients:
                rec["coefficients"][name] = z["coefficients"].tolist()
    return rec


def _small_dosc(run):
    from symode_amd import dataset as D
    old = D._RECIPES["dosc"], D.ode_dt_dict["dosc"]
    D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = DOSC_SMALL, 0.03
    try:
        return run()
    finally:
        D._RECIPES["dosc"], D.ode_dt_dict["dosc"] = old


def sweep_cpu_argv(case):
    """The set-up of test_main_sweep_eval_ltp_adds_its_keys_and_nothing_else_changes: small noise-free dosc, order 2, 4 seeds;
    ``lbfgs`` / ``stlsq``, with ``_ltp``: --eval_ltp."""
    argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--lbfgs_subsample", "0.5",
            "--lr_sindy", "0.1", "--w_sindy_x", "1.0", "--w_sindy_z", "0.0", "--w_sindy_reg", "0.0", "--w_sym_reg", "0.0",
            "--poly_order", "2", "--st_freq", "50", "--threshold", "5e-2", "--num_epochs", "60", "--gpu", "-1",
            "--n_seeds", "4", "--method", case.split("_")[0], "--seed", "0"]
    return argv + (["--eval_ltp", "--ltp_bound_rel", "0.01"] if case.endswith("_ltp") else [])


def run_sweep_cpu_case(case, workdir):
    """``sweep_cpu_argv(case)`` on the oracle engine, recorded."""
    from symode_amd import main_sweep
    from tests.test_host_ltp_sweep import LtpOracleEngine
    return _small_dosc(lambda: record_sweep(main_sweep, sweep_cpu_argv(case), str(workdir), case, engine=LtpOracleEngine()))


def run_sweep_gpu_case(case, workdir):
    """``adam``: the sweep of test_gpu_adam.py::test_main_sweep_adam_writes_every_seed_... (4 seeds); ``<task>_stream`` /
    ``<task>_gram``: the reversed-regulariser sweep of test_gpu_sym_sweep.py (its CASES, N_SEEDS) in ``workdir``, which must
    already hold that test's data files and LaLiGAN (its _prepare)."""
    from symode_amd import main_sweep
    if case == "adam":
        argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "adam", "--batch_size", "256",
                "--lr_sindy", "0.01", "--w_sindy_x", "1.0", "--w_sindy_z", "0.0", "--w_sindy_reg", "0.001", "--w_sym_reg", "0.0",
                "--poly_order", "2", "--st_freq", "2", "--threshold", "5e-2", "--num_epochs", "3", "--seed", "0", "--n_seeds", "4"]
        return _small_dosc(lambda: record_sweep(main_sweep, argv, str(workdir), case, coefficients=True))
    from tests.test_gpu_sym_sweep import CASES, N_SEEDS
    task, mode = case.split("_")
    argv = list(CASES[task][0]) + ["--n_seeds", str(N_SEEDS)] + (["--gram_closure"] if mode == "gram" else [])
    return record_sweep(main_sweep, argv, str(workdir), case, coefficients=True)


def record_sweep_gpu_cases(out_file):
    """Every GPU case in THIS process, in the order and from the state the golden file was recorded in: a fresh process, the
    Adam sweep first, each task's data files and LaLiGAN made just before its first sweep (the small LV and selkov fits
    amplify last-bit differences of g(x), J_g(x), and which GEMM kernels torch picks depends on what the process ran
    before).  Writes {case: record} as JSON."""
    import pathlib
    import shutil
    import tempfile
    from tests.test_gpu_sym_sweep import _prepare
    out, made = {}, {}
    for case in SWEEP_GPU_CASES:
        work = pathlib.Path(tempfile.mkdtemp())
        if case != "adam":
            task = case.split("_")[0]
            if task not in made:
                made[task] = pathlib.Path(tempfile.mkdtemp())
                _prepare(made[task], task)
            for sub in ("data", "saved_models"):
                shutil.copytree(made[task] / sub, work / sub)
        out[case] = run_sweep_gpu_case(case, work)
    with open(out_file, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":                                    # python -m tests.transcripts OUT.json
    import sys
    record_sweep_gpu_cases(sys.argv[1])
