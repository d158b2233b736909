"""Seed sweep of the reversed-symmetry-regularised configs: what one process for all seeds costs against the per-seed loop.

    python tests/perf/sym_sweep.py [--out profiles/r05_sym_sweep.json] [--seeds 64] [--skip-sweep]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/perf/sym_sweep.py --kernels-only     (kernel times, own run)

Set-up: LV at the config size (200 x 10^4 steps, noise 0.99, 1 % per seed) and selkov (10 x 10^4 steps, noise 0.2, 50 % per
seed), each with a frozen random LaLiGAN built as tests/helpers.make_config2 builds one, written where main.py reads it.
Recorded per task: the one-time g / J_g precompute over the rows the seeds use; the gathered reversed-Gram launch against the
dense launch on materialised copies of the same rows (event times; the --kernels-only run repeats just these launches for a
kernel trace); main_sweep's wall time in stream and Gram mode; 4 single-seed main.py fits in one process (each pays data
load, LaLiGAN load, its own precompute and its fit) and one cold ``python -m symode_amd.main`` start.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import symode_amd  # noqa: E402
from symode_amd import dataset as D  # noqa: E402
from symode_amd.parser_utils import get_args, parse_config  # noqa: E402

CONFIGS = {"lv": "lv/noise99_eq_rsymreg.cfg", "selkov": "selkov/noise20_eq_symreg3.cfg"}
CFG_DIR = os.path.join(ROOT, "symmetry-ode-discovery_amd", "run_configs")


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _argv(task, name, save_dir):
    toks = parse_config(os.path.join(CFG_DIR, CONFIGS[task]))
    toks[toks.index("--load_laligan") + 1] = name
    toks[toks.index("--save_dir") + 1] = save_dir
    for flag in ("--log_interval", "--save_interval"):                    # no per-epoch checkpoint files in a timing run
        toks[toks.index(flag) + 1] = "0"
    return [t for t in toks if t != "--print_eq"]


def _laligan(task, args, x, dx):
    """Frozen random autoencoder + generator, batch-norm statistics warmed on the data (tests/helpers.make_config2)."""
    from symode_amd.autoencoder import AutoEncoder
    from symode_amd.lie import LieGenerator
    torch.manual_seed(11)
    ae = AutoEncoder(**args).cuda()
    gen = LieGenerator(**args).cuda()
    ae.train()
    sel = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(0))[:20000].cuda()
    xs, dxs = x[sel], dx[sel]
    with torch.no_grad():
        for k in range(4):
            ae(torch.stack([xs[k::4], xs[k::4] + 0.1 * dxs[k::4]], dim=1))
    ae.eval()
    gen.eval()
    out = os.path.join("saved_models", args["load_laligan"])
    os.makedirs(out, exist_ok=True)
    torch.save(ae.state_dict(), f"{out}/autoencoder.pt")
    torch.save(gen.state_dict(), f"{out}/generator.pt")
    torch.save(gen.masks, f"{out}/generator_mask.pt")


def _launch_pair(x_used, gx, jgx, table, order, flags, reps=20):
    """(gathered ms, dense ms) per launch, best of ``reps``, plus whether the two are bit-equal."""
    eng = symode_amd.get_engine()
    il = table.long()
    xs = x_used[il].contiguous()
    gxs, jgxs = gx[:, il].transpose(0, 1).contiguous(), jgx[:, il].transpose(0, 1).contiguous()
    best = {}
    for name, fn in (("gather", lambda: eng.symreg_reversed_gram_gather(x_used, gx, jgx, table, order, flags)),
                     ("dense", lambda: eng.symreg_reversed_gram(xs, gxs, jgxs, order, flags))):
        fn()
        t = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        best[name] = (min(t), out)
    equal = bool(torch.equal(best["gather"][1], best["dense"][1]))
    return best["gather"][0], best["dense"][0], equal


def run_task(task, n_seeds, kernels_only, skip_sweep):
    from symode_amd.main_sweep import _load_laligan, symmetry_operands
    from symode_amd.sweep import seeded_subsamples
    name = f"perf-laligan-{task}"
    argv = _argv(task, name, f"perf-{task}")
    args = vars(get_args(argv=list(argv)))
    t0 = time.perf_counter()
    tr, _, args = D.get_dataset(args)
    t_data = time.perf_counter() - t0
    x, dx = tr.x.cuda(), tr.dx.cuda()
    if not os.path.exists(os.path.join("saved_models", name, "generator_mask.pt")):
        _laligan(task, args, x, dx)
    ae, gen = _load_laligan(args, torch.device("cuda"))
    m = int(x.shape[0] * args["lbfgs_subsample"])
    rows = seeded_subsamples(x.shape[0], m, list(range(n_seeds)), "cuda")
    symmetry_operands(x[:4096], rows[:1, :16] % 4096, ae, gen)          # warm-up (kernels, allocator)
    t0 = _sync()
    x_used, gx, jgx, table, used = symmetry_operands(x, rows, ae, gen)
    t_pre = _sync() - t0
    flags = symode_amd.engine.library_flags(args["include_sine"], args["include_exp"])
    g_ms, d_ms, equal = _launch_pair(x_used, gx, jgx, table, args["poly_order"], flags)
    rec = {"config": CONFIGS[task], "n_rows": int(x.shape[0]), "seeds": n_seeds, "rows_per_seed": m,
           "rows_used": int(used.numel()), "n_g": int(gx.shape[0]), "d_p": int(gx.shape[-1]) * symode_amd.get_engine().lib_size(
               int(gx.shape[-1]), args["poly_order"], flags),
           "data_load_s": round(t_data, 3), "precompute_gJg_s": round(t_pre, 4),
           "rev_gram_gather_ms": round(g_ms, 4), "rev_gram_dense_ms": round(d_ms, 4),
           "gather_over_dense": round(g_ms / d_ms, 3), "gather_bit_equal_dense": equal}
    if kernels_only or skip_sweep:
        return rec
    from symode_amd import main_sweep
    for mode, extra in (("stream", []), ("gram", ["--gram_closure"])):
        main_sweep.main(argv + ["--n_seeds", "2", "--save_dir", f"perf-{task}-warm"] + extra)   # code objects, allocator
        t0 = _sync()
        main_sweep.main(argv + ["--n_seeds", str(n_seeds), "--save_dir", f"perf-{task}-{mode}"] + extra)
        rec[f"sweep_{mode}_s"] = round(_sync() - t0, 3)
    from symode_amd import main as M
    times = []
    for s in range(4):
        t0 = _sync()
        M.main(argv + ["--seed", str(s), "--save_dir", f"perf-{task}-seed"])
        times.append(round(_sync() - t0, 3))
    rec["single_seed_in_process_s"] = times
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    subprocess.run([sys.executable, "-m", "symode_amd.main", "--seed", "0", "--save_dir", f"perf-{task}-cold"] + argv[:],
                   check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)
    rec["cold_process_s"] = round(time.perf_counter() - t0, 3)
    rec["per_seed_loop_estimate_50_s"] = round(50 * rec["cold_process_s"], 1)
    rec["sweep_stream_over_one_process"] = round(rec["sweep_stream_s"] / rec["cold_process_s"], 2)
    rec["sweep_gram_over_one_process"] = round(rec["sweep_gram_s"] / rec["cold_process_s"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--tasks", default="lv,selkov")
    ap.add_argument("--workdir", default=None, help="data / saved_models / eval_results go here (default: a temp dir)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--skip-sweep", action="store_true")
    a = ap.parse_args()
    out = os.path.abspath(a.out) if a.out else None
    work = a.workdir or tempfile.mkdtemp(prefix="sym_sweep_")
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    res = {"device": torch.cuda.get_device_name(0), "tasks": {}}
    for task in a.tasks.split(","):
        res["tasks"][task] = run_task(task, a.seeds, a.kernels_only, a.skip_sweep)
        print(json.dumps({task: res["tasks"][task]}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
