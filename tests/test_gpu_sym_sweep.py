"""Seed sweep of the reversed-symmetry-regularised configs (EquivSINDy-r) in one process:

  * the gathered reversed-regulariser Gram (symode_symreg_reversed_gram_gather) against the dense launch on materialised
    rows (bit-equal) and an fp64 torch restatement, and its range check;
  * GramStatistics.add_gathered against add on per-seed copies;
  * main_sweep end to end on small LV / selkov sets with a frozen random LaLiGAN in the files main.py writes: the first
    closure per seed against the oracle, masks against single-problem fits on the same rows, stream == Gram mode, the
    per-seed result files; and two gloo ranks on one GPU against one rank, with exactly one all-reduce in Gram mode.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import sindy_oracle as O
from tests.helpers import only_compiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eng():
    import symode_amd
    return symode_amd.get_engine()


# ---- the kernel --------------------------------------------------------------------------------------------------------
LIBS = only_compiled([(2, 2, 2), (2, 3, 0), (1, 3, 0), (3, 2, 0), (2, 5, 0)])       # LV (exp), selkov, and around them


def _operands(d, n_g, n_src, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_src, d, generator=g) * 0.8
    gx = x[None] + 0.05 * torch.randn(n_g, n_src, d, generator=g)
    jgx = torch.eye(d)[None, None] + 0.1 * torch.randn(n_g, n_src, d, d, generator=g)
    return x.to(DEV), gx.contiguous().to(DEV), jgx.contiguous().to(DEV)


def _table(S, m, n_src, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_src, (S, m), generator=g, dtype=torch.int32)
    idx[:, 1] = idx[:, 0]                                   # repeated rows inside a problem ...
    idx[:, -1] = idx[:, m // 2]
    if S > 1:
        idx[1] = idx[0]                                     # ... and a problem repeating another
    return idx.to(DEV)


def _rev_gram_fp64(x, gx, jgx, order, flags):
    """sum_g sum_n B^T B in fp64 from the fp32 library (the kernel's own Theta, so the restatement isolates the sums)."""
    eng = _eng()
    d = x.shape[-1]
    th = eng.theta(x, order, flags).double()                          # (N, p)
    R = 0.0
    for k in range(gx.shape[0]):
        thg = eng.theta(gx[k].contiguous(), order, flags).double()
        B = jgx[k].double()[:, :, :, None] * th[:, None, None, :]     # (N, i, j, a)
        B = B - torch.eye(d, dtype=torch.float64, device=x.device)[None, :, :, None] * thg[:, None, None, :]
        B = B.reshape(x.shape[0] * d, -1)
        R = R + B.T @ B
    return R


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("n_g", [1, 3])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_gathered_reversed_gram_bit_equals_the_dense_launch_on_copies(lib, n_g, S):
    d, order, flags = lib
    eng = _eng()
    n_src, m = 900, 203                                      # m not a multiple of any stage (<= 64 items)
    x, gx, jgx = _operands(d, n_g, n_src, seed=d * 100 + order * 10 + n_g)
    idx = _table(S, m, n_src, seed=S)
    R = eng.symreg_reversed_gram_gather(x, gx, jgx, idx, order, flags)
    il = idx.long()
    xs = x[il].contiguous()                                  # (S, m, d)
    gxs = gx[:, il].transpose(0, 1).contiguous()             # (S, n_g, m, d)
    jgxs = jgx[:, il].transpose(0, 1).contiguous()           # (S, n_g, m, d, d)
    dense = eng.symreg_reversed_gram(xs, gxs, jgxs, order, flags)
    assert R.shape == dense.shape and R.dtype == torch.float64
    assert torch.equal(R, dense)
    for s in sorted({0, S // 2, S - 1}):
        want = _rev_gram_fp64(xs[s], gxs[s], jgxs[s], order, flags)
        err = (R[s] - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-12, (s, err)
    if S > 1:
        assert torch.equal(R[0], R[1])                       # identical tables give identical matrices


def test_gathered_reversed_gram_refuses_an_out_of_range_table():
    eng = _eng()
    x, gx, jgx = _operands(2, 2, 300, seed=5)
    for bad in (300, -1, 1 << 20):
        idx = _table(4, 50, 300, seed=1)
        idx[2, 17] = bad
        with pytest.raises(Exception, match="outside"):
            eng.symreg_reversed_gram_gather(x, gx, jgx, idx, 3, 0)
    # the table is checked on every call, whatever the engine has seen before
    idx = _table(4, 50, 300, seed=1)
    eng.symreg_reversed_gram_gather(x, gx, jgx, idx, 3, 0)
    idx[0, 0] = 300
    with pytest.raises(Exception, match="outside"):
        eng.symreg_reversed_gram_gather(x, gx, jgx, idx, 3, 0)


@pytest.mark.parametrize("lib", only_compiled([(2, 2, 2), (2, 3, 0)]))
def test_add_gathered_equals_add_on_per_seed_copies(lib):
    from symode_amd.gram_closure import GramStatistics
    d, order, flags = lib
    n_src, S, m, n_g = 1200, 9, 333, 2
    x, gx, jgx = _operands(d, n_g, n_src, seed=7)
    dx = (torch.randn(n_src, d, generator=torch.Generator().manual_seed(8))).to(DEV)
    idx = _table(S, m, n_src, seed=9)
    il = idx.long()
    a = GramStatistics(S, d, order, flags, regulariser=True, device=DEV).add_gathered(x, dx, idx, gx, jgx)
    b = GramStatistics(S, d, order, flags, regulariser=True, device=DEV).add(
        x[il].contiguous(), dx[il].contiguous(), gx[:, il].transpose(0, 1).contiguous(), jgx[:, il].transpose(0, 1).contiguous())
    assert a.count == b.count == m
    assert ((a.G - b.G).abs().max() / b.G.abs().max()).item() < 1e-12
    assert torch.equal(a.R, b.R)
    # statistics without R take the points alone; with R they refuse a chunk without g(x), J_g(x)
    c = GramStatistics(S, d, order, flags, device=DEV).add_gathered(x, dx, idx)
    assert torch.equal(c.G, a.G) and c.R is None
    with pytest.raises(Exception, match="gx and jgx"):
        GramStatistics(S, d, order, flags, regulariser=True, device=DEV).add_gathered(x, dx, idx)


# ---- main_sweep end to end -------------------------------------------------------------------------------------------------
COMMON = ["--noise", "0.2", "--smoothing", "gp", "--sindy_optimizer", "lbfgs", "--w_sindy_z", "0.0", "--w_sindy_x", "1.0",
          "--w_sindy_reg", "0.0", "--sym_reg_type", "r", "--w_sym_reg", "0.1", "--latent_dim", "2", "--n_comps", "2",
          "--fix_laligan", "--ae_arch", "mlp", "--ortho_ae", "--batch_norm", "--group_idx", "0", "--seed", "0"]
CASES = {
    # small LV (lv/noise99_eq_rsymreg.cfg's model and library): 20 x 1000 steps, 5 % per seed
    "lv": (COMMON + ["--task", "lv", "--hidden_dim", "64", "--n_layers", "3", "--repr", "(2,1,2)", "--include_exp",
                     "--num_epochs", "100", "--lr_sindy", "0.1", "--st_freq", "100", "--threshold", "0.15",
                     "--lbfgs_subsample", "0.05", "--load_laligan", "laligan-lv"], (20, 2, 1000, 1, 0.002)),
    # small selkov (selkov/noise20_eq_symreg3.cfg: order 3, sim(2), 200 epochs): 10 x 2000 steps, 50 % per seed
    "selkov": (COMMON + ["--task", "selkov", "--hidden_dim", "32", "--n_layers", "4", "--repr", "(2,sim2)", "--poly_order",
                         "3", "--num_epochs", "200", "--lr_sindy", "1.0", "--st_freq", "50", "--threshold", "0.075",
                         "--lbfgs_subsample", "0.5", "--load_laligan", "laligan-selkov"], (10, 2, 2000, 1, 0.002)),
}
N_SEEDS = 8


def _prepare(tmp_path, case):
    """Data files and a frozen random LaLiGAN (batch-norm statistics warmed on the data) in the files main.py writes."""
    from symode_amd import dataset as D
    from symode_amd.autoencoder import AutoEncoder
    from symode_amd.lie import LieGenerator
    from symode_amd.parser_utils import get_args
    argv, recipe = CASES[case]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        task = argv[argv.index("--task") + 1]
        old = D._RECIPES[task]
        D._RECIPES[task] = recipe
        try:
            args = vars(get_args(argv=list(argv)))
            tr, _, args = D.get_dataset(args)
        finally:
            D._RECIPES[task] = old
        torch.manual_seed(11)
        ae = AutoEncoder(**args).to(DEV)
        gen = LieGenerator(**args).to(DEV)
        x, dx = tr.x.to(DEV), tr.dx.to(DEV)
        ae.train()
        with torch.no_grad():
            for k in range(4):
                ae(torch.stack([x[k::4], x[k::4] + 0.1 * dx[k::4]], dim=1))
        name = args["load_laligan"]
        out = tmp_path / "saved_models" / name
        out.mkdir(parents=True)
        torch.save(ae.state_dict(), out / "autoencoder.pt")
        torch.save(gen.state_dict(), out / "generator.pt")
        torch.save(gen.masks, out / "generator_mask.pt")
    finally:
        os.chdir(cwd)
    return args


def _run_sweep(tmp_path, case, save_dir, extra=()):
    """main_sweep in ``tmp_path`` with SeedSweepLBFGS.fit recorded: (aggregate, sweep, P0, fit output)."""
    from symode_amd import main_sweep
    from symode_amd.sweep import SeedSweepLBFGS
    rec = {}
    orig = SeedSweepLBFGS.fit

    def fit(self, P0, num_epochs, mask0=None, on_epoch=None):
        out = orig(self, P0, num_epochs, mask0, on_epoch)
        rec.update(sweep=self, P0=P0.clone(), out={k: v.clone() for k, v in out.items()})
        return out

    cwd = os.getcwd()
    os.chdir(tmp_path)
    SeedSweepLBFGS.fit = fit
    try:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        agg = main_sweep.main(list(CASES[case][0]) + ["--n_seeds", str(N_SEEDS), "--save_dir", save_dir] + list(extra))
    finally:
        SeedSweepLBFGS.fit = orig
        os.chdir(cwd)
    return agg, rec["sweep"], rec["P0"], rec["out"]


def _frozen(tmp_path, args):
    from symode_amd.main_sweep import _load_laligan
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        return _load_laligan(dict(args), torch.device(DEV))
    finally:
        os.chdir(cwd)


@pytest.fixture(scope="module", params=list(CASES))
def swept(request, tmp_path_factory):
    case = request.param
    tmp = tmp_path_factory.mktemp(f"sym-sweep-{case}")
    args = _prepare(tmp, case)
    stream = _run_sweep(tmp, case, f"{case}-stream")
    gram = _run_sweep(tmp, case, f"{case}-gram", ["--gram_closure"])
    return case, tmp, args, stream, gram


def _seed_rows(args, tmp):
    from symode_amd import dataset as D
    from symode_amd.sweep import seeded_subsamples
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        tr, _, _ = D.get_dataset(dict(args))
    finally:
        os.chdir(cwd)
    x, dx = tr.x.to(DEV), tr.dx.to(DEV)
    m = int(x.shape[0] * args["lbfgs_subsample"])
    return x, dx, seeded_subsamples(x.shape[0], m, list(range(N_SEEDS)), DEV)


def test_first_closure_per_seed_equals_the_oracle(swept):
    case, tmp, args, stream, gram = swept
    ae, gen = _frozen(tmp, args)
    x_all, dx_all, rows = _seed_rows(args, tmp)
    gel = gen.get_deterministic_group_elems(scale=0.01)
    zm = ae.encoder[-2].bias
    for mode, (_, sweep, P0, _) in (("stream", stream), ("gram", gram)):
        c = sweep.c
        S, d, p = c.S, c.d, c.p
        loss, gxi, _ = c.evaluate(P0.view(S, d, p).contiguous(), None, mask=None)
        for s in (0, 3, 7):
            xs, dxs = x_all[rows[s]], dx_all[rows[s]]
            with torch.no_grad():
                gx, jgx = O.precompute_group_jacobians(xs, ae.encode, ae.decode, zm, gel)
            xc, dxc = xs.cpu(), dxs.cpu()
            reg = O.OracleRegressor(d, args["poly_order"], args["include_sine"], args["include_exp"],
                                    Xi0=P0[s].view(d, p).cpu())
            want = torch.nn.functional.mse_loss(reg(xc), dxc) + \
                args["w_sym_reg"] * O.symreg_reversed_precomputed(xc, [g.cpu() for g in gx], [j.cpu() for j in jgx], reg)
            want.backward()
            assert np.isclose(loss[s].item(), want.item(), rtol=1e-5), (case, mode, s, loss[s].item(), want.item())
            gw = reg.Xi.grad
            err = (gxi[s].cpu() - gw).abs().max().item() / gw.abs().max().item()
            assert err < 1e-5, (case, mode, s, err)


def _exact_modes(case, stream, gram):
    """The modes whose masks must equal the single-problem stream fit.  The small selkov set's order-3 fit is ill-conditioned
    (a limit cycle, nearly every term kept): there the fp64 Gram closure and the fp32 stream closure may take a different
    thresholding decision on a coefficient that passes the threshold late in the fit, so the Gram sweep is held to its
    first closure (test above) and to finishing every seed; the LV set pins both modes exactly."""
    return (("stream", stream), ("gram", gram)) if case == "lv" else (("stream", stream),)


def test_masks_equal_single_problem_fits_on_the_same_rows(swept):
    from symode_amd.device_lbfgs import DeviceTrainer
    from symode_amd.model_utils import precompute_symmreg_r
    case, tmp, args, stream, gram = swept
    ae, gen = _frozen(tmp, args)
    x_all, dx_all, rows = _seed_rows(args, tmp)
    _, sweep, P0, out = stream
    c = sweep.c
    for mode, res in (("stream", stream), ("gram", gram)):
        assert bool(res[3]["finished"].all()), (case, mode, res[3]["epochs"].tolist())     # every seed stopped in its ball
    for s in (0, 3, 7):
        xs, dxs = x_all[rows[s]].contiguous(), dx_all[rows[s]].contiguous()
        gx, jgx = precompute_symmreg_r(xs, ae, gen, scale=0.01)
        gx, jgx = torch.stack(gx)[None].contiguous(), torch.stack(jgx)[None].contiguous()
        tr = DeviceTrainer(xs[None], dxs[None], c.order, c.flags, reversed_sym=(gx, jgx, args["w_sym_reg"] / args["w_sindy_x"]),
                           lr=args["lr_sindy"], threshold=args["threshold"], st_freq=args["st_freq"], w_x=args["w_sindy_x"],
                           w_reg=0.0, l1=True, tol=1e-3, engine=c.engine)
        one = tr.fit(P0[s:s + 1].clone(), args["num_epochs"])
        want_mask = one["mask"].view(c.d, c.p).cpu()
        want_xi = one["Xi"].view(c.d, c.p).cpu()
        for mode, (_, _, _, o) in _exact_modes(case, stream, gram):
            assert torch.equal(o["mask"][s].view(c.d, c.p).cpu().bool(), want_mask.bool()), (case, mode, s)
            scale = max(1.0, want_xi.abs().max().item())
            got = (o["Xi"][s].view(c.d, c.p).cpu() * want_mask)
            assert (got - want_xi * want_mask).abs().max().item() < 1e-3 * scale, (case, mode, s)


def test_stream_and_gram_modes_give_the_same_masks_and_write_the_seed_files(swept):
    from symode_amd.evaluation import aggregate_results
    case, tmp, args, stream, gram = swept
    if case == "lv":
        assert torch.equal(stream[3]["mask"].cpu(), gram[3]["mask"].cpu())
    assert gram[1].statistics is not None and not hasattr(gram[1].c, "x")       # the Gram sweep held no per-seed points
    for mode, res in (("stream", stream), ("gram", gram)):
        assert res[0] is not None
        d = tmp / "eval_results" / f"{case}-{mode}"
        assert sorted(f.name for f in d.iterdir()) == sorted(f"seed{s}.npz" for s in range(N_SEEDS))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            assert aggregate_results(f"{case}-{mode}", min_seed=0, max_seed=N_SEEDS) is not None
        finally:
            os.chdir(cwd)
        coef = np.stack([np.load(d / f"seed{s}.npz")["coefficients"] for s in range(N_SEEDS)])
        assert np.array_equal(coef != 0, res[3]["mask"].cpu().numpy().astype(bool) & (res[3]["Xi"].cpu().numpy() != 0))


# ---- two ranks on one GPU (gloo) -------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, cwd, argv, count_file):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.chdir(cwd)
    import torch.distributed as dist
    import symode_amd  # noqa: F401
    from symode_amd import main_sweep
    calls = [0]
    orig = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    dist.all_reduce = counted
    try:
        res = main_sweep.main(list(argv), backend="gloo", one_gpu=True)
    finally:
        dist.all_reduce = orig
    assert (res is None) == (rank != 0)
    with open(f"{count_file}.{rank}", "w") as f:
        f.write(str(calls[0]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_rank_with_one_all_reduce_in_gram_mode(tmp_path):
    case = "lv"
    _prepare(tmp_path, case)
    base = list(CASES[case][0]) + ["--n_seeds", str(N_SEEDS)]

    def coefs(save_dir):
        d = tmp_path / "eval_results" / save_dir
        return np.stack([np.load(d / f"seed{s}.npz")["coefficients"] for s in range(N_SEEDS)])

    for mode, extra in (("gram", ["--gram_closure"]), ("stream", [])):
        _run_sweep(tmp_path, case, f"one-{mode}", extra)
        argv = base + ["--save_dir", f"two-{mode}"] + extra
        cnt = str(tmp_path / f"allreduce-{mode}")
        mp.spawn(_rank, args=(2, _free_port(), str(tmp_path), argv, cnt), nprocs=2, join=True)
        one, two = coefs(f"one-{mode}"), coefs(f"two-{mode}")
        assert np.array_equal(one != 0, two != 0), mode
        assert np.allclose(one, two, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(one).max())), mode
        counts = [int(open(f"{cnt}.{r}").read()) for r in range(2)]
        if mode == "gram":
            assert counts == [1, 1], counts                    # ONE collective of [G | R | count] per rank and fit
        else:
            assert min(counts) > 1                              # the stream closure all-reduces [loss | grad] per evaluation
