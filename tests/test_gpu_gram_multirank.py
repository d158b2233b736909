"""The Gram-form fit on point shards: two processes through the HIP engine on the one GPU, gloo collectives.  The ranks
accumulate [G | R | count] of their shard, sum it in ONE all-reduce when the trainer is built and then fit without any
collective: both ranks end on the identical Xi and mask, equal to the one-rank Gram fit's up to the fp64 summation order."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gram_rank(rank, world, port, out_dir, kind):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.chdir(out_dir)
    import torch.distributed as dist
    import symode_amd
    from oracle import sindy_oracle as O
    from tests.helpers import load_fixture_autoencoder, load_fixture_generator
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = "cuda:0"
    xs, dxs = O.rk4_trajectories(O.rhs_dosc, O.ics_dosc(12, np.random.RandomState(5)), 0.02, 500)
    x = torch.from_numpy(xs.reshape(-1, 2)).float().to(dev)
    dx = torch.from_numpy(dxs.reshape(-1, 2)).float().to(dev)
    n = x.shape[0]
    cut = n // 2 + 10                                                   # uneven shards
    lo, hi = (0, n) if world == 1 else ((0, cut) if rank == 0 else (cut, n))
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f6_symreg.npz"))
    ae = load_fixture_autoencoder(g, "tanh_learn", "Tanh", device=dev)
    gen = load_fixture_generator(g, "tanh_learn", "(2,1,2)", device=dev)
    for p in list(ae.parameters()) + list(gen.parameters()):
        p.requires_grad = False
    r = symode_amd.SINDyRegression(2, 3, False, False, threshold=0.05, device=dev)
    r.Xi.data = (torch.randn(2, 10, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    calls = []
    real = dist.all_reduce

    def counted(*a, **k):
        calls.append(a[0].numel() if a else -1)
        return real(*a, **k)

    dist.all_reduce = counted                                           # what the fit sends over the ranks
    try:
        symode_amd.train.train_SIGED_lbfgs(
            train_loader=[(x[lo:hi].contiguous(), dx[lo:hi].contiguous())], test_loader=[], num_epochs=60, device=dev,
            log_interval=10 ** 9, save_interval=10 ** 9, save_dir=f"t{world}", autoencoder=ae, generator=gen, regressor=r,
            regressor_dst=None, use_latent=False, distill_latent=False, lr_sindy=0.1, w_sindy_z=0.0, w_sindy_x=1.0,
            sindy_reg_type="l1", w_sindy_reg=0.0, sym_reg_type="r", w_sym_reg=0.05 if kind == "r" else 0.0, st_freq=50,
            threshold=0.05, int_t=0.1, int_dt=0.01, print_eq=False, group=dist.group.WORLD if world > 1 else None,
            gram_closure=True)
    finally:
        dist.all_reduce = real
    np.savez(os.path.join(out_dir, f"gram_{kind}_{world}_{rank}.npz"), Xi=r.get_Xi().detach().cpu().numpy(),
             mask=r.mask.cpu().numpy(), calls=np.array(calls, dtype=np.int64))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["plain", "r"])
def test_gram_fit_on_two_point_shards_equals_one_rank(tmp_path, kind):
    """dosc, order 3, 6 000 points in uneven shards, with and without the reversed regulariser: exactly ONE all-reduce
    ([G | R | count], fp64) per rank from trainer construction to the end of the fit; identical Xi and mask on both ranks;
    the one-rank Gram fit's mask, and its Xi to 1e-5 (relative to the largest coefficient)."""
    mp.spawn(_gram_rank, args=(2, _free_port(), str(tmp_path), kind), nprocs=2, join=True)
    mp.spawn(_gram_rank, args=(1, _free_port(), str(tmp_path), kind), nprocs=1, join=True)
    a, b = [np.load(tmp_path / f"gram_{kind}_2_{r}.npz") for r in range(2)]
    one = np.load(tmp_path / f"gram_{kind}_1_0.npz")
    F, dp = 12, 20
    want_numel = F * F + (dp * dp if kind == "r" else 0) + 1                               # [G | R | count]
    assert a["calls"].tolist() == [want_numel] and b["calls"].tolist() == [want_numel]
    assert one["calls"].tolist() == []
    assert np.array_equal(a["Xi"], b["Xi"]) and np.array_equal(a["mask"], b["mask"])
    assert np.array_equal(a["mask"], one["mask"])
    assert np.abs(a["Xi"] - one["Xi"]).max() <= 1e-5 * np.abs(one["Xi"]).max()
