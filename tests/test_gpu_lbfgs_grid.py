"""The hyper-parameter grid of the device L-BFGS trainer on shared Gram matrices (symode_trainer_grid, symode_quad_closure_grid,
DeviceTrainer(hyper=), SeedSweepLBFGS.fit(hyper=), main_sweep --lbfgs_grid).

Every comparison is bit for bit, and that follows from the code, not from a measurement: in the three kernels a problem is
one wave that shares no arithmetic with any other problem, so problem s of a grid launch is the one-problem scalar launch on
set s % n_sets at row s's values.  3 sets x 3 points = 9 problems: the last quad-closure block (4 waves) is partly filled."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import trainer_cases as C
from tests.helpers import only_compiled
from tests.test_gpu_trainer_steps import GpuDevice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETS, POINTS, N_DATA = 3, 3, 203
COLUMNS = ("lr", "w_reg", "threshold", "w_sym")


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _bytes(a):
    return a.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


# ---- statistics: 3 sets of 203 points through GramStatistics.add, computed once per library ------------------------------------
@functools.lru_cache(maxsize=None)
def _statistics(d, order, flags, regulariser):
    from symode_amd.gram_closure import GramStatistics
    g = torch.Generator().manual_seed(1000 * d + 10 * order + flags)
    p = C.lib_terms(d, order, flags)
    x = 0.6 * torch.randn(SETS, N_DATA, d, generator=g)
    truth = torch.randn(SETS, d, p, generator=g) * (torch.rand(SETS, d, p, generator=g) < 0.3)
    st = GramStatistics(SETS, d, order, flags, regulariser=regulariser, device=DEV)
    theta = torch.stack([st.engine.theta(x[s].to(DEV), order, flags).cpu() for s in range(SETS)])
    dx = torch.einsum("snp,sdp->snd", theta, truth) + 0.05 * torch.randn(SETS, N_DATA, d, generator=g)
    gx = jgx = None
    if regulariser:                                          # a rotation-like action with a little distortion, two elements
        A = torch.eye(d) + 0.2 * torch.randn(SETS, 2, d, d, generator=g)
        gx = torch.einsum("sgij,snj->sgni", A, x).contiguous().to(DEV)
        jgx = (A[:, :, None] + 0.01 * torch.randn(SETS, 2, N_DATA, d, d, generator=g)).contiguous().to(DEV)
    return st.add(x.to(DEV), dx.to(DEV), gx, jgx)


def _one_set(st, k):
    """The statistics of set k alone."""
    from symode_amd.gram_closure import GramStatistics
    one = GramStatistics(1, st.d, st.order, st.flags, regulariser=st.regulariser, device=DEV)
    one.G.copy_(st.G[k:k + 1])
    if st.regulariser:
        one.R.copy_(st.R[k:k + 1])
    one._count.copy_(st._count)
    return one


def _filled(S, d, order, flags, regulariser, seed):
    """Statistics that only have to satisfy the descriptor (the closure is played by the test): any numbers, 200 points."""
    from symode_amd.gram_closure import GramStatistics
    st = GramStatistics(S, d, order, flags, regulariser=regulariser, device=DEV)
    st.buffer.copy_(torch.randn(st.buffer.numel(), generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
    st._count.fill_(200.0)
    return st


# ---- 1. symode_quad_closure_grid ---------------------------------------------------------------------------------------------
# (d = 2, order 2), (d = 2, order 5) and d p = 78 > 64 (two outputs per lane; the regulariser's Gram launch ends at d p = 88)
QUAD_LIBS = only_compiled([(2, 2, 0), (2, 5, 0), (3, 3, 3)])


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("rev", [False, True], ids=["plain", "pair"])
@pytest.mark.parametrize("lib", QUAD_LIBS, ids=lambda c: f"d{c[0]}o{c[1]}f{c[2]}")
def test_quad_closure_grid_is_the_scalar_launch_per_problem(eng, lib, rev, masked):
    d, order, flags = lib
    st = _statistics(d, order, flags, rev)
    p, n, inv = st.p, SETS * POINTS, st.inv_count()
    g = torch.Generator().manual_seed(7 + d * order)
    xi = (0.5 * torch.randn(n, d, p, generator=g)).to(DEV)
    mask = (torch.rand(n, d, p, generator=g) > 0.3).float().to(DEV) if masked else None
    sub = lambda t, q: None if t is None else t[q:q + 1]  # noqa: E731
    # n_sets == n_problems and a uniform table: the scalar launch
    table = torch.tensor([[0.5, 1e-3, 0.1, 0.37]] * SETS).to(DEV)
    want = eng.quad_closure(st.G, st.R, xi[:SETS], None if mask is None else mask[:SETS], inv, 0.37)
    got = eng.quad_closure(st.G, st.R, xi[:SETS], None if mask is None else mask[:SETS], inv, hyper=table, n_sets=SETS)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert got[0].shape == ((SETS, 2) if rev else (SETS,))
    # 3 sets, 9 problems, a weight per problem (without the regulariser the column is not read: NaN there changes nothing)
    table = torch.rand(n, 4, generator=g) + 0.05
    if not rev:
        table[:, 3] = float("nan")
    table = table.to(DEV)
    loss, grad = eng.quad_closure(st.G, st.R, xi, mask, inv, hyper=table, n_sets=SETS)
    assert loss.shape == ((n, 2) if rev else (n,)) and grad.shape == (n, d, p) and bool(torch.isfinite(grad).all())
    for q in range(n):
        k = q % SETS
        one_l, one_g = eng.quad_closure(st.G[k:k + 1], None if not rev else st.R[k:k + 1], xi[q:q + 1], sub(mask, q), inv,
                                        float(table[q, 3]) if rev else 1.0)
        assert _same(loss[q:q + 1], one_l) and _same(grad[q:q + 1], one_g), (lib, rev, masked, q)
    if rev:                                                   # the table is read: one set, one Xi, two weights, two gradients
        xi2 = xi.clone()
        xi2[SETS:2 * SETS] = xi[:SETS]
        m2 = None if mask is None else torch.cat([mask[:SETS]] * POINTS)
        _, g2 = eng.quad_closure(st.G, st.R, xi2, m2, inv, hyper=table, n_sets=SETS)
        assert not torch.equal(g2[0], g2[SETS])


def test_the_binding_refuses_a_table_that_does_not_fit(eng):
    from symode_amd.engine import SymodeError
    st = _statistics(2, 2, 0, True)
    xi = torch.zeros(4, 2, st.p, device=DEV)
    with pytest.raises(SymodeError, match="multiple of the 3 sets"):
        eng.quad_closure(st.G, st.R, xi, None, 1.0, hyper=torch.zeros(4, 4, device=DEV))
    with pytest.raises(SymodeError, match="n_sets goes with hyper"):
        eng.quad_closure(st.G, st.R, xi[:3], None, 1.0, n_sets=3)


# ---- 2. single launches: the closure played by the test ---------------------------------------------------------------------
class GramDevice(GpuDevice):
    """A Gram-form DeviceTrainer (scalar or grid) behind the interface of trainer_cases; a grid trainer's launches go through
    the grid entries on its wrapping descriptor."""

    def __init__(self, tr, mapped, history):
        self.tr, self.mapped = tr, mapped
        self.shapes = C.field_shapes(tr.S, tr.n, tr.dp, history)

    def _entry(self, name):
        return getattr(self.tr.engine.lib, ("symode_trainer_grid_" if self.tr.hyper is not None else "symode_trainer_") + name)

    def update(self, mode):
        self._launch(self._entry("update")(self.tr._Gp, mode, self.tr._st()))

    def epoch_end(self, epoch):
        self._launch(self._entry("epoch_end")(self.tr._Gp, epoch, self.tr._st()))


def _trainer(st, lib, cfg, Q, allow_const, pair, max_iter=C.MAX_ITER, hyper=None, **scalars):
    from symode_amd.device_lbfgs import DeviceTrainer
    s = dict(lr=cfg["lr"], w_reg=cfg["w_reg"], threshold=cfg["threshold"], w_sym=cfg["w_pair"])
    s.update(scalars)
    return DeviceTrainer(None, None, lib[1], lib[2], Q=Q, allow_constant=allow_const, reversed_sym=(None, None, s["w_sym"]) if pair else None,
                         lr=s["lr"], threshold=s["threshold"], st_freq=cfg["st_freq"], w_x=cfg["w_x"], w_reg=s["w_reg"], l1=cfg["l1"],
                         tol=cfg["tol_update"], max_iter=max_iter, history=cfg["history"], tol_grad=cfg["tol_grad"],
                         tol_change=cfg["tol_change"], detail=True, closure="gram", statistics=st, hyper=hyper)


def _devices(lib, cfg, Q, allow_const, pair, table, n_sets):
    """The grid trainer on ``table`` (n, 4) and one scalar one-problem trainer per row."""
    d, order, flags = lib
    n = table.shape[0]
    hyper = {name: table[:, c] for c, name in enumerate(COLUMNS) if pair or name != "w_sym"}
    grid = _trainer(_filled(n_sets, d, order, flags, pair, 1), lib, cfg, Q, allow_const, pair, hyper=hyper)
    assert grid.S == n and grid.G.n_sets == n_sets and grid._run_fn is grid.engine.lib.symode_trainer_grid_run
    one = _filled(1, d, order, flags, pair, 2)
    rows = [_trainer(one, lib, cfg, Q, allow_const, pair, **{name: float(table[q, c]) for c, name in enumerate(COLUMNS)}) for q in range(n)]
    assert all(r.S == 1 and r.hyper is None and r._run_fn is r.engine.lib.symode_trainer_run and r._Gp is r._Tp for r in rows)
    H = cfg["history"]
    return GramDevice(grid, Q is not None, H), [GramDevice(r, Q is not None, H) for r in rows]


def _assert_equal_states(grid, rows, where, logs=False):
    hs = grid.read()
    for q, row in enumerate(rows):
        one = row.read()
        for k in hs:
            if k in ("cl_loss", "test_grad"):                # inputs the test wrote (with decoys) / never written
                continue
            assert torch.equal(_bytes(hs[k][q]), _bytes(one[k][0])), (where, q, k)
    if logs:
        lg = grid.logs()
        for q, row in enumerate(rows):
            lo = row.logs()
            for k in lg:
                assert torch.equal(_bytes(lg[k][:, q]), _bytes(lo[k][:, 0])), (where, q, "record " + k)
    return hs


# history 3 and 100 of each: staged (one and two components per lane), and at (3, 4, 0) with 100 pairs the unstaged form
STEP_CASES = only_compiled(C.update_cases([(2, 3, 0), (2, 5, 0), (3, 4, 0)]))


@pytest.mark.parametrize("case", STEP_CASES, ids=C.case_id)
def test_grid_launches_are_the_scalar_launches_per_problem(eng, case):
    """BEGIN, ACCEPT x 3 and the epoch end (st_freq = 1: a thresholding event) on the 9-problem grid trainer and on nine
    one-problem scalar trainers, from the start states of trainer_cases with the closure played as test_gpu_trainer_steps
    plays it: after every launch every state field, and after the epoch end every record, is equal."""
    lib = case[:3]
    su = C.case_setup(case)
    cfg, pair = dict(su.cfg, st_freq=1), su.cfg["pair"]
    n = SETS * POINTS
    P0, mask0 = su.P0.repeat(POINTS, 1), su.mask0.repeat(POINTS, 1)                     # problem g * 3 + k starts where seed k starts
    hs0 = C.start_state(cfg, su.n, su.dp, cfg["history"], P0, mask0)
    # thresholds between the sorted live |Xi| of the seed's own start state: above a quarter, half and three quarters of them;
    # small steps, so that the coefficients are still about there when the epoch ends
    def cut(k, f):
        live = hs0["xi"][k].abs()[mask0[k] > 0].sort().values
        assert live.numel() >= 8
        at = int(f * live.numel())
        assert live[0] < live[at - 1] < live[at] <= live[-1]                             # it straddles live coefficients
        return float(0.5 * (live[at - 1] + live[at]))
    table = torch.tensor([[(0.1, 0.05, 0.2)[g], (1e-3, 5e-3, 0.0)[g], cut(k, (0.25, 0.5, 0.75)[g]), (0.37, 0.1, 1.5)[g]]
                          for g in range(POINTS) for k in range(SETS)])
    grid, rows = _devices(lib, cfg, su.Q, su.allow_const, pair, table, SETS)
    assert (grid.tr.n, grid.tr.dp) == (su.n, su.dp)
    grid.load(hs0)
    for q, row in enumerate(rows):
        row.load({k: v[q:q + 1] for k, v in hs0.items()})
    closure = C.Quadratic(n, su.dp, 31 + su.dp, pair, cfg["w_pair"])
    _assert_equal_states(grid, rows, "loaded")
    for it in range(C.MAX_ITER):
        hs = grid.read()
        loss2, grad = closure(hs["xi"], hs["mask"])
        C.put_closure(grid, loss2, grad, pair)
        for q, row in enumerate(rows):
            C.put_closure(row, loss2[q:q + 1], grad[q:q + 1], pair)
        mode = C.M.BEGIN if it == 0 else C.M.ACCEPT
        grid.update(mode)
        for row in rows:
            row.update(mode)
        hs = _assert_equal_states(grid, rows, ("update", it))
    assert int(hs["n_iter"].min()) >= 1 and len({float(t) for t in hs["t"][::SETS]}) == POINTS      # they moved, by their own lr
    grid.epoch_end(0)
    for row in rows:
        row.epoch_end(0)
    hs = _assert_equal_states(grid, rows, "epoch end", logs=True)
    codes = grid.logs()["log"][0, :, 0].tolist()
    assert codes == [float(C.M.EVENT_FREQ)] * n, codes
    # the table decided: the same seed ends with another mask under another threshold
    assert any(not torch.equal(hs["mask"][k], hs["mask"][2 * SETS + k]) for k in range(SETS))


EPOCH_CASES = only_compiled(C.epoch_cases([(2, 3, 0), (3, 4, 0)]))


@pytest.mark.parametrize("case", EPOCH_CASES, ids=lambda c: f"d{c[0]}o{c[1]}f{c[2]}-{'q5c' if c[3] else 'none'}-{'pair' if c[4] else 'plain'}-e{c[5]}")
def test_grid_epoch_launch_on_the_hand_written_events(eng, case):
    """The epoch cases of trainer_cases (6 problems, one per event, the threshold's edge values in Xi) on a grid trainer of 3
    sets whose table gives the two thresholding problems other thresholds, against six scalar trainers -- and against the
    uniform threshold, which must give those two another mask."""
    d, order, flags, mapped, pair, epoch = case
    cfg, Q, n, dp, hs0, cl = C.epoch_setup(case)
    thr = [0.3, cfg["threshold"], 0.05, cfg["threshold"], 0.2, 0.4]                     # problems 0 (conv) and 2 (period) threshold
    table = torch.tensor([[cfg["lr"], 0.0, thr[q], 0.37] for q in range(C.S_EPOCH)])
    grid, rows = _devices((d, order, flags), cfg, Q, True, pair, table, SETS)
    uniform = GramDevice(_trainer(_filled(C.S_EPOCH, d, order, flags, pair, 3), (d, order, flags), cfg, Q, True, pair), mapped, cfg["history"])
    zero = torch.zeros(C.S_EPOCH, dp, dtype=torch.float64)
    for dev, sl in [(grid, slice(None)), (uniform, slice(None))] + [(row, slice(q, q + 1)) for q, row in enumerate(rows)]:
        dev.load({k: v[sl] for k, v in hs0.items()})
        C.put_closure(dev, cl.double()[sl], zero[sl], pair)
        dev.epoch_end(epoch)
    hs = _assert_equal_states(grid, rows, "epoch end", logs=True)
    assert grid.logs()["log"][epoch % C.LOG_RING, :, 0].tolist() == [float(c) for c in C.WANT_CODES]
    base = uniform.read()
    for q in (0, 2):
        assert not torch.equal(hs["mask"][q], base["mask"][q]), q
    for q in (1, 3, 4, 5):
        assert torch.equal(hs["mask"][q], base["mask"][q]), q


# ---- 3. fits ------------------------------------------------------------------------------------------------------------------
FIT_LIB, FIT_EPOCHS = (2, 3, 0), 6
RECORD = ("code", "mse", "sym", "l1", "update_norm", "update_norm_2", "near", "epoch", "test", "xi", "mask", "params")
OUT = ("Xi", "mask", "params", "epochs", "finished", "nan", "near_threshold")


def _fit_table():
    rows = [[(1.0, 0.5, 0.8)[g], (0.0, 1e-3, 1e-2)[g], (0.02, 0.1, 0.3)[g], (0.1, 1.0, 0.01)[g]] for g in range(POINTS) for _ in range(SETS)]
    return torch.tensor(rows)


def _fit(st, P0, Q=None, hyper=None, **scalars):
    from symode_amd.device_lbfgs import DeviceTrainer
    s = dict(lr=1.0, w_reg=1e-3, threshold=0.1, w_sym=0.3)
    s.update(scalars)
    tr = DeviceTrainer(None, None, FIT_LIB[1], FIT_LIB[2], Q=Q, reversed_sym=(None, None, s["w_sym"]), lr=s["lr"], threshold=s["threshold"],
                       st_freq=2, w_reg=s["w_reg"], l1=True, max_iter=5, detail=True, closure="gram", statistics=st, hyper=hyper)
    recs = []
    out = tr.fit(P0, FIT_EPOCHS, on_epoch=lambda e, rec: recs.append(rec), test_eval=True)
    return tr, out, recs


@pytest.fixture(scope="module")
def fit_start():
    g = torch.Generator().manual_seed(5)
    p = C.lib_terms(*FIT_LIB)
    return {False: 0.3 * torch.randn(SETS, 2 * p, generator=g), True: 0.3 * torch.randn(SETS, 5 + 2, generator=g)}


@pytest.mark.parametrize("mapped", [False, True], ids=["free", "q5c"])
def test_a_grid_fit_is_the_scalar_fit_per_row(eng, fit_start, mapped):
    st = _statistics(*FIT_LIB, True)
    Q = C.householder_q(st.dp, 5) if mapped else None
    P0, table = fit_start[mapped], _fit_table()
    tr, out, recs = _fit(st, P0.repeat(POINTS, 1), Q, hyper={name: table[:, c] for c, name in enumerate(COLUMNS)})
    assert tr.S == SETS * POINTS and tr.stats.S == SETS and len(recs) >= 1
    for q in range(SETS * POINTS):
        k = q % SETS
        one_tr, one, one_recs = _fit(_one_set(st, k), P0[k:k + 1], Q, **{name: float(table[q, c]) for c, name in enumerate(COLUMNS)})
        assert one_tr.hyper is None and one_tr._run_fn is eng.lib.symode_trainer_run
        for key in OUT:
            assert _same(out[key][q:q + 1], one[key]), (q, key)
        assert len(one_recs) <= len(recs)
        for e, rec in enumerate(recs):
            if e >= len(one_recs):                            # the scalar fit had stopped: the grid's problem idles
                assert rec["code"][q] == -1, (q, e)
                continue
            for key in RECORD:
                assert rec[key][q].tobytes() == one_recs[e][key][0].tobytes(), (q, e, key)
    # the rows end differently: the same seed under two points
    assert any(not torch.equal(out["mask"][k], out["mask"][2 * SETS + k]) for k in range(SETS))
    assert not torch.equal(out["Xi"][0], out["Xi"][SETS])
    assert recs[0]["test"].shape == (SETS * POINTS,) and np.isfinite(recs[0]["test"]).all()


def test_a_uniform_table_is_the_fit_without_a_table(eng, fit_start):
    st = _statistics(*FIT_LIB, True)
    P0 = fit_start[False]
    _, plain, plain_recs = _fit(st, P0)
    full = {"lr": [1.0] * SETS, "w_reg": [1e-3] * SETS, "threshold": [0.1] * SETS, "w_sym": [0.3] * SETS}
    for hyper in (full, {"threshold": [0.1] * SETS}):         # missing columns: the scalar arguments
        tr, out, recs = _fit(st, P0, hyper=hyper)
        assert tr._run_fn is eng.lib.symode_trainer_grid_run
        assert all(_same(out[k], plain[k]) for k in OUT) and len(recs) == len(plain_recs)
        assert all(r[k].tobytes() == w[k].tobytes() for r, w in zip(recs, plain_recs) for k in RECORD)


def test_the_sweep_passes_the_table_through(eng, fit_start):
    from symode_amd.coef_map import CoefMap
    from symode_amd.sweep import GramClosure, SeedSweepLBFGS
    st, table = _statistics(*FIT_LIB, True), _fit_table()
    P0 = fit_start[False].to(DEV)

    def sweep(stats, lr=1.0, w_reg=1e-3, threshold=0.1, w_sym=0.3):
        clos = GramClosure(stats, w_sym=w_sym, coef=CoefMap(stats.d, stats.p))
        return SeedSweepLBFGS(clos, lr, threshold, 2, w_sindy_reg=w_reg, statistics=stats)

    sw = sweep(st)
    out = sw.fit(P0.repeat(POINTS, 1), FIT_EPOCHS, hyper={name: table[:, c] for c, name in enumerate(COLUMNS)})
    assert sw.trainer.S == SETS * POINTS and sw.trainer.hyper is not None and sw.mask.shape == (SETS * POINTS, 2, st.p)
    for q in range(SETS * POINTS):
        k = q % SETS
        one = sweep(_one_set(st, k), *[float(v) for v in table[q]]).fit(P0[k:k + 1], FIT_EPOCHS)
        for key in OUT:
            assert _same(out[key][q:q + 1], one[key]), (q, key)
    assert any(not torch.equal(out["mask"][k], out["mask"][2 * SETS + k]) for k in range(SETS))


def _sharded_rank(rank, world, port, out_dir):
    """One rank of the sharded grid fit: the statistics of its share of every set's points, the trainer with ``group``."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    import symode_amd
    from symode_amd.device_lbfgs import DeviceTrainer
    from symode_amd.gram_closure import GramStatistics
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(3)
    p = symode_amd.get_engine().lib_size(2, 3, 0)
    x = 0.6 * torch.randn(SETS, N_DATA, 2, generator=g)
    dx = torch.stack([-0.5 * x[..., 0] + 2.0 * x[..., 1], -2.0 * x[..., 0] - 0.5 * x[..., 1] + 0.4 * x[..., 0] ** 2], dim=-1)
    dx = dx + 0.05 * torch.randn(SETS, N_DATA, 2, generator=g)
    cut = N_DATA // 2 + 10                                                   # uneven shards
    lo, hi = (0, N_DATA) if world == 1 else ((0, cut) if rank == 0 else (cut, N_DATA))
    st = GramStatistics(SETS, 2, 3, 0, device=DEV).add(x[:, lo:hi].contiguous().to(DEV), dx[:, lo:hi].contiguous().to(DEV))
    calls, real = [], dist.all_reduce

    def counted(*a, **k):
        calls.append(a[0].numel() if a else -1)
        return real(*a, **k)

    dist.all_reduce = counted
    try:
        table = _fit_table()
        tr = DeviceTrainer(None, None, 3, 0, st_freq=2, max_iter=5, closure="gram", statistics=st, group=dist.group.WORLD if world > 1 else None,
                           hyper={name: table[:, c] for c, name in enumerate(COLUMNS[:3])})
        out = tr.fit(0.3 * torch.randn(SETS, 2 * p, generator=g).repeat(POINTS, 1), 4)
    finally:
        dist.all_reduce = real
    np.savez(os.path.join(out_dir, f"grid_{world}_{rank}.npz"), Xi=out["Xi"].numpy(), mask=out["mask"].numpy(), calls=np.array(calls, dtype=np.int64))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_a_grid_fit_on_two_point_shards_equals_one_rank(tmp_path):
    """``group=`` keeps working: two gloo ranks on the one GPU sum [G | count] of their uneven shards in ONE all-reduce when the
    grid trainer is built and fit the 9 problems without another; both end on identical Xi and mask, the one-rank grid
    fit's mask, and its Xi to 1e-5 of the largest coefficient (the fp64 sums of the two shards add in another order)."""
    import socket
    import torch.multiprocessing as mp
    for world in (2, 1):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.spawn(_sharded_rank, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b, one = (np.load(tmp_path / f"grid_{w}_{r}.npz") for w, r in ((2, 0), (2, 1), (1, 0)))
    numel = SETS * 12 * 12 + 1                                           # [G | count] of 3 sets, F = p + d = 12
    assert a["calls"].tolist() == [numel] and b["calls"].tolist() == [numel] and one["calls"].tolist() == []
    assert a["Xi"].shape == (SETS * POINTS, 2, 10)
    assert np.array_equal(a["Xi"], b["Xi"]) and np.array_equal(a["mask"], b["mask"])
    assert np.array_equal(a["mask"], one["mask"])
    assert np.abs(a["Xi"] - one["Xi"]).max() <= 1e-5 * np.abs(one["Xi"]).max()
    assert not np.array_equal(a["mask"][0], a["mask"][2 * SETS])         # the table decided on the shards too


def test_the_trainer_refuses_what_it_cannot_place(eng):
    from symode_amd.device_lbfgs import DeviceTrainer
    from symode_amd.engine import SymodeError
    st, plain = _statistics(*FIT_LIB, True), _statistics(*FIT_LIB, False)
    rev = (None, None, 0.3)
    gram = lambda stats, hyper, **kw: DeviceTrainer(None, None, 3, 0, closure="gram", statistics=stats, hyper=hyper, **kw)  # noqa: E731
    x = torch.zeros(SETS, 8, 2, device=DEV)
    with pytest.raises(SymodeError, match="is for closure='gram', got closure='stream'"):
        DeviceTrainer(x, x.clone(), 3, 0, hyper={"lr": [1.0] * SETS})
    with pytest.raises(SymodeError, match="4 rows, not a multiple of the statistics' 3 sets"):
        gram(st, {"lr": [1.0] * 4}, reversed_sym=rev)
    with pytest.raises(SymodeError, match="w_sym needs the regulariser's matrices"):
        gram(plain, {"w_sym": [1.0] * SETS})
    with pytest.raises(SymodeError, match=r"unknown keys \['max_iter'\]"):
        gram(st, {"max_iter": [4] * SETS}, reversed_sym=rev)
    with pytest.raises(SymodeError, match="65538 rows: one trainer takes at most 65535"):
        gram(st, {"lr": [1.0] * 65538}, reversed_sym=rev)
    with pytest.raises(SymodeError, match=r"got lengths \[3, 6\]"):
        gram(st, {"lr": [1.0] * 3, "threshold": [0.1] * 6}, reversed_sym=rev)
    with pytest.raises(SymodeError, match="must be a dict"):
        gram(st, [1.0] * SETS, reversed_sym=rev)
    assert gram(plain, {"threshold": [0.1] * 6}).S == 6


# ---- 4. main_sweep --lbfgs_grid ---------------------------------------------------------------------------------------------------
def _main(tmp, argv):
    from symode_amd import main_sweep
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        return main_sweep.main(list(argv))
    finally:
        os.chdir(cwd)


def _assert_points_equal_scalar_runs(root, res, points, scalar_of, names, seeds):
    coefs = []
    for g, point in enumerate(points):
        scalar = scalar_of(g, point)
        assert repr(res[g]) == repr(scalar), g                                           # the aggregates
        for s in seeds:
            want, got = np.load(root / f"point{g}" / f"seed{s}.npz"), np.load(root / "grid" / f"grid{g}" / f"seed{s}.npz")
            assert set(got.files) == set(want.files) | set(names)
            for key in want.files:
                assert got[key].tobytes() == want[key].tobytes(), (g, s, key)
            for name in names:
                assert float(got[name]) == point[name], (g, s, name)
            coefs.append(got["coefficients"])
    return coefs


def test_main_sweep_lbfgs_grid_with_the_regulariser_is_main_sweep_at_every_point(eng, tmp_path, capsys):
    """The small LV recipe of tests/test_gpu_sym_sweep.py (a frozen random LaLiGAN), 3 seeds, 8 epochs with thresholding every
    third: threshold x w_sym_reg, every point against main_sweep --gram_closure with that point's scalar flags."""
    from tests.test_gpu_sym_sweep import CASES, _prepare
    _prepare(tmp_path, "lv")
    base = list(CASES["lv"][0]) + ["--n_seeds", "3", "--num_epochs", "8", "--st_freq", "3", "--gram_closure"]
    T, W = ("0.05", "0.4"), ("0.02", "1.0")
    res = _main(tmp_path, base + ["--save_dir", "grid", "--lbfgs_grid", "threshold=" + ",".join(T), "--lbfgs_grid", "w_sym_reg=" + ",".join(W)])
    out = capsys.readouterr().out
    assert sorted(res) == [0, 1, 2, 3] and all(r["n_runs"] == 3 for r in res.values())
    assert "grid of 4 points x 3 seeds" in out and "grid 3: 3 seeds, epochs used" in out
    root = tmp_path / "eval_results"
    listed = json.loads((root / "grid" / "grid.json").read_text())
    points = [dict(threshold=float(t), w_sym_reg=float(w)) for t in T for w in W]       # the first axis given is the slowest
    assert [(p["threshold"], p["w_sym_reg"]) for p in listed["points"]] == [(p["threshold"], p["w_sym_reg"]) for p in points]
    assert listed["axes"] == [["threshold", [0.05, 0.4]], ["w_sym_reg", [0.02, 1.0]]] and listed["n_seeds"] == 3
    assert all(p["lr_sindy"] == 0.1 and p["w_sindy_reg"] == 0.0 for p in listed["points"])
    assert sorted(p.name for p in (root / "grid").iterdir()) == ["grid.json", "grid0", "grid1", "grid2", "grid3"]
    names = ("lr_sindy", "w_sindy_reg", "threshold", "w_sym_reg")
    full = [dict(lr_sindy=0.1, w_sindy_reg=0.0, **p) for p in points]
    coefs = _assert_points_equal_scalar_runs(
        root, res, full, lambda g, p: _main(tmp_path, base + ["--save_dir", f"point{g}", "--threshold", T[g // 2], "--w_sym_reg", W[g % 2]]),
        names, (0, 1, 2))
    capsys.readouterr()
    assert not np.array_equal(coefs[0], coefs[3]) and not np.array_equal(coefs[0], coefs[6])     # the weight and the threshold decide
    assert any(np.count_nonzero(coefs[k]) != np.count_nonzero(coefs[6 + k]) for k in range(3))   # thresholding happened


def _dosc(tmp, save_dir, extra):
    argv = ["--task", "dosc", "--noise", "0.0", "--ae_arch", "none", "--sindy_optimizer", "lbfgs", "--w_sindy_x", "1.0", "--w_sindy_z", "0.0",
            "--w_sym_reg", "0.0", "--poly_order", "2", "--threshold", "0.05", "--st_freq", "2", "--num_epochs", "6", "--seed", "4",
            "--n_seeds", "3", "--gram_closure", "--save_dir", save_dir]
    return _main(tmp, argv + extra)


def test_main_sweep_lbfgs_grid_without_a_regulariser_and_with_eval_ltp(eng, tmp_path, monkeypatch, capsys):
    from symode_amd import dataset as D
    monkeypatch.setitem(D._RECIPES, "dosc", (6, 3, 600, 3, 0.01))                # 6 + 3 trajectories x 200 samples, noise-free
    monkeypatch.setitem(D.ode_dt_dict, "dosc", 0.03)
    LR, WR = ("0.3", "1.0"), ("0.0001", "0.05")
    res = _dosc(tmp_path, "grid", ["--lbfgs_grid", "lr_sindy=" + ",".join(LR), "--lbfgs_grid", "w_sindy_reg=" + ",".join(WR)])
    assert sorted(res) == [0, 1, 2, 3] and "grid of 4 points x 3 seeds" in capsys.readouterr().out
    root = tmp_path / "eval_results"
    full = [dict(lr_sindy=float(lr), w_sindy_reg=float(w), threshold=0.05, w_sym_reg=0.0) for lr in LR for w in WR]
    coefs = _assert_points_equal_scalar_runs(
        root, res, full, lambda g, p: _dosc(tmp_path, f"point{g}", ["--lr_sindy", LR[g // 2], "--w_sindy_reg", WR[g % 2]]),
        ("lr_sindy", "w_sindy_reg", "threshold", "w_sym_reg"), (4, 5, 6))
    assert not np.array_equal(coefs[0], coefs[3]) and not np.array_equal(coefs[0], coefs[6])
    capsys.readouterr()
    # --eval_ltp: all G x S models in the one roll-out launch, the two medians in grid.json, a best point by name
    res = _dosc(tmp_path, "scored", ["--lr_sindy", "1.0", "--eval_ltp", "--ltp_bound_rel", "0.1", "--lbfgs_grid", "w_sindy_reg=" + ",".join(WR)])
    out = capsys.readouterr().out
    listed = json.loads((root / "scored" / "grid.json").read_text())["points"]
    assert sorted(res) == [0, 1] and [p["w_sindy_reg"] for p in listed] == [1e-4, 0.05]
    per_point = []
    for g in (0, 1):
        med = np.array([np.median(np.load(root / "scored" / f"grid{g}" / f"seed{s}.npz")["ltp_mean_error"]) for s in (4, 5, 6)])
        per_point.append(float(np.median(np.where(np.isfinite(med), med, np.inf))))
        assert listed[g]["ltp_median_error"] == (per_point[-1] if np.isfinite(per_point[-1]) else None) and "val_mse" in listed[g]
    best = int(np.argmin(per_point))
    assert f"best by validation roll-out error: grid {best} (lr_sindy=1 w_sindy_reg={[1e-4, 0.05][best]:g} threshold=0.05 w_sym_reg=0)" in out
