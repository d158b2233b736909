"""The two kernels under the default fit route, lbfgs_update_kernel (symode_trainer_update, BEGIN / ACCEPT) and
trainer_epoch_kernel (symode_trainer_epoch_end), one launch at a time against the fp64 model of tests/trainer_model.py;
and the sweep's entry to the first of them (symode_lbfgs_step) against the trainer's, byte for byte.

The test plays the closure: it writes cl_loss / cl_grad into the state block, launches, and copies the block to the host
before and after.  The model is handed the device's state before the launch, so no trajectory drift enters a comparison.
Cases, driver, comparisons and tolerances are those of tests/trainer_cases.py, which tests/test_host_trainer_model.py
replays on the CPU (float32 model in the device's place) to show the inputs decidable and to derive the tolerances."""
import ctypes

import pytest
import torch

from tests import trainer_cases as C
from tests.helpers import only_compiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd


class GpuDevice:
    """A DeviceTrainer's state block behind the interface of trainer_cases.  x, dx (and the reversed operands of the pair
    cases) are dummies that satisfy the descriptor's validation: symode_trainer_closure is never called."""

    def __init__(self, n_problems, d, order, flags, Q, allow_const, cfg, pair, max_iter=C.MAX_ITER):
        from symode_amd.device_lbfgs import DeviceTrainer
        g = torch.Generator().manual_seed(0)
        x, dx = torch.randn(n_problems, 8, d, generator=g).to(DEV), torch.randn(n_problems, 8, d, generator=g).to(DEV)
        rev = None
        if pair:
            rev = (torch.randn(n_problems, 1, 8, d, generator=g).to(DEV), torch.randn(n_problems, 1, 8, d, d, generator=g).to(DEV), cfg["w_pair"])
        self.tr = DeviceTrainer(x, dx, order, flags, Q=Q, allow_constant=allow_const, reversed_sym=rev, lr=cfg["lr"],
                                threshold=cfg["threshold"], st_freq=cfg["st_freq"], w_x=cfg["w_x"], w_reg=cfg["w_reg"], l1=cfg["l1"],
                                tol=cfg["tol_update"], max_iter=max_iter, history=cfg["history"], tol_grad=cfg["tol_grad"],
                                tol_change=cfg["tol_change"], detail=True, closure="stream")
        assert self.tr.LOG_RING == C.LOG_RING and self.tr.pair == pair
        self.mapped = Q is not None
        self.shapes = C.field_shapes(n_problems, self.tr.n, self.tr.dp, cfg["history"])

    def _launch(self, rc):
        assert rc == 0, rc
        torch.cuda.synchronize()

    def load(self, hs):
        tr = self.tr
        P0, m0 = hs["params"].to(DEV), hs["mask"].to(DEV)
        self._launch(tr.engine.lib.symode_trainer_init(tr._Tp, ctypes.c_void_p(P0.data_ptr()), ctypes.c_void_p(m0.data_ptr()), tr._st()))
        for k, v in hs.items():
            if k == "xi" and not self.mapped:
                continue                                     # unconstrained: Xi is the params array
            self.put(k, v)
        for k in ("log", "log_xi", "log_mask", "log_params"):
            getattr(tr, k).fill_(C.SENTINEL)

    def put(self, name, tensor):
        f = self.tr.field(name)
        f.copy_(tensor.to(f.dtype).reshape(f.shape))

    def read(self):
        torch.cuda.synchronize()
        tr = self.tr
        raw = tr.state.cpu()
        out = {}
        for k, shape in self.shapes.items():
            f = tr.field(k)
            assert f.numel() == int(torch.tensor(shape).prod()), (k, tuple(f.shape), shape)
            nbytes = f.numel() * f.element_size()
            out[k] = raw[tr._off[k]:tr._off[k] + nbytes].view(f.dtype).view(*shape).clone()
        return out

    def update(self, mode):
        self._launch(self.tr.engine.lib.symode_trainer_update(self.tr._Tp, mode, self.tr._st()))

    def epoch_end(self, epoch):
        self._launch(self.tr.engine.lib.symode_trainer_epoch_end(self.tr._Tp, epoch, self.tr._st()))

    def logs(self):
        torch.cuda.synchronize()
        return {k: getattr(self.tr, k).clone() for k in ("log", "log_xi", "log_mask", "log_params")}


def _verdict(title, rep, tol):
    for k in sorted(rep.worst):
        print(f"trainer steps on the device, {title}, {k}: worst {rep.worst[k][0]:.3e} at {rep.worst[k][1]} (tolerance {tol.get(k, float('nan')):.1e})")
    assert rep.mismatch == [], rep.mismatch[:5]
    assert rep.unsettled == [], rep.unsettled[:5]            # a cap, not a measurement: the model may not be trusted there
    assert rep.over(tol) == {}, rep.over(tol)


UPDATE_CASES = only_compiled(C.update_cases())


@pytest.mark.parametrize("case", UPDATE_CASES, ids=C.case_id)
def test_update_launches_match_the_model(S, case):
    """Two epochs of BEGIN, ACCEPT x 3 for 3 problems, a hand-made optimiser reset between them: after every launch the
    integer and flag fields equal the model's, the float fields and the stored pairs (in logical order) are within the
    tolerances, and what the model leaves untouched keeps its bytes."""
    d, order, flags = case[:3]
    su = C.case_setup(case)
    dev = GpuDevice(C.S_UPDATE, d, order, flags, su.Q, su.allow_const, su.cfg, su.cfg["pair"])
    assert (dev.tr.n, dev.tr.dp) == (su.n, su.dp)
    dev.load(C.start_state(su.cfg, su.n, su.dp, su.cfg["history"], su.P0, su.mask0))
    rep = C.Report()
    C.drive_update_case(case, dev, rep, su)
    assert rep.launches == 2 * C.MAX_ITER * C.S_UPDATE
    _verdict(C.case_id(case), rep, C.STEP_TOL)


CRAFTED = C.crafted_cases() if only_compiled([(2, 3, 0)]) else []


@pytest.mark.parametrize("crafted", CRAFTED, ids=lambda c: c.name.replace(" ", "_"))
def test_crafted_update_launches(S, crafted):
    """Single launches on exact float32 inputs at the edges of every stopping test (see trainer_cases.crafted_cases)."""
    cfg, hs = crafted.cfg, crafted.hs
    mp = cfg["map"]
    Q = None if mp is None else mp[0].float().contiguous()
    dev = GpuDevice(hs["params"].shape[0], 2, 3, 0, Q, True if mp is None else mp[3], cfg, crafted.pair)
    rep = C.Report()
    got = C.drive_crafted(crafted, dev, rep)
    assert got == crafted.expect, (crafted.name, got, crafted.expect)       # the model's own outcome is what the case was built for
    _verdict(crafted.name, rep, C.STEP_TOL)


# (d, order, flags, history): n = d p = 20 with a memory of 3 pairs (the ring wraps) and of 100 (staged, one component per
# lane), and the largest unconstrained library of the default build, n = 123: at history 3 staged with two components per
# lane, at history 100 the unstaged form (no default library has d p = 150; 123 parameters and 100 pairs are past the 60 KB
# the staged form may use, as 150 are).  Three components per lane need n > 128 (the d = 4 libraries of `make ALL=1` only), four
# n > 192 (no unconstrained library).  Not filtered by only_compiled: every default build has both libraries, and a row must not
# drop out silently.
STEP_ENTRY_CASES = [(2, 3, 0, 3), (2, 3, 0, 100), (3, 4, 3, 3), (3, 4, 3, 100)]
STATE_ARRAYS = (("params", "P"), ("g", "_g"), ("loss", "_loss"), ("act", "_act"), ("n_iter", "n_iter"), ("d", "d"), ("t", "t"),
                ("old_dirs", "old_dirs"), ("old_stps", "old_stps"), ("ro", "ro"), ("head", "head"), ("count", "hist"),
                ("h_diag", "H_diag"), ("prev_g", "prev_g"), ("prev_loss", "prev_loss"))


@pytest.mark.parametrize("case", STEP_ENTRY_CASES, ids=lambda c: f"d{c[0]}o{c[1]}f{c[2]}-h{c[3]}")
def test_the_sweep_entry_is_the_trainer_entry(S, case):
    """symode_lbfgs_step on plain tensors laid out as sweep.BatchedLBFGS state against symode_trainer_update on a
    DeviceTrainer state block: the same cl_loss / cl_grad (a convex quadratic's, evaluated on the host at the parameters
    the launches left) for one BEGIN and four ACCEPT launches of 3 unconstrained problems, one of them frozen / done, L1
    term on with w_x, w_reg off their defaults.  After every launch all fifteen state arrays hold the same bytes -- no
    tolerance: the sweep's kernel route is the launch the fp64 model above checks."""
    from symode_amd.engine import LBFGS_ACCEPT, LBFGS_BEGIN
    from symode_amd.sweep import BatchedLBFGS
    d, order, flags, H = case
    Sn, frozen_one = 3, 1
    cfg = C.M.make_cfg(lr=0.5, history=H, w_x=0.7, w_reg=0.013, l1=True, d=d)
    dev = GpuDevice(Sn, d, order, flags, None, True, cfg, False)
    tr, eng = dev.tr, dev.tr.engine
    n = tr.n
    assert n == tr.dp == (20 if d == 2 else 123)
    gen = torch.Generator().manual_seed(100 * n + H)
    A = torch.randn(Sn, n, n, generator=gen) / n ** 0.5
    A = A @ A.transpose(1, 2) + 0.5 * torch.eye(n)
    b, P0 = torch.randn(Sn, n, generator=gen), torch.randn(Sn, n, generator=gen)
    dev._launch(eng.lib.symode_trainer_init(tr._Tp, ctypes.c_void_p(P0.data_ptr()), None, tr._st()))
    frozen = torch.zeros(Sn, dtype=torch.bool)
    frozen[frozen_one] = True
    dev.put("done", frozen)
    P = P0.to(DEV).clone()
    opt = BatchedLBFGS(P, cfg["lr"], tolerance_grad=cfg["tol_grad"], tolerance_change=cfg["tol_change"], history_size=H, engine=eng)
    assert opt.fused
    frozen = frozen.to(DEV)
    for it in range(5):
        at = tr.field("params").cpu()
        AP = torch.einsum("sij,sj->si", A, at)
        cl_loss, cl_grad = (0.5 * (at * AP).sum(1) - (b * at).sum(1)).to(DEV), (AP - b).to(DEV)
        tr.field("cl_loss").view(-1)[:Sn] = cl_loss                              # (the plain closure fills the first S floats)
        dev.put("cl_grad", cl_grad)
        mode = LBFGS_BEGIN if it == 0 else LBFGS_ACCEPT
        dev.update(mode)
        eng.lbfgs_step(mode, cl_loss, cl_grad, P, opt._g, opt._loss, opt._act, opt, cfg["lr"], cfg["tol_grad"], cfg["tol_change"],
                       l1=(cfg["w_x"], cfg["w_reg"]), frozen=frozen)
        torch.cuda.synchronize()
        for field, attr in STATE_ARRAYS:
            a, b_ = tr.field(field), getattr(opt, attr)
            assert a.numel() == b_.numel() and a.element_size() == b_.element_size(), (field, a.shape, b_.shape)
            assert torch.equal(a.reshape(-1).view(torch.uint8), b_.reshape(-1).view(torch.uint8)), (case, it, field)
    # the launches did what the case is for: the live problems took every iteration and the memory of 3 wrapped
    live = [s for s in range(Sn) if s != frozen_one]
    assert opt._act.cpu().tolist() == [s != frozen_one for s in range(Sn)]
    assert opt.n_iter.cpu().tolist() == [0 if s == frozen_one else 5 for s in range(Sn)]
    assert opt.hist.cpu()[live].tolist() == [min(4, H)] * 2 and opt.head.cpu()[live].tolist() == [1 if H == 3 else 0] * 2
    assert torch.equal(P[frozen_one].cpu(), P0[frozen_one])


EPOCH_CASES = only_compiled(C.epoch_cases())


@pytest.mark.parametrize("case", EPOCH_CASES, ids=lambda c: f"d{c[0]}o{c[1]}f{c[2]}-{'q5c' if c[3] else 'none'}-{'pair' if c[4] else 'plain'}-e{c[5]}")
def test_epoch_launch_matches_the_model(S, case):
    """One epoch launch on a hand-written state of 6 problems, one per event: conv without final, final, period hit, period
    miss, NaN, done -- with the threshold's edge values in Xi and, under the map, update norms only the sum of the
    per-tensor norms places right."""
    d, order, flags, mapped, pair, epoch = case
    cfg, Q, n, dp, hs, cl = C.epoch_setup(case)
    dev = GpuDevice(C.S_EPOCH, d, order, flags, Q, True, cfg, pair)
    rep = C.Report()
    codes = C.drive_epoch_case(case, dev, rep)
    assert codes == C.WANT_CODES
    _verdict("epoch launch", rep, C.EPOCH_TOL)


@pytest.mark.parametrize("case", only_compiled(C.FREE_RUN_CASES))
def test_free_running_fit_matches_the_oracle_on_the_large_libraries(S, case):
    """DeviceTrainer(closure="stream") for three epochs of max_iter = 4 over a memory of 3 pairs on 257 points, against
    oracle.lbfgs_fit in fp64 on the same data: Xi after every epoch, no event on either side."""
    from symode_amd.device_lbfgs import DeviceTrainer
    d, order, flags, mapped = case
    x, dx, Q, P0 = C.free_run_data(case)
    want = C.free_run_oracle(case, torch.float64)
    assert want["events"] == [] and len(want["Xi"]) == C.FREE_RUN_EPOCHS
    tr = DeviceTrainer(x[None].to(DEV), dx[None].to(DEV), order, flags, Q=Q, allow_constant=True, lr=C.FREE_RUN_LR, st_freq=0, l1=False,
                       tol=C.FREE_RUN_TOL_UPDATE, max_iter=4, history=3, detail=True, closure="stream")
    seen = []
    tr.fit(P0[None], C.FREE_RUN_EPOCHS, on_epoch=lambda e, rec: seen.append((int(rec["code"][0]), torch.from_numpy(rec["xi"][0]).double())))
    assert [c for c, _ in seen] == [0] * C.FREE_RUN_EPOCHS
    for e, ((_, xi), ref) in enumerate(zip(seen, want["Xi"])):
        dev = float((xi - ref).abs().max() / ref.abs().max())
        print(f"free-running {case} epoch {e}: device against fp64 oracle {dev:.3e} (tolerance {C.FREE_RUN_TOL:.1e})")
    for (_, xi), ref in zip(seen, want["Xi"]):
        assert float((xi - ref).abs().max() / ref.abs().max()) <= C.FREE_RUN_TOL
