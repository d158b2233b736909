"""Single launches of the device Adam trainer (symode_adam_epochs / symode_adam_epochs_reversed) against the fp64 model of
tests/adam_model.py: every case of tests/adam_cases.py -- one epoch of one or two minibatch steps from an injected state --
is played on the device and compared field by field (params, m, v, xi and the log means within the derived tolerances;
step, mask and the counters exactly), plus the frozen-problem, thresholding-event and bit-for-bit structure cases.
tests/test_host_adam_model.py is the CPU witness of the model, the cases and the tolerances."""
import pytest
import torch

from tests import adam_cases as C
from tests.helpers import only_compiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIBS = only_compiled(C.LIBS)


class GpuDevice:
    """engine.adam_epochs / adam_epochs_reversed on fresh copies of the state: one launch, one synchronise."""

    def __init__(self, S):
        self.eng, self.fields = S.get_engine(), {}

    def launch(self, tables, state, cfg):
        d = cfg["d"]
        if d not in self.fields:
            self.fields[d] = {k: v.to(DEV) for k, v in C.field(d).items()}
        f = self.fields[d]
        p, m, v, step, mask = (state[k].to(DEV).clone() for k in C.STATE_KEYS)
        kw = dict(lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], w_x=cfg["w_x"], w_reg=cfg["w_reg"], l1=cfg["l1"],
                  threshold=cfg["threshold"], st_freq=cfg["st_freq"], epoch0=cfg["epoch0"], near_band=cfg["near_band"],
                  q_eff=None if cfg["q"] is None else cfg["q"].to(DEV), allow_constant=cfg["allow_const"])
        idx = tables.to(DEV).contiguous()
        if cfg["entry"] == "plain":
            xi, log = self.eng.adam_epochs(f["x"], f["dx"], idx, p, m, v, step, mask, cfg["order"], cfg["flags"], **kw)
        else:
            n_g = cfg["n_g"]
            gx, jgx = (f["gx"][:n_g].contiguous(), f["jgx"][:n_g].contiguous()) if n_g else (None, None)
            xi, log = self.eng.adam_epochs_reversed(f["x"], f["dx"], gx, jgx, idx, p, m, v, step, mask, cfg["order"], cfg["flags"],
                                                    w_sym=cfg["w_sym"], **kw)
        torch.cuda.synchronize()
        out = dict(params=p.cpu(), m=m.cpu(), v=v.cpu(), step=step.cpu(), mask=mask.cpu())
        return out, xi.reshape(mask.shape).cpu(), log.cpu()


@pytest.fixture(scope="module")
def dev():
    import symode_amd
    assert torch.cuda.is_available()
    return GpuDevice(symode_amd)


def _verdict(rep, title):
    for k in sorted(C.TOL):
        worst, where = rep.worst.get(k, (0.0, None))
        print(f"adam steps on the device, {title}, {k}: worst {worst:.3e} (tolerance {C.TOL[k]:.1e}) at {where}")
    assert rep.mismatch == [], rep.mismatch[:5]
    assert rep.unsettled == [], rep.unsettled[:5]
    assert rep.over(C.TOL) == {}, rep.over(C.TOL)


def test_every_compiled_library_of_the_grid_is_built():
    assert len(LIBS) >= 6, LIBS                               # d = 4 needs `make ALL=1`; everything else is in the default build


@pytest.mark.parametrize("lib", LIBS, ids=lambda lib: "d%do%df%d" % lib)
def test_single_launches_against_the_fp64_model(dev, lib):
    rep = C.Report()
    cases = C.grid_cases([lib])
    for case in cases:
        C.check_launch(rep, case, dev)
    assert len(cases) == C.PER_LIB + 3 and rep.launches >= len(cases)
    _verdict(rep, "grid d%do%df%d" % lib)


def test_a_frozen_problem_keeps_its_state_and_its_neighbours_do_not_notice(dev):
    rep, cases = C.Report(), C.freeze_cases(LIBS)
    assert cases
    for case in cases:
        C.check_freeze(rep, case, dev)
    _verdict(rep, "freezing")


def test_the_thresholding_event_and_the_near_count(dev):
    rep, cases = C.Report(), C.epoch_cases(LIBS)
    assert cases and any(sum(c.expect["near"]) > 0 for c in cases)
    for case in cases:
        C.check_epoch(rep, case, dev)
    _verdict(rep, "epoch end")


@pytest.mark.parametrize("case", C.structure_cases(LIBS), ids=lambda c: c.name)
def test_two_steps_in_one_launch_equal_two_launches_bit_for_bit(dev, case):
    C.check_structure(case, dev)
