"""Single launches of the device Adam trainer's latent entry (symode_adam_epochs_latent) against the fp64 model of
tests/adam_latent_model.py: every case of tests/adam_latent_cases.py -- one epoch of one or two minibatch steps from an
injected state -- is played on the device and compared field by field (params, m, v, xi and the log means within the
derived tolerances; step, mask and the counters exactly), plus the frozen-problem, thresholding-event and bit-for-bit
structure cases, the entry against symode_adam_epochs where the two losses coincide, and two identical calls.
tests/test_host_adam_latent_model.py is the CPU witness of the model, the cases and the tolerances."""
import pytest
import torch

from tests import adam_latent_cases as C
from tests.helpers import only_compiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIBS = only_compiled(C.LIBS)


class GpuDevice:
    """engine.adam_epochs_latent on fresh copies of the state: one launch, one synchronise."""

    def __init__(self, S):
        self.eng, self.fields = S.get_engine(), {}

    def field(self, d):
        if d not in self.fields:
            self.fields[d] = {k: v.to(DEV) for k, v in C.field(d).items()}
        return self.fields[d]

    def launch(self, tables, state, cfg):
        f = self.field(cfg["d"])
        p, m, v, step, mask = (state[k].to(DEV).clone() for k in C.STATE_KEYS)
        n_gen = cfg["n_gen"]
        xi, log = self.eng.adam_epochs_latent(
            f["z"], f["dz"], f["B"], f["y"], f["e"] if cfg["D_obs"] > cfg["d"] else None, cfg["D_obs"],
            f["L"][:n_gen].contiguous() if n_gen else None, tables.to(DEV).contiguous(), p, m, v, step, mask, cfg["order"], cfg["flags"],
            w_z=cfg["w_z"], w_sym=cfg["w_sym"], lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], w_x=cfg["w_x"],
            w_reg=cfg["w_reg"], l1=cfg["l1"], threshold=cfg["threshold"], st_freq=cfg["st_freq"], epoch0=cfg["epoch0"],
            near_band=cfg["near_band"], q_eff=None if cfg["q"] is None else cfg["q"].to(DEV), allow_constant=cfg["allow_const"])
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
        print(f"adam latent steps on the device, {title}, {k}: worst {worst:.3e} (tolerance {C.TOL[k]:.1e}) at {where}")
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


@pytest.mark.parametrize("lib, form, batch", [((2, 5, 0), "xi", 257), ((3, 3, 1), "q5c", 513), ((1, 3, 0), "q1", 64)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_without_generators_and_with_an_identity_decoder_it_is_the_plain_entry_bit_for_bit(dev, lib, form, batch):
    """n_gen = 0, B = I, y = dz, D_obs = d and any w_x: params, m, v and mask are those of symode_adam_epochs on (z, dz) with
    its w_x = w_z, bit for bit -- two epochs of two steps with a thresholding event between them."""
    d, (p, dp) = lib[0], C.lib_dims(lib)
    cfg = C._cfg(lib, "weighted", form, 0, 0, threshold=0.1, st_freq=1)
    gen = torch.Generator().manual_seed(61 + dp)
    n_par = dp if cfg["q"] is None else cfg["q"].shape[1] + d
    state = C._state(2, n_par, d, p, [0, 9], ["ones", "half"], True, gen)
    idx = torch.stack([torch.stack([torch.stack([C._rows(batch, pad, gen) for pad in ("scattered", "tail")]) for _ in range(2)])
                       for _ in range(2)]).contiguous().to(DEV)                  # (2 epochs, 2 problems, 2 steps, batch)
    f = dev.field(d)
    kw = dict(lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], w_reg=cfg["w_reg"], l1=cfg["l1"], threshold=cfg["threshold"],
              st_freq=cfg["st_freq"], epoch0=0, near_band=cfg["near_band"], q_eff=None if cfg["q"] is None else cfg["q"].to(DEV),
              allow_constant=cfg["allow_const"])
    a = [state[k].to(DEV).clone() for k in C.STATE_KEYS]
    b = [state[k].to(DEV).clone() for k in C.STATE_KEYS]
    eye = torch.eye(d, device=DEV).expand(C.N_SRC, d, d).contiguous()
    dev.eng.adam_epochs_latent(f["z"], f["dz"], eye, f["dz"], None, d, None, idx, *a, cfg["order"], cfg["flags"], w_z=cfg["w_z"],
                               w_sym=0.3, w_x=5.0, **kw)
    dev.eng.adam_epochs(f["z"], f["dz"], idx, *b, cfg["order"], cfg["flags"], w_x=cfg["w_z"], **kw)
    torch.cuda.synchronize()
    got, want = ({k: t.cpu() for k, t in zip(C.STATE_KEYS, side)} for side in (a, b))
    assert C.same_bits(got, want) == [], C.same_bits(got, want)
    assert got["step"].tolist() == [4, 13] and not C._bytes_equal(got["params"], state["params"])
    assert float(got["mask"].sum()) < float(state["mask"].sum())              # the events removed something


def test_two_identical_calls_are_bit_identical(dev):
    case = [c for c in C.structure_cases(LIBS) if c.cfg["n_gen"] == 3][-1]
    one, xi1, log1 = dev.launch(case.tables, case.state, case.cfg)
    two, xi2, log2 = dev.launch(case.tables, case.state, case.cfg)
    assert C.same_bits(one, two) == [] and C._bytes_equal(xi1, xi2) and C._bytes_equal(log1, log2)
