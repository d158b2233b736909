"""train_SIGED_lbfgs above the engine, on the CPU: which of its four routes a set of arguments takes, and what a fit
prints, logs and saves.

The transcript (tests/golden/train_lbfgs_transcript.json) is this project's OWN output, recorded at the commit before the
trainer was split into routes and closure builders -- not the reference's: it pins the text and the order of the per-epoch
report, the wandb payloads and the checkpoint names while the code above the engine is rearranged."""
import itertools

import pytest
import torch

import symode_amd
from symode_amd.train import _lbfgs_route
from tests import transcripts
from tests.oracle_engine import OracleEngine

torch.set_num_threads(4)

GROUP_MSG = "group=... (point shards) is implemented for the non-latent fit."
GRAM_MSG = ("gram_closure=True needs the device trainer: the non-latent fit with MSE [+ L1] [+ the reversed regulariser on a "
            "frozen autoencoder] on a GPU, without torch_lbfgs / numpy_lbfgs")
# the default fit of a GPU run: every row below changes what it names and nothing else
BASE = dict(is_cuda=True, use_latent=False, w_sym_reg=0.0, sym_reg_type="i", w_sindy_x=1.0, sindy_reg_type="l1", frozen=True,
            group=None, host_lbfgs=True, torch_lbfgs=False, numpy_lbfgs=False, gram_closure=False, torch_optim_env=False,
            mask_numel=256, has_trainer=True)
SHARDS = object()                                          # stands for a process group: the route only asks whether there is one
R = dict(w_sym_reg=0.1, sym_reg_type="r")
# read off the ladder of booleans (frozen / eligible / on_device / one shadow or the other) the trainer had before
TABLE = [
    ({}, "device"),
    (dict(sindy_reg_type="none"), "device"),
    (dict(mask_numel=257), "shadow"),
    (dict(has_trainer=False), "shadow"),
    (dict(w_sindy_x=0.0), "shadow"),
    (dict(torch_lbfgs=True), "shadow"),
    (dict(numpy_lbfgs=True), "shadow"),
    (dict(torch_optim_env=True), "shadow"),
    (R, "device"),
    (dict(R, torch_lbfgs=True), "shadow"),
    (dict(R, numpy_lbfgs=True), "shadow"),
    (dict(R, frozen=False), "host_params"),
    (dict(sym_reg_type="r", frozen=False), "device"),      # weight 0: the regulariser is not there
    (dict(w_sym_reg=0.1, sym_reg_type="i"), "host_params"),
    (dict(w_sym_reg=0.1, sym_reg_type="f"), "host_params"),
    (dict(w_sym_reg=0.1, sym_reg_type="f", numpy_lbfgs=True), "host_params"),
    (dict(use_latent=True), "host_params"),
    (dict(is_cuda=False), "plain"),
    (dict(is_cuda=False, numpy_lbfgs=True), "plain"),
    (dict(is_cuda=False, torch_lbfgs=True, **R), "plain"),
    (dict(host_lbfgs=False), "plain"),
    (dict(host_lbfgs=False, torch_lbfgs=True), "plain"),
    (dict(host_lbfgs=False, use_latent=True), "plain"),
    (dict(group=SHARDS), "device"),
    (dict(group=SHARDS, **R), "device"),
    (dict(group=SHARDS, torch_lbfgs=True), "host_params"),  # the shadow closure is single-rank: shards take the generic one
    (dict(group=SHARDS, mask_numel=257), "host_params"),
    (dict(group=SHARDS, w_sym_reg=0.1, sym_reg_type="i"), "host_params"),
    (dict(group=SHARDS, is_cuda=False), "plain"),
    (dict(group=SHARDS, host_lbfgs=False), "plain"),
    (dict(group=SHARDS, use_latent=True), GROUP_MSG),
    (dict(group=SHARDS, use_latent=True, is_cuda=False), GROUP_MSG),
    (dict(group=SHARDS, use_latent=True, gram_closure=True), GROUP_MSG),
    (dict(gram_closure=True), "device"),
    (dict(gram_closure=True, group=SHARDS, **R), "device"),
    (dict(gram_closure=True, torch_lbfgs=True), GRAM_MSG),
    (dict(gram_closure=True, numpy_lbfgs=True), GRAM_MSG),
    (dict(gram_closure=True, mask_numel=257), GRAM_MSG),
    (dict(gram_closure=True, is_cuda=False), GRAM_MSG),
    (dict(gram_closure=True, use_latent=True), GRAM_MSG),
    (dict(gram_closure=True, host_lbfgs=False), GRAM_MSG),
    (dict(gram_closure=True, w_sym_reg=0.1, sym_reg_type="f"), GRAM_MSG),
]


def _outcome(**kw):
    try:
        return _lbfgs_route(**kw)
    except ValueError as e:
        return str(e)


@pytest.mark.parametrize("change, want", TABLE, ids=[",".join(f"{k}={v}" for k, v in c.items() if k != "group") +
                                                     (",shards" if "group" in c else "") or "default" for c, _ in TABLE])
def test_route_table(change, want):
    assert _outcome(**dict(BASE, **change)) == want


def _ladder_before(is_cuda, use_latent, w_sym_reg, sym_reg_type, w_sindy_x, sindy_reg_type, frozen, group, host_lbfgs,
                   torch_lbfgs, numpy_lbfgs, gram_closure, torch_optim_env, mask_numel, has_trainer):
    """The statements that chose the closure before there was a route function, in their order, with the objects they built
    replaced by their names."""
    if group is not None and use_latent:
        return GROUP_MSG
    closure, shadow = "generic", None
    eligible = (is_cuda and not use_latent and host_lbfgs and (w_sym_reg <= 0.0 or (sym_reg_type == "r" and frozen)))
    on_device = (eligible and not torch_lbfgs and not numpy_lbfgs and not torch_optim_env and w_sindy_x > 0
                 and sindy_reg_type in ("l1", "none") and has_trainer and mask_numel <= 256)
    if eligible and not on_device and group is None:
        shadow, closure = "_HostShadow", "shadow"
    if shadow is None and not on_device and is_cuda and host_lbfgs:
        shadow, closure = "_HostParams", "wrapped generic"
    if gram_closure and not on_device:
        return GRAM_MSG
    if on_device:
        return "device"
    return {"shadow": "shadow", "wrapped generic": "host_params", "generic": "plain"}[closure]


def test_every_combination_of_the_route_inputs_resolves_as_the_ladder_did():
    axes = dict(is_cuda=(False, True), use_latent=(False, True), w_sym_reg=(0.0, 0.1), sym_reg_type=("i", "f", "r"),
                w_sindy_x=(0.0, 1.0), sindy_reg_type=("l1", "none"), frozen=(False, True), group=(None, SHARDS),
                host_lbfgs=(False, True), torch_lbfgs=(False, True), numpy_lbfgs=(False, True), gram_closure=(False, True),
                torch_optim_env=(False, True), mask_numel=(256, 257), has_trainer=(False, True))
    seen = set()
    for values in itertools.product(*axes.values()):
        kw = dict(zip(axes, values))
        got, want = _outcome(**kw), _ladder_before(**kw)
        assert got == want, (kw, got, want)
        seen.add(got)
    assert seen == {"device", "shadow", "host_params", "plain", GROUP_MSG, GRAM_MSG}


@pytest.mark.parametrize("case", transcripts.CPU_CASES)
def test_lbfgs_fit_prints_logs_and_saves_what_it_did_before(golden, case, tmp_path):
    """6 epochs on the damped oscillator through the oracle engine, log / save / threshold intervals 2 / 3 / 2, equations
    printed: without a regulariser and with the infinitesimal one through the stock autoencoder and generator fixture."""
    want = transcripts.load("train_lbfgs_transcript")[case]
    got = transcripts.run_case(symode_amd, golden, case, tmp_path, engine=OracleEngine())
    assert got["stdout"] == want["stdout"]
    assert got["wandb_keys"] == want["wandb_keys"]
    assert got["files"] == want["files"]
    assert torch.equal(torch.tensor(got["mask"]), torch.tensor(want["mask"]))
    assert len(got["params"]) == len(want["params"])
    for a, b in zip(got["params"], want["params"]):
        assert torch.equal(torch.tensor(a), torch.tensor(b))        # the same CPU operations in the same order
