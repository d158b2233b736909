"""Every GPU route of the trainers prints, logs and saves what it did before train_SIGED_lbfgs was split into routes and
closure builders.

tests/golden/train_gpu_transcript.json is this project's OWN output on an MI355X at the commit before that change, not the
reference's: 512 points of the damped oscillator, d = 2, order 3, 6 L-BFGS epochs (2 Adam epochs of batch 128), log / save
/ threshold intervals that all fall inside the run.  Text, payload keys, checkpoint names and the mask are compared for
equality; the coefficients within the tolerance the existing test of the same route uses."""
import numpy as np
import pytest
import torch

from tests import transcripts
from tests.test_gpu_adam import TOL as ADAM_TOL, _scaled_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# test_gpu_train.py::test_lbfgs_trainer_on_gpu_matches_reference_run (device, host_torch, host_numpy modes) /
# ::test_reversed_regulariser_host_and_device_lbfgs_agree / ::test_host_resident_variables_for_autograd_closures
CLOSE = {"device": dict(rtol=1e-3, atol=1e-4), "shadow_torch": dict(rtol=1e-3, atol=1e-4), "shadow_numpy": dict(rtol=1e-3, atol=1e-4),
         "device_r": dict(rtol=2e-2, atol=2e-3), "host_params_f": dict(rtol=2e-2, atol=2e-3)}


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd


@pytest.mark.parametrize("case", transcripts.GPU_CASES)
def test_route_prints_logs_and_saves_what_it_did_before(S, golden, case, tmp_path):
    want = transcripts.load("train_gpu_transcript")[case]
    got = transcripts.run_case(S, golden, case, tmp_path, dev=DEV)
    assert got["stdout"] == want["stdout"]
    assert got["wandb_keys"] == want["wandb_keys"]
    assert got["files"] == want["files"]
    mask = np.array(want["mask"])
    assert np.array_equal(np.array(got["mask"]), mask)
    a, b = np.array(got["params"][0]) * mask, np.array(want["params"][0]) * mask
    print(f"{case}: coefficient max abs diff {np.abs(a - b).max():.3e}")
    if case == "adam_r":                                   # test_gpu_adam_reversed.py's bound on the same trainer
        assert _scaled_err(a, b) <= ADAM_TOL
    else:
        assert np.allclose(a, b, **CLOSE[case])
