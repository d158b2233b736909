"""main_sweep on the MI355X prints and writes what it did before it was split into plan / fit / report.

tests/golden/main_sweep_gpu_transcript.json is this project's OWN output on an MI355X at the commit before that change: the
Adam sweep of test_gpu_adam.py (small noise-free dosc, 4 seeds) and the reversed-regulariser sweeps of
test_gpu_sym_sweep.py (its CASES and N_SEEDS, a frozen random LaLiGAN) in stream and in Gram form.  Masked stdout, file
lists, npz keys / dtypes / shapes and correct_form are compared for equality; the coefficients within the tolerance the
existing test of the same path uses.

The sweeps run in one fresh child process, as they did for the recording (transcripts.record_sweep_gpu_cases): the small LV
and selkov fits are ill-conditioned enough that stream and Gram form of one sweep differ by 3e-3 in a coefficient of
size 4, so last-bit differences in the frozen LaLiGAN's g(x), J_g(x) -- which follow from what the process ran on the GPU
before -- would otherwise be measured against a 1e-3 bound meant for the driver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import transcripts
from tests.test_gpu_adam import TOL as ADAM_TOL, _scaled_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """Each case: one fresh main_sweep.main call in its own directory, all in one child process."""
    out = tmp_path_factory.mktemp("sweep-transcripts") / "got.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    subprocess.run([sys.executable, "-m", "tests.transcripts", str(out)], cwd=ROOT, env=env, check=True, timeout=300,
                   stdout=subprocess.DEVNULL)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("case", transcripts.SWEEP_GPU_CASES)
def test_sweep_prints_and_writes_what_it_did_before(case, swept):
    want, got = transcripts.load("main_sweep_gpu_transcript")[case], swept[case]
    assert got["stdout"] == want["stdout"]
    assert got["files"] == want["files"]
    assert got["npz"] == want["npz"]
    assert got["correct_form"] == want["correct_form"]
    for name in want["files"]:
        a, b = np.array(got["coefficients"][name]), np.array(want["coefficients"][name])
        print(f"{case} {name}: coefficient max abs diff {np.abs(a - b).max():.3e}")
        if case == "adam":              # test_gpu_adam.py's bound on the same trainer (test_train_SIGED_device_adam_is_the_existing_path)
            assert _scaled_err(a, b) <= ADAM_TOL, name
        else:                           # test_gpu_sym_sweep.py::test_masks_equal_single_problem_fits_on_the_same_rows
            assert np.abs(a - b).max() < 1e-3 * max(1.0, np.abs(b).max()), name
