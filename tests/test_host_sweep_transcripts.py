"""main_sweep prints and writes what it did before it was split into plan / fit / report.

tests/golden/main_sweep_transcript.json is this project's OWN output at the commit before that change, on the CPU with the
oracle engine: the set-up of test_host_ltp_sweep.py::test_main_sweep_eval_ltp_adds_its_keys_and_nothing_else_changes (small
noise-free dosc, order 2, 4 seeds), --method lbfgs and stlsq, each with and without --eval_ltp.  Numbers in stdout are
masked on both sides (the file is recorded on one CPU and checked on another; aggregate_results prints four decimals): the
text, the order and the count of the lines are what is pinned, with the file list, every npz key's dtype and shape, and
correct_form."""
import pytest
import torch

from tests import transcripts

torch.set_num_threads(4)


def test_the_mask_covers_integer_decimal_and_exponent_forms():
    assert transcripts.mask_numbers(["4 seeds x 600 points, 1-2; 0: 1.2e-05, 199, -3.4E+2 .5 [0, 3] 1/1 nan"]) == \
        ["# seeds x # points, #-#; #: #, #, # # [#, #] #/# nan"]


@pytest.mark.parametrize("case", transcripts.SWEEP_CPU_CASES)
def test_sweep_prints_and_writes_what_it_did_before(case, tmp_path):
    want = transcripts.load("main_sweep_transcript")[case]
    got = transcripts.run_sweep_cpu_case(case, tmp_path)
    assert got["stdout"] == want["stdout"]
    assert got["files"] == want["files"]
    assert got["npz"] == want["npz"]
    assert got["correct_form"] == want["correct_form"]
