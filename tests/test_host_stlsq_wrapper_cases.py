"""The synthetic operands of tests/test_gpu_stlsq_wrappers.py flag nothing in the numpy models of the six kernels: that test asserts
``fell`` zero on the device so that it compares real fits, and this is why it may."""
import numpy as np
import pytest

from tests import stlsq_wrapper_cases as W


@pytest.mark.parametrize("d,p", W.SHAPES)
@pytest.mark.parametrize("allow_constant", (False, True))
def test_no_model_flags_a_problem(d, p, allow_constant):
    o = W.operands(d, p, allow_constant)
    assert o["G"].shape == (W.S, p + d, p + d) and o["V"].shape == (1, p + d, p + d) and o["R"].shape == (W.S, d * p, d * p)
    assert o["q_xi"].shape == (d * p, W.R_FREE) and o["q_solve"].shape == (d * p, W.R_FREE + (d if allow_constant else 0))
    assert np.linalg.eigvalsh(o["R"]).min() > -1e-9 and np.linalg.eigvalsh(o["G"]).min() > 0
    fell = W.modelled_fell(d, p, allow_constant)
    assert sorted(fell) == ["stlsq_path", "stlsq_path_symreg", "stlsq_sweep", "stlsq_sweep_constrained", "stlsq_sweep_minnorm",
                            "stlsq_sweep_symreg"]
    for name, flags in fell.items():
        assert len(flags) in (W.GRID, W.S + W.GRID) and not any(flags), (name, flags)
