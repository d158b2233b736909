"""tests/weak_sweep_model.py -- the fp64 restatement of the weak-SINDy seed sweep that the GPU tests compare with -- against
the per-seed route it restates: WSINDyWrapper + the loop of train_WSINDy on tests.oracle_engine.OracleEngine, driver gels,
on every copied window.  Masks and passes are equal; the coefficients agree within 1e-6 of the largest one (1.2e-7 was
seen: the model takes gamma = sqrt(w_sindy_reg) rounded to fp32, as the device launch does, the wrapper w_sindy_reg itself)."""
import numpy as np
import pytest
import torch

from symode_amd.sindy import weak_test_functions
from symode_amd.sweep import weak_windows
from tests import weak_sweep_model as W
from tests.oracle_engine import OracleEngine

SEEDS = range(8)


@pytest.fixture(scope="module")
def problem():
    x3 = W.dosc_data()
    win = weak_windows(SEEDS, W.N_ICS, W.N_STEPS, W.N_T)
    _, _, V, V_drv, M = weak_test_functions(torch.arange(W.N_T) * W.DT, W.N_T * W.DT, W.K, "trig", "cpu")
    return x3, win, W.normals(x3, win, W.N_T, V, V_drv, M, W.ORDER)


def test_the_windows_are_valid_and_differ(problem):
    _, win, Ns = problem
    assert ((win[:, 0] >= 0) & (win[:, 0] < W.N_ICS) & (win[:, 1] >= 0) & (win[:, 1] <= W.N_STEPS - W.N_T)).all()
    assert len({tuple(r) for r in win.tolist()}) > 1
    assert all(np.allclose(N, N.T, rtol=1e-12, atol=0) for N in Ns)


@pytest.mark.parametrize("w_sindy_reg, threshold", W.FIT_POINTS + ((0.0, 0.05), (1e-2, 0.1)))
def test_model_against_the_per_seed_route(problem, w_sindy_reg, threshold):
    x3, win, Ns = problem
    xi, mask, passes, near = W.per_seed(x3, win, W.N_T, W.DT, W.ORDER, w_sindy_reg, threshold, engine=OracleEngine())
    mxi, mmask, mpasses, mnear = W.sweep(Ns, 2, W.N_T, w_sindy_reg, threshold)
    assert (near == 0).all() and (mnear == 0).all()             # no decision of either side hangs on a rounding
    assert np.array_equal(mask, mmask) and np.array_equal(passes, mpasses)
    for s in range(len(win)):
        assert np.abs(xi[s] - mxi[s]).max() <= 1e-6 * np.abs(xi[s]).max(), s


@pytest.mark.parametrize("w_sindy_reg, threshold", W.FIT_POINTS)
def test_the_fit_points_meet_the_conditions_the_gpu_test_asserts(problem, w_sindy_reg, threshold):
    _, _, Ns = problem
    _, mask, passes, near = W.sweep(Ns, 2, W.N_T, w_sindy_reg, threshold)
    assert W.conditions(mask, passes, near) == (True, True, True)
