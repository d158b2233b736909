"""CPU-side checks of symode_rollout_error's C ABI: argument validation returns error codes before any launch (no GPU
needed), the entry is declared, exported and bound, and is additive (it came with ABI version 7, the L-BFGS trainer descriptor's)."""
import ctypes
import os

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # a non-null, aligned pointer that is never dereferenced (validation fails first)
ODD = ctypes.c_void_p(0x1002)
INF = float("inf")


def test_rollout_error_argument_validation_needs_no_gpu(lib):
    f = lib.symode_rollout_error
    # (x_true, n_ics, n_steps, d, order, flags, xi, mask, n_models, dt, method, bound, err, mean_err, horizon, stream)
    assert f(JUNK, 10, 100, 7, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -1       # no such library
    assert f(JUNK, 10, 100, 2, 6, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -1       # order outside the set
    assert f(JUNK, 10, 100, 2, 2, 4, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -1       # flags outside the set
    assert f(JUNK, 10, 0, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -3         # n_steps <= 0
    assert f(JUNK, 10, -5, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -3
    assert f(JUNK, -1, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -3       # n_ics < 0
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, -1, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -3      # n_models < 0
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 2, INF, JUNK, JUNK, JUNK, NULL) == -3       # method: 0 or 1
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, -1, INF, JUNK, JUNK, JUNK, NULL) == -3
    assert f(JUNK, 1 << 20, 100, 2, 2, 0, JUNK, NULL, 1 << 20, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -3   # > 2^31 - 1 lanes
    assert f(NULL, 0, 100, 2, 2, 0, NULL, NULL, 4, 0.2, 1, INF, NULL, NULL, NULL, NULL) == 0         # empty: nothing to do
    assert f(NULL, 10, 100, 2, 2, 0, NULL, NULL, 0, 0.2, 1, INF, NULL, NULL, NULL, NULL) == 0
    assert f(NULL, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -2       # x_true
    assert f(JUNK, 10, 100, 2, 2, 0, NULL, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -2       # xi
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, NULL, JUNK, NULL) == -2       # mean_err
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, NULL, NULL) == -2       # horizon
    assert f(ODD, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -5
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, ODD, 4, 0.2, 1, INF, JUNK, JUNK, JUNK, NULL) == -5
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, ODD, JUNK, JUNK, NULL) == -5
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, ctypes.c_void_p(0x1004), JUNK, NULL) == -5   # fp64: 8-aligned
    assert f(JUNK, 10, 100, 2, 2, 0, JUNK, NULL, 4, 0.2, 1, INF, JUNK, JUNK, ODD, NULL) == -5


def test_the_entry_is_additive_abi_version_is_the_bindings(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert "symode_rollout_error" in engine._SIGNATURES
    assert "symode_rollout_error" in open(os.path.join(ROOT, "include", "symode.h")).read()
    assert hasattr(lib, "symode_rollout_error")


def test_python_layer_names_the_new_entry_points():
    from symode_amd import evaluation
    assert hasattr(engine.HipEngine, "rollout_error")
    assert hasattr(evaluation, "eval_ltp_sweep") and hasattr(evaluation, "val_mse_sweep")


def test_engine_rollout_error_refuses_cpu_tensors():
    """No CPU fallback: a host tensor is refused before anything else is looked at.  (The shape refusals need device
    tensors: tests/test_gpu_ltp_sweep.py::test_engine_rollout_error_refuses_bad_shapes.)"""
    import torch
    import symode_amd
    eng = symode_amd.get_engine()
    with pytest.raises(symode_amd.SymodeError, match="x_true must be a CUDA/HIP tensor"):
        eng.rollout_error(torch.zeros(3, 11, 2), torch.zeros(4, 2, 6), None, 2, 0, 0.1)
