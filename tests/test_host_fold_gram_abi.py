"""CPU-side checks of symode_loss_grad_reversed_linear_gram: an addition to ABI version 8 with the _linear entry's arguments
plus the fp64 Gram table behind the M table; it refuses what that entry refuses, and a null or misaligned Gram table, before
anything is launched (-1 unsupported, -2 null, -3 size, -4 workspace, -5 alignment)."""
import ctypes
import inspect
import os

import pytest

from symode_amd import engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # a non-null, aligned pointer that is never dereferenced (validation fails first)
ODD = ctypes.c_void_p(0x1002)
ODD_DEGREES_O5 = 0x1F83C7
NAME = "symode_loss_grad_reversed_linear_gram"


def test_the_entry_is_an_addition_to_the_same_abi_version(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8
    assert hasattr(lib, NAME) and NAME in engine._SIGNATURES
    mine, theirs = engine._SIGNATURES[NAME], engine._SIGNATURES["symode_loss_grad_reversed_linear"]
    assert mine[0] is theirs[0] and mine[1][:5] + mine[1][6:] == theirs[1] and mine[1][5] is ctypes.c_void_p
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "symode.h")).read()
    assert NAME + "(" in src and "const double* g_table" in src


@pytest.mark.parametrize("knob", [None, "0", "2"])
def test_argument_checks(lib, knob):
    f = getattr(lib, NAME)
    need = lib.symode_workspace_bytes(2, 5, 0, 1, 100)
    # (x, dx, gx, table, m, g, n_g, S, n, d, order, flags, xi, mask, live, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
    ok = [JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, NULL, ODD_DEGREES_O5, 1.0, 0.1, JUNK, JUNK, JUNK, 1 << 34, NULL]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    old = os.environ.get("SYMODE_FOLD_GRAM")
    if knob is not None:
        os.environ["SYMODE_FOLD_GRAM"] = knob
    lib.symode_reload_env()
    try:
        assert call(a9=3) == -1 and call(a11=1) == -1 and call(a10=6) == -1 and call(a10=0) == -1 and call(a6=2) == -1
        assert call(a6=0) == -3 and call(a7=0) == -3 and call(a7=65536) == -3 and call(a8=0) == -3
        for k in (0, 1, 2, 3, 4, 5, 12, 17, 18):
            assert call(**{f"a{k}": NULL}) == -2, k
        for k in (0, 1, 2, 3, 4, 5, 12, 13, 17, 18):
            assert call(**{f"a{k}": ODD}) == -5, k
        assert call(a5=ctypes.c_void_p(0x1004)) == -5 and call(a4=ctypes.c_void_p(0x1004)) == -5          # fp64 tables
        assert call(a19=NULL) == -4 and call(a20=need - 8) == -4 and call(a20=0) == -4
        # the same answers whichever kernel family the column set would take
        for live in (0, 0xFFFFFFFFFFFFFFFF, ODD_DEGREES_O5 | 1 << 3):
            assert call(a14=live, a19=NULL) == -4 and call(a14=live, a7=0) == -3 and call(a14=live, a0=NULL) == -2
            assert call(a14=live, a5=NULL) == -2
    finally:
        if old is None:
            os.environ.pop("SYMODE_FOLD_GRAM", None)
        else:
            os.environ["SYMODE_FOLD_GRAM"] = old
        lib.symode_reload_env()


def test_python_layer_names_the_gram_form():
    from symode_amd.batched import BatchedClosure
    assert inspect.signature(engine.HipEngine.loss_grad_reversed).parameters["gram"].default is None
    assert inspect.signature(BatchedClosure.__init__).parameters["regulariser_gram"].default is None
    assert hasattr(engine.HipEngine, "closure_gram")
    assert len(inspect.signature(engine.HipEngine.closure_levers).parameters) == 1
