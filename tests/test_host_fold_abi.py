"""CPU-side checks of the two entries of the folded linear action (symode_linear_action, symode_loss_grad_reversed_linear):
additions to ABI version 8 that refuse what lies outside their scope (d = 2, flags = 0, orders 1-5, one group element) and bad
arguments before anything is launched (-1 unsupported, -2 null, -3 size, -4 workspace, -5 alignment)."""
import ctypes
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


def test_the_entries_are_additions_to_the_same_abi_version(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8
    for name in ("symode_linear_action", "symode_loss_grad_reversed_linear"):
        assert hasattr(lib, name) and name in engine._SIGNATURES
    # the closure entry: its _constj_live sibling's arguments with the fp64 M table behind the Jacobian table
    mine, theirs = engine._SIGNATURES["symode_loss_grad_reversed_linear"], engine._SIGNATURES["symode_loss_grad_reversed_constj_live"]
    assert mine[0] is theirs[0] and mine[1][:4] + mine[1][5:] == theirs[1] and mine[1][4] is ctypes.c_void_p
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "symode.h")).read()
    assert "symode_linear_action(" in src and "symode_loss_grad_reversed_linear(" in src


def test_detector_argument_checks(lib):
    f = lib.symode_linear_action
    # (x, gx, table, n_g, S, n, d, order, flags, m_out, flag_out, stream)
    ok = [JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, JUNK, NULL]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    assert call(a6=3) == -1 and call(a6=1) == -1                               # d != 2
    assert call(a8=1) == -1 and call(a8=2) == -1 and call(a8=3) == -1          # sine / exp columns
    assert call(a7=6) == -1 and call(a7=0) == -1                               # order outside 1-5
    assert call(a3=2) == -1                                                    # one group element
    assert call(a3=0) == -3 and call(a4=0) == -3 and call(a4=65536) == -3 and call(a5=0) == -3
    for k in (0, 1, 2, 9, 10):
        assert call(**{f"a{k}": NULL}) == -2, k
        assert call(**{f"a{k}": ODD}) == -5, k
    assert call(a9=ctypes.c_void_p(0x1004)) == -5                              # M is fp64


def test_closure_argument_checks(lib):
    f = lib.symode_loss_grad_reversed_linear
    need = lib.symode_workspace_bytes(2, 5, 0, 1, 100)
    # (x, dx, gx, table, m, n_g, S, n, d, order, flags, xi, mask, live, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
    ok = [JUNK, JUNK, JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, NULL, ODD_DEGREES_O5, 1.0, 0.1, JUNK, JUNK, JUNK, 1 << 34, NULL]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    assert call(a8=3) == -1 and call(a10=1) == -1 and call(a9=6) == -1 and call(a5=2) == -1
    assert call(a5=0) == -3 and call(a6=0) == -3 and call(a6=65536) == -3 and call(a7=0) == -3
    for k in (0, 1, 2, 3, 4, 11, 16, 17):
        assert call(**{f"a{k}": NULL}) == -2, k
    for k in (0, 1, 2, 3, 4, 11, 12, 16, 17):
        assert call(**{f"a{k}": ODD}) == -5, k
    assert call(a18=NULL) == -4 and call(a19=need - 8) == -4 and call(a19=0) == -4
    # the same answers whichever kernel family the column set would take, and with the fold turned off
    for live in (0, 0xFFFFFFFFFFFFFFFF, ODD_DEGREES_O5 | 1 << 3):
        assert call(a13=live, a18=NULL) == -4 and call(a13=live, a6=0) == -3 and call(a13=live, a0=NULL) == -2
    old = os.environ.get("SYMODE_CLOSURE_FOLD")
    os.environ["SYMODE_CLOSURE_FOLD"] = "0"
    lib.symode_reload_env()
    try:
        assert call(a18=NULL) == -4 and call(a6=0) == -3 and call(a0=NULL) == -2 and call(a0=ODD) == -5 and call(a4=NULL) == -2
    finally:
        if old is None:
            os.environ.pop("SYMODE_CLOSURE_FOLD")
        else:
            os.environ["SYMODE_CLOSURE_FOLD"] = old
        lib.symode_reload_env()


def test_python_layer_names_the_linear_action():
    import inspect
    from symode_amd.batched import BatchedClosure
    assert inspect.signature(engine.HipEngine.loss_grad_reversed).parameters["linear_m"].default is None
    assert inspect.signature(BatchedClosure.__init__).parameters["linear_action"].default is None
    assert hasattr(engine.HipEngine, "linear_action")
