"""CPU-side checks of symode_loss_grad_latent, the closure of the latent L-BFGS fit: the symbol is exported and bound,
the entry is an addition (it came with ABI version 7, the trainer descriptor naming it as a closure kind), and bad arguments are refused
before anything is launched (codes: -1 unsupported, -2 null, -3 size, -4 workspace, -5 alignment) in the order of the
reversed closure's checks."""
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
# (z, dz, B, y, S, n, d, order, flags, xi, mask, inv_count, w_pair, loss2, grad, ws, ws_bytes, stream)
OK = [JUNK, JUNK, JUNK, JUNK, 1, 100, 2, 3, 0, JUNK, NULL, 1.0, 0.5, JUNK, JUNK, JUNK, 1 << 34, NULL]
PTRS = (0, 1, 2, 3, 9, 13, 14)


def _call(lib, **kw):
    a = list(OK)
    for k, v in kw.items():
        a[int(k[1:])] = v
    return lib.symode_loss_grad_latent(*a)


def test_the_entry_is_exported_bound_and_additive(lib):
    assert hasattr(lib, "symode_loss_grad_latent") and "symode_loss_grad_latent" in engine._SIGNATURES
    res, args = engine._SIGNATURES["symode_loss_grad_latent"]
    assert res is ctypes.c_int and len(args) == len(OK)
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert hasattr(engine.HipEngine, "loss_grad_latent")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "symode.h")).read()
    decl = header[:header.index("int symode_loss_grad_latent(")]
    assert "train.py:647-661 + 689" in decl[decl.rindex("/*"):]                # the reference lines the entry replaces


def test_bad_arguments_are_refused_without_a_gpu(lib):
    assert _call(lib, a6=0) == -1 and _call(lib, a6=9) == -1                   # d = 0, d outside the compiled set
    assert _call(lib, a7=6) == -1 and _call(lib, a7=0) == -1 and _call(lib, a8=4) == -1
    assert _call(lib, a5=0) == -3 and _call(lib, a5=-1) == -3                  # n < 1
    assert _call(lib, a4=0) == -3 and _call(lib, a4=65536) == -3               # problems beyond grid.y
    for k in PTRS:
        assert _call(lib, **{f"a{k}": NULL}) == -2, k                          # every required pointer
    for k in PTRS + (10,):                                                     # (mask may be null, not odd)
        assert _call(lib, **{f"a{k}": ODD}) == -5, k
    need = lib.symode_workspace_bytes(2, 3, 0, 1, 100)
    assert need > 8
    assert _call(lib, a15=NULL) == -4 and _call(lib, a15=ctypes.c_void_p(0x1004)) == -4
    assert _call(lib, a16=need - 8) == -4 and _call(lib, a16=0) == -4


def test_the_checks_come_in_the_order_of_the_reversed_closure(lib):
    # library, sizes, null, alignment, workspace
    assert _call(lib, a6=9, a4=0) == -1
    assert _call(lib, a4=0, a0=NULL) == -3
    assert _call(lib, a0=NULL, a1=ODD) == -2
    assert _call(lib, a0=ODD, a15=NULL) == -5
    # a null mask is "no mask", as everywhere: the call gets as far as the workspace
    assert _call(lib, a10=NULL, a15=NULL) == -4
    # w_pair = 0 is a legal weight (the x-term is still reported)
    assert _call(lib, a12=0.0, a15=NULL) == -4
