"""CPU-side checks of symode_loss_grad_reversed_linear_quad, an addition to ABI version 8: the declaration, the binding's
argument count, and the argument validation, which returns its codes before anything is launched (-1 unsupported, -2 null,
-3 size, -4 workspace, -5 alignment)."""
import ctypes
import os
import re

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "symode_loss_grad_reversed_linear_quad"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def test_declaration_and_binding_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "symode.h")).read(), flags=re.S)
    decl = re.search(NAME + r"\s*\(([^)]*)\)", src)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(engine._SIGNATURES[NAME][1]) == 29


def call(lib, **over):
    buf = (ctypes.c_double * 5000)()
    good = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(None)
    a = dict(aug=good, m=good, table=good, n_g=1, S=3, d=2, order=5, flags=0, xi=good, q=null, beta=null, ldb=0, const=null, ldc=0,
             r=0, use_kron=1, mask=null, live=0xFFFFFFFFFFFFFFFF, inv=1.0, w=0.1, loss2=good, loss=null, grad=good, xi_out=null,
             g_beta=null, g_const=null, ws=good, ws_bytes=0, stream=null)
    a.update(over)
    return getattr(lib, NAME)(*a.values())


def test_argument_validation_needs_no_gpu(lib):
    buf = (ctypes.c_double * 8)()
    good = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    null = ctypes.c_void_p(None)
    assert call(lib, d=3) == -1 and call(lib, order=6) == -1 and call(lib, flags=1) == -1 and call(lib, n_g=2) == -1
    assert call(lib, n_g=0) == -3 and call(lib, S=0) == -3
    for name in ("aug", "m", "table", "xi", "loss2", "grad"):
        assert call(lib, **{name: null}) == -2, name
    # the map: q brings beta and g_beta and takes xi's place; without it the map's operands must be absent
    assert call(lib, q=good) == -2 and call(lib, beta=good) == -2 and call(lib, g_beta=good) == -2 and call(lib, xi_out=good) == -2
    mapped = dict(xi=null, q=good, beta=good, ldb=6, g_beta=good, r=6)
    assert call(lib, **mapped) == -4                                   # everything in order up to the workspace
    assert call(lib, **dict(mapped, xi=good)) == -2 and call(lib, **dict(mapped, g_beta=null)) == -2
    assert call(lib, **dict(mapped, r=0)) == -3 and call(lib, **dict(mapped, r=43)) == -3 and call(lib, **dict(mapped, ldb=5)) == -3
    assert call(lib, **dict(mapped, const=good, ldc=1)) == -3
    for name in ("aug", "m", "table", "xi", "mask", "loss2", "loss", "grad"):
        assert call(lib, **{name: odd}) == -5, name
    assert call(lib) == -4 and call(lib, ws=null, ws_bytes=1 << 20) == -4 and call(lib, ws=odd, ws_bytes=1 << 20) == -4


def test_the_switches_refuse_the_call(lib):
    for knob in ("SYMODE_FOLD_RESID_GRAM", "SYMODE_FOLD_GRAM", "SYMODE_CLOSURE_FOLD"):
        old = os.environ.get(knob)
        os.environ[knob] = "0"
        try:
            lib.symode_reload_env()
            assert call(lib) == -1, knob
            assert not engine.HipEngine.closure_quad_enabled()
        finally:
            if old is None:
                os.environ.pop(knob)
            else:
                os.environ[knob] = old
            lib.symode_reload_env()
    assert call(lib) == -4 and engine.HipEngine.closure_quad_enabled()
