"""CPU-side checks of symode_quad_reduce and symode_quad_step, additions to ABI version 8: the declarations, the bindings'
argument counts, and the argument validation, which returns its codes before anything is launched (-1 unsupported, -2 null,
-3 size, -4 workspace, -5 alignment)."""
import ctypes
import os
import re

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SYMODE_QUAD_REDUCED", "SYMODE_FOLD_RESID_GRAM", "SYMODE_FOLD_GRAM", "SYMODE_CLOSURE_FOLD")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


@pytest.mark.parametrize("name,count", [("symode_quad_reduce", 15), ("symode_quad_step", 16)])
def test_declaration_and_binding_agree(name, count):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "symode.h")).read(), flags=re.S)
    decl = re.search(name + r"\s*\(([^)]*)\)", src)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(engine._SIGNATURES[name][1]) == count


def test_abi_version_stays(lib):
    assert lib.symode_abi_version() == 8


BUF = (ctypes.c_double * 5000)()
GOOD = ctypes.cast(BUF, ctypes.c_void_p)
ODD = ctypes.c_void_p(ctypes.addressof(BUF) + 2)
NULL = ctypes.c_void_p(None)


def reduce_(lib, **over):
    a = dict(aug=GOOD, m=GOOD, table=GOOD, S=3, order=5, q=GOOD, r=6, use_kron=1, has_const=1, live=0xFFFFFFFFFFFFFFFF, inv=1.0, w=0.1,
             mask=NULL, b=GOOD, stream=NULL)
    a.update(over)
    return lib.symode_quad_reduce(*a.values())


def step(lib, **over):
    a = dict(b=GOOD, S=3, k=8, d_c=2, order=5, live=0xFFFFFFFFFFFFFFFF, beta=GOOD, ldb=6, const=GOOD, ldc=2, loss=GOOD, g_beta=GOOD,
             g_const=GOOD, ws=GOOD, ws_bytes=0, stream=NULL)
    a.update(over)
    return lib.symode_quad_step(*a.values())


def test_reduce_validation_needs_no_gpu(lib):
    assert reduce_(lib, order=0) == -1 and reduce_(lib, order=6) == -1
    assert reduce_(lib, S=0) == -3 and reduce_(lib, r=0) == -3 and reduce_(lib, r=43) == -3
    # K + 1 <= 16: r + 2 constants + 1, and r + 1 without them
    assert reduce_(lib, r=14) == -3 and reduce_(lib, r=16, has_const=0) == -3
    for name in ("aug", "m", "table", "q", "b"):
        assert reduce_(lib, **{name: NULL}) == -2, name
    for name in ("aug", "m", "table", "q", "mask", "b"):
        assert reduce_(lib, **{name: ODD}) == -5, name
    half = ctypes.c_void_p(ctypes.addressof(BUF) + 4)               # fp32 alignment is enough for fp32 operands, not for fp64
    assert reduce_(lib, b=half) == -5 and reduce_(lib, aug=half) == -5 and reduce_(lib, m=half) == -5


def test_step_validation_needs_no_gpu(lib):
    assert step(lib, order=0) == -1 and step(lib, order=6) == -1
    assert step(lib, S=0) == -3 and step(lib, k=0) == -3 and step(lib, k=16, ldb=14) == -3
    assert step(lib, d_c=-1) == -3 and step(lib, d_c=8) == -3
    assert step(lib, ldb=5) == -3 and step(lib, ldc=1) == -3
    for name in ("b", "beta", "loss", "g_beta", "const", "g_const"):
        assert step(lib, **{name: NULL}) == -2, name
    # without constants their operands must be absent
    bare = dict(d_c=0, k=6, const=NULL, ldc=0, g_const=NULL)
    assert step(lib, **bare) == -4
    assert step(lib, **dict(bare, const=GOOD)) == -2 and step(lib, **dict(bare, g_const=GOOD)) == -2
    for name in ("b", "beta", "const", "loss", "g_beta", "g_const"):
        assert step(lib, **{name: ODD}) == -5, name
    assert step(lib, b=ctypes.c_void_p(ctypes.addressof(BUF) + 4)) == -5
    # everything in order up to the workspace header
    assert step(lib) == -4 and step(lib, ws=NULL, ws_bytes=1 << 20) == -4 and step(lib, ws=ODD, ws_bytes=1 << 20) == -4


def test_the_switches_refuse_the_calls(lib):
    for knob in KNOBS:
        old = os.environ.get(knob)
        os.environ[knob] = "0"
        try:
            lib.symode_reload_env()
            assert step(lib) == -1 and reduce_(lib, b=NULL) == -1, knob
            assert not engine.HipEngine.closure_reduced_enabled()
        finally:
            if old is None:
                os.environ.pop(knob)
            else:
                os.environ[knob] = old
            lib.symode_reload_env()
    assert step(lib) == -4 and reduce_(lib, b=NULL) == -2 and engine.HipEngine.closure_reduced_enabled()
    # the new switch leaves the closure it stands for alone
    os.environ["SYMODE_QUAD_REDUCED"] = "0"
    try:
        lib.symode_reload_env()
        assert engine.HipEngine.closure_quad_enabled() and not engine.HipEngine.closure_reduced_enabled()
    finally:
        os.environ.pop("SYMODE_QUAD_REDUCED")
        lib.symode_reload_env()
