"""CPU-side checks of symode_weak_normal_windows: the entry is an addition (declared, exported, bound with the header's
argument count, the ABI version unchanged), and every refusal of the header is an error code before any device work -- the
pointers below are junk and none is dereferenced."""
import os
import re

import numpy as np
import pytest
import torch

import symode_amd
from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
POINTERS = ("x", "windows", "V", "V_drv", "M", "aug", "bad")
HEADER_DOUBLES = 8 + 32768                     # WS_HEADER_DOUBLES of csrc/kernels.hpp


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _need(n_windows, n_t, n_test, F):
    """bytes of workspace the entry asks for"""
    gx = min(64, (n_t + 255) // 256)
    return 8 * (HEADER_DOUBLES + n_windows * ((2 * n_test + 15) // 16) * gx * ((F + 15) // 16) * 256)


def _call(lib, x=JUNK, n_ics=3, n_steps=200, d=2, order=3, flags=0, windows=JUNK, n_windows=7, n_t=160, V=JUNK, V_drv=JUNK,
          n_test=50, M=JUNK, aug=JUNK, z=NULL, bad=JUNK, ws=JUNK, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.symode_weak_normal_windows(x, n_ics, n_steps, d, order, flags, windows, n_windows, n_t, V, V_drv, n_test, M, aug,
                                          z, bad, ws, ws_bytes, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_weak_normal_windows\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_weak_normal_windows")
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_weak_normal_windows"][1]) == 19
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "x", "n_ics", "n_steps", "d", "order", "flags", "windows", "n_windows", "n_t", "V", "V_drv", "n_test", "M", "aug_out",
        "z_out", "bad_out", "workspace", "workspace_bytes", "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    assert "replaces:" in comment and "main_wsindy.py:24-29 + sindy.py:362-370" in comment
    # the single-trajectory entry keeps its signature
    one = re.search(r"\bint symode_weak_gram\(([^;]*)\);", header)
    assert len(one.group(1).split(",")) == len(engine._SIGNATURES["symode_weak_gram"][1]) == 12


def test_every_refusal_is_decided_without_a_device(lib):
    for n_t in (0, -1, 201, 10 ** 6):                                   # n_t < 1, n_t > n_steps
        assert _call(lib, n_t=n_t) == BADSIZE, n_t
    for n_ics in (0, -1):
        assert _call(lib, n_ics=n_ics) == BADSIZE, n_ics
    for n_windows in (0, -7, 65536):
        assert _call(lib, n_windows=n_windows) == BADSIZE, n_windows
    for n_test in (0, -1, 129):
        assert _call(lib, n_test=n_test) == BADSIZE, n_test
    assert _call(lib, n_test=128) != BADSIZE
    # d > 4 and libraries outside the compiled set have no ops table: the code the neighbouring entries give
    for d, order, flags in ((5, 1, 0), (0, 1, 0), (2, 6, 0), (2, 3, 4)):
        assert _call(lib, d=d, order=order, flags=flags) == UNSUPPORTED, (d, order, flags)
    for name in POINTERS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
    assert _call(lib, z=NULL, ws=NULL) == WORKSPACE                     # z_out alone may be NULL
    for name in ("x", "windows", "V", "V_drv", "bad"):
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
    for name in ("M", "aug", "z"):
        assert _call(lib, **{name: 0x1004}) == ALIGN, name
    assert _call(lib, ws=0x1004) == WORKSPACE
    # a workspace one byte short of the windows' partials (d = 2, order 3: F = 12), and of a three-slab launch
    assert _call(lib, ws_bytes=_need(7, 160, 50, 12) - 1) == WORKSPACE
    assert _call(lib, n_steps=711, n_t=700, ws_bytes=_need(7, 700, 50, 12) - 1) == WORKSPACE
    assert _call(lib, ws_bytes=0) == WORKSPACE
    # a size before a pointer, as the other entries decide
    assert _call(lib, n_t=201, x=NULL) == BADSIZE and _call(lib, n_test=129, aug=NULL) == BADSIZE


def test_the_engine_checks_the_table_on_the_host():
    """engine.weak_normal_windows raises on an out-of-range row before anything is uploaded or launched: here there is no
    device, and the tensors are host tensors the entry would refuse next."""
    eng = symode_amd.get_engine()
    x = torch.zeros(3, 171, 2)
    V, M = torch.zeros(5, 160), torch.zeros(5, 5, dtype=torch.float64)
    good = [[0, 0], [1, 5], [2, 11]]
    for row, bad in ((1, [3, 0]), (2, [0, 12]), (0, [-1, 0]), (1, [0, -1])):
        table = np.array(good)
        table[row] = bad
        with pytest.raises(symode_amd.SymodeError, match=rf"windows\[{row}\] = \[{bad[0]}, {bad[1]}\] is out of range"):
            eng.weak_normal_windows(x, table, 160, V, V, M, 3)
    assert engine.HipEngine.check_windows(np.array(good), 3, 171, 160).dtype == np.int32
    with pytest.raises(symode_amd.SymodeError, match="host integer array"):
        eng.weak_normal_windows(x, np.zeros((3, 2)), 160, V, V, M, 3)
    with pytest.raises(symode_amd.SymodeError, match="n_t = 172"):
        eng.weak_normal_windows(x, np.array(good), 172, V, V, M, 3)
