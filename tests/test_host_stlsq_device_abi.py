"""CPU-side checks of symode_stlsq_sweep, the device twin of symode_host_stlsq_sweep: the entry is an addition (declared,
exported, bound with the header's argument count, the ABI version the binding's), and every refusal of the header is an
error code before any device work -- the pointers below are junk and none is dereferenced."""
import os
import re

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
OUTPUTS = ("xi", "mask", "passes", "near", "fell")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _call(lib, aug=JUNK, n_sets=3, n_problems=3, d=2, p=10, n_points=200, hyper=NULL, gamma=0.1, threshold=0.05, max_iter=10,
          near_band=1e-4, xi=JUNK, mask=JUNK, passes=JUNK, near=JUNK, fell=JUNK):
    return lib.symode_stlsq_sweep(aug, n_sets, n_problems, d, p, n_points, hyper, gamma, threshold, max_iter, near_band, xi, mask,
                                  passes, near, fell, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_stlsq_sweep\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_stlsq_sweep")
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_stlsq_sweep"][1]) == 17
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "aug_gram", "n_sets", "n_problems", "d", "p", "n_points", "hyper", "gamma", "threshold", "max_iter", "near_band", "xi_out",
        "mask_out", "passes_out", "near_out", "fell_out", "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    assert "replaces: train.py:872-887 over sindy.py:250-315, unconstrained case." in comment
    assert engine.STLSQ_HYPER == 2
    # the host twin keeps its signature
    host = re.search(r"\bint symode_host_stlsq_sweep\(([^;]*)\);", header)
    assert len(host.group(1).split(",")) == len(engine._SIGNATURES["symode_host_stlsq_sweep"][1]) == 15


def test_every_refusal_is_decided_without_a_device(lib):
    for p in (0, -1, 65, 1000):
        assert _call(lib, p=p) == BADSIZE, p
    for d in (0, -2, 5):
        assert _call(lib, d=d) == BADSIZE, d
    for max_iter in (0, -1):
        assert _call(lib, max_iter=max_iter) == BADSIZE, max_iter
    for n_sets in (0, -3):
        assert _call(lib, n_sets=n_sets, n_problems=3, hyper=JUNK) == BADSIZE, n_sets
    assert _call(lib, n_sets=3, n_problems=2, hyper=JUNK) == BADSIZE                # fewer problems than sets
    assert _call(lib, n_sets=3, n_problems=0, hyper=JUNK) == BADSIZE
    assert _call(lib, n_sets=3, n_problems=2 ** 31, hyper=JUNK) == BADSIZE
    for n_problems in (4, 9, 27):                                                   # without a table: one problem per set
        assert _call(lib, n_sets=3, n_problems=n_problems, hyper=NULL) == BADSIZE, n_problems
    assert _call(lib, aug=NULL) == NULLPTR
    for name in OUTPUTS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
        assert _call(lib, hyper=JUNK, n_problems=27, **{name: NULL}) == NULLPTR, name
    assert _call(lib, aug=0x1004) == ALIGN and _call(lib, hyper=0x1002, n_problems=9) == ALIGN
    for name in ("xi", "passes", "near", "fell"):
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
    # a size before a pointer, as the other entries decide
    assert _call(lib, p=65, aug=NULL) == BADSIZE and _call(lib, n_problems=4, xi=NULL) == BADSIZE


def test_the_engine_takes_device_tensors_only():
    import inspect

    import torch

    import symode_amd
    sig = inspect.signature(engine.HipEngine.stlsq_sweep).parameters
    assert list(sig)[:8] == ["self", "G", "n_points", "gamma", "threshold", "max_iter", "hyper", "n_problems"]
    assert sig["hyper"].default is None and sig["n_problems"].default is None
    with pytest.raises(symode_amd.SymodeError):
        symode_amd.get_engine().stlsq_sweep(torch.zeros(3, 12, 12, dtype=torch.float64), 200, 0.0, 0.1, 10, d=2)
