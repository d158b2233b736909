"""CPU-side checks of symode_stlsq_sweep_symreg: the entry is an addition (declared, exported, bound with the header's argument
count, the ABI version unchanged), every refusal of the header is an error code before any device work -- the pointers below
are junk and none is dereferenced -- and the solve the kernel performs is stated once (csrc/stlsq_joint.hpp), shared with the
constrained kernel."""
import os
import re

import pytest
import torch

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc")
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
POINTERS = ("aug", "rev", "xi", "mask", "passes", "near", "fell")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _call(lib, aug=JUNK, rev=JUNK, n_sets=3, n_problems=3, d=2, p=10, n_points=200, hyper=NULL, gamma=0.1, threshold=0.05, w_sym=1.0,
          max_iter=10, near_band=1e-4, pivot_floor=1e-14, xi=JUNK, mask=JUNK, passes=JUNK, near=JUNK, fell=JUNK):
    return lib.symode_stlsq_sweep_symreg(aug, rev, n_sets, n_problems, d, p, n_points, hyper, gamma, threshold, w_sym, max_iter,
                                         near_band, pivot_floor, xi, mask, passes, near, fell, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8         # an added entry leaves the version (include/symode.h)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_stlsq_sweep_symreg\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_stlsq_sweep_symreg")
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_stlsq_sweep_symreg"][1]) == 20
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "aug_gram", "rev_gram", "n_sets", "n_problems", "d", "p", "n_points", "hyper", "gamma", "threshold", "w_sym", "max_iter",
        "near_band", "pivot_floor", "xi_out", "mask_out", "passes_out", "near_out", "fell_out", "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    assert "replaces: nothing in the reference; the stationarity condition of train.py:663-679 (sym_reg_type 'r')" in comment
    assert "train.py:626-629" in comment and "train.py:872-887" in comment
    # the sibling entries keep their signatures
    for name, count in (("symode_stlsq_sweep", 17), ("symode_stlsq_sweep_constrained", 23), ("symode_stlsq_sweep_minnorm", 25)):
        sibling = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert len(sibling.group(1).split(",")) == len(engine._SIGNATURES[name][1]) == count, name
    assert engine.STLSQ_HYPER == 2 and engine.STLSQ_SYMREG_HYPER == 3


def test_the_solve_is_stated_once():
    """Only the C ABI's translation unit sees the kernel; kernel and constrained kernel take factorisation and back
    substitution from csrc/stlsq_joint.hpp, and neither holds a pivot search of its own."""
    read = lambda f: open(os.path.join(CSRC, f)).read()                                        # noqa: E731
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp"))]
    assert [f for f in sources if '#include "stlsq_symreg.hpp"' in read(f)] == ["capi.hip"]
    assert sorted(f for f in sources if '#include "stlsq_joint.hpp"' in read(f)) == ["stlsq_constrained.hpp", "stlsq_symreg.hpp"]
    for f in ("stlsq_constrained.hpp", "stlsq_symreg.hpp"):
        text = read(f)
        assert "stlsq_joint_factor<" in text and "stlsq_joint_back(" in text, f
        assert "__shfl_xor" not in text and "sqrt(" not in text.replace("sqrt(dbb)", ""), f       # (the min-norm factor of Wm Wm^T is its own)
    joint = read("stlsq_joint.hpp")
    assert joint.count("__shfl_xor(bv") == 1 and joint.count("dkk > pivot_floor * first") == 1


def test_every_refusal_is_decided_without_a_device(lib):
    for d in (0, -2, 5):
        assert _call(lib, d=d) == BADSIZE, d
    for p in (0, -1, 65, 1000):
        assert _call(lib, p=p) == BADSIZE, p
    for d, p in ((2, 33), (3, 22), (4, 17), (2, 64)):                                   # d p > 64
        assert _call(lib, d=d, p=p) == BADSIZE, (d, p)
    for d, p in ((1, 64), (2, 32), (3, 21), (4, 16)):                                   # d p <= 64 passes the size rules
        assert _call(lib, d=d, p=p, aug=NULL) == NULLPTR, (d, p)
    for max_iter in (0, -1):
        assert _call(lib, max_iter=max_iter) == BADSIZE, max_iter
    for n_sets in (0, -3):
        assert _call(lib, n_sets=n_sets, n_problems=3, hyper=JUNK) == BADSIZE, n_sets
    assert _call(lib, n_sets=3, n_problems=2, hyper=JUNK) == BADSIZE                # fewer problems than sets
    assert _call(lib, n_sets=3, n_problems=0, hyper=JUNK) == BADSIZE
    assert _call(lib, n_sets=3, n_problems=2 ** 31, hyper=JUNK) == BADSIZE
    for n_problems in (4, 9, 27):                                                   # without a table: one problem per set
        assert _call(lib, n_sets=3, n_problems=n_problems, hyper=NULL) == BADSIZE, n_problems
    for name in ("gamma", "threshold", "w_sym", "pivot_floor"):
        for bad in (-1e-14, -1.0, float("nan"), float("inf"), float("-inf")):
            assert _call(lib, **{name: bad}) == BADSIZE, (name, bad)
        assert _call(lib, aug=NULL, **{name: 0.0}) == NULLPTR, name                 # zero is a value
    for name in POINTERS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
        assert _call(lib, hyper=JUNK, n_problems=27, **{name: NULL}) == NULLPTR, name
    assert _call(lib, aug=0x1004) == ALIGN and _call(lib, rev=0x1004) == ALIGN
    assert _call(lib, hyper=0x1002, n_problems=9) == ALIGN
    for name in ("xi", "passes", "near", "fell"):
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
    # a size before a pointer, as the other entries decide
    assert _call(lib, p=65, aug=NULL) == BADSIZE and _call(lib, n_problems=4, xi=NULL) == BADSIZE and _call(lib, w_sym=-1.0, rev=NULL) == BADSIZE


def test_the_engine_takes_device_tensors_only():
    import inspect

    import symode_amd
    sig = inspect.signature(engine.HipEngine.stlsq_sweep_symreg).parameters
    assert list(sig)[:10] == ["self", "G", "R", "n_points", "gamma", "threshold", "w_sym", "max_iter", "hyper", "n_problems"]
    assert sig["hyper"].default is None and sig["n_problems"].default is None
    for name in ("d", "pivot_floor", "near_band", "to_host", "tail"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["to_host"].default is False and sig["tail"].default is None
    with pytest.raises(symode_amd.SymodeError):
        symode_amd.get_engine().stlsq_sweep_symreg(torch.zeros(3, 12, 12, dtype=torch.float64), torch.zeros(3, 20, 20, dtype=torch.float64),
                                                   200, 0.0, 0.1, 1.0, 10, d=2, pivot_floor=1e-14)
