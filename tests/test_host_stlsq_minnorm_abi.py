"""CPU-side checks of symode_stlsq_sweep_minnorm: the entry is an addition (declared, exported, bound with the header's argument
count, the ABI version unchanged, the constrained entry's signature untouched), and every refusal of the header is an error
code before any device work -- the pointers below are junk and none is dereferenced."""
import inspect
import os
import re

import pytest
import torch

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
POINTERS = ("aug", "q_solve", "q_xi", "xi", "var", "mask", "passes", "near", "fell", "trunc", "rank")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _call(lib, aug=JUNK, n_sets=3, n_problems=3, d=2, p=10, n_points=200, q_solve=JUNK, q_xi=JUNK, r=4, allow_constant=1, hyper=NULL,
          gamma=0.1, threshold=0.05, max_iter=10, near_band=1e-4, rcond=1e-7, xi=JUNK, var=JUNK, mask=JUNK, passes=JUNK, near=JUNK,
          fell=JUNK, trunc=JUNK, rank=JUNK):
    return lib.symode_stlsq_sweep_minnorm(aug, n_sets, n_problems, d, p, n_points, q_solve, q_xi, r, allow_constant, hyper, gamma,
                                          threshold, max_iter, near_band, rcond, xi, var, mask, passes, near, fell, trunc, rank, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8         # an added entry leaves the version (include/symode.h)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_stlsq_sweep_minnorm\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_stlsq_sweep_minnorm")
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_stlsq_sweep_minnorm"][1]) == 25
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "aug_gram", "n_sets", "n_problems", "d", "p", "n_points", "q_solve", "q_xi", "r", "allow_constant", "hyper", "gamma",
        "threshold", "max_iter", "near_band", "rcond", "xi_out", "var_out", "mask_out", "passes_out", "near_out", "fell_out",
        "trunc_out", "rank_out", "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    for cited in ("sindy.py:250-315", "csrc/host_lstsq.cpp:55", "csrc/host_lstsq.cpp:67-84", "csrc/host_lstsq.cpp:102-132", "csrc/laic1.hpp"):
        assert cited in comment, cited
    # the lines cited are the ones meant
    host = open(os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc", "host_lstsq.cpp")).read().split("\n")
    assert "fact = kk; break;" in host[54] and "xGELSY rank loop" in host[66] and "minimum norm" in host[101]
    assert "Y[(size_t)t * k + col] = acc;" in host[129]
    # the constrained entry keeps its signature
    old = re.search(r"\bint symode_stlsq_sweep_constrained\(([^;]*)\);", header)
    assert len(old.group(1).split(",")) == len(engine._SIGNATURES["symode_stlsq_sweep_constrained"][1]) == 23
    # xLAIC1 is stated once, for the host routine and the kernel
    csrc = os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".cpp"))
             and '#include "laic1.hpp"' in open(os.path.join(csrc, f)).read()]
    assert users == ["host_lstsq.cpp", "stlsq_constrained.hpp"]
    assert "absgam" not in open(os.path.join(csrc, "host_lstsq.cpp")).read()
    assert "absgam" not in open(os.path.join(csrc, "stlsq_constrained.hpp")).read()


def test_every_refusal_is_decided_without_a_device(lib):
    # ---- what the constrained entry refuses
    for d in (0, -2, 5):
        assert _call(lib, d=d) == BADSIZE, d
    for p in (0, -1, 65, 1000):
        assert _call(lib, p=p) == BADSIZE, p
    for r in (0, -3):
        assert _call(lib, r=r) == BADSIZE, r
    assert _call(lib, p=64, r=63, allow_constant=1) == BADSIZE                         # r' = 65 > 64
    assert _call(lib, p=64, r=65, allow_constant=0) == BADSIZE
    assert _call(lib, p=64, r=62, allow_constant=1, aug=NULL) == NULLPTR               # r' = 64 passes the size rules
    assert _call(lib, p=64, r=64, allow_constant=0, aug=NULL) == NULLPTR
    assert _call(lib, d=2, p=10, r=19, allow_constant=1) == BADSIZE                    # r' = 21 > d p = 20
    assert _call(lib, d=2, p=10, r=21, allow_constant=0) == BADSIZE
    assert _call(lib, d=2, p=10, r=18, allow_constant=1, aug=NULL) == NULLPTR          # r' = d p passes the size rules
    for max_iter in (0, -1):
        assert _call(lib, max_iter=max_iter) == BADSIZE, max_iter
    for n_sets in (0, -3):
        assert _call(lib, n_sets=n_sets, n_problems=3, hyper=JUNK) == BADSIZE, n_sets
    assert _call(lib, n_sets=3, n_problems=2, hyper=JUNK) == BADSIZE                # fewer problems than sets
    assert _call(lib, n_sets=3, n_problems=0, hyper=JUNK) == BADSIZE
    assert _call(lib, n_sets=3, n_problems=2 ** 31, hyper=JUNK) == BADSIZE
    for n_problems in (4, 9, 27):                                                   # without a table: one problem per set
        assert _call(lib, n_sets=3, n_problems=n_problems, hyper=NULL) == BADSIZE, n_problems
    # ---- rcond in place of the pivot floor: finite, inside (0, 1)
    for rcond in (float("nan"), float("inf"), float("-inf"), 0.0, -1e-7, -1.0, 1.0, 1.5, 1e7):
        assert _call(lib, rcond=rcond) == BADSIZE, rcond
    for rcond in (1e-300, 1e-7, 0.5, 1.0 - 2.0 ** -53):
        assert _call(lib, rcond=rcond, aug=NULL) == NULLPTR, rcond                    # ... these pass the size rules
    # ---- pointers, the two new ones included
    for name in POINTERS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
        assert _call(lib, hyper=JUNK, n_problems=27, **{name: NULL}) == NULLPTR, name
    assert _call(lib, aug=0x1004) == ALIGN and _call(lib, q_solve=0x1004) == ALIGN
    assert _call(lib, hyper=0x1002, n_problems=9) == ALIGN
    for name in ("q_xi", "xi", "var", "passes", "near", "fell", "trunc", "rank"):
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
    # a size before a pointer, a pointer before an alignment, as the other entries decide
    assert _call(lib, p=65, aug=NULL) == BADSIZE and _call(lib, n_problems=4, xi=NULL) == BADSIZE and _call(lib, rcond=2.0, rank=NULL) == BADSIZE
    assert _call(lib, trunc=NULL, rank=0x1002) == NULLPTR


def test_the_engine_takes_device_tensors_only():
    import symode_amd
    sig = inspect.signature(engine.HipEngine.stlsq_sweep_minnorm).parameters
    old = inspect.signature(engine.HipEngine.stlsq_sweep_constrained).parameters
    assert list(sig)[:11] == list(old)[:11]
    assert [k for k in sig if k not in old] == ["rcond"] and [k for k in old if k not in sig] == ["pivot_floor"]
    assert sig["rcond"].kind is inspect.Parameter.KEYWORD_ONLY and sig["rcond"].default is inspect.Parameter.empty
    with pytest.raises(symode_amd.SymodeError):
        symode_amd.get_engine().stlsq_sweep_minnorm(torch.zeros(3, 12, 12, dtype=torch.float64), 200, 0.0, 0.1, 10,
                                                    torch.zeros(20, 6, dtype=torch.float64), torch.zeros(20, 4), True, d=2, rcond=1e-7)
