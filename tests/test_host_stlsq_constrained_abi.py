"""CPU-side checks of symode_stlsq_sweep_constrained: the entry is an addition (declared, exported, bound with the header's
argument count, the ABI version unchanged), every refusal of the header is an error code before any device work -- the
pointers below are junk and none is dereferenced -- and ``CoefMap.solve_matrix()`` is the matrix ``solve_SINDy_one_step``
builds inline."""
import os
import re

import numpy as np
import pytest
import torch

from symode_amd import engine
from symode_amd.coef_map import CoefMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
POINTERS = ("aug", "q_solve", "q_xi", "xi", "var", "mask", "passes", "near", "fell")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _call(lib, aug=JUNK, n_sets=3, n_problems=3, d=2, p=10, n_points=200, q_solve=JUNK, q_xi=JUNK, r=4, allow_constant=1, hyper=NULL,
          gamma=0.1, threshold=0.05, max_iter=10, near_band=1e-4, pivot_floor=1e-14, xi=JUNK, var=JUNK, mask=JUNK, passes=JUNK,
          near=JUNK, fell=JUNK):
    return lib.symode_stlsq_sweep_constrained(aug, n_sets, n_problems, d, p, n_points, q_solve, q_xi, r, allow_constant, hyper, gamma,
                                              threshold, max_iter, near_band, pivot_floor, xi, var, mask, passes, near, fell, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8         # an added entry leaves the version (include/symode.h)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_stlsq_sweep_constrained\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_stlsq_sweep_constrained")
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_stlsq_sweep_constrained"][1]) == 23
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "aug_gram", "n_sets", "n_problems", "d", "p", "n_points", "q_solve", "q_xi", "r", "allow_constant", "hyper", "gamma",
        "threshold", "max_iter", "near_band", "pivot_floor", "xi_out", "var_out", "mask_out", "passes_out", "near_out", "fell_out",
        "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    assert "sindy.py:250-315, constrained branch" in comment
    # the unconstrained entry keeps its signature
    plain = re.search(r"\bint symode_stlsq_sweep\(([^;]*)\);", header)
    assert len(plain.group(1).split(",")) == len(engine._SIGNATURES["symode_stlsq_sweep"][1]) == 17
    # only the C ABI's translation unit sees the kernel
    csrc = os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".cpp"))
             and '#include "stlsq_constrained.hpp"' in open(os.path.join(csrc, f)).read()]
    assert users == ["capi.hip"]


def test_every_refusal_is_decided_without_a_device(lib):
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
    for floor in (-1e-14, -1.0, float("nan"), float("inf"), float("-inf")):
        assert _call(lib, pivot_floor=floor) == BADSIZE, floor
    for name in POINTERS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
        assert _call(lib, hyper=JUNK, n_problems=27, **{name: NULL}) == NULLPTR, name
    assert _call(lib, aug=0x1004) == ALIGN and _call(lib, q_solve=0x1004) == ALIGN
    assert _call(lib, hyper=0x1002, n_problems=9) == ALIGN
    for name in ("q_xi", "xi", "var", "passes", "near", "fell"):
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
    # a size before a pointer, as the other entries decide
    assert _call(lib, p=65, aug=NULL) == BADSIZE and _call(lib, n_problems=4, xi=NULL) == BADSIZE and _call(lib, pivot_floor=-1.0, var=NULL) == BADSIZE


def test_the_engine_takes_device_tensors_only():
    import inspect

    import symode_amd
    sig = inspect.signature(engine.HipEngine.stlsq_sweep_constrained).parameters
    assert list(sig)[:11] == ["self", "G", "n_points", "gamma", "threshold", "max_iter", "q_solve", "q_xi", "allow_constant", "hyper",
                              "n_problems"]
    assert sig["hyper"].default is None and sig["n_problems"].default is None and sig["pivot_floor"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(symode_amd.SymodeError):
        symode_amd.get_engine().stlsq_sweep_constrained(torch.zeros(3, 12, 12, dtype=torch.float64), 200, 0.0, 0.1, 10,
                                                        torch.zeros(20, 6, dtype=torch.float64), torch.zeros(20, 4), True, d=2,
                                                        pivot_floor=1e-14)


# ---- CoefMap.solve_matrix / xi_matrix ----------------------------------------------------------------------------------------------
def _inline(Q, d, allow_constant):
    """The construction inside solve_SINDy_one_step (sindy.py:277-280 of the reference), copied statement by statement."""
    Q = np.asarray(Q, dtype=np.float64)
    if allow_constant:
        Q = np.concatenate([Q, np.zeros((Q.shape[0], d))], axis=1)
        for i in range(d):
            Q[i * Q.shape[0] // d, Q.shape[1] - d + i] = 1.0
    return Q


@pytest.mark.parametrize("d, p, r", [(2, 6, 2), (2, 10, 4), (3, 10, 8)])
@pytest.mark.parametrize("allow_constant", [True, False])
@pytest.mark.parametrize("use_kron", [True, False])
def test_solve_matrix_is_the_inline_construction(d, p, r, allow_constant, use_kron):
    Q = torch.from_numpy(np.random.RandomState(d * p + r).randn(d * p, r).astype(np.float32))
    coef = CoefMap(d, p, Q, use_kron, allow_constant)
    qs, qx = coef.solve_matrix(), coef.xi_matrix()
    assert qs.dtype == np.float64 and qs.flags["C_CONTIGUOUS"] and qs.shape == (d * p, r + (d if allow_constant else 0))
    assert np.array_equal(qs, _inline(Q.numpy(), d, allow_constant))                # equation-major rows whatever use_kron is
    assert qx.dtype == np.float32 and qx.shape == (d * p, r) and np.array_equal(qx, coef.effective_Q())
    assert np.array_equal(qx, qs[:, :r].astype(np.float32)) == use_kron             # the two differ exactly when use_kron is false
    beta = np.random.RandomState(1).randn(r).astype(np.float32)
    const = np.arange(1, d + 1, dtype=np.float32)
    want = coef.xi(beta, const)
    got = (qx @ beta).reshape(d, p)
    if allow_constant:
        got[:, 0] += const
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)
    if allow_constant:                                                              # column r + j is the constant of equation j
        for j in range(d):
            unit = np.zeros(d * p)
            unit[j * p] = 1.0
            assert np.array_equal(qs[:, r + j], unit)


def test_solve_sindy_one_step_solves_in_solve_matrix():
    """The regressor's own pass and the Gram restatement (which reads ``solve_matrix``) give the same coefficients."""
    from symode_amd.sindy import SINDyRegression, solve_SINDy_one_step, stlsq_constrained_from_gram
    from tests import stlsq_constrained_cases as C
    from tests.oracle_engine import OracleEngine
    g = C.golden()
    for tag in C.SOLVE_TAGS:
        d, order, cc = [int(v) for v in g[f"{tag}_cfg"]]
        gamma, thr = [float(v) for v in g[f"{tag}_hp"]]
        x, dx = torch.from_numpy(g[f"{tag}_x"]), torch.from_numpy(g[f"{tag}_dx"])
        eng = OracleEngine()
        reg = SINDyRegression(d, order, False, False, L_list=[torch.from_numpy(g[f"{tag}_L"])], threshold=thr, device="cpu",
                              constrain_constant=bool(cc), engine=eng, lstsq_driver="gels")
        solve_SINDy_one_step(reg, x, dx, gamma, thr)
        G = eng.aug_gram(x, dx, order).numpy()
        xi, full, _ = stlsq_constrained_from_gram(G, x.shape[0], np.ones((d, reg.coef.p), dtype=bool), gamma, d, reg.coef, "gels")
        assert np.allclose(xi, reg.get_Xi().detach().numpy(), rtol=1e-6, atol=1e-7)   # (get_Xi is torch's product, xi numpy's)
        assert np.array_equal(full[:reg.coef.r].astype(np.float32), reg.beta.detach().numpy())
