"""CPU-side checks of symode_stlsq_path_symreg: the entry is an addition (declared, exported, bound with the header's argument
count, the ABI version unchanged), every refusal of the header is an error code before any device work -- the pointers below
are junk and none is dereferenced --, the pass it walks is stated once (stlsqs_pass_solve, shared with stlsq_symreg_kernel),
and the refusals of ``engine.stlsq_path_symreg`` and ``SeedSweepSTLSQ.solve_path(rev=...)`` are decided on the host."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc")
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
POINTERS = ("aug", "rev", "val", "path", "order", "mse_train", "reg_train", "mse_val", "best", "xi", "mask", "near", "fell")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _call(lib, aug=JUNK, rev=JUNK, val=JUNK, n_sets=3, n_val_sets=1, n_problems=3, d=2, p=10, n_points=200, hyper=NULL, gamma=0.1,
          w_sym=1.0, tol=0.02, floor_rel=1e-10, near_band=1e-4, pivot_floor=1e-14, path=JUNK, order=JUNK, mse_train=JUNK, reg_train=JUNK,
          mse_val=JUNK, best=JUNK, xi=JUNK, mask=JUNK, near=JUNK, fell=JUNK):
    return lib.symode_stlsq_path_symreg(aug, rev, val, n_sets, n_val_sets, n_problems, d, p, n_points, hyper, gamma, w_sym, tol,
                                        floor_rel, near_band, pivot_floor, path, order, mse_train, reg_train, mse_val, best, xi, mask,
                                        near, fell, None)


def test_the_entry_is_an_addition(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8         # an added entry leaves the version (include/symode.h)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    decl = re.search(r"\bint symode_stlsq_path_symreg\(([^;]*)\);", header)
    assert decl and hasattr(lib, "symode_stlsq_path_symreg")
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(engine._SIGNATURES["symode_stlsq_path_symreg"][1]) == 27
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "aug_gram", "rev_gram", "val_gram", "n_sets", "n_val_sets", "n_problems", "d", "p", "n_points", "hyper", "gamma", "w_sym", "tol",
        "floor_rel", "near_band", "pivot_floor", "path_xi", "order", "mse_train", "reg_train", "mse_val", "best", "xi_out", "mask_out",
        "near_out", "fell_out", "stream"]
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    assert "Added to ABI version 8 (nothing existing changed)" in comment and "replaces: nothing in the reference" in comment
    assert "The regulariser is not scored on held-out data" in " ".join(comment.replace(" * ", " ").split())
    # the sibling entries keep their signatures
    for name, count in (("symode_stlsq_sweep", 17), ("symode_stlsq_sweep_constrained", 23), ("symode_stlsq_sweep_minnorm", 25),
                        ("symode_stlsq_sweep_symreg", 20), ("symode_stlsq_path", 22)):
        sibling = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert len(sibling.group(1).split(",")) == len(engine._SIGNATURES[name][1]) == count, name
    assert engine.STLSQ_PATH_SYMREG_HYPER == 2 and engine.STLSQ_SYMREG_HYPER == 3


def test_the_pass_is_stated_once():
    """Only the C ABI's translation unit sees the kernel; it and stlsq_symreg_kernel call one stlsqs_pass_solve, and the new
    header holds no factorisation of its own (that the two passes are one is what the bit-for-bit step-0 GPU test shows)."""
    read = lambda f: open(os.path.join(CSRC, f)).read()                                        # noqa: E731
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp"))]
    assert [f for f in sources if '#include "stlsq_path_symreg.hpp"' in read(f)] == ["capi.hip"]
    symreg, path = read("stlsq_symreg.hpp"), read("stlsq_path_symreg.hpp")
    assert "stlsqs_pass_solve(" in symreg and "stlsqs_pass_solve(" in path
    assert "stlsq_joint_factor" not in path and "sqrt(" not in path                          # no factorisation of its own
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in path                              # 130.5 KiB of LDS at n = 64


def test_every_refusal_is_decided_without_a_device(lib):
    for d in (0, -2, 5):
        assert _call(lib, d=d) == BADSIZE, d
    for p in (0, -1, 65, 1000):
        assert _call(lib, p=p) == BADSIZE, p
    for d, p in ((2, 33), (3, 22), (4, 17), (2, 64)):                                  # d p > 64
        assert _call(lib, d=d, p=p) == BADSIZE, (d, p)
    for d, p in ((1, 1), (1, 64), (2, 32), (3, 21), (4, 16), (4, 1)):                  # d p <= 64 passes the size rules
        assert _call(lib, d=d, p=p, aug=NULL) == NULLPTR, (d, p)
    for n_sets in (0, -3):
        assert _call(lib, n_sets=n_sets) == BADSIZE, n_sets
    assert _call(lib, n_sets=3, n_problems=2) == BADSIZE                               # fewer problems than sets
    assert _call(lib, n_sets=3, n_problems=0) == BADSIZE
    assert _call(lib, n_sets=3, n_problems=2 ** 31) == BADSIZE
    for n_problems in (3, 4, 27):                                                      # problem s on set s % n_sets
        assert _call(lib, n_sets=3, n_problems=n_problems, aug=NULL) == NULLPTR, n_problems
        assert _call(lib, n_sets=3, n_problems=n_problems, hyper=JUNK, aug=NULL) == NULLPTR, n_problems
    for n_val_sets in (0, -1, 4, 28):
        assert _call(lib, n_val_sets=n_val_sets) == BADSIZE, n_val_sets
    for n_val_sets in (1, 2, 3):
        assert _call(lib, n_val_sets=n_val_sets, val=NULL) == NULLPTR, n_val_sets
    for name in ("gamma", "w_sym", "tol", "floor_rel", "near_band", "pivot_floor"):
        for bad in (-1e-14, -1.0, float("nan"), float("inf"), float("-inf")):
            assert _call(lib, **{name: bad}) == BADSIZE, (name, bad)
        assert _call(lib, aug=NULL, **{name: 0.0}) == NULLPTR, name                    # zero is a value
    assert _call(lib, gamma=1e39) == BADSIZE and _call(lib, w_sym=1e39) == BADSIZE     # not finite in fp32, as the launch holds them
    for name in POINTERS:
        assert _call(lib, **{name: NULL}) == NULLPTR, name
        assert _call(lib, hyper=JUNK, n_problems=27, **{name: NULL}) == NULLPTR, name
    for name in ("aug", "rev", "val", "mse_train", "reg_train", "mse_val"):            # fp64: 8 bytes
        assert _call(lib, **{name: 0x1004}) == ALIGN, name
    for name in ("path", "order", "best", "xi", "near", "fell"):                       # fp32 / int: 4 bytes
        assert _call(lib, **{name: 0x1002}) == ALIGN, name
        assert _call(lib, aug=NULL, **{name: 0x1004}) == NULLPTR, name
    assert _call(lib, hyper=0x1002, n_problems=9) == ALIGN
    assert _call(lib, aug=NULL, mask=0x1001) == NULLPTR                                # bytes: any address
    # a size before a pointer, a pointer before an alignment, as the other entries decide
    assert _call(lib, p=65, aug=NULL) == BADSIZE and _call(lib, n_val_sets=0, xi=NULL) == BADSIZE and _call(lib, w_sym=-1.0, rev=NULL) == BADSIZE


def test_the_engine_takes_device_tensors_only():
    import symode_amd
    sig = inspect.signature(engine.HipEngine.stlsq_path_symreg).parameters
    assert list(sig)[:11] == ["self", "G", "R", "V", "n_points", "gamma", "w_sym", "tol", "floor_rel", "hyper", "n_problems"]
    assert sig["hyper"].default is None and sig["n_problems"].default is None
    for name in ("d", "pivot_floor", "near_band", "to_host", "keep_path"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["to_host"].default is False and sig["keep_path"].default is False
    with pytest.raises(symode_amd.SymodeError):
        symode_amd.get_engine().stlsq_path_symreg(torch.zeros(3, 12, 12, dtype=torch.float64), torch.zeros(3, 20, 20, dtype=torch.float64),
                                                  torch.zeros(1, 12, 12, dtype=torch.float64), 200, 0.0, 1.0, 0.02, 1e-10, d=2,
                                                  pivot_floor=1e-14)


def _sweep(S=3, d=2, order=2):
    """A SeedSweepSTLSQ on the host: nothing here reaches a launch."""
    from symode_amd.sweep import SeedSweepSTLSQ
    sw = SeedSweepSTLSQ(torch.zeros(8, d), torch.zeros(8, d), order, n_seeds=S, idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.zeros((S, sw.p + d, sw.p + d)), 4
    return sw


def test_solve_path_refuses_by_name():
    sw = _sweep()
    p, d, S = sw.p, sw.d, sw.S
    assert (d, p) == (2, 6)
    V, R = np.zeros((1, p + d, p + d)), np.zeros((S, d * p, d * p))
    sig = inspect.signature(type(sw).solve_path).parameters
    assert list(sig) == ["self", "w_sindy_reg", "val_gram", "tol", "floor_rel", "device", "keep_path", "rev", "hyper"]
    assert sig["rev"].default is None and sig["hyper"].default is None
    with pytest.raises(ValueError, match=r"hyper \(a per-problem table of w_reg / w_sym\) needs rev=\(R, w_sym\)"):
        sw.solve_path(0.0, V, 0.02, hyper={"w_sym": [1.0] * S})
    with pytest.raises(ValueError, match=r"rev must be \(R, w_sym\) with R \(S, d p, d p\) = \(3, 12, 12\)"):
        sw.solve_path(0.0, V, 0.02, rev=(R[:, :5], 1.0))
    for kw, name in (({"rev": (R, -1.0)}, "w_sym"), ({"rev": (R, float("nan"))}, "w_sym"), ({"rev": (R, float("inf"))}, "w_sym"),
                     ({"rev": (R, 1.0), "tol": -0.1}, "tol"), ({"rev": (R, 1.0), "floor_rel": float("nan")}, "floor_rel")):
        a = dict(w_sindy_reg=0.0, val_gram=V, tol=0.02)
        a.update(kw)
        with pytest.raises(ValueError, match=f"solve_path: {name} must be finite and >= 0"):
            sw.solve_path(**a)
    with pytest.raises(ValueError, match="solve_path: w_sindy_reg must be finite and >= 0"):
        sw.solve_path(-1.0, V, 0.02, rev=(R, 1.0))
    for bad in (np.zeros((2, p + d, p + d)), np.zeros((1, p + d, p + d + 1)), np.zeros((p + d, p + d))):
        with pytest.raises(ValueError, match=r"val_gram must be \(n_val, p \+ d, p \+ d\) = \(1 or 3, 8, 8\)"):
            sw.solve_path(0.0, bad, 0.02, rev=(R, 1.0))
    with pytest.raises(ValueError, match="the per-problem columns of the regularised path are w_reg and w_sym"):
        sw.solve_path(0.0, V, 0.02, rev=(R, 1.0), hyper={"threshold": [0.1] * S})
    with pytest.raises(ValueError, match="one value per problem, a multiple of the 3 seeds"):
        sw.solve_path(0.0, V, 0.02, rev=(R, 1.0), hyper={"w_sym": [1.0] * 4})
    with pytest.raises(ValueError, match="the ridge weight and w_sym of every problem must be finite and >= 0"):
        sw.solve_path(0.0, V, 0.02, rev=(R, 1.0), hyper={"w_sym": [1.0, -2.0, 1.0]})
    with pytest.raises(ValueError, match="hyper .* needs device=True"):
        sw.solve_path(0.0, V, 0.02, device=False, rev=(R, 1.0), hyper={"w_sym": [1.0] * S})
    big = _sweep(S=1)
    big.p = 36                                                                         # order 7: d p = 72
    with pytest.raises(ValueError, match=r"d p = 2 x 36 = 72 unknowns, the joint system of a step takes at most 64"):
        big.solve_path(0.0, np.zeros((1, 38, 38)), 0.02, rev=(np.zeros((1, 72, 72)), 1.0))


def test_solve_path_on_the_host_is_the_twin_per_seed():
    """device=False with rev: sindy.stlsq_path_symreg_from_gram per seed, the record per PROBLEM."""
    from symode_amd.sindy import stlsq_path_symreg_from_gram
    from tests import stlsq_path_symreg_cases as P
    pairs = [P.C.pair("osc_o2", v) for v in range(3)]
    G, R = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
    V = P.C.pair("osc_o2", 5)[0][None]
    sw = _sweep()
    sw._gram, sw.n_points = G, P.N_POINTS
    Xi, mask, rec = sw.solve_path(0.01, V, 0.02, device=False, keep_path=True, rev=(R, 10.0))
    assert Xi.shape == mask.shape == (3, 2, 6) and rec["order"].shape == (3, 12) and rec["best"].shape == rec["near"].shape == (3,)
    assert rec["mse_train"].shape == rec["reg_train"].shape == rec["mse_val"].shape == (3, 13) and rec["path_xi"].shape == (3, 13, 2, 6)
    assert "ONE chain per PROBLEM" in " ".join(type(sw).solve_path.__doc__.split())
    gamma = float(np.float32(np.sqrt(0.01)))
    for s in range(3):
        xi, m, r = stlsq_path_symreg_from_gram(G[s], R[s], V[0], gamma, 10.0, 0.02, 1e-10, 1e-4, 2, P.N_POINTS)
        assert Xi[s].numpy().tobytes() == xi.tobytes() and np.array_equal(mask[s].numpy() > 0, m)
        assert np.array_equal(rec["order"][s], r["order"]) and rec["best"][s] == r["best"] and rec["mse_val"][s].tobytes() == r["mse_val"].tobytes()
    without = sw.solve_path(0.01, V, 0.02, device=False, rev=(R, 10.0))[2]
    assert sorted(without) == ["best", "mse_train", "mse_val", "near", "order", "reg_train"]
