"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
that include/symode.h declares; argument validation returns error codes without a GPU."""
import ctypes
import os
import re

import pytest

import symode_amd
from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "symode.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(symode_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = declared_symbols()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/symode.h but not exported"
        assert n in engine._SIGNATURES, f"{n} has no ctypes signature in engine.py"
    assert sorted(engine._SIGNATURES) == names


def test_abi_version_and_error_strings(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8      # 8: the three sweep L-BFGS entries became symode_lbfgs_step
    assert lib.symode_error_string(0) == b"ok"
    for code in (-1, -2, -3, -4, -5):
        assert len(lib.symode_error_string(code)) > 3


def test_lib_size_matches_reference_term_count(lib):
    # reference sindy.py:179-189 (orders <= 3), C(d+n-1, n) beyond
    from math import comb
    for d in (1, 2, 3, 4):
        for order in (1, 2, 3, 4, 5):
            for fl in (0, 1, 2, 3):
                p = 1 + sum(comb(d + n - 1, n) for n in range(1, order + 1)) + d * bin(fl).count("1")
                got = lib.symode_lib_size(d, order, fl)
                supported = (d <= 2) or (d == 3 and order <= 4)
                if d == 4 and order <= 3:            # compiled in by `make ALL=1` only (no task of the reference has d = 4)
                    assert got in (p, -1), (d, order, fl)
                else:
                    assert got == (p if supported else -1), (d, order, fl)
    assert lib.symode_lib_size(2, 3, 0) == 10 and lib.symode_lib_size(2, 2, 2) == 8 and lib.symode_lib_size(2, 5, 0) == 21
    assert lib.symode_lib_size(5, 2, 0) == -1 and lib.symode_lib_size(2, 6, 0) == -1 and lib.symode_lib_size(2, 2, 4) == -1


def test_argument_validation_needs_no_gpu(lib):
    null = ctypes.c_void_p(None)
    assert lib.symode_theta(null, -1, 2, 3, 0, null, null) == -3          # bad size
    assert lib.symode_theta(null, 0, 2, 3, 0, null, null) == 0            # empty input: nothing to do
    assert lib.symode_theta(null, 8, 2, 3, 0, null, null) == -2           # null pointers
    assert lib.symode_theta(null, 8, 7, 3, 0, null, null) == -1           # unsupported library
    assert lib.symode_loss_grad(null, null, 1, 8, 2, 3, 0, null, null, 1.0, null, null, null, 0, null) == -2
    assert lib.symode_loss_grad(null, null, 0, 8, 2, 3, 0, null, null, 1.0, null, null, null, 0, null) == -3
    assert lib.symode_workspace_bytes(2, 3, 0, 1, 125000) > 0
    assert lib.symode_workspace_bytes(9, 3, 0, 1, 125000) == 0


def test_argument_validation_of_the_seed_table_entry(lib):
    null, junk = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)
    f = lib.symode_seeded_subsamples
    assert f(0, 1, junk, 1, junk, null) == -3 and f(10, 0, junk, 1, junk, null) == -3        # n, m >= 1
    assert f(10, 11, junk, 1, junk, null) == -3 and f(10, 5, junk, 0, junk, null) == -3      # m <= n, n_seeds >= 1
    assert f(2 ** 31, 5, junk, 1, junk, null) == -3                                          # rows are int32
    assert f(10, 5, null, 1, junk, null) == -2 and f(10, 5, junk, 1, null, null) == -2       # null pointers
    assert f(10, 5, ctypes.c_void_p(0x1004), 1, junk, null) == -5                            # seeds are int64


def test_argument_validation_of_the_round2_entries(lib):
    """Every entry added with ABI version 2 rejects bad sizes / null or misaligned pointers / short workspaces before it
    touches the GPU (codes: -1 unsupported, -2 null, -3 size, -4 workspace, -5 alignment)."""
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_double * 64)()
    good = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    assert lib.symode_workspace_init(null, 1 << 20, null) == -2
    assert lib.symode_workspace_init(odd, 1 << 20, null) == -5
    assert lib.symode_workspace_init(good, 64, null) == -4             # shorter than the ticket header
    # symreg_reversed_batched(x, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, loss, grad, ws, ws_bytes, stream)
    f = lib.symode_symreg_reversed_batched
    assert f(good, good, good, 1, 1, 8, 9, 3, 0, good, null, 1.0, good, good, good, 512, null) == -1
    assert f(good, good, good, 1, 0, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -3
    assert f(good, good, good, 1, 65536, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -3
    assert f(good, good, good, -1, 1, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -3
    assert f(good, null, null, 1, 1, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -2
    assert f(odd, good, good, 1, 1, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -5
    assert f(good, good, good, 1, 1, 8, 2, 3, 0, good, null, 1.0, good, good, null, 0, null) == -4
    assert f(good, good, good, 1, 1, 8, 2, 3, 0, good, null, 1.0, good, good, good, 512, null) == -4
    # loss_grad_reversed(x, dx, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
    f = lib.symode_loss_grad_reversed
    assert f(good, good, good, good, 1, 1, 8, 2, 6, 0, good, null, 1.0, 1.0, good, good, good, 512, null) == -1
    assert f(good, good, good, good, 0, 1, 8, 2, 3, 0, good, null, 1.0, 1.0, good, good, good, 512, null) == -3    # needs a generator
    assert f(good, good, good, good, 1, 1, 0, 2, 3, 0, good, null, 1.0, 1.0, good, good, good, 512, null) == -3
    assert f(good, null, good, good, 1, 1, 8, 2, 3, 0, good, null, 1.0, 1.0, good, good, good, 512, null) == -2
    assert f(good, good, good, good, 1, 1, 8, 2, 3, 0, good, odd, 1.0, 1.0, good, good, good, 512, null) == -5
    assert f(good, good, good, good, 1, 1, 8, 2, 3, 0, good, null, 1.0, 1.0, good, good, good, 512, null) == -4
    # weak_gram(x, n_t, d, order, flags, V, V_drv, n_test, out, ws, ws_bytes, stream)
    f = lib.symode_weak_gram
    assert f(good, 8, 2, 3, 4, good, good, 4, good, good, 512, null) == -1
    assert f(good, 0, 2, 3, 0, good, good, 4, good, good, 512, null) == -3
    assert f(good, 8, 2, 3, 0, good, good, 129, good, good, 512, null) == -3
    assert f(good, 8, 2, 3, 0, good, null, 4, good, good, 512, null) == -2
    assert f(good, 8, 2, 3, 0, good, good, 4, odd, good, 512, null) == -5
    assert f(good, 8, 2, 3, 0, good, good, 4, good, good, 512, null) == -4


def test_argument_validation_of_the_lbfgs_iteration_entries(lib):
    """symode_lbfgs_step / symode_selftest_wave_sum: an unknown mode, sizes and null pointers are refused before any launch
    (n <= 256 parameters, history <= 128 pairs); ``frozen`` alone may be NULL."""
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_double * 64)()
    good = ctypes.cast(buf, ctypes.c_void_p)
    st = [good] * 15                     # params, g, loss, act, n_iter, d, t, old_dirs, old_stps, ro, head, count, h_diag, prev_g, prev_loss
    f = lib.symode_lbfgs_step            # mode, new_loss, new_g, frozen, tol_grad, l1, w_x, w_reg, <15 state pointers>, S, n, history, lr, tol_change, stream
    for mode in (engine.LBFGS_ACCEPT, engine.LBFGS_BEGIN):
        head = (mode, good, good, null, 1e-7, 0, 1.0, 0.0)
        assert f(*head, *st, 0, 20, 100, 1.0, 1e-9, null) == -3
        assert f(*head, *st, -1, 20, 100, 1.0, 1e-9, null) == -3
        assert f(*head, *st, 4, 257, 100, 1.0, 1e-9, null) == -3
        assert f(*head, *st, 4, 300, 100, 1.0, 1e-9, null) == -3
        assert f(*head, *st, 4, 0, 100, 1.0, 1e-9, null) == -3
        assert f(*head, *st, 4, 20, 129, 1.0, 1e-9, null) == -3
        assert f(*head, *st, 4, 20, 0, 1.0, 1e-9, null) == -3
        for k in range(15):
            args = list(st)
            args[k] = null
            assert f(*head, *args, 4, 20, 100, 1.0, 1e-9, null) == -2, (mode, k)
            assert f(mode, good, good, good, 1e-7, 1, 1.0, 0.0, *args, 4, 20, 100, 1.0, 1e-9, null) == -2, (mode, k)
        assert f(mode, null, good, null, 1e-7, 0, 1.0, 0.0, *st, 4, 20, 100, 1.0, 1e-9, null) == -2          # new_loss
        assert f(mode, good, null, null, 1e-7, 0, 1.0, 0.0, *st, 4, 20, 100, 1.0, 1e-9, null) == -2          # new_g
    for mode in (0, 3, -1):                                                                                  # (0 was the removed update-only form)
        assert f(mode, good, good, null, 1e-7, 0, 1.0, 0.0, *st, 4, 20, 100, 1.0, 1e-9, null) == -3, mode
    f = lib.symode_selftest_wave_sum
    assert f(good, good, good, 0, null) == -3 and f(null, good, good, 1, null) == -2


def test_engine_refuses_cpu_tensors():
    import torch
    eng = symode_amd.get_engine()
    with pytest.raises(symode_amd.SymodeError):
        eng.theta(torch.zeros(4, 2), 3)
    with pytest.raises(symode_amd.SymodeError):
        eng.loss_grad(torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(2, 10), None, 3)


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(symode_amd.SymodeError):
        engine.load_library(str(tmp_path / "nope.so"))


def test_header_is_plain_c_and_the_c_example_compiles():
    """The boundary must be bindable from C / any FFI: include/symode.h parses as C99, examples/capi_demo.c type-checks
    against it (gcc, no ROCm needed), and with the HIP runtime headers it links against the built library as C."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo, inc = os.path.join(root, "examples", "capi_demo.c"), os.path.join(root, "include")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", "-DSYMODE_DEMO_NO_HIP", demo],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")) and os.path.exists(engine.LIB_PATH):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "symode_capi_demo")
        libdir = os.path.dirname(engine.LIB_PATH)
        r = subprocess.run(["gcc", "-std=c99", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{inc}", demo, f"-L{libdir}",
                            "-lsymode_hip", f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rocm}/lib",
                            "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_no_scratch_inside_the_reference_domain():
    """No kernel of a library the reference can build (any latent_dim here <= 3, order <= 3, sine / exp on or off --
    sindy.py:42-77) nor any d <= 2 kernel of the order 4-5 extension touches scratch memory: the gfx950 code objects are
    pulled out of the built library and disassembled (tools/scratch_report.py)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not (os.path.exists(engine.LIB_PATH) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")):
        pytest.skip("needs the built library and llvm-objdump")
    spec = importlib.util.spec_from_file_location("scratch_report", os.path.join(root, "tools", "scratch_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.scratch_by_kernel(engine.LIB_PATH)
    assert len(res) > 500                                            # the extraction found the kernels
    import re
    inside = re.compile(r"Library<(?:[123], [123]|[12], [45]), ")
    bad = {k: v for k, v in res.items() if v > 0 and inside.search(k)}
    assert not bad, bad
