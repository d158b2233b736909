"""CPU-side checks of the Gram-form closure's C ABI: argument validation of symode_symreg_reversed_gram /
symode_quad_closure / the workspace query without a GPU, and the appended symode_trainer fields laid out as the ctypes
TrainerDesc says (sizeof and offsets from a C program compiled against include/symode.h)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # a non-null, aligned pointer that is never dereferenced (validation fails first)


def test_abi_version_is_the_bindings(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)


def test_reversed_gram_workspace_query(lib):
    f = lib.symode_symreg_reversed_gram_workspace_bytes
    # d = 2, order 3: d p = 20, 5 x 5 tiles -> 15 upper tiles of 16 doubles per workgroup partial
    one = f(2, 3, 0, 1, 1, 64)
    assert one == 15 * 16 * 8                                   # 64 items: one workgroup
    assert f(2, 3, 0, 1, 1, 1 << 20) == 1024 * 15 * 16 * 8      # capped at 1024 workgroups for one problem
    assert f(2, 3, 0, 3, 4, 1000) > 0
    assert f(2, 5, 0, 1, 1, 1000) > 0 and f(3, 3, 3, 1, 1, 1000) > 0      # order 5; d = 3 order 3 with sine + exp (d p = 78)
    assert f(3, 4, 0, 1, 1, 1000) == 0                          # d p = 105 > 88: not instantiated
    assert f(9, 3, 0, 1, 1, 1000) == 0                          # no such library
    assert f(2, 3, 0, 0, 1, 1000) == 0 and f(2, 3, 0, 1, 0, 1000) == 0 and f(2, 3, 0, 1, 1, 0) == 0
    # the closure workspace query is unchanged by the new entry
    assert lib.symode_workspace_bytes(2, 3, 0, 1, 125000) > 0


def test_reversed_gram_argument_validation_needs_no_gpu(lib):
    f = lib.symode_symreg_reversed_gram
    big = 1 << 30
    # (x, gx, jgx, n_g, S, n, d, order, flags, gram, ws, ws_bytes, stream)
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 7, 3, 0, JUNK, JUNK, big, NULL) == -1          # no such library
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 3, 4, 0, JUNK, JUNK, big, NULL) == -1          # library outside the Gram kernel's set
    assert f(JUNK, JUNK, JUNK, 1, 1, 0, 2, 3, 0, JUNK, JUNK, big, NULL) == -3            # n < 1
    assert f(JUNK, JUNK, JUNK, 0, 1, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -3          # n_g < 1
    assert f(JUNK, JUNK, JUNK, 1, 0, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -3          # S < 1
    assert f(JUNK, JUNK, JUNK, 1, 70000, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -3      # S > 65535
    assert f(NULL, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -2
    assert f(JUNK, NULL, JUNK, 1, 1, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -2
    assert f(JUNK, JUNK, NULL, 1, 1, 100, 2, 3, 0, JUNK, JUNK, big, NULL) == -2
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, NULL, JUNK, big, NULL) == -2
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, ctypes.c_void_p(0x1004), JUNK, big, NULL) == -5   # fp64 output 8-aligned
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, NULL, big, NULL) == -4          # no workspace
    need = lib.symode_symreg_reversed_gram_workspace_bytes(2, 3, 0, 1, 1, 100)
    assert f(JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, JUNK, need - 8, NULL) == -4     # workspace too small


def test_quad_closure_argument_validation_needs_no_gpu(lib):
    f = lib.symode_quad_closure
    # (G, R, S, d, p, xi, mask, inv_count, w_sym, loss, grad, stream)
    assert f(JUNK, NULL, 0, 2, 10, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -3          # S < 1
    assert f(JUNK, NULL, 1, 0, 10, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -3          # d < 1
    assert f(JUNK, NULL, 1, 2, 0, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -3           # p < 1
    assert f(JUNK, NULL, 1, 3, 86, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -3          # d p = 258 > 256
    assert f(NULL, NULL, 1, 2, 10, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -2
    assert f(JUNK, NULL, 1, 2, 10, NULL, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -2
    assert f(JUNK, NULL, 1, 2, 10, JUNK, NULL, 1.0, 0.0, NULL, JUNK, NULL) == -2
    assert f(JUNK, NULL, 1, 2, 10, JUNK, NULL, 1.0, 0.0, JUNK, NULL, NULL) == -2
    assert f(ctypes.c_void_p(0x1004), NULL, 1, 2, 10, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -5
    assert f(JUNK, ctypes.c_void_p(0x1004), 1, 2, 10, JUNK, NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -5
    assert f(JUNK, NULL, 1, 2, 10, ctypes.c_void_p(0x1002), NULL, 1.0, 0.0, JUNK, JUNK, NULL) == -5


def test_trainer_in_gram_mode_needs_no_point_data_but_its_state(lib):
    """The closure kind alone says what the descriptor needs: with SYMODE_CLOSURE_GRAM x / dx / workspace may be NULL; the
    state and the records are still required.  Every case fails before a launch."""
    T = engine.TrainerDesc()
    call = lambda: lib.symode_trainer_closure(ctypes.byref(T), None, None, NULL)  # noqa: E731
    T.closure, T.aug_gram = engine.CLOSURE_GRAM, 0x1000
    T.n_problems, T.n_points, T.d, T.order, T.flags = 1, 100, 2, 3, 0
    T.n_params, T.max_iter, T.history, T.log_epochs = 20, 20, 100, 8
    T.state, T.log, T.log_test = None, 0x1000, 0x1000
    assert call() == -2                                                                # no state block
    T.state, T.state_bytes = 0x1000, 0                                                 # state present, too small
    assert call() == -4
    T.closure = engine.CLOSURE_STREAM                                                  # streaming form: x, dx needed again
    assert call() == -2
    for unknown in (3, -1):
        T.closure = unknown
        assert call() == -3
    T.closure, T.aug_gram = engine.CLOSURE_GRAM, None                                  # the Gram form without its matrix
    assert call() == -2
    T.closure, T.x, T.dx, T.workspace = engine.CLOSURE_STREAM, 0x1000, 0x1000, 0x1000
    assert call() == -4                                                                # the plain closure is complete
    T.n_g, T.gx = 1, 0x1000                                                            # the reversed one is not: no jgx
    assert call() == -2
    T.closure = engine.CLOSURE_LATENT                                                  # gx / jgx / n_g are not this kind's
    T.latent_B, T.latent_y = None, 0x1000
    assert call() == -2
    T.latent_B, T.latent_y = 0x1000, None
    assert call() == -2
    T.latent_y = 0x1000                                                                # complete: past the pointer checks
    assert call() == -4


def test_trainer_struct_layout_matches_ctypes():
    """sizeof(symode_trainer) and the offsets of the appended fields, as a C compiler lays them out."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    names = ["aug_gram", "rev_gram", "log_epochs", "closure", "latent_B", "latent_y"]
    src = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"symode_trainer_layout_{os.getpid()}.c")
    exe = src[:-2]
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "symode.h"\n'
                'int main(void) { printf("%zu' + ' %zu' * len(names) + '\\n", sizeof(symode_trainer), '
                + ', '.join(f'offsetof(symode_trainer, {n})' for n in names) + '); return 0; }\n')
    try:
        r = subprocess.run([cc, "-std=c99", f"-I{os.path.join(ROOT, 'include')}", src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    D = engine.TrainerDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in names]
    # the fields appended after aug_gram, rev_gram are exactly these three, in this order
    assert D._fields_[-5:] == [("aug_gram", ctypes.c_void_p), ("rev_gram", ctypes.c_void_p), ("closure", ctypes.c_int),
                               ("latent_B", ctypes.c_void_p), ("latent_y", ctypes.c_void_p)]
    assert (D.aug_gram.offset, D.rev_gram.offset, D.log_epochs.offset) == (224, 232, 216)     # what they were before the append


def test_python_layer_names_the_new_entry_points():
    from symode_amd import gram_closure, parser_utils
    assert hasattr(engine.HipEngine, "symreg_reversed_gram") and hasattr(engine.HipEngine, "quad_closure")
    assert hasattr(gram_closure, "GramStatistics")
    args = vars(parser_utils.get_args(argv=["--gram_closure"]))
    assert args["gram_closure"] is True
    assert not vars(parser_utils.get_args(argv=[]))["gram_closure"]
