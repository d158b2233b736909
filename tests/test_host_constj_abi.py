"""CPU-side checks of the point-constant-Jacobian entries of the C ABI: symode_jacobian_constant,
symode_loss_grad_reversed_constj and symode_symreg_reversed_batched_constj refuse bad arguments before anything is
launched (codes: -1 unsupported, -2 null, -3 size, -4 workspace, -5 alignment), and the Python layer names them."""
import ctypes
import os

import pytest

from symode_amd import engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # a non-null, aligned pointer that is never dereferenced (validation fails first)
ODD = ctypes.c_void_p(0x1002)


def test_binding_and_library_agree_on_the_abi_version(lib):
    # the three entries are additions: no existing signature changed, so the version the earlier ABI tests pin still holds
    assert lib.symode_abi_version() == engine.ABI_VERSION
    for name in ("symode_jacobian_constant", "symode_loss_grad_reversed_constj", "symode_symreg_reversed_batched_constj"):
        assert hasattr(lib, name) and name in engine._SIGNATURES


def test_jacobian_constant_argument_validation_needs_no_gpu(lib):
    f = lib.symode_jacobian_constant
    # (jgx, n_g, S, n, d, table, flag, stream)
    assert f(JUNK, 1, 1, 100, 0, JUNK, JUNK, NULL) == -1 and f(JUNK, 1, 1, 100, 5, JUNK, JUNK, NULL) == -1      # d outside 1..4
    assert f(JUNK, 0, 1, 100, 2, JUNK, JUNK, NULL) == -3                                                        # n_g < 1
    assert f(JUNK, 1, 0, 100, 2, JUNK, JUNK, NULL) == -3 and f(JUNK, 1, 65536, 100, 2, JUNK, JUNK, NULL) == -3
    assert f(JUNK, 1, 1, 0, 2, JUNK, JUNK, NULL) == -3
    assert f(JUNK, 40000, 65535, 100, 2, JUNK, JUNK, NULL) == -3                                                # S n_g beyond the grid
    assert f(NULL, 1, 1, 100, 2, JUNK, JUNK, NULL) == -2
    assert f(JUNK, 1, 1, 100, 2, NULL, JUNK, NULL) == -2
    assert f(JUNK, 1, 1, 100, 2, JUNK, NULL, NULL) == -2
    assert f(ODD, 1, 1, 100, 2, JUNK, JUNK, NULL) == -5
    assert f(JUNK, 1, 1, 100, 2, ODD, JUNK, NULL) == -5
    assert f(JUNK, 1, 1, 100, 2, JUNK, ODD, NULL) == -5


def test_regulariser_constj_argument_validation_needs_no_gpu(lib):
    f = lib.symode_symreg_reversed_batched_constj
    big = 1 << 34
    # (x, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, loss, grad, ws, ws_bytes, stream)
    ok = [JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, NULL, 1.0, JUNK, JUNK, JUNK, big, NULL]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    assert call(a6=9) == -1 and call(a7=6) == -1 and call(a8=4) == -1         # no such library
    assert call(a3=0) == -3 and call(a3=-1) == -3                              # n_g < 1 (the materialised entry allows 0)
    assert call(a4=0) == -3 and call(a4=65536) == -3 and call(a5=0) == -3
    for k in (0, 1, 2, 9, 12, 13):
        assert call(**{f"a{k}": NULL}) == -2, k
    for k in (0, 1, 2, 9, 10, 12, 13):
        assert call(**{f"a{k}": ODD}) == -5, k
    assert call(a14=NULL) == -4 and call(a14=ctypes.c_void_p(0x1004)) == -4
    need = lib.symode_workspace_bytes(2, 3, 0, 1, 100)
    assert need > 8 and call(a15=need - 8) == -4 and call(a15=0) == -4


def test_fused_closure_constj_argument_validation_needs_no_gpu(lib):
    f = lib.symode_loss_grad_reversed_constj
    big = 1 << 34
    # (x, dx, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
    ok = [JUNK, JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, NULL, 1.0, 0.1, JUNK, JUNK, JUNK, big, NULL]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    assert call(a7=9) == -1 and call(a8=6) == -1 and call(a9=4) == -1         # no such library
    assert call(a4=0) == -3 and call(a4=-2) == -3                              # n_g < 1
    assert call(a5=0) == -3 and call(a5=65536) == -3 and call(a6=0) == -3
    for k in (0, 1, 2, 3, 10, 14, 15):
        assert call(**{f"a{k}": NULL}) == -2, k
    for k in (0, 1, 2, 3, 10, 11, 14, 15):
        assert call(**{f"a{k}": ODD}) == -5, k
    assert call(a16=NULL) == -4 and call(a16=ctypes.c_void_p(0x1004)) == -4
    need = lib.symode_workspace_bytes(2, 5, 0, 1, 100)
    assert need > 8 and call(a17=need - 8) == -4 and call(a17=0) == -4


# The four batched entries of the reversed closure share one validation path.  Per entry: where its operands sit.
_REG = dict(ptrs=(0, 1, 2, 9, 12, 13), mask=10, n_g=3, S=4, n=5, lib=(6, 7, 8), ws=14, ws_bytes=15,
            # (x, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, loss, grad, ws, ws_bytes, stream)
            ok=lambda big: [JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, NULL, 1.0, JUNK, JUNK, JUNK, big, NULL])
_FUSED = dict(ptrs=(0, 1, 2, 3, 10, 14, 15), mask=11, n_g=4, S=5, n=6, lib=(7, 8, 9), ws=16, ws_bytes=17,
              # (x, dx, gx, jgx, n_g, S, n, d, order, flags, xi, mask, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
              ok=lambda big: [JUNK, JUNK, JUNK, JUNK, 1, 1, 100, 2, 3, 0, JUNK, NULL, 1.0, 0.1, JUNK, JUNK, JUNK, big, NULL])
BATCHED_ENTRIES = {"symode_symreg_reversed_batched": _REG, "symode_symreg_reversed_batched_constj": _REG,
                   "symode_loss_grad_reversed": _FUSED, "symode_loss_grad_reversed_constj": _FUSED}


@pytest.mark.parametrize("name", sorted(BATCHED_ENTRIES))
def test_batched_reversed_entries_share_one_table_of_bad_arguments(lib, name):
    f, lay = getattr(lib, name), BATCHED_ENTRIES[name]
    ok = lay["ok"](1 << 34)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[lay[k] if isinstance(lay.get(k), int) else int(k[1:])] = v
        return f(*a)

    k_d, k_order, k_flags = lay["lib"]
    bad_lib = [{f"a{k_d}": 9}, {f"a{k_order}": 6}, {f"a{k_flags}": 4}]
    for kw in bad_lib:
        assert call(**kw) == -1, kw                                            # library outside the compiled set
    assert call(S=0) == -3 and call(S=65536) == -3 and call(n=0) == -3
    for k in lay["ptrs"]:
        assert call(**{f"a{k}": NULL}) == -2, k                                # every required pointer
    for k in lay["ptrs"] + (lay["mask"],):                                     # (mask may be null, not odd)
        assert call(**{f"a{k}": ODD}) == -5, k
    need = lib.symode_workspace_bytes(2, 3, 0, 1, 100)
    assert need > 8
    assert call(ws=NULL) == -4 and call(ws=ctypes.c_void_p(0x1004)) == -4 and call(ws_bytes=need - 8) == -4
    # n_g = 0: a regulariser of no group element is what only the materialised regulariser accepts (it goes on to the
    # later checks: here it stops at the workspace)
    if name == "symode_symreg_reversed_batched":
        assert call(n_g=0, ws=NULL) == -4 and call(n_g=0, a1=NULL, a2=NULL, ws=NULL) == -4
    else:
        assert call(n_g=0) == -3
    assert call(n_g=-1) == -3
    # the order of the checks: library, sizes, null, alignment, workspace
    p0 = lay["ptrs"][0]
    assert call(**bad_lib[0], S=0) == -1
    assert call(S=0, **{f"a{p0}": NULL}) == -3
    assert call(**{f"a{p0}": NULL, f"a{lay['ptrs'][1]}": ODD}) == -2
    assert call(**{f"a{p0}": ODD}, ws=NULL) == -5


def test_python_layer_names_the_new_entry_points():
    import inspect
    from symode_amd.batched import BatchedClosure
    assert hasattr(engine.HipEngine, "jacobian_constant")
    assert hasattr(engine.HipEngine, "loss_grad_reversed") and hasattr(engine.HipEngine, "symreg_reversed")
    assert inspect.signature(BatchedClosure.__init__).parameters["const_jacobian"].default is None
