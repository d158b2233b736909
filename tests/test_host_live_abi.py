"""CPU-side checks of the _live entries of the reversed closure (symode_loss_grad_reversed_constj_live,
symode_symreg_reversed_batched_constj_live): they take their siblings' arguments plus one 64-bit column set and refuse bad
arguments with the siblings' codes, in the siblings' order, before anything is launched (-1 unsupported, -2 null, -3 size,
-4 workspace, -5 alignment).  No column set is a bad argument: one the library has no kernel for runs the dense kernel."""
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
ODD_DEGREES_O5 = 0x1F83C7                # {0, 1, 2, 6-9, 15-20}

# where the operands sit; the sibling's layout with `live` behind the mask
_REG = dict(sibling="symode_symreg_reversed_batched_constj", ptrs=(0, 1, 2, 9, 13, 14), mask=10, live=11, n_g=3, S=4, n=5, lib=(6, 7, 8),
            ws=15, ws_bytes=16,
            # (x, gx, jgx, n_g, S, n, d, order, flags, xi, mask, live, inv_count, loss, grad, ws, ws_bytes, stream)
            ok=lambda big: [JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, NULL, ODD_DEGREES_O5, 1.0, JUNK, JUNK, JUNK, big, NULL])
_FUSED = dict(sibling="symode_loss_grad_reversed_constj", ptrs=(0, 1, 2, 3, 10, 15, 16), mask=11, live=12, n_g=4, S=5, n=6, lib=(7, 8, 9),
              ws=17, ws_bytes=18,
              # (x, dx, gx, jgx, n_g, S, n, d, order, flags, xi, mask, live, inv_count, w_sym, loss2, grad, ws, ws_bytes, stream)
              ok=lambda big: [JUNK, JUNK, JUNK, JUNK, 1, 1, 100, 2, 5, 0, JUNK, NULL, ODD_DEGREES_O5, 1.0, 0.1, JUNK, JUNK, JUNK, big,
                              NULL])
LIVE_ENTRIES = {"symode_symreg_reversed_batched_constj_live": _REG, "symode_loss_grad_reversed_constj_live": _FUSED}


def test_the_entries_are_additions_to_the_same_abi_version(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8
    for name, lay in LIVE_ENTRIES.items():
        assert hasattr(lib, name) and name in engine._SIGNATURES
        mine, theirs = engine._SIGNATURES[name], engine._SIGNATURES[lay["sibling"]]
        assert mine[0] is theirs[0]
        assert mine[1][:lay["live"]] + mine[1][lay["live"] + 1:] == theirs[1]          # the sibling's arguments ...
        assert mine[1][lay["live"]] is ctypes.c_ulonglong                               # ... and the set behind the mask


@pytest.mark.parametrize("name", sorted(LIVE_ENTRIES))
def test_live_entries_refuse_what_their_siblings_refuse(lib, name):
    lay = LIVE_ENTRIES[name]
    f, g = getattr(lib, name), getattr(lib, lay["sibling"])
    ok = lay["ok"](1 << 34)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[lay[k] if isinstance(lay.get(k), int) else int(k[1:])] = v
        b = a[:lay["live"]] + a[lay["live"] + 1:]
        rc = f(*a)
        assert rc == g(*b), (kw, rc)                                            # the sibling's code, whatever it is
        return rc

    k_d, k_order, k_flags = lay["lib"]
    bad_lib = [{f"a{k_d}": 9}, {f"a{k_order}": 6}, {f"a{k_flags}": 4}]
    for kw in bad_lib:
        assert call(**kw) == -1, kw                                            # library outside the compiled set
    assert call(S=0) == -3 and call(S=65536) == -3 and call(n=0) == -3
    assert call(n_g=0) == -3 and call(n_g=-1) == -3                            # the compact table needs a group element
    for k in lay["ptrs"]:
        assert call(**{f"a{k}": NULL}) == -2, k                                # every required pointer
    for k in lay["ptrs"] + (lay["mask"],):                                     # (mask may be null, not odd)
        assert call(**{f"a{k}": ODD}) == -5, k
    need = lib.symode_workspace_bytes(2, 5, 0, 1, 100)
    assert need > 8
    assert call(ws=NULL) == -4 and call(ws=ctypes.c_void_p(0x1004)) == -4 and call(ws_bytes=need - 8) == -4 and call(ws_bytes=0) == -4
    # the order of the checks: library, sizes, null, alignment, workspace
    p0 = lay["ptrs"][0]
    assert call(**bad_lib[0], S=0) == -1
    assert call(S=0, **{f"a{p0}": NULL}) == -3
    assert call(**{f"a{p0}": NULL, f"a{lay['ptrs'][1]}": ODD}) == -2
    assert call(**{f"a{p0}": ODD}, ws=NULL) == -5
    # no column set is refused, and none changes which check answers: empty, all ones, one even-degree bit, bits past p
    for live in (0, 0xFFFFFFFFFFFFFFFF, ODD_DEGREES_O5 | 1 << 3, 1 << 63):
        assert call(live=live, ws=NULL) == -4 and call(live=live, S=0) == -3 and call(live=live, **{f"a{p0}": NULL}) == -2


def test_python_layer_names_the_column_set():
    import inspect
    from symode_amd.batched import BatchedClosure
    from symode_amd.coef_map import CoefMap
    assert inspect.signature(engine.HipEngine.loss_grad_reversed).parameters["live_columns"].default is None
    assert inspect.signature(engine.HipEngine.symreg_reversed).parameters["live_columns"].default is None
    assert inspect.signature(BatchedClosure.__init__).parameters["live_columns"].default is True
    assert inspect.signature(BatchedClosure.loss_grad_xi).parameters["live_columns"].default is None
    assert hasattr(CoefMap, "live_columns") and hasattr(CoefMap, "live_mask")
