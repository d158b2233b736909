"""CPU-side checks of the grid trainer's C ABI (symode_trainer_grid and its four entries, symode_quad_closure_grid): the
entries are additive (the ABI version stays the binding's, ``symode_trainer`` gains no field), ``symode_trainer_grid`` is
laid out as the ctypes mirror ``engine.TrainerGrid`` says (sizeof and every offset from a C program compiled against
include/symode.h), and every refusal of the header is an error code before any device work: the pointers below are junk
and none is dereferenced."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK, ODD = None, 0x1000, 0x1004         # JUNK: non-null, 256-byte aligned; ODD: 4-byte but not 16-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
ENTRIES = ("symode_trainer_grid_closure", "symode_trainer_grid_update", "symode_trainer_grid_epoch_end", "symode_trainer_grid_run")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _grid(hyper=JUNK, n_sets=3, **over):
    """A complete Gram-form descriptor: 9 problems of the (2, 2, 0) library (p = 6, d p = 12) on 3 sets of matrices."""
    a = dict(closure=engine.CLOSURE_GRAM, aug_gram=JUNK, rev_gram=JUNK, n_problems=9, n_points=200, d=2, order=2, flags=0,
             inv_count=1.0 / 400, n_params=12, w_x=1.0, l1=1, tol_grad=1e-7, tol_change=1e-9, max_iter=4, history=3, tol_update=1e-3,
             near_band=1e-4, st_freq=2, state=JUNK, state_bytes=1 << 30, log=JUNK, log_test=JUNK, log_epochs=8)
    a.update(over)
    G = engine.TrainerGrid()
    G.base = engine.TrainerDesc(**a)
    G.hyper, G.n_sets = hyper, n_sets
    return G


def _calls(lib, G):
    """The four entries on one descriptor (or NULL): their return codes."""
    p = None if G is None else ctypes.byref(G)
    return [lib.symode_trainer_grid_closure(p, None, None, None), lib.symode_trainer_grid_update(p, engine.LBFGS_BEGIN, None),
            lib.symode_trainer_grid_epoch_end(p, 0, None), lib.symode_trainer_grid_run(p, 0, 1, 0, None)]


def test_the_entries_are_additive(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    assert re.search(r"#define SYMODE_TRAINER_HYPER 4\b", header) and engine.TRAINER_HYPER == 4
    for name in ENTRIES + ("symode_quad_closure_grid",):
        assert hasattr(lib, name), name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(args.split(",")) == len(engine._SIGNATURES[name][1]), name
    # the scalar entries are not widened: the table travels in the descriptor that wraps the old one
    for name in ("symode_trainer_closure", "symode_trainer_update", "symode_trainer_epoch_end", "symode_trainer_run", "symode_quad_closure"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and "hyper" not in decl.group(1) and "symode_trainer_grid" not in decl.group(1), name
        assert len(decl.group(1).split(",")) == len(engine._SIGNATURES[name][1]), name
    body = re.search(r"typedef struct symode_trainer \{(.*?)\} symode_trainer;", header, re.S).group(1)
    assert "hyper" not in body and "n_sets" not in body


def test_the_struct_is_laid_out_as_the_ctypes_mirror_says():
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    outer = [n for n, _ in engine.TrainerGrid._fields_]
    inner = [n for n, _ in engine.TrainerDesc._fields_]
    assert outer == ["base", "hyper", "n_sets"]
    src = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"symode_trainer_grid_layout_{os.getpid()}.c")
    exe = src[:-2]
    exprs = ["sizeof(symode_trainer_grid)", "sizeof(symode_trainer)"] + [f"offsetof(symode_trainer_grid, {n})" for n in outer] \
        + [f"offsetof(symode_trainer_grid, base.{n})" for n in inner]
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "symode.h"\n'
                'int main(void) { printf("' + ' '.join(["%zu"] * len(exprs)) + '\\n", ' + ', '.join(exprs) + '); return 0; }\n')
    try:
        r = subprocess.run([cc, "-std=c99", f"-I{os.path.join(ROOT, 'include')}", src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]                    # a field the header does not have fails here
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    D, T = engine.TrainerGrid, engine.TrainerDesc
    assert got == [ctypes.sizeof(D), ctypes.sizeof(T)] + [getattr(D, n).offset for n in outer] \
        + [D.base.offset + getattr(T, n).offset for n in inner]
    assert D.base.offset == 0                                          # &G->base is G: layout and init serve it unchanged
    # ... and the header has no field the mirror lacks: the struct's declarators, in order
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    body = re.search(r"typedef struct symode_trainer_grid \{(.*?)\} symode_trainer_grid;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip())]
    assert declared == outer


def test_every_entry_refuses_before_any_launch(lib):
    assert _calls(lib, None) == [NULLPTR] * 4                                            # G == NULL
    assert _calls(lib, _grid(hyper=NULL)) == [NULLPTR] * 4
    assert _calls(lib, _grid(aug_gram=NULL)) == [NULLPTR] * 4
    for kind in (engine.CLOSURE_STREAM, engine.CLOSURE_LATENT, 7):                       # the Gram form only
        assert _calls(lib, _grid(closure=kind, x=JUNK, dx=JUNK, workspace=JUNK, latent_B=JUNK, latent_y=JUNK)) == [BADSIZE] * 4, kind
    for n_sets in (0, -3, 2, 4, 18):                                                     # 9 problems: 1, 3 and 9 sets divide them
        assert _calls(lib, _grid(n_sets=n_sets)) == [BADSIZE] * 4, n_sets
    assert _calls(lib, _grid(hyper=ODD)) == [ALIGN] * 4 and _calls(lib, _grid(hyper=0x1008)) == [ALIGN] * 4
    # in the order of the header: a NULL table before the kind, the kind before the sets, the sets before the alignment
    assert _calls(lib, _grid(hyper=NULL, closure=engine.CLOSURE_STREAM)) == [NULLPTR] * 4
    assert _calls(lib, _grid(hyper=ODD, n_sets=2)) == [BADSIZE] * 4


def test_what_the_scalar_trainer_refuses_keeps_its_code(lib):
    scalar = lambda G: [lib.symode_trainer_closure(ctypes.byref(G.base), None, None, None),  # noqa: E731
                        lib.symode_trainer_update(ctypes.byref(G.base), engine.LBFGS_BEGIN, None),
                        lib.symode_trainer_epoch_end(ctypes.byref(G.base), 0, None), lib.symode_trainer_run(ctypes.byref(G.base), 0, 1, 0, None)]
    cases = [dict(d=7), dict(order=9), dict(n_problems=65536, n_sets=1), dict(n_points=0), dict(n_params=11), dict(history=0),
             dict(history=129), dict(max_iter=0), dict(log_epochs=0), dict(state=NULL), dict(log=NULL), dict(log_test=NULL),
             dict(state_bytes=16), dict(state=0x1010), dict(q_eff=JUNK, r=0, n_params=2)]
    want = {"d": UNSUPPORTED, "order": UNSUPPORTED, "state": NULLPTR, "log": NULLPTR, "log_test": NULLPTR, "state_bytes": WORKSPACE}
    for over in cases:
        n_sets = over.pop("n_sets", 3)
        G = _grid(n_sets=n_sets, **over)
        got = _calls(lib, G)
        assert got == scalar(G), over                                  # the same code as the scalar entry on &G->base
        key = next(iter(over))
        code = ALIGN if over.get("state") == 0x1010 else want.get(key, BADSIZE)
        assert got == [code] * 4, (over, got)
    G = _grid()
    assert lib.symode_trainer_grid_update(ctypes.byref(G), 3, None) == BADSIZE           # a mode that is neither BEGIN nor ACCEPT
    assert lib.symode_trainer_grid_epoch_end(ctypes.byref(G), -1, None) == BADSIZE
    assert lib.symode_trainer_grid_run(ctypes.byref(G), -1, 1, 0, None) == BADSIZE
    assert lib.symode_trainer_grid_run(ctypes.byref(G), 0, -1, 0, None) == BADSIZE
    assert lib.symode_trainer_grid_run(ctypes.byref(G), 0, 0, 0, None) == OK             # no epochs: nothing is launched
    assert lib.symode_trainer_grid_epoch_end(ctypes.byref(_grid(log_xi=JUNK)), 0, None) == NULLPTR   # the detail rows: all or none


def test_the_quad_closure_grid_refuses_before_any_launch(lib):
    def call(aug=JUNK, rev=JUNK, n_sets=3, n=9, d=2, p=6, xi=JUNK, mask=JUNK, hyper=JUNK, loss=JUNK, grad=JUNK):
        return lib.symode_quad_closure_grid(aug, rev, n_sets, n, d, p, xi, mask, 0.5, hyper, loss, grad, None)
    assert call(n=0) == BADSIZE and call(d=0) == BADSIZE and call(p=0) == BADSIZE and call(d=2, p=129) == BADSIZE
    assert call(n_sets=0) == BADSIZE and call(n_sets=2) == BADSIZE and call(n_sets=18) == BADSIZE and call(n=2 ** 31) == BADSIZE
    for name in ("aug", "xi", "hyper", "loss", "grad"):
        assert call(**{name: NULL}) == NULLPTR, name
    for name in ("aug", "rev", "xi", "mask", "hyper", "loss", "grad"):
        assert call(**{name: 0x1002}) == ALIGN, name


def test_the_python_layers_take_the_keyword():
    import inspect
    from symode_amd.device_lbfgs import HYPER_COLUMNS, MAX_PROBLEMS, DeviceTrainer
    from symode_amd.sweep import SeedSweepLBFGS
    assert inspect.signature(DeviceTrainer.__init__).parameters["hyper"].default is None
    assert inspect.signature(SeedSweepLBFGS.fit).parameters["hyper"].default is None
    q = inspect.signature(engine.HipEngine.quad_closure).parameters
    assert q["hyper"].default is None and q["n_sets"].default is None
    assert HYPER_COLUMNS == ("lr", "w_reg", "threshold", "w_sym") and len(HYPER_COLUMNS) == engine.TRAINER_HYPER
    assert MAX_PROBLEMS == 65535
