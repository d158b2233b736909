"""CPU-side checks of the seed sweep with the reversed symmetry regulariser: the gathered reversed-Gram entry of the C ABI
(exported, bound, its workspace query, argument validation without a GPU) and what main_sweep refuses, with the per-seed
command it names instead."""
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
ODD4 = ctypes.c_void_p(0x1002)           # not 4-byte aligned
ODD8 = ctypes.c_void_p(0x1004)           # 4- but not 8-byte aligned


def test_gathered_reversed_gram_is_exported_and_bound(lib):
    for name in ("symode_symreg_reversed_gram_gather", "symode_symreg_reversed_gram_gather_workspace_bytes"):
        assert hasattr(lib, name)
        assert name in engine._SIGNATURES
    assert hasattr(engine.HipEngine, "symreg_reversed_gram_gather")


def test_gathered_workspace_query_is_zero_exactly_where_the_kernel_is_not_instantiated(lib):
    f = lib.symode_symreg_reversed_gram_gather_workspace_bytes
    dense = lib.symode_symreg_reversed_gram_workspace_bytes
    for d, order in [(1, 1), (1, 3), (1, 5), (2, 1), (2, 3), (2, 5), (3, 1), (3, 2), (3, 3), (3, 4)]:
        for flags in range(4):
            p = lib.symode_lib_size(d, order, flags)
            if p < 0:
                continue
            got = f(d, order, flags, 2, 7, 1001)
            assert (got == 0) == (d * p > 88), (d, order, flags, p, got)
            assert got == dense(d, order, flags, 2, 7, 1001)          # same grid, same partials as the dense sibling
    assert f(9, 3, 0, 1, 1, 1000) == 0                                 # no such library
    assert f(2, 3, 0, 0, 1, 1000) == 0 and f(2, 3, 0, 1, 0, 1000) == 0 and f(2, 3, 0, 1, 1, 0) == 0


def test_gathered_reversed_gram_argument_validation_needs_no_gpu(lib):
    f = lib.symode_symreg_reversed_gram_gather
    big = 1 << 30

    # (x, gx, jgx, n_g, n_src, idx, S, m, d, order, flags, gram, ws, ws_bytes, stream)
    def call(x=JUNK, gx=JUNK, jgx=JUNK, n_g=1, n_src=500, idx=JUNK, S=3, m=100, d=2, order=3, flags=0, gram=JUNK, ws=JUNK,
             ws_bytes=big):
        return f(x, gx, jgx, n_g, n_src, idx, S, m, d, order, flags, gram, ws, ws_bytes, NULL)

    assert call(d=7) == -1                                   # no such library
    assert call(d=3, order=4) == -1                          # d p = 105 > 88: outside the Gram kernel's set
    assert call(m=0) == -3 and call(m=-5) == -3
    assert call(n_g=0) == -3 and call(n_g=-1) == -3
    assert call(S=0) == -3 and call(S=-1) == -3 and call(S=70000) == -3
    assert call(n_src=0) == -3 and call(n_src=-1) == -3 and call(n_src=1 << 31) == -3
    assert call(x=NULL) == -2 and call(gx=NULL) == -2 and call(jgx=NULL) == -2
    assert call(idx=NULL) == -2 and call(gram=NULL) == -2
    assert call(x=ODD4) == -5 and call(gx=ODD4) == -5 and call(jgx=ODD4) == -5 and call(idx=ODD4) == -5
    assert call(gram=ODD8) == -5                             # fp64 output 8-aligned
    assert call(ws=NULL) == -4 and call(ws=ODD8) == -4
    need = lib.symode_symreg_reversed_gram_gather_workspace_bytes(2, 3, 0, 1, 3, 100)
    assert need > 0 and call(ws_bytes=need - 8) == -4


# ---- main_sweep's refusals: decided from the arguments alone, before any data or device is touched ----------------------
BASE = ["--task", "lv", "--sindy_optimizer", "lbfgs", "--w_sindy_x", "1.0", "--w_sym_reg", "0.1", "--n_seeds", "4"]


def _refused(argv):
    from symode_amd import main_sweep
    with pytest.raises(SystemExit) as e:
        main_sweep.main(argv)
    msg = str(e.value.code)
    assert "python -m symode_amd.main --seed" in msg, msg       # the per-seed command to run instead
    return msg


@pytest.mark.parametrize("kind", ["i", "f"])
def test_main_sweep_refuses_the_i_and_f_regularisers(kind):
    msg = _refused(BASE + ["--sym_reg_type", kind, "--load_laligan", "some-laligan", "--fix_laligan"])
    assert "--sym_reg_type r" in msg and f"'{kind}'" in msg


def test_main_sweep_refuses_the_regulariser_without_a_loaded_laligan():
    assert "--load_laligan" in _refused(BASE + ["--sym_reg_type", "r", "--fix_laligan"])


def test_main_sweep_refuses_the_regulariser_on_a_laligan_that_is_not_frozen():
    assert "--fix_laligan" in _refused(BASE + ["--sym_reg_type", "r", "--load_laligan", "some-laligan"])


def test_main_sweep_refuses_latent_fits():
    assert "--use_latent" in _refused(BASE + ["--sym_reg_type", "r", "--load_laligan", "some-laligan", "--fix_laligan",
                                              "--use_latent"])


def test_main_sweep_refusal_names_the_config():
    from symode_amd import main_sweep
    args = {"sindy_optimizer": "lbfgs", "use_latent": False, "w_sym_reg": 0.1, "sym_reg_type": "f", "load_laligan": "x",
            "fix_laligan": True, "config": "lv/noise99_eq_freg.cfg"}
    assert "--config lv/noise99_eq_freg.cfg" in main_sweep._refusal(args)
    assert main_sweep._refusal(dict(args, sym_reg_type="r")) is None
    assert main_sweep._refusal(dict(args, w_sym_reg=0.0, load_laligan=None, fix_laligan=None)) is None
