"""CPU-side checks of the device shuffle's surface: the three keyed epoch entries and symode_adam_order_table are additive
(the ABI version stays the bindings'), their bindings carry the declared number of arguments, every refusal of
include/symode.h is an error code before any launch, and the nothing-to-do cases look at no pointer."""
import ctypes
import os
import re

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("symode_adam_epochs_keyed", "symode_adam_epochs_reversed_keyed", "symode_adam_epochs_latent_keyed",
           "symode_adam_order_table")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # non-null, aligned, never dereferenced: validation fails first
ODD = ctypes.c_void_p(0x1002)

_STATE = ("params", "m", "v", "step", "mask", "xi", "log")


def _tail(a):
    return (a["S"], a["d"], a["order"], a["flags"], a["q"], a["r"], 1, a["n_params"], 1e-2, 0.9, 0.999, 1e-8)


def _plain(lib, **over):
    a = dict(x=JUNK, dx=JUNK, n_src=300, seeds=JUNK, n_seeds=1, shuffle=1, n_epochs=3, batch=77, S=2, d=2, order=2, flags=0,
             q=NULL, r=0, n_params=12, epoch0=0, **{k: JUNK for k in _STATE})
    a.update(over)
    return lib.symode_adam_epochs_keyed(a["x"], a["dx"], a["n_src"], a["seeds"], a["n_seeds"], a["shuffle"], a["n_epochs"],
                                        a["batch"], *_tail(a), 1.0, 1e-3, 1, 0.1, 2, a["epoch0"], 1e-4,
                                        *(a[k] for k in _STATE), NULL)


def _reversed(lib, **over):
    a = dict(x=JUNK, dx=JUNK, gx=JUNK, jgx=JUNK, n_g=2, n_src=300, seeds=JUNK, n_seeds=1, shuffle=1, n_epochs=3, batch=77, S=2,
             d=2, order=2, flags=0, q=NULL, r=0, n_params=12, epoch0=0, w_x=1.0, **{k: JUNK for k in _STATE})
    a.update(over)
    return lib.symode_adam_epochs_reversed_keyed(a["x"], a["dx"], a["gx"], a["jgx"], a["n_g"], a["n_src"], a["seeds"],
                                                 a["n_seeds"], a["shuffle"], a["n_epochs"], a["batch"], *_tail(a), a["w_x"],
                                                 1e-3, 0.25, 1, 0.1, 2, a["epoch0"], 1e-4, *(a[k] for k in _STATE), NULL)


def _latent(lib, **over):
    a = dict(x=JUNK, dx=JUNK, B=JUNK, y=JUNK, e=JUNK, D_obs=4, L=JUNK, n_gen=1, n_src=300, seeds=JUNK, n_seeds=1, shuffle=1,
             n_epochs=3, batch=77, S=2, d=2, order=2, flags=0, q=NULL, r=0, n_params=12, epoch0=0, w_z=1.0,
             **{k: JUNK for k in _STATE})
    a.update(over)
    return lib.symode_adam_epochs_latent_keyed(a["x"], a["dx"], a["B"], a["y"], a["e"], a["D_obs"], a["L"], a["n_gen"],
                                               a["n_src"], a["seeds"], a["n_seeds"], a["shuffle"], a["n_epochs"], a["batch"],
                                               *_tail(a), a["w_z"], 0.5, 1e-3, 1e-3, 1, 0.1, 2, a["epoch0"], 1e-4,
                                               *(a[k] for k in _STATE), NULL)


def _table(lib, n_src=300, batch=77, seeds=JUNK, n_seeds=3, shuffle=1, epoch0=0, n_epochs=3, out=JUNK):
    return lib.symode_adam_order_table(n_src, batch, seeds, n_seeds, shuffle, epoch0, n_epochs, out, NULL)


def test_the_four_entries_are_additive(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    for name in ENTRIES:
        assert name in engine._SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(engine._SIGNATURES[name][1]), name       # the binding's argument count
    for name in ("adam_epochs_keyed", "adam_epochs_reversed_keyed", "adam_epochs_latent_keyed", "adam_order_table"):
        assert hasattr(engine.HipEngine, name)


def test_a_keyed_entry_takes_its_siblings_arguments_with_the_table_replaced():
    for name in ENTRIES[:3]:
        keyed, sibling = engine._SIGNATURES[name][1], engine._SIGNATURES[name[:-len("_keyed")]][1]
        assert len(keyed) == len(sibling), name              # (idx, n_idx, n_epochs, n_steps, batch) -> (seeds, n, shuffle, n_epochs, batch)
        at = next(k for k in range(len(sibling)) if sibling[k:k + 5] == [ctypes.c_void_p, ctypes.c_long] + [ctypes.c_int] * 3
                  and sibling[k - 1] is ctypes.c_long)
        assert keyed[:at] == sibling[:at] and keyed[at + 5:] == sibling[at + 5:], name


@pytest.mark.parametrize("call", [_plain, _reversed, _latent], ids=["plain", "reversed", "latent"])
def test_the_keyed_entries_refuse_before_any_launch(lib, call):
    assert call(lib, seeds=NULL) == -2 and call(lib, seeds=ODD) == -5
    assert call(lib, n_seeds=0) == -3 and call(lib, n_seeds=3) == -3 and call(lib, n_seeds=-1) == -3     # 1 or S
    assert call(lib, n_seeds=2, log=NULL) == -2                                                       # (S seeds accepted)
    assert call(lib, n_src=0) == -3 and call(lib, n_src=-5) == -3 and call(lib, n_src=2 ** 31) == -3      # rows are int32
    assert call(lib, n_src=2 ** 31 - 1, log=NULL) == -2
    assert call(lib, batch=0) == -3 and call(lib, batch=-1) == -3
    assert call(lib, batch=2 ** 31 - 1, log=NULL) == -2                                               # one padded step
    # everything the siblings refuse
    assert call(lib, d=7) == -1 and call(lib, order=6) == -1 and call(lib, flags=4) == -1
    assert call(lib, n_epochs=-1) == -3 and call(lib, S=-1) == -3 and call(lib, epoch0=-1) == -3
    assert call(lib, n_params=11) == -3
    assert call(lib, q=JUNK, r=3, n_params=12) == -3 and call(lib, q=JUNK, r=0, n_params=2) == -3
    for name in ("x", "dx") + _STATE:
        assert call(lib, **{name: NULL}) == -2, name
        assert call(lib, **{name: ODD}) == -5, name
    # nothing to do: no pointer is looked at
    empty = dict(x=NULL, dx=NULL, seeds=NULL, **{k: NULL for k in _STATE})
    assert call(lib, n_epochs=0, **empty) == 0 and call(lib, S=0, **empty) == 0
    assert call(lib, d=7, n_epochs=0, **empty) == -1                                                  # ... but the library is


def test_the_reversed_and_latent_entries_keep_their_own_refusals(lib):
    assert _reversed(lib, n_g=-1) == -3 and _reversed(lib, w_x=0.0) == -3
    assert _reversed(lib, gx=NULL) == -2 and _reversed(lib, jgx=ODD) == -5
    assert _reversed(lib, n_g=0, gx=NULL, jgx=NULL, log=NULL) == -2                                   # no elements: none read
    assert _latent(lib, n_gen=-1) == -3 and _latent(lib, w_z=0.0) == -3 and _latent(lib, D_obs=1) == -3
    assert _latent(lib, e=NULL) == -3 and _latent(lib, L=NULL) == -3                                  # D_obs > d, n_gen > 0
    assert _latent(lib, B=NULL) == -2 and _latent(lib, y=ODD) == -5


def test_the_order_table_refuses_before_any_launch(lib):
    assert _table(lib, seeds=NULL) == -2 and _table(lib, out=NULL) == -2
    assert _table(lib, seeds=ODD) == -5 and _table(lib, out=ODD) == -5
    assert _table(lib, n_src=0) == -3 and _table(lib, n_src=2 ** 31) == -3
    assert _table(lib, batch=0) == -3 and _table(lib, n_seeds=0) == -3
    assert _table(lib, n_epochs=-1) == -3 and _table(lib, epoch0=-1) == -3
    assert _table(lib, n_epochs=0, seeds=NULL, out=NULL) == 0


def test_the_existing_entries_still_refuse_a_null_table(lib):
    out = lib.symode_adam_epochs(JUNK, JUNK, 300, NULL, 1, 3, 4, 77, 2, 2, 2, 0, NULL, 0, 1, 12, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1e-3,
                                 1, 0.1, 2, 0, 1e-4, JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, NULL)
    assert out == -2


def test_the_parser_has_the_flag_and_it_is_off_by_default():
    from symode_amd.parser_utils import get_args
    assert get_args(argv=[]).device_shuffle is False
    assert get_args(argv=["--device_shuffle"]).device_shuffle is True


def _sweep_args(**over):
    a = {"config": None, "sindy_optimizer": "adam", "use_latent": False, "w_sym_reg": 0.0, "sym_reg_type": "i",
         "load_laligan": None, "fix_laligan": False, "sindy_reg_type": "l1", "eq_constraint": False, "device_shuffle": True}
    a.update(over)
    return a


def test_main_sweep_takes_the_flag_with_adam_alone():
    from symode_amd.main_sweep import _refusal
    assert _refusal(_sweep_args()) is None and _refusal(_sweep_args(eq_constraint=True)) is None
    for why in (_refusal(_sweep_args(sindy_optimizer="lbfgs")), _refusal(_sweep_args(sindy_optimizer="lbfgs"), "stlsq")):
        assert why is not None and why.startswith("--device_shuffle") and "--sindy_optimizer adam" in why
    # the rule comes after the existing ones: what was refused before is refused in the same words
    for args, method in ((_sweep_args(use_latent=True), "lbfgs"), (_sweep_args(w_sym_reg=0.1), "lbfgs"), (_sweep_args(), "stlsq"),
                         (_sweep_args(sindy_optimizer="lbfgs", eq_constraint=True), "stlsq")):
        assert _refusal(args, method) == _refusal(dict(args, device_shuffle=False), method) is not None


def test_main_and_train_SIGED_name_the_flag_they_refuse():
    from symode_amd import main as main_mod, train
    with pytest.raises(SystemExit, match="--device_shuffle .* needs --device_adam"):
        main_mod.main(["--task", "dosc", "--ae_arch", "none", "--sindy_optimizer", "adam", "--device_shuffle"])
    with pytest.raises(SystemExit, match="--device_shuffle .* needs --device_adam"):
        main_mod.main(["--task", "dosc", "--sindy_optimizer", "lbfgs", "--device_adam", "--device_shuffle"])
    with pytest.raises(ValueError, match="device_shuffle .* needs device_adam"):
        train.train_SIGED(*([None] * 34), device_shuffle=True)
