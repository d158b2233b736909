"""CPU-side checks of the device Adam trainer's reversed symmetry regulariser: symode_adam_epochs_reversed is an additive
entry (it came with ABI version 7, the L-BFGS trainer descriptor's) whose argument validation returns error codes before any launch; main_sweep keeps refusing
Adam with a symmetry regulariser;
DeviceAdam checks the shapes of ``reversed_sym``; train_SIGED(device_adam=True) refuses the i / f regularisers and an
unfrozen LaLiGAN without touching a device."""
import ctypes
import os
import re

import pytest
import torch

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


NULL = ctypes.c_void_p(None)
JUNK = ctypes.c_void_p(0x1000)           # non-null, aligned, never dereferenced: validation fails first
ODD = ctypes.c_void_p(0x1002)


def _call(lib, x=JUNK, dx=JUNK, gx=JUNK, jgx=JUNK, n_g=2, n_src=300, idx=JUNK, n_tab=1, n_epochs=3, n_steps=4, batch=77, S=2,
          d=2, order=2, flags=0, q=NULL, r=0, allow_const=1, n_params=12, w_x=1.0, w_sym=0.1, params=JUNK, m=JUNK, v=JUNK,
          step=JUNK, mask=JUNK, xi=JUNK, log=JUNK, epoch0=0):
    return lib.symode_adam_epochs_reversed(x, dx, gx, jgx, n_g, n_src, idx, n_tab, n_epochs, n_steps, batch, S, d, order, flags,
                                           q, r, allow_const, n_params, 1e-2, 0.9, 0.999, 1e-8, w_x, 1e-3, w_sym, 1, 0.1, 2,
                                           epoch0, 1e-4, params, m, v, step, mask, xi, log, NULL)


def test_the_entry_is_additive_with_the_documented_signature(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert hasattr(lib, "symode_adam_epochs_reversed") and hasattr(engine.HipEngine, "adam_epochs_reversed")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "symode.h")).read(), flags=re.S)
    decl = {name: re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1).split(",")
            for name in ("symode_adam_epochs", "symode_adam_epochs_reversed")}
    words = {name: [" ".join(a.split()) for a in args] for name, args in decl.items()}
    plain, rev = words["symode_adam_epochs"], words["symode_adam_epochs_reversed"]
    # the arguments of symode_adam_epochs plus gx, jgx, n_g (after dx) and w_sym (after w_reg)
    at = plain.index("float w_reg") + 1
    assert rev == plain[:2] + ["const float* gx", "const float* jgx", "int n_g"] + plain[2:at] + ["float w_sym"] + plain[at:]
    res, args = engine._SIGNATURES["symode_adam_epochs_reversed"]
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    assert res is ctypes.c_int and args == [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in rev]


def test_argument_errors_are_returned_before_any_launch(lib):
    assert _call(lib, d=7) == -1 and _call(lib, order=6) == -1 and _call(lib, flags=4) == -1      # no such library
    assert _call(lib, n_g=-1) == -3
    assert _call(lib, gx=NULL) == -2 and _call(lib, jgx=NULL) == -2                               # n_g > 0 needs both
    assert _call(lib, gx=ODD) == -5 and _call(lib, jgx=ODD) == -5
    # without group elements the two arrays are not looked at (the call fails on the NEXT thing that is wrong)
    assert _call(lib, n_g=0, gx=NULL, jgx=NULL, log=NULL) == -2 and _call(lib, n_g=0, gx=NULL, jgx=NULL, n_params=11) == -3
    assert _call(lib, n_g=0, gx=ODD, jgx=ODD, log=ODD) == -5
    # the regulariser is weighed against the residual: w_x > 0 with group elements; without them any w_x, as the plain entry
    assert _call(lib, w_x=0.0) == -3 and _call(lib, w_x=-1.0) == -3 and _call(lib, w_x=float("nan")) == -3
    assert _call(lib, n_g=0, w_x=0.0, log=NULL) == -2
    # the checks of symode_adam_epochs hold here too
    assert _call(lib, n_tab=3) == -3 and _call(lib, n_tab=0) == -3 and _call(lib, n_tab=2, log=NULL) == -2
    assert _call(lib, n_epochs=-1) == -3 and _call(lib, S=-1) == -3 and _call(lib, n_src=0) == -3 and _call(lib, n_src=2 ** 31) == -3
    assert _call(lib, n_steps=0) == -3 and _call(lib, batch=0) == -3 and _call(lib, epoch0=-1) == -3 and _call(lib, n_params=11) == -3
    for name in ("x", "dx", "idx", "params", "m", "v", "step", "mask", "xi", "log"):
        assert _call(lib, **{name: NULL}) == -2, name
        assert _call(lib, **{name: ODD}) == -5, name
    empty = dict(x=NULL, dx=NULL, gx=NULL, jgx=NULL, idx=NULL, params=NULL, m=NULL, v=NULL, step=NULL, mask=NULL, xi=NULL, log=NULL)
    assert _call(lib, n_epochs=0, **empty) == 0 and _call(lib, S=0, **empty) == 0                 # nothing to do
    assert _call(lib, n_epochs=0, n_g=-1, **empty) == -3


def test_main_sweep_keeps_refusing_adam_with_a_symmetry_regulariser():
    """The sweep is not part of this entry's surface: Adam with any symmetry regulariser, the reversed one on a loaded and
    frozen LaLiGAN included, is still sent to the per-seed command."""
    from symode_amd.main_sweep import _refusal
    base = {"config": None, "sindy_optimizer": "adam", "use_latent": False, "w_sym_reg": 0.1, "load_laligan": "some-laligan",
            "fix_laligan": True, "sindy_reg_type": "l1", "eq_constraint": False}
    for kind in ("i", "f", "r"):
        why = _refusal(dict(base, sym_reg_type=kind))
        assert why is not None and "symmetry regulariser" in why and "symode_amd.main --seed $i" in why
    assert "--use_latent" in _refusal(dict(base, sym_reg_type="r", use_latent=True))
    assert _refusal(dict(base, sym_reg_type="r", w_sym_reg=0.0)) is None


def test_symmetry_operands_keeps_its_old_name():
    from symode_amd import main_sweep, model_utils
    assert main_sweep.symmetry_operands is model_utils.symmetry_operands
    assert main_sweep.PRECOMPUTE_CHUNK == model_utils.PRECOMPUTE_CHUNK == 65536


def _device_adam(reversed_sym, n=10, d=2, w_x=1.0):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    return DeviceAdam(torch.zeros(n, d), torch.zeros(n, d), 2, False, False, CoefMap(d, 6), 1e-2, w_x, 1e-3, 0.1, 2, 4,
                      reversed_sym=reversed_sym)


def test_DeviceAdam_checks_reversed_sym_against_x():
    from symode_amd import device_adam
    z = torch.zeros
    tr = _device_adam((z(2, 10, 2), z(2, 10, 2, 2), 0.1))
    assert tr.reversed_sym[2] == 0.1 and tr.log_columns == device_adam.LOG_COLUMNS + ("loss_sym_reg",)
    assert _device_adam(None).reversed_sym is None and _device_adam(None).log_columns == device_adam.LOG_COLUMNS
    with pytest.raises(ValueError, match="gx must be"):
        _device_adam((z(2, 9, 2), z(2, 10, 2, 2), 0.1))                  # rows
    with pytest.raises(ValueError, match="gx must be"):
        _device_adam((z(10, 2), z(1, 10, 2, 2), 0.1))                    # no group axis
    with pytest.raises(ValueError, match="jgx must be"):
        _device_adam((z(2, 10, 2), z(2, 10, 2), 0.1))                    # a vector where the Jacobian belongs
    with pytest.raises(ValueError, match="jgx must be"):
        _device_adam((z(2, 10, 2), z(2, 10, 2, 3), 0.1))
    with pytest.raises(ValueError, match="group elements"):
        _device_adam((z(2, 10, 2), z(3, 10, 2, 2), 0.1))
    with pytest.raises(ValueError, match="fp32"):
        _device_adam((z(2, 10, 2, dtype=torch.float64), z(2, 10, 2, 2), 0.1))
    with pytest.raises(ValueError, match="w_sindy_x > 0"):
        _device_adam((z(2, 10, 2), z(2, 10, 2, 2), 0.1), w_x=0.0)


class _Untouchable:
    """Stands in for every object train_SIGED must not look at before it has refused."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before refusing")


def _train_kwargs(**over):
    kw = dict(train_loader=_Untouchable(), test_loader=_Untouchable(), num_epochs=2, device="cuda:0", log_interval=1,
              save_interval=10 ** 9, save_dir="t", autoencoder=_Untouchable(), discriminator=_Untouchable(),
              generator=_Untouchable(), lr_ae=0, lr_d=0, lr_g=0, w_recon=0, w_gan=0, w_reg_norm=0, w_reg_ortho=0,
              w_reg_closure=0, use_original_x=False, gan_st_freq=0, gan_st_thres=0.0, ae_arch="none", regressor=_Untouchable(),
              use_latent=False, lr_sindy=1e-2, w_sindy_z=0.0, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=1e-3,
              w_sym_reg=0.1, sym_reg_type="r", st_freq=2, threshold=0.05, int_t=0.1, int_dt=0.01, device_adam=True)
    kw.update(over)
    return kw


def test_train_SIGED_device_adam_refuses_what_the_reversed_kernel_does_not_cover():
    from symode_amd import train
    for kind in ("i", "f"):
        with pytest.raises(ValueError, match=f"sym_reg_type 'r' only, not '{kind}'"):
            train.train_SIGED(**_train_kwargs(sym_reg_type=kind))
    with pytest.raises(ValueError, match="use_latent"):
        train.train_SIGED(**_train_kwargs(use_latent=True))
    frozen, live = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    for q in frozen.parameters():
        q.requires_grad = False
    for ae, gen in ((live, frozen), (frozen, live)):
        with pytest.raises(ValueError, match="frozen autoencoder and generator"):
            train.train_SIGED(**_train_kwargs(autoencoder=ae, generator=gen))
    # frozen on both sides: the refusals are passed, the next check looks at the loader
    with pytest.raises(ValueError, match="DeviceBatches"):
        train.train_SIGED(**_train_kwargs(autoencoder=frozen, generator=frozen, train_loader=[(torch.zeros(4, 2), torch.zeros(4, 2))]))
