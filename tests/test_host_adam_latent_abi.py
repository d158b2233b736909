"""CPU-side checks of the device Adam trainer's latent entry: symode_adam_epochs_latent is an additive entry (the ABI
version stays where it was) whose argument validation returns error codes before any launch; DeviceAdam checks the
``latent`` tuple; train_SIGED(device_adam=True, use_latent=True) makes its checks in the documented order without touching
what it has not yet been allowed to look at; model_utils.latent_operands hands out the per-row constant on request only."""
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


def _call(lib, z=JUNK, dz=JUNK, B=JUNK, y=JUNK, e=JUNK, D_obs=4, L=JUNK, n_gen=2, n_src=300, idx=JUNK, n_tab=1, n_epochs=3, n_steps=4,
          batch=77, S=2, d=2, order=2, flags=0, q=NULL, r=0, allow_const=1, n_params=12, w_z=1.0, w_x=0.5, w_sym=0.1, params=JUNK,
          m=JUNK, v=JUNK, step=JUNK, mask=JUNK, xi=JUNK, log=JUNK, epoch0=0):
    return lib.symode_adam_epochs_latent(z, dz, B, y, e, D_obs, L, n_gen, n_src, idx, n_tab, n_epochs, n_steps, batch, S, d, order,
                                         flags, q, r, allow_const, n_params, 1e-2, 0.9, 0.999, 1e-8, w_z, w_x, 1e-3, w_sym, 1, 0.1, 2,
                                         epoch0, 1e-4, params, m, v, step, mask, xi, log, NULL)


def test_the_entry_is_additive_with_the_documented_signature(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert hasattr(lib, "symode_adam_epochs_latent") and hasattr(engine.HipEngine, "adam_epochs_latent")
    text = open(os.path.join(ROOT, "include", "symode.h")).read()
    assert re.search(r"#define SYMODE_ADAM_LOG_LATENT 10\b", text) and "train.py:491-508, 522-547" in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {name: re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1).split(",")
            for name in ("symode_adam_epochs", "symode_adam_epochs_latent")}
    words = {name: [" ".join(a.split()) for a in args] for name, args in decl.items()}
    plain, lat = words["symode_adam_epochs"], words["symode_adam_epochs_latent"]
    # the arguments of symode_adam_epochs with z, dz for x, dx, then B, y, e, D_obs, L, n_gen; w_z before w_x, w_sym after w_reg
    wx, wreg = plain.index("float w_x"), plain.index("float w_reg") + 1
    assert lat == (["const float* z", "const float* dz", "const float* B", "const float* y", "const float* e", "int D_obs", "const float* L",
                    "int n_gen"] + plain[2:wx] + ["float w_z"] + plain[wx:wreg] + ["float w_sym"] + plain[wreg:])
    res, args = engine._SIGNATURES["symode_adam_epochs_latent"]
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    assert res is ctypes.c_int and args == [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in lat]


def test_argument_errors_are_returned_before_any_launch(lib):
    assert _call(lib, d=7) == -1 and _call(lib, order=6) == -1 and _call(lib, flags=4) == -1      # no such library
    # what this entry refuses beyond symode_adam_epochs, all SYMODE_E_BADSIZE
    assert _call(lib, n_gen=-1) == -3
    assert _call(lib, w_z=0.0) == -3 and _call(lib, w_z=-1.0) == -3 and _call(lib, w_z=float("nan")) == -3
    assert _call(lib, n_gen=0, L=NULL, w_z=0.0) == -3                                             # with or without generators
    assert _call(lib, D_obs=1) == -3
    assert _call(lib, e=NULL) == -3                                                               # D_obs 4 > d 2 needs e
    assert _call(lib, L=NULL) == -3                                                               # n_gen 2 needs L
    # D_obs == d: e is not looked at; n_gen == 0: L is not looked at (the call fails on the NEXT thing that is wrong)
    assert _call(lib, D_obs=2, e=NULL, log=NULL) == -2 and _call(lib, D_obs=2, e=ODD, log=ODD) == -5
    assert _call(lib, n_gen=0, L=NULL, log=NULL) == -2 and _call(lib, n_gen=0, L=ODD, n_params=11) == -3
    assert _call(lib, e=ODD) == -5 and _call(lib, L=ODD) == -5
    assert _call(lib, w_x=0.0, w_sym=0.0, log=NULL) == -2                                         # any w_x, any w_sym
    # the checks of symode_adam_epochs hold here too
    assert _call(lib, n_tab=3) == -3 and _call(lib, n_tab=0) == -3 and _call(lib, n_tab=2, log=NULL) == -2
    assert _call(lib, n_epochs=-1) == -3 and _call(lib, S=-1) == -3 and _call(lib, n_src=0) == -3 and _call(lib, n_src=2 ** 31) == -3
    assert _call(lib, n_steps=0) == -3 and _call(lib, batch=0) == -3 and _call(lib, epoch0=-1) == -3 and _call(lib, n_params=11) == -3
    for name in ("z", "dz", "B", "y", "idx", "params", "m", "v", "step", "mask", "xi", "log"):
        assert _call(lib, **{name: NULL}) == -2, name
        assert _call(lib, **{name: ODD}) == -5, name
    empty = dict(z=NULL, dz=NULL, B=NULL, y=NULL, e=NULL, L=NULL, idx=NULL, params=NULL, m=NULL, v=NULL, step=NULL, mask=NULL, xi=NULL, log=NULL)
    assert _call(lib, n_epochs=0, **empty) == 0 and _call(lib, S=0, **empty) == 0                 # nothing to do
    assert _call(lib, n_epochs=0, n_gen=-1, **empty) == -3


class _FakeEngine:
    def lib_size(self, d, order, flags):
        return 6


def _device_adam(latent, n=10, d=2, **kw):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    return DeviceAdam(torch.zeros(n, d), torch.zeros(n, d), 2, False, False, CoefMap(d, 6), 1e-2, 0.5, 1e-3, 0.1, 2, 4,
                      engine=_FakeEngine(), latent=latent, **kw)


def test_DeviceAdam_checks_latent_against_x():
    from symode_amd import device_adam
    z = torch.zeros
    good = (z(10, 2, 2), z(10, 2), z(10), 4, z(3, 2, 2), 0.7, 0.1)
    tr = _device_adam(good)
    assert tr.latent[3] == 4 and tr.latent[5:] == (0.7, 0.1) and tr.log_columns == device_adam.LOG_COLUMNS_LATENT
    assert len(device_adam.LOG_COLUMNS_LATENT) == 10 and device_adam.LOG_COLUMNS_LATENT[:7] == device_adam.LOG_COLUMNS
    assert device_adam.LOG_COLUMNS_LATENT[7:9] == ("loss_sym_reg", "loss_sindy_z")
    assert _device_adam(None).latent is None and _device_adam(None).log_columns == device_adam.LOG_COLUMNS
    assert _device_adam((z(10, 2, 2), z(10, 2), None, 2, None, 0.7, 0.0)).latent[2] is None          # D_obs == d, no generators

    def bad(match, **over):
        t = dict(zip(("B", "y", "e", "D_obs", "L", "w_z", "w_sym"), good))
        t.update(over)
        with pytest.raises(ValueError, match=match):
            _device_adam(tuple(t.values()))

    bad("B must be", B=z(9, 2, 2))
    bad("B must be", B=z(10, 2))
    bad("y must be", y=z(10, 3))
    bad("e must be", e=z(10, 1))
    bad("e must be", e=None)                                                    # D_obs 4 > d 2
    bad("L must be", L=z(2, 2))                                                 # no generator axis
    bad("L must be", L=z(1, 3, 3))
    bad("fp32", B=z(10, 2, 2, dtype=torch.float64))
    bad("D_obs", D_obs=1)
    bad("w_sindy_z > 0", w_z=0.0)
    with pytest.raises(ValueError, match="reversed_sym and latent"):
        _device_adam(good, reversed_sym=(z(1, 10, 2), z(1, 10, 2, 2), 0.1))


class _Untouchable:
    """Stands in for every object train_SIGED must not look at before it has refused."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before refusing")


def _train_kwargs(**over):
    kw = dict(train_loader=_Untouchable(), test_loader=_Untouchable(), num_epochs=2, device="cuda:0", log_interval=1,
              save_interval=10 ** 9, save_dir="t", autoencoder=_Untouchable(), discriminator=_Untouchable(),
              generator=_Untouchable(), lr_ae=0, lr_d=0, lr_g=0, w_recon=0, w_gan=0, w_reg_norm=0, w_reg_ortho=0,
              w_reg_closure=0, use_original_x=False, gan_st_freq=0, gan_st_thres=0.0, ae_arch="none", regressor=_Untouchable(),
              use_latent=True, lr_sindy=1e-2, w_sindy_z=0.5, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=1e-3,
              w_sym_reg=0.1, sym_reg_type="no-such-kind", st_freq=2, threshold=0.05, int_t=0.1, int_dt=0.01, device_adam=True)
    kw.update(over)
    return kw


class _Loader:
    """A loader that is no DeviceBatches but shows its arrays."""

    def __init__(self, *shape):
        self.arrays = [torch.zeros(*shape), torch.zeros(*shape)]


def test_train_SIGED_device_adam_use_latent_checks_in_order():
    from symode_amd import train
    # 1. from the arguments alone: w_sindy_z > 0, and the message names use_latent
    for w in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="use_latent needs w_sindy_z > 0"):
            train.train_SIGED(**_train_kwargs(w_sindy_z=w))
    # 2. the autoencoder: frozen, and in eval mode where a layer reads the mode (the regressor, the loader and the generator
    # stay untouched)
    frozen, live = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    normed = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.BatchNorm1d(2))
    for q in list(frozen.parameters()) + list(normed.parameters()):
        q.requires_grad = False
    with pytest.raises(ValueError, match="frozen autoencoder in eval mode"):
        train.train_SIGED(**_train_kwargs(autoencoder=live.eval()))
    with pytest.raises(ValueError, match="frozen autoencoder in eval mode"):
        train.train_SIGED(**_train_kwargs(autoencoder=normed.train()))
    with pytest.raises(ValueError, match="DeviceBatches"):                       # in eval mode it passes on to the later checks
        train.train_SIGED(**_train_kwargs(autoencoder=normed.eval(), train_loader=_Loader(8, 2)))
    frozen.train()                                                              # no layer of it reads the mode
    # 3. one latent point per row, before the regulariser type and the loader's type are looked at
    with pytest.raises(ValueError, match="n_comps > 1"):
        train.train_SIGED(**_train_kwargs(autoencoder=frozen, train_loader=_Loader(8, 3, 2), sindy_reg_type="l2"))
    # 4. the regulariser type, 5. the loader
    with pytest.raises(ValueError, match="sindy_reg_type 'l1', not 'l2'"):
        train.train_SIGED(**_train_kwargs(autoencoder=frozen, train_loader=_Loader(8, 2), sindy_reg_type="l2"))
    with pytest.raises(ValueError, match="DeviceBatches"):
        train.train_SIGED(**_train_kwargs(autoencoder=frozen, train_loader=_Loader(8, 2)))
    # sym_reg_type was never read: every call above carried a kind that does not exist


def test_main_sweep_keeps_refusing_use_latent():
    from symode_amd.main_sweep import _refusal
    base = {"config": None, "sindy_optimizer": "adam", "use_latent": True, "w_sym_reg": 0.0, "load_laligan": "some-laligan",
            "fix_laligan": True, "sindy_reg_type": "l1", "eq_constraint": False, "sym_reg_type": "r"}
    assert "--use_latent" in _refusal(base)


def test_latent_operands_per_row_is_opt_in_and_sums_to_the_constant():
    from symode_amd.autoencoder import AutoEncoder
    from symode_amd.model_utils import latent_operands
    torch.manual_seed(3)
    ae = AutoEncoder(ae_arch="mlp", input_dim=4, latent_dim=2, hidden_dim=8, n_layers=2, n_comps=1, batch_norm=True, activation="ReLU").eval()
    x, dx = torch.randn(50, 4), torch.randn(50, 4)
    z, dz, B, y, e0, D = latent_operands(x, dx, ae, chunk=20)
    z2, dz2, B2, y2, e, D2 = latent_operands(x, dx, ae, chunk=20, per_row=True)
    assert isinstance(e0, float) and D == D2 == 4 and all(torch.equal(a, b) for a, b in ((z, z2), (dz, dz2), (B, B2), (y, y2)))
    assert e.shape == (50,) and e.dtype == x.dtype and bool((e >= 0).all()) and abs(float(e.double().sum()) - e0) <= 1e-5 * e0
    with pytest.raises(ValueError, match="eval mode"):
        latent_operands(x, dx, ae.train(), per_row=True)
