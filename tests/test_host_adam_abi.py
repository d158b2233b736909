"""CPU-side checks of the device Adam trainer's surface: symode_adam_epochs is an additive entry (it came with the ABI version of the
L-BFGS trainer descriptor, 7) whose argument validation returns error codes before any launch, main_sweep accepts the plain
Adam configuration and keeps its other refusals, train_SIGED(device_adam=True) refuses what it does not cover without
touching a device, and DeviceBatches.epoch_order() is the permutation __iter__ draws."""
import ctypes
import os

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


def _call(lib, x=JUNK, dx=JUNK, n_src=300, idx=JUNK, n_tab=1, n_epochs=3, n_steps=4, batch=77, S=2, d=2, order=2, flags=0,
          q=NULL, r=0, allow_const=1, n_params=12, params=JUNK, m=JUNK, v=JUNK, step=JUNK, mask=JUNK, xi=JUNK, log=JUNK,
          epoch0=0):
    return lib.symode_adam_epochs(x, dx, n_src, idx, n_tab, n_epochs, n_steps, batch, S, d, order, flags, q, r, allow_const,
                                  n_params, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1e-3, 1, 0.1, 2, epoch0, 1e-4, params, m, v, step, mask,
                                  xi, log, NULL)


def test_the_entry_is_additive_abi_version_is_the_bindings(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert "symode_adam_epochs" in engine._SIGNATURES and hasattr(lib, "symode_adam_epochs")
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    assert "int symode_adam_epochs(" in header and "torch.optim.Adam.step" in header
    assert hasattr(engine.HipEngine, "adam_epochs")


def test_argument_validation_needs_no_gpu(lib):
    assert _call(lib, d=7) == -1 and _call(lib, order=6) == -1 and _call(lib, flags=4) == -1      # no such library
    assert _call(lib, n_tab=3) == -3 and _call(lib, n_tab=0) == -3                                # tables: 1 or S
    assert _call(lib, n_tab=2, log=NULL) == -2                                                    # (sizes accepted)
    assert _call(lib, n_epochs=-1) == -3 and _call(lib, S=-1) == -3
    assert _call(lib, n_src=0) == -3 and _call(lib, n_src=2 ** 31) == -3                          # rows are int32
    assert _call(lib, n_steps=0) == -3 and _call(lib, batch=0) == -3 and _call(lib, epoch0=-1) == -3
    assert _call(lib, n_params=11) == -3                                                          # d p = 12 without a constraint
    assert _call(lib, q=JUNK, r=3, n_params=12) == -3 and _call(lib, q=JUNK, r=0, n_params=2) == -3   # r + d with one
    assert _call(lib, d=3, order=4, flags=0, n_params=105, log=NULL) == -2
    for name in ("x", "dx", "idx", "params", "m", "v", "step", "mask", "xi", "log"):
        assert _call(lib, **{name: NULL}) == -2, name
        assert _call(lib, **{name: ODD}) == -5, name
    assert _call(lib, q=ODD, r=3, n_params=5) == -5
    # nothing to do: no pointer is looked at
    empty = dict(x=NULL, dx=NULL, idx=NULL, params=NULL, m=NULL, v=NULL, step=NULL, mask=NULL, xi=NULL, log=NULL)
    assert _call(lib, n_epochs=0, **empty) == 0 and _call(lib, S=0, **empty) == 0
    assert _call(lib, d=7, n_epochs=0, **empty) == -1                                             # ... but the library is


def test_engine_adam_epochs_refuses_cpu_tensors():
    import symode_amd
    eng = symode_amd.get_engine()
    z = torch.zeros
    with pytest.raises(symode_amd.SymodeError, match="x must be a CUDA/HIP tensor"):
        eng.adam_epochs(z(10, 2), z(10, 2), z(1, 1, 1, 10, dtype=torch.int32), z(1, 12), z(1, 12), z(1, 12),
                        z(1, dtype=torch.int32), z(1, 2, 6), 2, lr=1e-2)


def _sweep_args(**over):
    a = {"config": None, "sindy_optimizer": "adam", "use_latent": False, "w_sym_reg": 0.0, "sym_reg_type": "i",
         "load_laligan": None, "fix_laligan": False, "sindy_reg_type": "l1", "eq_constraint": False}
    a.update(over)
    return a


def test_main_sweep_accepts_plain_adam_and_keeps_its_refusals():
    from symode_amd.main_sweep import _refusal
    assert _refusal(_sweep_args()) is None
    assert _refusal(_sweep_args(eq_constraint=True)) is None
    assert _refusal(_sweep_args(sindy_optimizer="lbfgs")) is None
    why = _refusal(_sweep_args(use_latent=True))
    assert why is not None and "--use_latent" in why and "symode_amd.main --seed $i" in why
    why = _refusal(_sweep_args(w_sym_reg=0.1, sym_reg_type="r", load_laligan="x", fix_laligan=True))
    assert why is not None and "symmetry regulariser" in why and "symode_amd.main --seed $i" in why
    assert _refusal(_sweep_args(sindy_optimizer="sgd")) is not None
    # --method stlsq has no optimiser: it keeps asking for --sindy_optimizer lbfgs, as before
    assert "--sindy_optimizer lbfgs" in _refusal(_sweep_args(), "stlsq") and _refusal(_sweep_args(sindy_optimizer="lbfgs"), "stlsq") is None
    # the L-BFGS refusals are as they were
    assert "--sym_reg_type r" in _refusal(_sweep_args(sindy_optimizer="lbfgs", w_sym_reg=0.1, sym_reg_type="f", load_laligan="x"))


def test_main_sweep_refuses_adam_on_several_ranks(monkeypatch):
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit, match="--seed <first> --n_seeds <count>"):
        main_sweep.main(["--task", "dosc", "--sindy_optimizer", "adam", "--n_seeds", "2"])


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
              w_sym_reg=0.0, st_freq=2, threshold=0.05, int_t=0.1, int_dt=0.01, device_adam=True)
    kw.update(over)
    return kw


def test_train_SIGED_device_adam_names_the_condition_it_refuses():
    from symode_amd import train
    with pytest.raises(ValueError, match="use_latent"):
        train.train_SIGED(**_train_kwargs(use_latent=True))
    with pytest.raises(ValueError, match="w_sym_reg"):
        train.train_SIGED(**_train_kwargs(w_sym_reg=0.1))
    with pytest.raises(ValueError, match="sindy_reg_type"):
        train.train_SIGED(**_train_kwargs(sindy_reg_type="l2"))
    with pytest.raises(ValueError, match="DeviceBatches"):
        train.train_SIGED(**_train_kwargs(train_loader=[(torch.zeros(4, 2), torch.zeros(4, 2))]))
    from symode_amd.dataset import DeviceBatches
    windows = DeviceBatches([torch.zeros(12, 2), torch.zeros(12, 2)], 10, 4, True, "cpu", window=3)
    with pytest.raises(ValueError, match="window"):
        train.train_SIGED(**_train_kwargs(train_loader=windows))


def test_the_parser_has_the_flag_and_it_is_off_by_default():
    from symode_amd.parser_utils import get_args
    assert get_args(argv=[]).device_adam is False
    assert get_args(argv=["--device_adam"]).device_adam is True


@pytest.mark.parametrize("n, bs, shuffle", [(10, 4, True), (12, 4, True), (7, 16, True), (9, 2, False)])
def test_epoch_order_is_the_permutation_iter_draws(n, bs, shuffle):
    from symode_amd.dataset import DeviceBatches
    a, b = torch.arange(n * 2, dtype=torch.float32).view(n, 2), -torch.arange(n * 3, dtype=torch.float32).view(n, 3)
    loader = DeviceBatches([a, b], n, bs, shuffle, "cpu")
    torch.manual_seed(5)
    first, second = list(loader), list(loader)
    after = torch.rand(3)
    torch.manual_seed(5)
    for batches in (first, second):                        # two epochs: the generator advances as two passes do
        order = loader.epoch_order()
        assert order.shape == (n,) and sorted(order.tolist()) == list(range(n))
        assert len(batches) == len(loader)
        for k, (xa, xb) in enumerate(batches):
            rows = order[k * bs:(k + 1) * bs]
            assert torch.equal(xa, a[rows]) and torch.equal(xb, b[rows])
    assert torch.equal(torch.rand(3), after)
