"""symode_adam_order_table -- the device function the keyed epoch launches compute their rows with, written out as a table --
against its numpy twin device_adam.epoch_order: exact equality, the pad -1 in the right places, for every size at which the
bit split or the cycle walk changes, batches that divide n, do not, and exceed it, shared and per-problem seeds, and a
continued epoch count."""
import numpy as np
import pytest
import torch

from symode_amd.device_adam import epoch_order

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 257, 1000, 1024, 1025]
SEEDS = [2 ** 40 + 3, 0, -7]
N_EPOCHS = 3


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd.get_engine()


_ORDERS = {}


def _order(seed, epoch, n):
    if (seed, epoch, n) not in _ORDERS:
        _ORDERS[seed, epoch, n] = epoch_order(seed, epoch, n)
    return _ORDERS[seed, epoch, n]


def _want(n, batch, seeds, epoch0, shuffle):
    steps = (n + batch - 1) // batch
    out = np.full((N_EPOCHS, len(seeds), steps * batch), -1, dtype=np.int32)
    for e in range(N_EPOCHS):
        for k, seed in enumerate(seeds):
            out[e, k, :n] = _order(seed, epoch0 + e, n) if shuffle else np.arange(n)
    return out.reshape(N_EPOCHS, len(seeds), steps, batch)


@pytest.mark.parametrize("n", SIZES)
def test_the_device_order_is_the_twins(eng, n):
    for batch in (1, 7, 256, 300, n + 5):
        for seeds in (SEEDS[:1], SEEDS):
            for epoch0 in (0, 5):
                for shuffle in (0, 1):
                    got = eng.adam_order_table(n, batch, seeds, N_EPOCHS, epoch0=epoch0, shuffle=shuffle).cpu().numpy()
                    want = _want(n, batch, seeds, epoch0, shuffle)
                    assert got.shape == want.shape and got.dtype == np.int32, (n, batch, got.shape, want.shape)
                    assert np.array_equal(got, want), (n, batch, len(seeds), epoch0, shuffle)


def test_the_sweeps_own_size(eng):
    n, batch = 125000, 256
    got = eng.adam_order_table(n, batch, SEEDS, N_EPOCHS, epoch0=5).cpu().numpy()
    assert np.array_equal(got, _want(n, batch, SEEDS, 5, 1))
    assert (got[:, :, -1, n % batch:] == -1).all() and (got.reshape(N_EPOCHS, 3, -1)[:, :, :n] >= 0).all()


def test_seeds_as_a_device_tensor_and_no_epochs(eng):
    seeds = torch.tensor([3, 4], dtype=torch.int64, device="cuda:0")
    got = eng.adam_order_table(65, 7, seeds, 1).cpu().numpy()
    assert np.array_equal(got.reshape(2, -1)[:, :65], np.stack([epoch_order(3, 0, 65), epoch_order(4, 0, 65)]))
    assert tuple(eng.adam_order_table(65, 7, seeds, 0).shape) == (0, 2, 10, 7)
