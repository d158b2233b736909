"""The epoch order of the device shuffle on its numpy twin alone (device_adam.epoch_order, the readable specification of
adam_order_row in csrc/adam_order.hpp): a permutation for every n, another one for every epoch and seed, a function of
(seed, epoch, n) and nothing else, and uniform in the sense a true shuffle is -- every (position, row) pair equally often
over many keys.  tests/test_gpu_adam_order.py holds the device function equal to this twin entry for entry."""
import math

import numpy as np
import pytest

from symode_amd.device_adam import ORDER_ROUNDS, epoch_order

SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 257, 1000, 1024, 1025, 125000]      # 2^k + 1: the walked domain is largest against n
SEEDS = [0, 1, 2, 2 ** 40 + 3]


@pytest.mark.parametrize("n", SIZES)
def test_the_order_is_a_permutation(n):
    for seed, epoch in ((0, 0), (1, 3), (2 ** 40 + 3, 7)) if n > 1000 else [(s, e) for s in SEEDS for e in (0, 1, 7)]:
        order = epoch_order(seed, epoch, n)
        assert order.dtype == np.int32 and order.shape == (n,)
        assert np.array_equal(np.sort(order), np.arange(n)), (n, seed, epoch)


def test_one_row_is_the_identity_and_the_range_of_n_is_checked():
    assert epoch_order(5, 3, 1).tolist() == [0]
    for n in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="n must be in"):
            epoch_order(0, 0, n)


@pytest.mark.parametrize("n", [64, 65, 1000])
def test_orders_differ_across_epochs_and_seeds(n):
    orders = {(s, e): epoch_order(s, e, n).tobytes() for s in SEEDS for e in range(8)}
    assert len(set(orders.values())) == len(orders)


def test_two_rows_take_both_orders():
    seen = {tuple(epoch_order(s, e, 2)) for s in range(4) for e in range(8)}
    assert seen == {(0, 1), (1, 0)}


def test_the_order_is_a_function_of_seed_epoch_and_n_alone():
    a = epoch_order(2 ** 40 + 3, 5, 1025)
    for s in SEEDS:                                        # other seeds and epochs drawn in between leave it alone
        epoch_order(s, 4, 1000)
    assert np.array_equal(a, epoch_order(2 ** 40 + 3, 5, 1025))
    assert np.array_equal(a, epoch_order(np.int64(2 ** 40 + 3), np.int32(5), np.int64(1025)))
    assert np.array_equal(epoch_order(-1, 0, 300), epoch_order(2 ** 64 - 1, 0, 300))      # seeds are taken modulo 2^64
    # a prefix is no shorter data set's order: n is part of the key's domain, not a cut
    assert not np.array_equal(epoch_order(1, 0, 1000)[:999], epoch_order(1, 0, 999))


def _chi_square(orders):
    """(position, row) counts of 16 384 orders of 16 rows against the flat expectation of 1024 per cell."""
    counts = np.zeros((16, 16))
    n = 0
    for order in orders:
        counts[np.arange(16), order] += 1
        n += 1
    assert n == 16384
    return float(((counts - 1024.0) ** 2 / 1024.0).sum())


def _chi2_quantile(df, z):
    """Wilson-Hilferty: the quantile of chi-square with df degrees of freedom at the normal quantile z."""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def test_position_row_pairs_are_uniform_over_the_keys():
    bound = _chi2_quantile(225, 3.0902323)                 # 99.9 %: rows and columns of the table are fixed, 15 x 15 free
    assert 295.0 < bound < 297.0, bound
    rng = np.random.default_rng(20261019)
    true_shuffle = _chi_square(rng.permutation(16) for _ in range(16384))
    twin = _chi_square(epoch_order(seed, epoch, 16) for seed in range(64) for epoch in range(256))
    print(f"chi-square over 16 x 16 (position, row) cells, 16 384 keys: twin {twin:.1f} at {ORDER_ROUNDS} rounds, "
          f"numpy permutation {true_shuffle:.1f}, bound {bound:.1f}")
    assert true_shuffle < bound                            # the bound is one a true shuffle meets
    assert twin < bound


def test_one_round_fewer_fails_the_uniformity_check():
    """ORDER_ROUNDS is the smallest count that passes: the network with one round fewer leaves half of the word in place."""
    bound = _chi2_quantile(225, 3.0902323)
    fewer = _chi_square(epoch_order(seed, epoch, 16, rounds=ORDER_ROUNDS - 1) for seed in range(64) for epoch in range(256))
    assert fewer > bound, fewer
