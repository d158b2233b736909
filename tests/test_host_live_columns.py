"""CoefMap.live_columns: which entries of Xi the constrained map can fill.  The rows of Q that belong to the entries the
rotation constraint keeps at zero are NOT zero (all but one carry the round-off of the SVD that made the basis), so the set
is decided by a threshold, 64 eps_fp32 max|Q|, which may only err towards calling an entry live."""
import numpy as np
import pytest
import torch

from symode_amd.coef_map import CoefMap
from symode_amd.constraint import constraint_Q

SO2 = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
# (order): p, the columns dead in both equation rows, dead (row, column) entries in all
DEAD = {3: (10, [0, 3, 4, 5], 8),
        4: (15, [0, 3, 4, 5, 10, 11, 12, 13, 14], 18),
        5: (21, [0, 3, 4, 5, 10, 11, 12, 13, 14], 18)}
EPS = float(np.finfo(np.float32).eps)


def _map(order, allow_constant):
    Q, use_kron = constraint_Q([SO2], 2, order)
    p = DEAD[order][0]
    assert Q.shape[0] == 2 * p
    return CoefMap(2, p, Q, use_kron, allow_constant)


@pytest.mark.parametrize("order", sorted(DEAD))
@pytest.mark.parametrize("allow_constant", [False, True])
def test_rotation_constraint_leaves_the_odd_degrees(order, allow_constant):
    p, dead_cols, n_dead = DEAD[order]
    cm = _map(order, allow_constant)
    live = cm.live_columns()
    assert live.shape == (2, p) and live.dtype == bool
    want_dead = [k for k in dead_cols if not (allow_constant and k == 0)]
    assert np.flatnonzero(~live.any(axis=0)).tolist() == want_dead
    # a dead column is dead in both rows, a live one live in both: the entries are the columns, twice
    assert (live[0] == live[1]).all()
    assert int((~live).sum()) == n_dead - (2 if allow_constant else 0)
    # what makes the threshold necessary and safe: the dead rows are not zero, and nowhere near the live ones
    rows = np.abs(cm.effective_Q()).max(axis=1).reshape(2, p)
    q_max = rows.max()
    structural = np.ones((2, p), dtype=bool)
    structural[:, dead_cols] = False
    assert np.count_nonzero(rows[~structural]) >= n_dead - 1
    assert rows[~structural].max() < 16.0 * EPS * q_max           # a quarter of the threshold
    assert rows[structural].min() > 0.1 * q_max
    # the mask the launches take: one bit per live column
    mask = cm.live_mask()
    assert [k for k in range(p) if not (mask >> k) & 1] == want_dead and mask >> p == 0


def test_order_5_with_the_constant_is_the_set_the_sparse_kernels_are_built_for():
    assert _map(5, True).live_mask() == sum(1 << k for k in [0, 1, 2, 6, 7, 8, 9, 15, 16, 17, 18, 19, 20]) == 0x1F83C7
    assert _map(4, True).live_mask() == sum(1 << k for k in [0, 1, 2, 6, 7, 8, 9]) == 0x3C7


def test_without_a_constraint_everything_is_live():
    for allow_constant in (False, True):
        cm = CoefMap(2, 21, None, True, allow_constant)
        assert cm.live_columns().all() and cm.live_columns().shape == (2, 21)
        assert cm.live_mask() == 0xFFFFFFFFFFFFFFFF
    # nothing dead under a constraint, or more columns than the mask has bits: all ones as well
    full = CoefMap(2, 3, torch.eye(6), True, False)
    assert full.live_columns().all() and full.live_mask() == 0xFFFFFFFFFFFFFFFF
    wide = CoefMap(1, 70, torch.eye(70)[:, :5], True, False)
    assert not wide.live_columns().all() and wide.live_mask() == 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("use_kron", [True, False])
def test_a_row_between_the_threshold_and_the_live_range_counts_as_live(use_kron):
    d, p = 2, 6
    Q = torch.zeros(d * p, 3)
    Q[0, 0], Q[1, 1] = 0.5, -0.4                       # live
    thr = 64.0 * EPS * 0.5
    Q[2, 2] = 2.0 * thr                                # in between: four orders under the live rows, above the threshold
    Q[3, 0] = 0.5 * thr                                # round-off: dead
    Q[4, 1] = -0.9 * thr                               # still under it: dead
    Q[5, 2] = 1.0e-3                                   # small but far above: live
    cm = CoefMap(d, p, Q, use_kron, False)
    flat = np.zeros(d * p, dtype=bool)
    flat[[0, 1, 2, 5]] = True
    # rows of Q are in Xi's (d, p) order on the Kronecker branch, in (p, d) order on the transposed one
    want = flat.reshape(d, p) if use_kron else flat.reshape(p, d).T
    assert (cm.live_columns() == want).all()
    # a column is live if any of its rows is; the constant column joins when the model reads const
    cols = want.any(axis=0)
    assert cm.live_mask() == sum(1 << k for k in np.flatnonzero(cols).tolist())
    with_const = CoefMap(d, p, Q, use_kron, True).live_columns()
    assert with_const[:, 0].all() and (with_const[:, 1:] == want[:, 1:]).all()
