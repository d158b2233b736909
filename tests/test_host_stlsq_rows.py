"""Why one wave per equation row is the host's loop: the per-row statement of the device kernel (tests/stlsq_cases.py,
``row_solve`` / ``per_row_sweep``: csrc/stlsq.hpp in numpy fp64, statement by statement) against symode_host_stlsq_sweep with
driver 1, which solves a masked pass as ONE block-diagonal system over the rows.  Under the full-rank driver the blocks never
mix, so the two agree bit for bit -- on the inputs of the GPU test, without a GPU."""
import numpy as np
import pytest

from tests import stlsq_cases as C

CASES = [((2, 3, 0), 0.0, 10), ((2, 3, 0), 0.1, 2), ((2, 5, 0), 0.1, 10), ((3, 2, C.FLAG_EXP), 0.0, 10), ((3, 2, C.FLAG_EXP), 0.1, 10),
         ((1, 1, 0), 0.0, 10), ((3, 4, C.FLAG_SINE | C.FLAG_EXP), 0.1, 10)]


@pytest.mark.parametrize("shape, gamma, max_iter", CASES, ids=lambda v: "d%d_o%d_f%d" % v if isinstance(v, tuple) else str(v))
def test_rows_solved_alone_equal_the_joint_system(shape, gamma, max_iter):
    G = C.gram_cpu(shape)
    host = C.host_sweep(G, shape[0], gamma, C.THRESHOLD, max_iter)
    rows = C.per_row_sweep(G, shape[0], gamma, C.THRESHOLD, max_iter)
    assert np.array_equal(rows[0].view(np.int32), host[0].view(np.int32))            # fp32 coefficients, bit for bit
    assert np.array_equal(rows[1], host[1]) and np.array_equal(rows[2], host[2]) and np.array_equal(rows[3], host[3])
    assert not rows[4].any() and not host[4].any()
    if max_iter == 10 and shape[0] > 1:
        assert (host[2] >= 2).any() and not host[1].all()                           # masked passes ran: the joint system was used


def test_a_pivot_that_is_not_positive_ends_the_problem():
    A = np.array([[4.0, 0.0, 2.0], [0.0, 0.0, 0.0], [2.0, 0.0, 3.0]])
    assert C.row_solve(A, np.ones(3)) is None
    assert np.allclose(C.row_solve(A[np.ix_([0, 2], [0, 2])], np.ones(2)), np.linalg.solve(A[np.ix_([0, 2], [0, 2])], np.ones(2)))
    G = np.zeros((1, 4, 4))
    G[0, :3, :3], G[0, :3, 3] = A, 1.0
    assert C.per_row_sweep(G, 1, 0.0, 0.1, 10)[4].tolist() == [1]
    assert C.per_row_sweep(G, 1, 0.5, 0.1, 10)[4].tolist() == [0]                     # a ridge makes it regular
