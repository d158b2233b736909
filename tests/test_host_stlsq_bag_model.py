"""The numpy side of the bagged STLSQ fit, on the CPU: the host twin (sindy.stlsq_bag_from_gram) against the model of the entry
(tests/stlsq_bag_model.py: dense solves), the twin of the draw (sweep.resample_counts) against the model of the resample entry
(tests/gram_resample_model.py), the uniformity of the draw, and the block-bootstrap identity the design rests on: the chunk
matrices of a seed add up to the Gram matrix of its first C L rows."""
import math
import warnings

import numpy as np
import pytest

from symode_amd.sindy import stlsq_bag_from_gram, stlsq_bag_statistics
from symode_amd.sweep import resample_counts, resample_grams
from tests import gram_resample_cases as RC
from tests import gram_resample_model as RM
from tests import stlsq_bag_model as M


@pytest.mark.parametrize("size", ((3, 2, 1, 5, 0), (3, 2, 10, 5, 1), (2, 1, 64, 4, 0), (2, 4, 64, 3, 1), (3, 3, 23, 33, 2)),
                         ids=lambda s: "S%d_d%d_p%d_B%d_f%d" % s)
def test_the_twin_equals_the_model(size):
    S, d, p, B, n_fell = size
    gamma = 0.1
    G, _ = M.random_grams(S, d, p, seed=p)
    assert max(np.linalg.cond(G[k, :p, :p] + gamma * gamma * np.eye(p)) for k in range(S)) <= M.COND_BOUND
    rxi, rmask, rfell = M.random_replicas(S, B, d, p, seed=p, n_fell=n_fell)
    tau = [t for t in (0, 500, 600, 1000) for _ in range(S)]
    want = M.bag(G, rxi, rmask, rfell, tau, gamma)
    for s, t in enumerate(tau):
        k = s % S
        rows = slice(k * B, (k + 1) * B)
        xi, mask, rec = stlsq_bag_from_gram(G[k], rxi[rows], rmask[rows], rfell[rows], t, gamma, d)
        assert xi.dtype == np.float32 and mask.dtype == bool
        assert np.array_equal(mask, want["mask"][s] != 0)
        assert np.array_equal(rec["count"], want["count"][k]) and rec["valid"] == want["valid"][k] == B - n_fell
        # the same fp64 operations in the same order: numpy arrays against Python floats
        assert rec["mean"].tobytes() == want["mean"][k].tobytes() and rec["std"].tobytes() == want["std"][k].tobytes()
        assert (np.abs(xi.astype(np.float64) - want["xi"][s]) <= M.row_bound(want["xi"][s])).all()
        assert not xi[~mask].any()


def test_the_statistics_by_hand():
    xi = np.array([[[1.0, 5.0]], [[2.0, 7.0]], [[100.0, 100.0]], [[6.0, 9.0]]], dtype=np.float32)
    mask = np.array([[[1, 1]], [[1, 0]], [[1, 1]], [[1, 0]]], dtype=np.uint8)
    count, valid, mean, std = stlsq_bag_statistics(xi, mask, np.array([0, 0, 1, 0]))
    assert valid == 3 and count.tolist() == [[3, 1]]
    assert mean.tolist() == [[3.0, 5.0]] and std[0, 1] == 0.0 and std[0, 0] == math.sqrt(14.0 / 3.0)
    count, valid, mean, std = stlsq_bag_statistics(xi, mask, np.ones(4, dtype=np.int32))
    assert valid == 0 and not count.any() and not mean.any() and not std.any()
    # the inclusion rule at the edge: 2 of 3 is 666.67 thousandths
    G, _ = M.random_grams(1, 1, 2)
    mask2 = np.array([[[1, 1]], [[1, 1]], [[1, 0]]], dtype=np.uint8)
    for tau, kept in ((666, [True, True]), (667, [True, False]), (0, [True, True]), (1000, [True, False])):
        assert stlsq_bag_from_gram(G[0], xi[:3], mask2, np.zeros(3), tau, 0.0, 1)[1].tolist() == [kept], tau
    for bad in (-1, 1001):
        with pytest.raises(ValueError, match="0 .. 1000"):
            stlsq_bag_from_gram(G[0], xi[:3], mask2, np.zeros(3), bad, 0.0, 1)


def test_a_singular_support_takes_the_minimum_norm_fallback():
    from symode_amd import lstsq
    rng = np.random.RandomState(5)
    A = rng.randint(-3, 4, size=(40, 8)).astype(np.float64)
    A[:, 0], A[:, 2] = 1.0, 0.0
    G = A.T @ A
    full = np.ones((1, 2, 6), dtype=np.uint8)
    lstsq._warned_singular = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        xi, mask, _ = stlsq_bag_from_gram(G, np.ones((1, 2, 6), dtype=np.float32), full, np.zeros(1), 1000, 0.0, 2)
    assert [w for w in rec if w.category is RuntimeWarning and "minimum-norm solution" in str(w.message)]
    assert mask.all() and not xi[:, 2].any() and np.isfinite(xi).all() and xi.any()
    less = full.copy()
    less[0, :, 2] = 0
    xi2 = stlsq_bag_from_gram(G, np.ones((1, 2, 6), dtype=np.float32), less, np.zeros(1), 1000, 0.0, 2)[0]
    assert (np.abs(xi.astype(np.float64) - xi2) <= 4 * M.row_bound(xi2)).all()       # the minimum-norm answer IS the fit without it


def test_the_twin_of_the_draw():
    for C in (1, 2, 7, 128, 1024):
        for seed in (0, 7, 1_000_003 * 5, 2 ** 63 + 11, -3):
            for b in (0, 1, 32):
                c = resample_counts(seed, b, C)
                assert c.dtype == np.int32 and c.shape == (C,) and c.sum() == C and c.min() >= 0          # every row sums to C
                assert np.array_equal(c, RM.counts(seed, b, C)), (C, seed, b)
    assert resample_counts(7, 0, 1).tolist() == [1]
    assert not np.array_equal(resample_counts(7, 0, 128), resample_counts(7, 1, 128))
    assert not np.array_equal(resample_counts(7, 0, 128), resample_counts(8, 0, 128))
    case = RC.DECK[4]
    out, counts = resample_grams(RC.chunks(case), RC.seeds_of(case), case[2])
    want, want_counts = RM.resample(RC.chunks(case), RC.seeds_of(case), case[2])
    assert out.tobytes() == want.tobytes() and counts.tobytes() == want_counts.tobytes()


def _chi2_upper(df, z):
    """Wilson-Hilferty: the chi-square quantile at the normal quantile z"""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def test_the_draw_is_uniform_over_the_chunks():
    """Chi-square of the chunk totals over many (seed, b) against the uniform law, at significance 1e-6 two-sided (|z| <
    4.89): the draws are fixed numbers, so the test cannot flicker; it fails when the hash or the scaling is broken (a chunk
    never drawn, the last chunk short).  C = 128 with 64 seeds x 32 replicas (262 144 draws, 2048 expected per chunk) and C = 7
    with 64 x 8 (3584 draws, 512 expected)."""
    z = 4.89
    for C, S, B in ((128, 64, 32), (7, 64, 8)):
        total = np.zeros(C, dtype=np.int64)
        for k in range(S):
            for b in range(B):
                total += RM.counts(1_000_003 * k, b, C)
        expect = S * B * C / C
        chi2 = float(((total - expect) ** 2 / expect).sum())
        lo, hi = _chi2_upper(C - 1, -z), _chi2_upper(C - 1, z)
        print("C", C, "chi2 %.1f" % chi2, "df", C - 1, "accept (%.1f, %.1f)" % (lo, hi))
        assert lo < chi2 < hi, (C, chi2)
        assert total.min() > 0
    # and within a replica the counts are those of C independent draws: the share of chunks never drawn tends to 1/e
    empty = np.mean([np.mean(RM.counts(1_000_003 * k, b, 1024) == 0) for k in range(16) for b in range(4)])
    assert abs(empty - math.exp(-1.0)) < 4.89 * math.sqrt(math.exp(-1.0) * (1 - math.exp(-1.0)) / (64 * 1024))


def test_the_chunk_matrices_add_up_to_the_gram_of_their_rows():
    """A Gram matrix is a sum over rows: the C chunk matrices of L rows each add up to the matrix of the first C L rows within
    the rounding of the two summation orders, |sum_c G_c - G| <= (C L) 2^-52 sum |a_i a_j| entrywise (each side is a sum of C L
    products, its error at most (C L - 1) u times the sum of their magnitudes), and a replica with every count 1 is that sum."""
    rng = np.random.RandomState(2)
    m, C, n = 403, 8, 12
    L = m // C
    a = rng.randn(m, n) * 10.0 ** rng.uniform(-2, 2, size=n)
    chunk = np.stack([a[c * L:(c + 1) * L].T @ a[c * L:(c + 1) * L] for c in range(C)])
    G = a[:C * L].T @ a[:C * L]
    bound = C * L * 2.0 ** -52 * (np.abs(a[:C * L]).T @ np.abs(a[:C * L]))
    assert (np.abs(chunk.sum(axis=0) - G) <= bound).all()
    assert m - C * L == 3 and m - C * L < C                                           # fewer than C rows are in no chunk
    out, counts = resample_grams(chunk[None], [7], 40)
    assert (counts.sum(axis=1) == C).all()
    acc = np.zeros((n, n))
    for c in range(C):
        acc = acc + 1.0 * chunk[c]
    b = int(np.argmax((counts > 0).sum(axis=1)))
    want = np.zeros((n, n))
    for c in range(C):
        if counts[b, c]:
            want = want + float(counts[b, c]) * chunk[c]
    assert out[b].tobytes() == want.tobytes() and np.array_equal(out[b], out[b].T)
    assert (np.abs(acc - G) <= bound).all()
