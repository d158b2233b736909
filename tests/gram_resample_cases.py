"""The deck of tests/test_gpu_gram_resample.py, with no GPU in it: (n, C, B, S) and the inputs of a case.

n takes 1, 3, 12, 23, 68 (the entry's smallest and largest; 12 = p + d of the flagship; 23 x 23 = 529 entries is no multiple of
the 256 threads; 68 x 68 = 4624 entries is 19 strides of the workgroup), C takes 1, 2, 7, 128, 1024 (one chunk: the replica IS
the chunk; 1024: four strides of the count loops and the whole LDS array), B takes 1, 3, 33 and S takes 1, 3.  Every value of
each axis appears, every axis's extremes meet the extremes of the others, and the cases stay small: the largest input is
1024 x 68 x 68 fp64 = 38 MB, the largest model sum 99 replicas."""
import functools

import numpy as np

# (n, C, B, S)
DECK = (
    (1, 1, 1, 1),
    (1, 1024, 33, 3),
    (3, 2, 3, 3),
    (3, 1024, 1, 1),
    (12, 7, 33, 3),
    (12, 128, 33, 3),        # the flagship's n and C
    (23, 128, 3, 1),
    (23, 1024, 3, 3),
    (23, 7, 1, 3),
    (68, 1, 3, 1),
    (68, 2, 33, 1),
    (68, 128, 3, 3),
    (68, 1024, 1, 1),
)
IDS = ["n%d_C%d_B%d_S%d" % c for c in DECK]


def seeds_of(case):
    """S seeds per case: a small one, the sweeps' 1_000_003 * s form, and one with the top bit set (negative as int64)"""
    n, C, B, S = case
    return [7, 1_000_003 * (n + C), -(2 ** 63) + 12345 * B + n][:S]


@functools.lru_cache(maxsize=None)
def chunks(case):
    """(S, C, n, n) fp64, every matrix symmetric to the bit: (R + R^T) scaled by s_i s_j with s spread over 12 decades (even
    cases), or plain (R + R^T) (odd cases)."""
    n, C, B, S = case
    rng = np.random.RandomState(DECK.index(case) + 1)
    R = rng.randn(S, C, n, n)
    M = R + R.transpose(0, 1, 3, 2)
    if DECK.index(case) % 2 == 0:
        s = 10.0 ** rng.uniform(-3.0, 3.0, size=(S, C, n))
        M = M * (s[..., :, None] * s[..., None, :])
    assert np.array_equal(M, M.transpose(0, 1, 3, 2))
    return np.ascontiguousarray(M)
