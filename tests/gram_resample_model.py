"""numpy model of ``symode_gram_resample``, written from the formula include/symode.h documents at that entry, not from the
kernel, and knowing nothing of workgroups or LDS: the draw in uint64 / uint32 array arithmetic (which wraps as the words of the
device do), the sum entry by entry in fp64 -- numpy neither contracts a multiply-add nor reorders a sum it is handed term by
term, so the device's bytes are the model's bytes."""
import numpy as np

_U64, _U32 = np.uint64, np.uint32


def _seed_words(z):
    """the 64-bit mix of csrc/adam_order.hpp on a uint64 array"""
    z = z * _U64(0x9E3779B97F4A7C15) + _U64(0x632BE59BD9B4E019)
    z = z ^ (z >> _U64(30))
    z = z * _U64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> _U64(27))
    z = z * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def _subsample_key(a, b, row):
    """fmix32((row ^ a) * 0x9E3779B1 + b) on uint32 arrays"""
    h = (row ^ a) * _U32(0x9E3779B1) + b
    h = h ^ (h >> _U32(16))
    h = h * _U32(0x85EBCA6B)
    h = h ^ (h >> _U32(13))
    h = h * _U32(0xC2B2AE35)
    return h ^ (h >> _U32(16))


def counts(seed, b, n_chunks):
    """(C,) int32: how often each chunk is drawn for replica ``b`` of ``seed``"""
    with np.errstate(over="ignore"):
        w = _seed_words(_seed_words(np.array([int(seed) & (2 ** 64 - 1)], dtype=_U64)) + _U64(b))
        lo, hi = (w & _U64(0xFFFFFFFF)).astype(_U32), (w >> _U64(32)).astype(_U32)
        u = _subsample_key(lo, hi, np.arange(n_chunks, dtype=_U32))
    where = (u.astype(_U64) * _U64(n_chunks)) >> _U64(32)
    assert where.max() < n_chunks
    return np.bincount(where.astype(np.int64), minlength=n_chunks).astype(np.int32)


def resample(chunk, seeds, n_replicas):
    """chunk (S, C, n, n) fp64, seeds (S,) -> (out (S B, n, n) fp64, counts (S B, C) int32)"""
    S, C = chunk.shape[:2]
    out = np.zeros((S * n_replicas,) + chunk.shape[2:])
    cnt = np.zeros((S * n_replicas, C), dtype=np.int32)
    for k in range(S):
        for b in range(n_replicas):
            r = k * n_replicas + b
            cnt[r] = counts(seeds[k], b, C)
            acc = np.zeros(chunk.shape[2:])
            for c in range(C):
                if cnt[r, c]:
                    acc = acc + np.float64(cnt[r, c]) * chunk[k, c]
            out[r] = acc
    return out, cnt
