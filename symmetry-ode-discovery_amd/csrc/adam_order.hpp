// The counter hashes the seed sweeps draw from (seed_words, subsample_key: subsample.hip's keys) and the epoch order of the
// device Adam trainer built on them: the row at position pos of epoch e's shuffle of range(n) as a FUNCTION of
// (seed, e, n, pos), so the epoch launch needs no index table.  A keyed bijection of [0, 2^bits), bits = ceil(log2 n) -- an
// alternating unbalanced Feistel network -- walked along its own cycle until it lands below n (the construction of
// thrust::shuffle).  device_adam.epoch_order is the same function in numpy integer arithmetic, constant for constant; the
// tests hold the two equal entry for entry.
// replaces: the per-epoch shuffle of DataLoader(train_dataset, batch_size, shuffle=True) (main.py:36-38 of the reference)
#pragma once
#include <hip/hip_runtime.h>

namespace symode {

// key(seed, row) = fmix32((row ^ a) * 0x9E3779B1 + b), (a, b) = the two halves of a 64-bit mix of the seed: three 32-bit
// multiplies per row (the subsample kernel recomputes every key in each of its four passes; a 64-bit mixer per row -- twelve
// quarter-rate multiplies -- made the hash most of its time: 103 us for 64 seeds of 10^5 rows).  Every step is a bijection
// of the 32-bit word, so for n <= 2^32 rows no two rows of a seed share a key.
__device__ __forceinline__ unsigned long long seed_words(unsigned long long seed) {
    unsigned long long z = seed * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ unsigned subsample_key(unsigned a, unsigned b, unsigned row) {
    unsigned h = (row ^ a) * 0x9E3779B1u + b;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// Feistel rounds of the epoch order: the smallest count at which the twin passes the uniformity check of
// tests/test_host_adam_order.py (profiles/adam_device_shuffle.txt has the statistic for every count tried)
constexpr int ADAM_ORDER_ROUNDS = 2;

// the round keys of one (seed, epoch): round r draws subsample_key at counter epoch * ROUNDS + r from the seed's two words.
// Uniform over the workgroup (seed and epoch are), so the multiplies are scalar ones, once per chunk.
struct AdamOrderKey {
    unsigned k[ADAM_ORDER_ROUNDS];
};

__device__ __forceinline__ AdamOrderKey adam_order_key(unsigned long long seed_w, int epoch) {
    AdamOrderKey key;
#pragma unroll
    for (int r = 0; r < ADAM_ORDER_ROUNDS; ++r)
        key.k[r] = subsample_key((unsigned)seed_w, (unsigned)(seed_w >> 32), (unsigned)epoch * ADAM_ORDER_ROUNDS + r);
    return key;
}

// the round function on a half of at most 16 bits: one 24-bit multiply (full rate, unlike the 32-bit one) spreads the half
// over the word, the key is added, and a shift-add-xor avalanche (no further multiply) brings every bit down to the low
// ones the caller keeps
__device__ __forceinline__ unsigned adam_order_mix(unsigned k, unsigned half) {
    unsigned h = k + __umul24(half + 1u, 0x9E3779u);
    h ^= h >> 15;
    h += h << 3;
    h ^= h >> 11;
    h += h << 7;
    h ^= h >> 13;
    h += h << 5;
    h ^= h >> 16;
    return h;
}

// the row at position pos (0 <= pos < n) of the permutation of [0, n), 1 <= n < 2^31.  n == 1 is the identity.  Otherwise the
// position is a word of bits = ceil(log2 n) bits, (hi | lo) with lo the low lb bits; a round is
//   (hi | lo) -> (lo | hi ^ F(k_r, lo))
// so lb alternates between bits - bits / 2 and bits / 2: each round is a bijection of [0, 2^bits) whatever F is, and
// 2^bits < 2 n.
// The walk ends: the rounds together are a permutation pi of [0, 2^bits), and pos, pi(pos), pi(pi(pos)), ... is the cycle of
// pos, which comes back to pos < n itself; the loop stops at the first member below n, after fewer than two rounds of pi in
// the mean and never more than 2^bits - n + 1.  Taking the first return to [0, n) of every start is a bijection of [0, n).
__device__ __forceinline__ int adam_order_row(const AdamOrderKey& key, int n, int pos) {
    if (n == 1) return 0;
    const int bits = 32 - __clz(n - 1), half = bits / 2;
    unsigned x = (unsigned)pos;
    do {
        int lb = bits - half;
#pragma unroll
        for (int r = 0; r < ADAM_ORDER_ROUNDS; ++r) {
            const int hb = bits - lb;
            const unsigned lo = x & ((1u << lb) - 1u), hi = x >> lb;
            x = (lo << hb) | ((hi ^ adam_order_mix(key.k[r], lo)) & ((1u << hb) - 1u));
            lb = hb;
        }
    } while (x >= (unsigned)n);
    return (int)x;
}

}  // namespace symode
