// Block-bootstrap replicas of Gram matrices (symode_gram_resample).  A Gram matrix is a sum over rows, so a bootstrap replica
// of a seed that resamples whole CHUNKS of its rows is an integer-weighted sum of the chunks' Gram matrices: one launch turns
// the (n_seeds, n_chunks, n, n) chunk matrices into (n_seeds * n_replicas, n, n) replica matrices, with no data pass and no
// index table.  Library independent (it reads matrices, not points), so only capi.hip includes this header.
// replaces: nothing in the reference (the block bootstrap of ensemble SINDy, restated on Gram matrices)
#pragma once
#include <hip/hip_runtime.h>

#include "adam_order.hpp"
#include "kernels.hpp"

namespace symode {

constexpr int RESAMPLE_MAX_CHUNKS = 1024;   // the counts of one replica live in LDS
constexpr int RESAMPLE_MAX_N = 68;          // p + d at its largest: 64 + 4
constexpr int RESAMPLE_THREADS = 256;

// The draw of replica b of a seed, stated once for the kernel (sweep.resample_counts is the same function in numpy integer
// arithmetic, constant for constant): the replica's two words are w = seed_words(seed_words(seed) + b) modulo 2^64, draw t of
// its C draws is u = subsample_key(low32(w), high32(w), t), and the chunk it lands on is (u * C) >> 32 -- below C for every
// 32-bit u, so it can index a C-entry array without a further check.
__device__ __forceinline__ unsigned long long resample_words(unsigned long long seed, int b) {
    return seed_words(seed_words(seed) + (unsigned long long)b);
}

__device__ __forceinline__ int resample_chunk(unsigned long long w, int t, int n_chunks) {
    const unsigned u = subsample_key((unsigned)w, (unsigned)(w >> 32), (unsigned)t);
    return (int)(((unsigned long long)u * (unsigned long long)n_chunks) >> 32);
}

// One workgroup per replica r = k * n_replicas + b.  The C draws are counted in LDS (the only place a drawn value is used as
// an index, and it is below C by construction); then thread i owns entries i, i + 256, ... of the n x n output and adds
// count[c] * chunk[k, c, entry] for c ascending, one multiply and one add per term (-ffp-contract=off), chunks that were not
// drawn skipped -- count[c] is the same for every thread, so that branch is uniform.  Every entry is computed by itself from
// its own inputs in the same order, so a symmetric input gives a symmetric output, and replica b of a seed does not depend on
// the launch it is part of.  Every global index is bounded by the sizes: no address depends on data.
__global__ __launch_bounds__(RESAMPLE_THREADS) void gram_resample_kernel(const double* __restrict__ chunk,
                                                                          const long long* __restrict__ seeds, int n_chunks, int n,
                                                                          int n_replicas, double* __restrict__ out,
                                                                          int* __restrict__ counts_out) {
    __shared__ int count[RESAMPLE_MAX_CHUNKS];
    const long r = blockIdx.x;
    const long k = r / n_replicas;
    const int b = (int)(r % n_replicas);
    for (int c = threadIdx.x; c < n_chunks; c += RESAMPLE_THREADS) count[c] = 0;
    __syncthreads();
    const unsigned long long w = resample_words((unsigned long long)seeds[k], b);
    for (int t = threadIdx.x; t < n_chunks; t += RESAMPLE_THREADS) atomicAdd(&count[resample_chunk(w, t, n_chunks)], 1);
    __syncthreads();
    if (counts_out)
        for (int c = threadIdx.x; c < n_chunks; c += RESAMPLE_THREADS) counts_out[r * n_chunks + c] = count[c];
    const int n2 = n * n;
    const double* src = chunk + k * (long)n_chunks * n2;
    for (int e = threadIdx.x; e < n2; e += RESAMPLE_THREADS) {
        double acc = 0.0;
        for (int c = 0; c < n_chunks; ++c) {
            const int m = count[c];
            if (m == 0) continue;
            acc = acc + (double)m * src[(long)c * n2 + e];
        }
        out[r * n2 + e] = acc;
    }
}

inline hipError_t launch_gram_resample(const double* chunk, const long long* seeds, long n_seeds, int n_chunks, int n, int n_replicas,
                                       double* out, int* counts_out, hipStream_t st) {
    gram_resample_kernel<<<dim3((unsigned)(n_seeds * n_replicas)), dim3(RESAMPLE_THREADS), 0, st>>>(chunk, seeds, n_chunks, n,
                                                                                                     n_replicas, out, counts_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
