// Bagging of the device STLSQ sweep (symode_stlsq_bag): the replica fits of a seed (symode_stlsq_sweep on the matrices of
// symode_gram_resample) are counted term by term, the terms that survive in enough replicas are kept, and the model is refit
// on that support from the seed's OWN matrix -- the aggregation and refit of ensemble SINDy, one launch for all seeds and all
// inclusion levels.  Geometry, LDS and the solve are stlsq_sweep_kernel's; only capi.hip includes this header.
// replaces: nothing in the reference
#pragma once
#include <hip/hip_runtime.h>

#include "stlsq.hpp"

namespace symode {

constexpr int STLSQ_BAG_TAU_MAX = 1000;     // the inclusion level in thousandths

// One workgroup per problem s, one wave per equation row j, lane k of the wave owns library column k.  Problem s works on
// seed ks = s % n_seeds at the inclusion level tau[s] (TABLE) or the launch-wide one: a grid of levels is more problems on
// the same replica outputs.
//   statistics  over replicas b ascending of seed ks (rows ks * n_replicas + b of rep_xi, rep_mask, rep_fell), a replica with
//               rep_fell set left out: valid = the replicas that remain, count = those of them that keep the term, and over
//               those, in fp64, sum, mean = sum / count, ss = sum of (x - mean)^2 in a second pass, std = sqrt(ss / count);
//               count == 0: mean = std = 0.  rep_fell is read by every lane at the same index, so that branch is uniform.
//   inclusion   keep the term iff valid > 0 and 1000 count >= tau valid, in 64-bit integers: exact on both sides.
//   refit       stlsq_row_solve on the seed's own matrix (set ks of aug) on the kept support with ridge gamma, rounded to fp32;
//               an empty row is zeros; a pivot that is not positive sets fell_out[s] and leaves that row zeros.
// Problems s < n_seeds also write the seed's statistics (they do not depend on the level).  Every LDS and global index is
// bounded by the sizes: no address depends on data.
template <bool TABLE>
__global__ __launch_bounds__(WAVE * STLSQ_MAX_D) void stlsq_bag_kernel(const double* __restrict__ aug, int n_seeds, int d, int p,
                                                                        int n_replicas, const float* __restrict__ rep_xi,
                                                                        const unsigned char* __restrict__ rep_mask,
                                                                        const int* __restrict__ rep_fell,
                                                                        const int* __restrict__ tau_table, int tau_milli, double gamma,
                                                                        float* __restrict__ xi_out, unsigned char* __restrict__ mask_out,
                                                                        int* __restrict__ fell_out, int* __restrict__ count_out,
                                                                        int* __restrict__ valid_out, double* __restrict__ mean_out,
                                                                        double* __restrict__ std_out) {
    extern __shared__ double stlsq_bag_smem[];
    const int lane = threadIdx.x % WAVE;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long s = blockIdx.x;
    const long ks = s % n_seeds;
    const int F = p + d;
    double* A = stlsq_bag_smem + (size_t)j * ((size_t)p * p + p);
    double* xrow = A + (size_t)p * p;
    int* ints = (int*)(stlsq_bag_smem + (size_t)d * ((size_t)p * p + p));
    int* sel = ints + j * p;
    int* f_bad = ints + d * p;
    if constexpr (TABLE) tau_milli = tau_table[s];
    const double* G = aug + ks * (long)F * F;
    const bool col = lane < p;
    const long row0 = ks * n_replicas;                       // the seed's first replica
    const long at = (long)j * p + (col ? lane : 0);          // this lane's entry of a replica's (d, p) outputs
    const long dp = (long)d * p;

    int valid = 0, count = 0;
    double sum = 0.0;
    for (int b = 0; b < n_replicas; ++b) {
        if (rep_fell[row0 + b] != 0) continue;
        ++valid;
        if (col && rep_mask[(row0 + b) * dp + at] != 0) {
            ++count;
            sum = sum + (double)rep_xi[(row0 + b) * dp + at];
        }
    }
    const double mean = count > 0 ? sum / (double)count : 0.0;
    double ss = 0.0;
    for (int b = 0; b < n_replicas; ++b) {
        if (rep_fell[row0 + b] != 0) continue;
        if (col && rep_mask[(row0 + b) * dp + at] != 0) {
            const double dev = (double)rep_xi[(row0 + b) * dp + at] - mean;
            ss = ss + dev * dev;
        }
    }
    const double sd = count > 0 ? sqrt(ss / (double)count) : 0.0;
    if (s < n_seeds) {
        if (col) {
            count_out[s * dp + at] = count;
            mean_out[s * dp + at] = mean;
            std_out[s * dp + at] = sd;
        }
        if (threadIdx.x == 0) valid_out[s] = valid;
    }

    const bool m = col && valid > 0 && 1000ll * (long long)count >= (long long)tau_milli * (long long)valid;
    const unsigned long long support = __ballot(m);
    const int n = __popcll(support);
    if (m) sel[__popcll(support & ((1ull << lane) - 1ull))] = lane;
    if (col) xrow[lane] = 0.0;
    stlsq_wave_sync();
    const bool bad = n > 0 && stlsq_row_solve(G, F, p, j, gamma * gamma, n, lane, A, xrow, sel);
    stlsq_wave_sync();
    if (col) {
        xi_out[s * dp + at] = bad ? 0.0f : (float)xrow[lane];
        mask_out[s * dp + at] = m ? 1 : 0;
    }
    if (lane == 0) f_bad[j] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any_bad = 0;
        for (int w = 0; w < d; ++w) any_bad |= f_bad[w];
        fell_out[s] = any_bad;
    }
}

inline hipError_t launch_stlsq_bag(const double* aug, long n_seeds, long n_problems, int d, int p, int n_replicas, const float* rep_xi,
                                   const unsigned char* rep_mask, const int* rep_fell, const int* tau_table, int tau_milli, double gamma,
                                   float* xi_out, unsigned char* mask_out, int* fell_out, int* count_out, int* valid_out,
                                   double* mean_out, double* std_out, hipStream_t st) {
    const size_t lds = stlsq_lds_bytes(d, p);
    auto kernel = tau_table ? stlsq_bag_kernel<true> : stlsq_bag_kernel<false>;
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    kernel<<<dim3((unsigned)n_problems), dim3((unsigned)(WAVE * d)), lds, st>>>(aug, (int)n_seeds, d, p, n_replicas, rep_xi, rep_mask,
                                                                                rep_fell, tau_table, tau_milli, gamma, xi_out, mask_out,
                                                                                fell_out, count_out, valid_out, mean_out, std_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
