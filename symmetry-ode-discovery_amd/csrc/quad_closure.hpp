// The closure of the non-latent fit as a quadratic form of fixed fp64 matrices (symode_quad_closure): library independent,
// so one kernel for every library (only capi.hip includes this header).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace symode {

// One wave per problem, W = Xi * M in LDS,
//   aug (S, p+d, p+d) = [Theta | dx]^T [Theta | dx]:  mse = inv (tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy)),
//                                                     grad_mse = 2 inv (W Gtt - Gty^T) * M;
//   rev (S, d p, d p) or null:                        reg = inv v^T R v,  grad_reg = 2 inv (R v) * M.
// Lane o of the wave owns outputs o, o + 64, ... of the d p gradient; rows of G and R are read along o (both symmetric),
// so every load of the wave is one contiguous segment.  fp64 throughout, one rounding to fp32 at the end.
//
// HYPER (symode_quad_closure_grid): S problems on n_sets sets of matrices, problem s reads set s % n_sets and takes its w_sym
// from column 3 of row s of the (S, 4) table hyper -- a template bit, so the scalar instantiation keeps its code.  The wave's
// problem comes from threadIdx.x / 64, which the compiler cannot prove uniform: set index and weight are read through
// readfirstlane, or every use of them would be per-lane arithmetic.
constexpr int QUAD_MAX_DP = 256;
constexpr int QUAD_HYPER = 4;         // columns of a row of the table (SYMODE_TRAINER_HYPER)

template <bool HYPER>
__global__ __launch_bounds__(BLOCK) void quad_closure_kernel(const double* __restrict__ aug, const double* __restrict__ rev, long S,
                                                             int d, int p, const float* __restrict__ xi,
                                                             const float* __restrict__ mask, double inv, float w_sym,
                                                             float* __restrict__ loss, float* __restrict__ grad,
                                                             const float* __restrict__ hyper, int n_sets) {
    constexpr int NW = BLOCK / WAVE;
    __shared__ double wsh[NW][QUAD_MAX_DP];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long s = (long)blockIdx.x * NW + wave;
    const int dp = d * p, F = p + d;
    const bool live = s < S;
    double* W = wsh[wave];
    if (live)
        for (int o = lane; o < dp; o += WAVE) W[o] = (double)(mask ? xi[s * dp + o] * mask[s * dp + o] : xi[s * dp + o]);
    __syncthreads();
    if (!live) return;
    long set = s;
    if constexpr (HYPER) {
        set = __builtin_amdgcn_readfirstlane((int)(s % n_sets));
        if (rev) w_sym = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hyper[s * QUAD_HYPER + 3])));
    }
    const double* Gs = aug + set * (long)F * F;
    const double* Rs = rev ? rev + set * (long)dp * dp : nullptr;
    double lsum = 0.0, rsum = 0.0;
    for (int o = lane; o < dp; o += WAVE) {
        const int j = o / p, a = o - j * p;
        const double* Wj = W + j * p;
        double wg = 0.0;                                    // (W Gtt)[j, a]
        for (int b = 0; b < p; ++b) wg = fma(Wj[b], Gs[(long)b * F + a], wg);
        const double gty = Gs[(long)a * F + p + j];
        lsum = fma(W[o], wg - 2.0 * gty, lsum);
        double g = wg - gty;
        if (Rs) {
            double rv = 0.0;                                // (R v)[o]
            for (int q = 0; q < dp; ++q) rv = fma(W[q], Rs[(long)q * dp + o], rv);
            rsum = fma(W[o], rv, rsum);
            g = fma((double)w_sym, rv, g);
        }
        const double m = mask ? (double)mask[s * dp + o] : 1.0;
        grad[s * dp + o] = (float)(2.0 * inv * g * m);
    }
    if (lane < d) lsum += Gs[(long)(p + lane) * F + p + lane];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off /= 2) {
        lsum += __shfl_xor(lsum, off, WAVE);
        rsum += __shfl_xor(rsum, off, WAVE);
    }
    if (lane == 0) {
        if (Rs) {
            loss[2 * s] = (float)(inv * lsum);
            loss[2 * s + 1] = (float)(inv * rsum);
        } else {
            loss[s] = (float)(inv * lsum);
        }
    }
}

inline hipError_t launch_quad_closure(const double* aug, const double* rev, long S, int d, int p, const float* xi, const float* mask,
                                      double inv, float w_sym, float* loss, float* grad, hipStream_t st) {
    constexpr int NW = BLOCK / WAVE;
    quad_closure_kernel<false><<<dim3((unsigned)((S + NW - 1) / NW)), dim3(BLOCK), 0, st>>>(aug, rev, S, d, p, xi, mask, inv, w_sym,
                                                                                            loss, grad, nullptr, 0);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

inline hipError_t launch_quad_closure_grid(const double* aug, const double* rev, int n_sets, long S, int d, int p, const float* xi,
                                           const float* mask, double inv, const float* hyper, float* loss, float* grad,
                                           hipStream_t st) {
    constexpr int NW = BLOCK / WAVE;
    quad_closure_kernel<true><<<dim3((unsigned)((S + NW - 1) / NW)), dim3(BLOCK), 0, st>>>(aug, rev, S, d, p, xi, mask, inv, 0.0f,
                                                                                           loss, grad, hyper, n_sets);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
