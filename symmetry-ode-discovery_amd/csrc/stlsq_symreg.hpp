// Sequential-threshold least squares with the reversed symmetry regulariser on the device (symode_stlsq_sweep_symreg,
// EquivSINDy-r): per pass the minimiser of mse + w_sym * reg on the support, one linear system, for one launch over all
// problems.  Library independent (it reads Gram matrices, not points), so only capi.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "stlsq.hpp"
#include "stlsq_joint.hpp"

namespace symode {

constexpr int STLSQS_MAX_DP = WAVE;    // unknowns d p: one lane per position of the pivot order
constexpr int STLSQS_HYPER = 3;        // columns of a row of the per-problem table: gamma, threshold, w_sym

// LDS of a workgroup: the system (d p x d p fp64, rows of stride d p), the support masks of the STLSQ_MAX_D rows (64-bit
// words), the support list (d p ints) and the fp32 coefficients (d p floats).  33.3 KiB at d p = 64: under the 64 KiB a
// launch gets by default.
inline size_t stlsqs_lds_bytes(int dp) {
    return (size_t)dp * dp * sizeof(double) + STLSQ_MAX_D * sizeof(unsigned long long) + (size_t)dp * (sizeof(int) + sizeof(float));
}

// One pass's solve, stated once for stlsq_symreg_kernel and stlsq_path_symreg_kernel (stlsq_path_symreg.hpp): support,
// system, factorisation and substitutions as the comment of stlsq_symreg_kernel states them.  M holds the d mask words (the
// same in every lane), G the (p+d, p+d) and Rv the (d p, d p) raw sums -- global memory or LDS, the statements are the same.
// On return n_out is the size of the support, xs (d p floats) the solution rounded to fp32 and scattered to (d, p), zeros off the
// support; true for a flagged pivot (xs is then unspecified).  The caller synchronises the wave before it reads xs.
__device__ __forceinline__ bool stlsqs_pass_solve(const double* G, const double* Rv, int d, int p, double g2, double w_sym,
                                                  double pivot_floor, const unsigned long long* M, int lane, double* A, int* sel,
                                                  float* xs, int& n_out) {
    const int F = p + d, DP = d * p;
    // ---- support
    int n = 0;                          // (a local: the size reaches the caller once, at the end)
    for (int j = 0; j < d; ++j) {
        const unsigned long long mj = M[j];
        if ((mj >> lane) & 1ull) sel[n + __popcll(mj & ((1ull << lane) - 1ull))] = (j << 8) | lane;
        n += __popcll(mj);
    }
    if (lane < DP) xs[lane] = 0.0f;
    stlsq_wave_sync();
    bool bad = false;
    if (n > 0) {
        const bool on = lane < n;
        const int eb = on ? sel[lane] : 0;
        const int jb = eb >> 8, kb = eb & 255;
        const int ob = jb * p + kb;
        // ---- system
        for (int a = 0; a < n; ++a) {
            const int ea = __builtin_amdgcn_readfirstlane(sel[a]);
            const int ja = ea >> 8, ka = ea & 255;
            if (on && a <= lane) {
                const double block = ja == jb ? G[(long)ka * F + kb] + (ka == kb ? g2 : 0.0) : 0.0;
                A[a * DP + lane] = block + w_sym * Rv[((long)ja * p + ka) * DP + ob];
            }
        }
        double c = on ? G[(long)kb * F + p + jb] : 0.0;
        stlsq_wave_sync();
        for (int a = 0; a < n; ++a)
            if (on && a < lane) A[lane * DP + a] = A[a * DP + lane];
        stlsq_wave_sync();
        // ---- factor and solve
        int orig, fact;
        bad = stlsq_joint_factor<false>(A, DP, n, lane, orig, c, pivot_floor, fact);
        if (!bad) {
            stlsq_joint_back(A, DP, n, lane, orig, c);
            if (on) {
                const int eo = sel[orig];
                xs[(eo >> 8) * p + (eo & 255)] = (float)c;
            }
        }
    }
    n_out = n;
    return bad;
}

// One workgroup of ONE wave per problem.  The regulariser's R couples the equation rows -- v^T R v has entries between
// (j, k) and (j', k') for j != j' -- so a pass is one joint system of n <= d p <= 64 unknowns, the constrained kernel's
// situation: the factorisation, one lane per position of the pivot order, is a single wave's work whatever d is, the
// build in front of it is n steps per lane, and no __syncthreads is needed.
//
// Per pass, with the (d, p) mask M held as d 64-bit words in LDS (the same in every lane), lane b the owner of column b:
//   support   the entries (j, k) with M set in ascending (j, k): sel[0 .. n), each packed as (j << 8) | k;
//   system    A[a, b] = [j_a == j_b] (Gtt[k_a, k_b] + gamma^2 [k_a == k_b]) + w_sym R[j_a p + k_a, j_b p + k_b] in fp64 for
//             a <= b -- the bracket first (an exact 0.0 across rows), then the one addition of the one product --, the lower
//             triangle the mirror of the upper one, so A is exactly symmetric; b[a] = Gty[k_a, j_a].  With w_sym = 0 and a
//             finite R the product is a zero and A is blockdiag(Gtt + gamma^2 I)[M, M] to the bit;
//   solve     stlsq_joint.hpp: pivoted Cholesky with fused forward substitution and the pivot floor (a pivot that is not
//             > pivot_floor * (first pivot), or not > 0, flags the problem -- fell -- and ends it), back substitution;
//   Xi        (float) of the solution scattered into (d, p), zeros off the support;
//   threshold the host's rule (strict >, in fp32) on the still-active entries, near counted on them; stop when the mask
//             repeats.  An empty support (n = 0) gives Xi = 0, whose thresholding repeats the mask: the pass ends the problem.
// The stationarity condition solved is that of mse + w_sym reg with mse = inv (..), reg = inv v^T R v on the raw sums G, R:
// inv cancels, so w_sym multiplies R as the closure's weight multiplies the regulariser.
// No multiply-add is contracted (-ffp-contract=off).  Every LDS and global index is bounded by d, p: no address depends on
// data.  gamma, threshold and w_sym arrive in fp32, as the table holds them: HYPER reads them from row s of the
// (n_problems, 3) table -- s is the workgroup's index, so the three loads are wave-uniform --, a template bit, so the scalar
// instantiation keeps its code; problem s reads matrix set s % n_sets in both.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): profiles/stlsq_symreg.txt.
template <bool HYPER>
__global__ __launch_bounds__(WAVE) void stlsq_symreg_kernel(const double* __restrict__ aug, const double* __restrict__ rev,
                                                            int n_sets, int d, int p, const float* __restrict__ hyper,
                                                            float gamma32, float threshold32, float w_sym32, int max_iter,
                                                            double near_band, double pivot_floor, float* __restrict__ xi_out,
                                                            unsigned char* __restrict__ mask_out, int* __restrict__ passes_out,
                                                            int* __restrict__ near_out, int* __restrict__ fell_out) {
    extern __shared__ double stlsqs_smem[];
    const int lane = threadIdx.x;
    const long s = blockIdx.x;
    const int F = p + d, DP = d * p;
    double* A = stlsqs_smem;
    unsigned long long* M = (unsigned long long*)(A + (size_t)DP * DP);
    int* sel = (int*)(M + STLSQ_MAX_D);
    float* xs = (float*)(sel + DP);
    if constexpr (HYPER) {
        gamma32 = hyper[s * STLSQS_HYPER];
        threshold32 = hyper[s * STLSQS_HYPER + 1];
        w_sym32 = hyper[s * STLSQS_HYPER + 2];
    }
    const double gamma = (double)gamma32, threshold = (double)threshold32, w_sym = (double)w_sym32;
    const long set = s % n_sets;
    const double* G = aug + set * (long)F * F;
    const double* Rv = rev + set * (long)DP * DP;
    const double g2 = gamma * gamma;
    if (lane < STLSQ_MAX_D) M[lane] = lane < d ? (p == 64 ? ~0ull : (1ull << p) - 1ull) : 0ull;
    stlsq_wave_sync();
    int near = 0, passes = 0, fell = 0;
    for (int it = 0; it < max_iter; ++it) {
        int n;
        const bool bad = stlsqs_pass_solve(G, Rv, d, p, g2, w_sym, pivot_floor, M, lane, A, sel, xs, n);
        passes = it + 1;
        if (bad) {
            fell = 1;
            break;
        }
        stlsq_wave_sync();
        // ---- threshold
        int changed = 0;
        for (int j = 0; j < d; ++j) {
            const unsigned long long mj = M[j];
            float v = 0.0f;
            if (lane < p) {
                v = xs[j * p + lane];
                xi_out[(s * d + j) * p + lane] = v;
            }
            const bool m = (mj >> lane) & 1ull;
            const float av = fabsf(v);
            near += __popcll(__ballot(m && fabs((double)av - threshold) < near_band));
            const unsigned long long nm = __ballot(m && av > threshold32);
            changed |= nm != mj;
            stlsq_wave_sync();                      // every lane has read M[j]
            if (lane == 0) M[j] = nm;
        }
        stlsq_wave_sync();
        if (!changed) break;
    }
    for (int j = 0; j < d; ++j)
        if (lane < p) mask_out[(s * d + j) * p + lane] = (M[j] >> lane) & 1ull ? 1 : 0;
    if (lane == 0) {
        passes_out[s] = passes;
        near_out[s] = near;
        fell_out[s] = fell;
    }
}

inline hipError_t launch_stlsq_symreg(const double* aug, const double* rev, long n_sets, long n_problems, int d, int p,
                                      const float* hyper, float gamma, float threshold, float w_sym, int max_iter, double near_band,
                                      double pivot_floor, float* xi_out, unsigned char* mask_out, int* passes_out, int* near_out,
                                      int* fell_out, hipStream_t st) {
    auto kernel = hyper ? stlsq_symreg_kernel<true> : stlsq_symreg_kernel<false>;
    kernel<<<dim3((unsigned)n_problems), dim3(WAVE), stlsqs_lds_bytes(d * p), st>>>(aug, rev, (int)n_sets, d, p, hyper, gamma,
                                                                                    threshold, w_sym, max_iter, near_band,
                                                                                    pivot_floor, xi_out, mask_out, passes_out,
                                                                                    near_out, fell_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
