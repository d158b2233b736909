// The sparsity path of the fit with the reversed symmetry regulariser on the device (symode_stlsq_path_symreg): backward
// elimination over the joint (d, p) support from the full library down to the empty model, every model scored on a held-out
// matrix, the sparsest one that is as good as the best kept.  Library independent (it reads Gram matrices, not points), so
// only capi.hip includes this header -- behind stlsq_path.hpp (stlsq_path_rss, stlsq_path_smallest) and stlsq_symreg.hpp
// (stlsqs_pass_solve), which it builds on and which stay included by that translation unit alone.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "stlsq.hpp"

namespace symode {

constexpr int STLSQPS_HYPER = 2;       // columns of a row of the per-problem table: gamma, w_sym

// LDS of a workgroup: the UNFACTORED operands -- the training and the validation matrix ((p+d)^2 fp64 each) and R ((d p)^2
// fp64) --, the system ((d p)^2 fp64), then stlsq_symreg_kernel's mask words, support list and fp32 coefficients.  Every step
// rebuilds the system from G and R and evaluates three quadratic forms whose lanes walk ROWS of G, V and R: from global memory
// those are 64 cache lines per read (what made the first path's launch nine times its estimate), from LDS a bank pattern.
// 130.5 KiB at d = 1, p = 64; gfx950 has 160 KiB per workgroup.
inline size_t stlsqps_lds_bytes(int d, int p) {
    const size_t F = (size_t)(p + d), DP = (size_t)d * p;
    return (2 * F * F + 2 * DP * DP) * sizeof(double) + STLSQ_MAX_D * sizeof(unsigned long long) + DP * (sizeof(int) + sizeof(float));
}

// v^T R v of the coefficients (lane b holds v_b of flat index b = j p + k, 0 off the support) in the order symode.h states:
// lane b forms q_b = sum_a R[b][a] v_a over the support ascending from 0.0 and r_b = v_b q_b, then the form starts at 0.0 and
// takes r_b for b ascending over the support.  The same value in every lane.
__device__ __forceinline__ double stlsqps_form(const double* Rs, int DP, unsigned long long flat, double v, int lane) {
    const double* row = Rs + (lane < DP ? lane : 0) * DP;
    double q = 0.0;
    for (int a = 0; a < DP; ++a)
        if ((flat >> a) & 1ull) q += row[a] * stlsq_lane(v, a);
    const double r = v * q;
    double e = 0.0;
    for (int b = 0; b < DP; ++b)
        if ((flat >> b) & 1ull) e += stlsq_lane(r, b);
    return e;
}

// sum_j (Hyy_j - 2 w_j^T c_j + w_j^T Htt w_j) on the raw sums H (p+d, p+d) with xs the (d, p) fp32 coefficients in LDS: from 0.0,
// rows ascending, each row's term stlsq_path_rss (lane k holds the row's w_k).  The same value in every lane.
__device__ __forceinline__ double stlsqps_mse(const double* H, int d, int p, const unsigned long long* M, const float* xs,
                                              int lane) {
    double e = 0.0;
    for (int j = 0; j < d; ++j)
        e += stlsq_path_rss(H, p + d, p, j, M[j], (double)(lane < p ? xs[j * p + lane] : 0.0f), lane);
    return e;
}

// stlsq_symreg_kernel's geometry: one workgroup of ONE wave per problem, the joint system of n <= d p <= 64 unknowns, one lane
// per position of the pivot order; in the scores and the elimination lane b owns flat index b = j p + k.  The support is the
// 64-bit word `flat` (bit j p + k), the same in every lane; the d mask words stlsqs_pass_solve reads are cut from it by lanes
// 0 .. d - 1.  Step t = 0 .. d p has t entries removed:
//   solve      stlsqs_pass_solve -- the statements of one pass of stlsq_symreg_kernel -- v = (float) of the solution on the
//              support, 0 off it (t = d p: the empty model, v = 0); a flagged pivot sets fell and ends the problem;
//   scores     on (double)v: mse_train = stlsqps_mse on G, reg_train = stlsqps_form on R, mse_val = stlsqps_mse on V; lane t
//              keeps mse_val of step t (the empty model's is Vyy itself, so d p = 64 needs no 65th lane);
//   eliminate  the active entry with the smallest |v| leaves (stlsq_path_smallest over the flat index); with two or more
//              active, the step counts in `near` when runner-up minus smallest, widened to fp64, is < near_band.  Lane b
//              remembers the step `rem` at which its entry left: it is active at step t exactly when rem >= t.
// Then best = the largest t with mse_val[t] <= (1 + tol) max(min_t mse_val[t], 0) + floor_rel Vyy, and the support of step
// `best` is solved once more (the same statements on the same numbers: the bits of path_xi[best]) -- so no address depends on
// data: every LDS and global index is bounded by d, p.  gamma and w_sym arrive in fp32, as the table holds them: HYPER reads
// them from row s of the (n_problems, 2) table, wave-uniformly.  No multiply-add is contracted (-ffp-contract=off).
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): profiles/stlsq_path_symreg.txt.
template <bool HYPER>
__global__ __launch_bounds__(WAVE) void stlsq_path_symreg_kernel(
    const double* __restrict__ aug, const double* __restrict__ rev, const double* __restrict__ val, int n_sets, int n_val_sets,
    int d, int p, const float* __restrict__ hyper, float gamma32, float w_sym32, double tol, double floor_rel, double near_band,
    double pivot_floor, float* __restrict__ path_xi, int* __restrict__ order, double* __restrict__ mse_train,
    double* __restrict__ reg_train, double* __restrict__ mse_val, int* __restrict__ best_out, float* __restrict__ xi_out,
    unsigned char* __restrict__ mask_out, int* __restrict__ near_out, int* __restrict__ fell_out) {
    extern __shared__ double stlsqps_smem[];
    const int lane = threadIdx.x;
    const long s = blockIdx.x;
    const int F = p + d, DP = d * p;
    double* Gs = stlsqps_smem;
    double* Vs = Gs + (size_t)F * F;
    double* Rs = Vs + (size_t)F * F;
    double* A = Rs + (size_t)DP * DP;
    unsigned long long* M = (unsigned long long*)(A + (size_t)DP * DP);
    int* sel = (int*)(M + STLSQ_MAX_D);
    float* xs = (float*)(sel + DP);
    if constexpr (HYPER) {
        gamma32 = hyper[s * STLSQPS_HYPER];
        w_sym32 = hyper[s * STLSQPS_HYPER + 1];
    }
    const double gamma = (double)gamma32, w_sym = (double)w_sym32;
    const double g2 = gamma * gamma;
    {
        const double* G = aug + (s % n_sets) * (long)F * F;
        const double* V = val + (s % n_val_sets) * (long)F * F;
        const double* R = rev + (s % n_sets) * (long)DP * DP;
        for (int i = lane; i < F * F; i += WAVE) {
            Gs[i] = G[i];
            Vs[i] = V[i];
        }
        for (int i = lane; i < DP * DP; i += WAVE) Rs[i] = R[i];
    }
    const unsigned long long row_bits = p == 64 ? ~0ull : (1ull << p) - 1ull;
    unsigned long long flat = DP == 64 ? ~0ull : (1ull << DP) - 1ull;
    if (lane < STLSQ_MAX_D) M[lane] = lane < d ? row_bits : 0ull;
    stlsq_wave_sync();
    double Vyy = 0.0;
    for (int j = 0; j < d; ++j) Vyy += Vs[(p + j) * F + p + j];
    int rem = -1;
    double ev = 0.0;
    int near = 0, fell = 0;
    for (int t = 0; t <= DP; ++t) {
        int n;
        if (stlsqs_pass_solve(Gs, Rs, d, p, g2, w_sym, pivot_floor, M, lane, A, sel, xs, n)) {
            fell = 1;
            break;
        }
        stlsq_wave_sync();
        const float v = lane < DP ? xs[lane] : 0.0f;
        if (lane < DP) path_xi[(s * (DP + 1) + t) * DP + lane] = v;
        const double e_train = stlsqps_mse(Gs, d, p, M, xs, lane);
        const double e_reg = stlsqps_form(Rs, DP, flat, (double)v, lane);
        const double e_val = stlsqps_mse(Vs, d, p, M, xs, lane);
        if (lane == 0) {
            mse_train[s * (DP + 1) + t] = e_train;
            reg_train[s * (DP + 1) + t] = e_reg;
            mse_val[s * (DP + 1) + t] = e_val;
        }
        if (lane == t) ev = e_val;
        if (n > 0) {
            const bool m = (flat >> lane) & 1ull;
            const float av = fabsf(v);
            float lo, up;
            const int out = stlsq_path_smallest(m, av, lane, lo);
            if (n > 1) {
                stlsq_path_smallest(m && lane != out, av, lane, up);
                near += ((double)up - (double)lo < near_band) ? 1 : 0;
            }
            if (lane == 0) order[s * DP + t] = out;
            if (lane == out) rem = t;
            flat &= ~(1ull << out);
            stlsq_wave_sync();                      // every lane has read M
            if (lane < d) M[lane] = (flat >> (lane * p)) & row_bits;
            stlsq_wave_sync();
        }
    }
    int best = DP;
    flat = 0ull;
    if (!fell) {
        double e_min = lane < DP ? ev : Vyy;
#pragma unroll
        for (int off = WAVE / 2; off > 0; off /= 2) {
            const double o = __shfl_xor(e_min, off, WAVE);
            if (o < e_min) e_min = o;
        }
        if (Vyy < e_min) e_min = Vyy;
        const double cut = (1.0 + tol) * (e_min > 0.0 ? e_min : 0.0) + floor_rel * Vyy;
        const unsigned long long ok = __ballot(lane < DP && ev <= cut);
        if (!(Vyy <= cut) && ok != 0ull) best = 63 - __clzll((long long)ok);
        flat = __ballot(lane < DP && rem >= best);
        stlsq_wave_sync();
        if (lane < d) M[lane] = (flat >> (lane * p)) & row_bits;
        stlsq_wave_sync();
        int n;
        stlsqs_pass_solve(Gs, Rs, d, p, g2, w_sym, pivot_floor, M, lane, A, sel, xs, n);   // solved before at step `best`: not flagged
        stlsq_wave_sync();
    }
    if (lane < DP) {
        xi_out[s * DP + lane] = fell ? 0.0f : xs[lane];
        mask_out[s * DP + lane] = (flat >> lane) & 1ull ? 1 : 0;
    }
    if (lane == 0) {
        best_out[s] = best;
        near_out[s] = near;
        fell_out[s] = fell;
    }
}

inline hipError_t launch_stlsq_path_symreg(const double* aug, const double* rev, const double* val, long n_sets, long n_val_sets,
                                           long n_problems, int d, int p, const float* hyper, float gamma, float w_sym, double tol,
                                           double floor_rel, double near_band, double pivot_floor, float* path_xi, int* order,
                                           double* mse_train, double* reg_train, double* mse_val, int* best_out, float* xi_out,
                                           unsigned char* mask_out, int* near_out, int* fell_out, hipStream_t st) {
    const size_t lds = stlsqps_lds_bytes(d, p);
    auto kernel = hyper ? stlsq_path_symreg_kernel<true> : stlsq_path_symreg_kernel<false>;
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    kernel<<<dim3((unsigned)n_problems), dim3(WAVE), lds, st>>>(aug, rev, val, (int)n_sets, (int)n_val_sets, d, p, hyper, gamma,
                                                                w_sym, tol, floor_rel, near_band, pivot_floor, path_xi, order,
                                                                mse_train, reg_train, mse_val, best_out, xi_out, mask_out, near_out,
                                                                fell_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
