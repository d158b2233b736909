// Sequential-threshold least squares on the device (symode_stlsq_sweep): the threshold loop of host_lstsq.cpp's
// symode_host_stlsq_sweep under the full-rank driver (gels), restated for one launch over all problems.  Library
// independent (it reads Gram matrices, not points), so only capi.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace symode {

constexpr int STLSQ_MAX_P = WAVE;      // one lane per library column
constexpr int STLSQ_MAX_D = 4;         // one wave per equation row
constexpr int STLSQ_HYPER = 2;         // columns of a row of the per-problem table: gamma, threshold

// LDS of a workgroup: per wave the support's system (p x p fp64, rows of stride p) and the row's coefficients (p fp64),
// then per wave the support list (p ints), then three groups of STLSQ_MAX_D flags.  131 KiB at d = 4, p = 64.
inline size_t stlsq_lds_bytes(int d, int p) {
    return (size_t)d * ((size_t)p * p + p) * sizeof(double) + ((size_t)d * p + 3 * STLSQ_MAX_D) * sizeof(int);
}

// The lanes of a wave run in lockstep and its LDS operations complete in order; what is left to rule out is the compiler
// moving a lane's read above another lane's write.
__device__ __forceinline__ void stlsq_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// v of lane `lane` (the same for the whole wave), in every lane
__device__ __forceinline__ double stlsq_lane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// The solve of one pass on one equation row, stated once for stlsq_sweep_kernel and stlsq_path_kernel (stlsq_path.hpp):
// the support's n > 0 columns are listed in sel (ascending), xrow holds zeros; on return xrow[column] is the solution on
// the support (system, factor and solve as the comment of stlsq_sweep_kernel states them).  True at a pivot that is not
// > 0, with xrow untouched.  The caller syncs the wave before (sel, xrow) and after (xrow).
__device__ __forceinline__ bool stlsq_row_solve(const double* __restrict__ G, int F, int p, int j, double g2, int n, int lane,
                                                double* A, double* xrow, const int* sel) {
    const bool on = lane < n;
    const int col = on ? sel[lane] : 0;
    for (int a = 0; a < n; ++a) {
        const int ra = sel[a];
        if (on) A[a * p + lane] = G[(long)ra * F + col] + (ra == col ? g2 : 0.0);
    }
    double c = on ? G[(long)col * F + p + j] : 0.0;
    stlsq_wave_sync();
    int orig = lane;
    double dg = on ? A[lane * p + lane] : 0.0;
    for (int kk = 0; kk < n; ++kk) {
        double bv = dg;
        int bi = (lane >= kk && lane < n) ? lane : WAVE;
#pragma unroll
        for (int off = WAVE / 2; off > 0; off /= 2) {
            const double ov = __shfl_xor(bv, off, WAVE);
            const int oi = __shfl_xor(bi, off, WAVE);
            if (oi < WAVE && (bi == WAVE || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        const int jp = __builtin_amdgcn_readfirstlane(bi);
        if (jp != kk) {
            const int src = lane == kk ? jp : (lane == jp ? kk : lane);
            orig = __shfl(orig, src, WAVE);
            dg = __shfl(dg, src, WAVE);
            c = __shfl(c, src, WAVE);
        }
        const double dkk = stlsq_lane(dg, kk);
        if (!(dkk > 0.0)) return true;
        const double r = sqrt(dkk);
        const int jo = __builtin_amdgcn_readlane(orig, kk);
        const bool rest = lane > kk && lane < n;
        double Rt = 0.0;
        if (rest) {
            Rt = A[jo * p + orig] / r;
            A[jo * p + orig] = Rt;
        }
        if (lane == kk) A[jo * p + jo] = r;
        for (int a = kk + 1; a < n; ++a) {
            const double Ra = stlsq_lane(Rt, a);
            const int oa = __builtin_amdgcn_readlane(orig, a);
            if (rest) A[oa * p + orig] -= Ra * Rt;
        }
        const double q = stlsq_lane(c, kk) / r;
        if (rest) {
            c -= Rt * q;
            dg -= Rt * Rt;
        }
        if (lane == kk) c = q;
        stlsq_wave_sync();
    }
    for (int i = n - 1; i >= 0; --i) {
        const int jo = __builtin_amdgcn_readlane(orig, i);
        const double prod = (lane > i && lane < n) ? A[jo * p + orig] * c : 0.0;
        double acc = stlsq_lane(c, i);
        for (int t = i + 1; t < n; ++t) acc -= stlsq_lane(prod, t);
        const double y = acc / A[jo * p + jo];
        if (lane == i) c = y;
    }
    if (on) xrow[sel[orig]] = c;
    return false;
}

// One workgroup per problem, one wave per equation row j; lane k of the wave owns library column k (mask bit, fp32
// coefficient).  Per pass the wave solves the ridge system on row j's support -- the host solves the masked case as ONE
// block-diagonal system over the rows, whose blocks never mix (a zero off-block entry of the factor leaves every sum it
// enters unchanged), so a block's eliminations, substitutions and their order are the ones below:
//   system    A = Gtt[sel, sel] + gamma^2 I and c = Gty[sel, j] on the support sel (ascending columns), A in LDS;
//   factor    pivoted Cholesky as symode_host_lstsq_normal states it.  Lane t holds POSITION t of the pivot order: the
//             index `orig` of its row / column of A, the running diagonal and the right-hand side, and the host's swap of
//             positions kk and j is an exchange of those three between two lanes.  Largest remaining diagonal first, the
//             lowest position of equals (the host's scan), stop at a pivot that is not > 0.  The row of the factor takes
//             the place of the pivot's row of A; the trailing update is one LDS row per step of a, 64 columns wide;
//   solve     forward substitution inside the factor loop (q_kk as soon as row kk exists, subtracted from the positions
//             behind it: the host's order of terms per entry), back substitution row by row with the products formed
//             across the lanes and subtracted in the host's order t = i + 1 .. n - 1.
// No multiply-add is contracted (-ffp-contract=off), so every entry sees the host's operations in the host's order.
// Then the host's thresholding on the fp32-rounded row; the rows' "mask changed" and "pivot not positive" flags meet in
// LDS, so the whole problem stops together.  Every LDS and global index is bounded by p and d: no address depends on data.
// HYPER: gamma and threshold come from row s of the (n_problems, 2) table -- a template bit, so the scalar instantiation
// keeps its code; problem s reads matrix set s % n_sets in both.
template <bool HYPER>
__global__ __launch_bounds__(WAVE * STLSQ_MAX_D) void stlsq_sweep_kernel(const double* __restrict__ aug, int n_sets, int d, int p,
                                                                          const float* __restrict__ hyper, double gamma,
                                                                          double threshold, int max_iter, double near_band,
                                                                          float* __restrict__ xi_out,
                                                                          unsigned char* __restrict__ mask_out,
                                                                          int* __restrict__ passes_out, int* __restrict__ near_out,
                                                                          int* __restrict__ fell_out) {
    extern __shared__ double stlsq_smem[];
    const int lane = threadIdx.x % WAVE;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long s = blockIdx.x;
    const int F = p + d;
    double* A = stlsq_smem + (size_t)j * ((size_t)p * p + p);
    double* xrow = A + (size_t)p * p;
    int* ints = (int*)(stlsq_smem + (size_t)d * ((size_t)p * p + p));
    int* sel = ints + j * p;
    int* f_changed = ints + d * p;
    int* f_bad = f_changed + STLSQ_MAX_D;
    int* f_near = f_bad + STLSQ_MAX_D;
    if constexpr (HYPER) {
        gamma = (double)hyper[s * STLSQ_HYPER];
        threshold = (double)hyper[s * STLSQ_HYPER + 1];
    }
    const double* G = aug + (s % n_sets) * (long)F * F;
    const double g2 = gamma * gamma;
    const float thr32 = (float)threshold;
    bool m = lane < p;
    float v = 0.0f;
    int near = 0, passes = 0, fell = 0;
    for (int it = 0; it < max_iter; ++it) {
        const unsigned long long support = __ballot(m);
        const int n = __popcll(support);
        if (m) sel[__popcll(support & ((1ull << lane) - 1ull))] = lane;
        if (lane < p) xrow[lane] = 0.0;
        stlsq_wave_sync();
        const bool bad = n > 0 && stlsq_row_solve(G, F, p, j, g2, n, lane, A, xrow, sel);
        stlsq_wave_sync();
        int changed = 0;
        if (!bad) {
            v = (float)(lane < p ? xrow[lane] : 0.0);
            const float av = fabsf(v);
            near += __popcll(__ballot(m && fabs((double)av - threshold) < near_band));
            const bool nm = m && av > thr32;
            changed = __ballot(nm != m) != 0ull;
            m = nm;
        }
        if (lane == 0) {
            f_changed[j] = changed;
            f_bad[j] = bad;
        }
        __syncthreads();
        int any_changed = 0, any_bad = 0;
        for (int w = 0; w < d; ++w) {
            any_changed |= f_changed[w];
            any_bad |= f_bad[w];
        }
        __syncthreads();
        passes = it + 1;
        if (any_bad) {
            fell = 1;
            break;
        }
        if (!any_changed) break;
    }
    if (lane < p) {
        xi_out[(s * d + j) * p + lane] = v;
        mask_out[(s * d + j) * p + lane] = m ? 1 : 0;
    }
    if (lane == 0) f_near[j] = near;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < d; ++w) total += f_near[w];
        passes_out[s] = passes;
        near_out[s] = total;
        fell_out[s] = fell;
    }
}

inline hipError_t launch_stlsq_sweep(const double* aug, long n_sets, long n_problems, int d, int p, const float* hyper, double gamma,
                                     double threshold, int max_iter, double near_band, float* xi_out, unsigned char* mask_out,
                                     int* passes_out, int* near_out, int* fell_out, hipStream_t st) {
    const size_t lds = stlsq_lds_bytes(d, p);
    auto kernel = hyper ? stlsq_sweep_kernel<true> : stlsq_sweep_kernel<false>;
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    kernel<<<dim3((unsigned)n_problems), dim3((unsigned)(WAVE * d)), lds, st>>>(aug, (int)n_sets, d, p, hyper, gamma, threshold,
                                                                                max_iter, near_band, xi_out, mask_out, passes_out,
                                                                                near_out, fell_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
