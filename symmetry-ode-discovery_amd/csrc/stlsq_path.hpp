// The sparsity path of the least-squares fit on the device (symode_stlsq_path): backward elimination from the full library
// down to the empty model, every model scored on a held-out matrix, the sparsest one that is as good as the best kept.
// Library independent (it reads Gram matrices, not points), so only capi.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "stlsq.hpp"

namespace symode {

// e = Hyy - 2 w^T c + w^T H w of row j's coefficients w (lane k holds w_k, 0 off the support) on the raw sums H (p+d, p+d), in
// the order symode.h states: lane k forms q_k = sum_l H[k][l] w_l over the support ascending and r_k = w_k (q_k - 2 H[k][p+j]),
// then e starts at H[p+j][p+j] and takes r_k for k ascending over the support.  The same value in every lane.
__device__ __forceinline__ double stlsq_path_rss(const double* __restrict__ H, int F, int p, int j, unsigned long long support,
                                                 double w, int lane) {
    const double* row = H + (long)(lane < p ? lane : 0) * F;
    double q = 0.0;
    for (int l = 0; l < p; ++l)
        if ((support >> l) & 1ull) q += row[l] * stlsq_lane(w, l);
    const double r = w * (q - 2.0 * row[p + j]);
    double e = H[(long)(p + j) * F + p + j];
    for (int k = 0; k < p; ++k)
        if ((support >> k) & 1ull) e += stlsq_lane(r, k);
    return e;
}

// The active column with the smallest |v| (fp32 compare), the lowest index of equals: its |v| in bv, its index returned
// (WAVE when no lane is active).  The same values in every lane.
__device__ __forceinline__ int stlsq_path_smallest(bool active, float av, int lane, float& bv) {
    bv = active ? av : 0.0f;
    int bi = active ? lane : WAVE;
#pragma unroll
    for (int off = WAVE / 2; off > 0; off /= 2) {
        const float ov = __shfl_xor(bv, off, WAVE);
        const int oi = __shfl_xor(bi, off, WAVE);
        if (oi < WAVE && (bi == WAVE || ov < bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    return __builtin_amdgcn_readfirstlane(bi);
}

// stlsq_sweep_kernel's geometry and LDS (stlsq_lds_bytes): one workgroup per problem, one wave per equation row j, lane k
// owns library column k.  Step t = 0 .. p of row j has t columns removed:
//   solve      stlsq_row_solve on the active columns -- the statements of one pass of stlsq_sweep_kernel -- v = (float) of
//              the solution on the support, 0 off it (t = p: the empty model, v = 0);
//   errors     stlsq_path_rss on the training set's and the validation set's matrix; lane t keeps the validation error of
//              step t (the empty model's is Vyy itself, so p = 64 needs no 65th lane);
//   eliminate  the active column with the smallest |v| leaves; with two or more active, the step counts in `near` when the
//              runner-up's |v| minus the smallest, both widened to fp64, is < near_band.  Lane k remembers the step `rem` at
//              which its column left: it is active at step t exactly when rem >= t.
// Then best = the largest t with rss_val[t] <= (1 + tol) max(min_t rss_val[t], 0) + floor_rel Vyy, and the row is solved
// once more on the support of step `best` (the same statements on the same numbers: the bits of path_xi[best]) -- so no
// address depends on data: every LDS and global index is bounded by p and d.  The rows' "pivot not positive" flags meet in
// LDS after every solve, as in stlsq_sweep_kernel (all rows have p - t active columns, so the barriers are uniform), and
// the whole problem ends together.
__global__ __launch_bounds__(WAVE * STLSQ_MAX_D) void stlsq_path_kernel(
    const double* __restrict__ aug, const double* __restrict__ val, int n_sets, int n_val_sets, int d, int p, double gamma,
    double tol, double floor_rel, double near_band, float* __restrict__ path_xi, int* __restrict__ order,
    double* __restrict__ rss_train, double* __restrict__ rss_val, int* __restrict__ best_out, float* __restrict__ xi_out,
    unsigned char* __restrict__ mask_out, int* __restrict__ near_out, int* __restrict__ fell_out) {
    extern __shared__ double stlsq_smem[];
    const int lane = threadIdx.x % WAVE;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long s = blockIdx.x;
    const int F = p + d;
    double* A = stlsq_smem + (size_t)j * ((size_t)p * p + p);
    double* xrow = A + (size_t)p * p;
    int* ints = (int*)(stlsq_smem + (size_t)d * ((size_t)p * p + p));
    int* sel = ints + j * p;
    int* f_bad = ints + d * p + STLSQ_MAX_D;
    int* f_near = f_bad + STLSQ_MAX_D;
    const double* G = aug + (s % n_sets) * (long)F * F;
    const double* V = val + (s % n_val_sets) * (long)F * F;
    const double g2 = gamma * gamma;
    const double Vyy = V[(long)(p + j) * F + p + j];
    const long row = s * d + j;
    bool m = lane < p;
    int rem = -1;
    float v = 0.0f;
    double ev = 0.0;
    int near = 0, fell = 0;
    for (int t = 0; t <= p; ++t) {
        const unsigned long long support = __ballot(m);
        const int n = __popcll(support);
        if (n > 0) {
            if (m) sel[__popcll(support & ((1ull << lane) - 1ull))] = lane;
            if (lane < p) xrow[lane] = 0.0;
            stlsq_wave_sync();
            const bool bad = stlsq_row_solve(G, F, p, j, g2, n, lane, A, xrow, sel);
            stlsq_wave_sync();
            if (lane == 0) f_bad[j] = bad;
            __syncthreads();
            int any_bad = 0;
            for (int w = 0; w < d; ++w) any_bad |= f_bad[w];
            __syncthreads();
            if (any_bad) {
                fell = 1;
                break;
            }
            v = (float)(lane < p ? xrow[lane] : 0.0);
        } else {
            v = 0.0f;
        }
        if (lane < p) path_xi[(row * (p + 1) + t) * p + lane] = v;
        const double e_train = stlsq_path_rss(G, F, p, j, support, (double)v, lane);
        const double e_val = stlsq_path_rss(V, F, p, j, support, (double)v, lane);
        if (lane == 0) {
            rss_train[row * (p + 1) + t] = e_train;
            rss_val[row * (p + 1) + t] = e_val;
        }
        if (lane == t) ev = e_val;
        if (n > 0) {
            const float av = fabsf(v);
            float lo, up;
            const int out = stlsq_path_smallest(m, av, lane, lo);
            if (n > 1) {
                stlsq_path_smallest(m && lane != out, av, lane, up);
                near += ((double)up - (double)lo < near_band) ? 1 : 0;
            }
            if (lane == 0) order[row * p + t] = out;
            if (lane == out) {
                m = false;
                rem = t;
            }
        }
    }
    int best = p;
    m = false;
    v = 0.0f;
    if (!fell) {
        double e_min = lane < p ? ev : Vyy;
#pragma unroll
        for (int off = WAVE / 2; off > 0; off /= 2) {
            const double o = __shfl_xor(e_min, off, WAVE);
            if (o < e_min) e_min = o;
        }
        if (Vyy < e_min) e_min = Vyy;
        const double cut = (1.0 + tol) * (e_min > 0.0 ? e_min : 0.0) + floor_rel * Vyy;
        const unsigned long long ok = __ballot(lane < p && ev <= cut);
        if (!(Vyy <= cut) && ok != 0ull) best = 63 - __clzll((long long)ok);
        m = lane < p && rem >= best;
        const unsigned long long support = __ballot(m);
        const int n = __popcll(support);
        if (n > 0) {
            if (m) sel[__popcll(support & ((1ull << lane) - 1ull))] = lane;
            if (lane < p) xrow[lane] = 0.0;
            stlsq_wave_sync();
            stlsq_row_solve(G, F, p, j, g2, n, lane, A, xrow, sel);      // solved before at step `best`: its pivots are > 0
            stlsq_wave_sync();
            v = (float)(lane < p ? xrow[lane] : 0.0);
        }
    }
    if (lane < p) {
        xi_out[row * p + lane] = v;
        mask_out[row * p + lane] = m ? 1 : 0;
    }
    if (lane == 0) {
        best_out[row] = best;
        f_near[j] = near;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < d; ++w) total += f_near[w];
        near_out[s] = total;
        fell_out[s] = fell;
    }
}

inline hipError_t launch_stlsq_path(const double* aug, const double* val, long n_sets, long n_val_sets, long n_problems, int d,
                                    int p, double gamma, double tol, double floor_rel, double near_band, float* path_xi,
                                    int* order, double* rss_train, double* rss_val, int* best_out, float* xi_out,
                                    unsigned char* mask_out, int* near_out, int* fell_out, hipStream_t st) {
    const size_t lds = stlsq_lds_bytes(d, p);
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t e = hipFuncSetAttribute((const void*)stlsq_path_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    stlsq_path_kernel<<<dim3((unsigned)n_problems), dim3((unsigned)(WAVE * d)), lds, st>>>(
        aug, val, (int)n_sets, (int)n_val_sets, d, p, gamma, tol, floor_rel, near_band, path_xi, order, rss_train, rss_val, best_out,
        xi_out, mask_out, near_out, fell_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
