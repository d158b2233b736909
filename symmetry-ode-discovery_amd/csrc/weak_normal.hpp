// Normal matrices of the weak-SINDy fit for S windows (symode_weak_normal_windows): from the time-slab partials the
// window contraction left (weak.hpp) to the (p+d, p+d) matrix an STLSQ fit reads,
//   N = Z^T M Z,   Z = [G | b] (K, p+d),   G = V Theta(x_window),   b = -V' x_window,   M = V V^T (K, K) fp64
// (WSINDyWrapper.solve, sindy.py:365-370: G^T M G and G^T M b are N[:p, :p] and N[:p, p:]).  Library independent (it
// reads partials, not points), so only capi.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace symode {

constexpr int WEAK_NORMAL_MAX_K = 128;

// LDS of a workgroup: Z and Y = M Z, (K, F) fp64 each.  139 264 bytes at K = 128, F = 68.
inline size_t weak_normal_lds_bytes(int K, int F) { return 2 * (size_t)K * F * sizeof(double); }

// One workgroup per window s.
//   sum     every entry of the (16 RT, 16 CT) tile grid = its gx time-slab partials added in ascending order from 0.0: the
//           additions of weak_gram_finalize_kernel, so z_out[s] (if given) is symode_weak_gram's output for the window;
//   Z       the two blocks the fit keeps go to LDS: rows < K, columns < p (G) and rows K .. 2K-1, columns p .. p+d-1 (b);
//   Y       Y[k][f] = sum_l M[k][l] Z[l][f], l ascending;
//   N       N[i][j] = sum_k Z[k][i] Y[k][j], k ascending, for i <= j, stored to (i, j) and (j, i): exactly symmetric.
// fp64 on the vector pipe (K F (K + F/2) multiply-adds per window, 0.9 M at most: the launch is latency-bound, and the
// 4x4x4 matrix-core form would spend more code on operand layout than it saves in issue slots).  One thread owns an
// entry from first term to last and no multiply-add is contracted, so the launch is bit-deterministic.  Every index is
// bounded by the sizes in the arguments: no address depends on data.
__global__ __launch_bounds__(BLOCK) void weak_normal_kernel(const double* __restrict__ part, int gx, int RT, int CT, int K, int p,
                                                            int d, const double* __restrict__ M, double* __restrict__ aug_out,
                                                            double* __restrict__ z_out) {
    extern __shared__ double weak_normal_smem[];
    const int F = p + d;
    double* Z = weak_normal_smem;
    double* Y = Z + (size_t)K * F;
    const long s = blockIdx.x;
    const int e = threadIdx.x, row = e >> 4, col = e & 15;
    const long tile = (long)CT * 256;
    for (int rt = 0; rt < RT; ++rt) {
        const int r = 16 * rt + row;
        for (int c = 0; c < CT; ++c) {
            const double* src = part + ((s * RT + rt) * gx) * tile + c * 256 + e;
            double v = 0.0;
            int g = 0;
            for (; g + 8 <= gx; g += 8) {                // eight partials in flight, added in order
                double t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = src[(long)(g + u) * tile];
#pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
            for (; g < gx; ++g) v += src[(long)g * tile];
            const int f = 16 * c + col;
            if (z_out) z_out[(s * RT * 16 + r) * (CT * 16) + f] = v;
            if (r < K && f < p) Z[r * F + f] = v;
            if (r >= K && r < 2 * K && f >= p && f < F) Z[(r - K) * F + f] = v;
        }
    }
    __syncthreads();
    for (int o = e; o < K * F; o += BLOCK) {
        const int k = o / F, f = o - k * F;
        const double* Mk = M + (long)k * K;
        double v = 0.0;
        for (int l = 0; l < K; ++l) v += Mk[l] * Z[l * F + f];
        Y[o] = v;
    }
    __syncthreads();
    double* N = aug_out + s * (long)F * F;
    for (int o = e; o < F * F; o += BLOCK) {
        const int i = o / F, j = o - i * F;
        if (i > j) continue;
        double v = 0.0;
        for (int k = 0; k < K; ++k) v += Z[k * F + i] * Y[k * F + j];
        N[i * F + j] = v;
        N[j * F + i] = v;
    }
}

inline hipError_t launch_weak_normal(const double* part, int gx, long S, int K, int p, int d, const double* M, double* aug_out,
                                     double* z_out, hipStream_t st) {
    const int F = p + d, RT = (2 * K + 15) / 16, CT = (F + 15) / 16;
    const size_t lds = weak_normal_lds_bytes(K, F);
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t err = hipFuncSetAttribute((const void*)weak_normal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
    }
    weak_normal_kernel<<<dim3((unsigned)S), dim3(BLOCK), lds, st>>>(part, gx, RT, CT, K, p, d, M, aug_out, z_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
