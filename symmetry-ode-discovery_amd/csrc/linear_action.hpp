// Is g(x) the linear image J x of x under the compact Jacobian table?  One streaming pass over x and gx, run once per data
// set, next to the constant-J pass (jconst.hpp).  Where it is, the fused reversed closure needs neither g(x) nor Theta(g x):
// Theta(J x) = M Theta(x) for the plain polynomial libraries (closure_fold.hpp), and this pass also leaves M.
//
// Acceptance, per component a of every point, evaluated in fp64 on the fp32 inputs (u = 2^-24):
//   | gx_a - sum_b J_ab x_b |  <=  4 u sum_b |J_ab| |x_b|.
// Any fp32 evaluation of the length-2 dot product, with or without FMA, lies within about 2 u of that sum; the factor 4
// leaves room for a g(x) produced another way at the same accuracy.  A NaN or an infinity in x, gx or J answers no; so does
// an offset (an affine action mixes the degrees of Theta).  d = 2, one group element.
//
// M (p x p, fp64, built from the fp32 table): row k holds Theta_k(J x) in terms of Theta(x), rows and columns in the column
// order of Library<2, ORDER, 0>::eval -- the degree-g block is [x0^g, x0^(g-1) x1, .., x1^g], column lo_g + m has m factors
// x1, and its row is the row of its prefix column (PolyTable::parent) times the linear form of its last variable.
// Block diagonal by degree: everything outside the blocks is written as exactly 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace symode {

constexpr int LINACT_BLOCK = 256;
constexpr int LINACT_MAX_P = 21;         // d = 2, order 5

__global__ void linact_flag_init_kernel(int* flag) { *flag = 1; }

__device__ __forceinline__ bool linact_finite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u; }

// grid = (problems, blocks per problem); x, gx (n, 2) per problem, table (2, 2), m_out (p, p)
__global__ __launch_bounds__(LINACT_BLOCK) void linact_kernel(const float* __restrict__ x, const float* __restrict__ gx,
                                                              const float* __restrict__ table, long n, int order, int p, bool vec,
                                                              double* __restrict__ m_out, int* __restrict__ flag) {
    __shared__ double msh[LINACT_MAX_P * LINACT_MAX_P];
    __shared__ int any_bad;
    const long s = blockIdx.x;
    const float* xs = x + s * n * 2;
    const float* gs = gx + s * n * 2;
    const float j00 = table[s * 4 + 0], j01 = table[s * 4 + 1], j10 = table[s * 4 + 2], j11 = table[s * 4 + 3];
    if (threadIdx.x == 0) any_bad = 0;
    __syncthreads();
    int bad = !(linact_finite(j00) && linact_finite(j01) && linact_finite(j10) && linact_finite(j11));
    if (blockIdx.y == 0) {
        for (int t = threadIdx.x; t < p * p; t += LINACT_BLOCK) msh[t] = 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            msh[0] = 1.0;
            for (int g = 1; g <= order; ++g) {
                const int lo = g * (g + 1) / 2, plo = (g - 1) * g / 2;
                for (int m = 0; m <= g; ++m) {
                    const int v = m > 0 ? 1 : 0, q = plo + (m > 0 ? m - 1 : 0), t = lo + m;
                    const double jv0 = v ? (double)j10 : (double)j00, jv1 = v ? (double)j11 : (double)j01;
                    for (int c = 0; c < g; ++c) {              // the prefix's row lives in the degree g-1 block
                        const double o = msh[q * p + plo + c];
                        msh[t * p + lo + c] += o * jv0;
                        msh[t * p + lo + c + 1] += o * jv1;
                    }
                }
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < p * p; t += LINACT_BLOCK) m_out[s * p * p + t] = msh[t];
    }
    const double a00 = fabs((double)j00), a01 = fabs((double)j01), a10 = fabs((double)j10), a11 = fabs((double)j11);
    const double four_u = 4.0 / 16777216.0;
    auto check = [&](float x0, float x1, float g0, float g1) {
        const double d0 = (double)x0, d1 = (double)x1;
        const double e0 = fabs((double)g0 - ((double)j00 * d0 + (double)j01 * d1));
        const double e1 = fabs((double)g1 - ((double)j10 * d0 + (double)j11 * d1));
        const double b0 = four_u * (a00 * fabs(d0) + a01 * fabs(d1)), b1 = four_u * (a10 * fabs(d0) + a11 * fabs(d1));
        const bool fin = linact_finite(x0) && linact_finite(x1) && linact_finite(g0) && linact_finite(g1);
        bad |= !(fin && e0 <= b0 && e1 <= b1);
    };
    const long tid = (long)blockIdx.y * LINACT_BLOCK + threadIdx.x, nthreads = (long)gridDim.y * LINACT_BLOCK;
    if (vec) {
        const float4* qx = reinterpret_cast<const float4*>(xs);
        const float4* qg = reinterpret_cast<const float4*>(gs);
        const long nvec = n / 2;
        for (long i = tid; i < nvec; i += nthreads) {
            const float4 a = qx[i], b = qg[i];
            check(a.x, a.y, b.x, b.y);
            check(a.z, a.w, b.z, b.w);
        }
        if (tid == 0 && (n & 1)) check(xs[2 * (n - 1)], xs[2 * (n - 1) + 1], gs[2 * (n - 1)], gs[2 * (n - 1) + 1]);
    } else {
        for (long i = tid; i < n; i += nthreads) check(xs[2 * i], xs[2 * i + 1], gs[2 * i], gs[2 * i + 1]);
    }
    if (bad) any_bad = 1;                                    // (benign race: every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && any_bad) atomicAnd(flag, 0);
}

inline hipError_t launch_linear_action(const float* x, const float* gx, const float* table, long S, long n, int order, double* m_out,
                                       int* flag, hipStream_t st) {
    const int p = (order + 1) * (order + 2) / 2;
    // 16-byte vectors: every problem's slab of x and gx starts on a 16-byte boundary
    const bool vec = ((uintptr_t)x % 16 == 0) && ((uintptr_t)gx % 16 == 0) && (S == 1 || (n * 2) % 4 == 0);
    long gy = (n + (long)LINACT_BLOCK * 8 - 1) / ((long)LINACT_BLOCK * 8);
    const long want = S >= 8192 ? 1 : (8192 + S - 1) / S;
    if (gy > want) gy = want;
    if (gy > 64) gy = 64;
    if (gy < 1) gy = 1;
    linact_flag_init_kernel<<<dim3(1), dim3(1), 0, st>>>(flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    linact_kernel<<<dim3((unsigned)S, (unsigned)gy), dim3(LINACT_BLOCK), 0, st>>>(x, gx, table, n, order, p, vec, m_out, flag);
    return hipGetLastError();
}

}  // namespace symode
