// Is J_g(x) the same matrix at every point?  One streaming pass over jgx (S, n_g, N, D, D), run once per data set.
//
// The reversed regulariser's interface mirrors precompute_symmreg_r (reference model_utils.py:172-211), which stores a
// Jacobian per point whatever the map is.  For a linear or affine group action on the observed coordinates, or a frozen
// linear autoencoder, every point of a (problem, group element) slab holds the same D x D matrix, and the closure kernels
// have a form that reads it from a compact (S, n_g, D, D) table instead of streaming 4 D D bytes per point
// (closure_rev.hpp, symreg_reversed_kernel<.., CJ = true>).  This pass decides whether that form may be used.
//
// Every word of a slab is compared BITWISE (as 32-bit integers) with the word at the same matrix position of the slab's
// point 0: -0.0 differs from +0.0 and a NaN payload only matches itself, so anything doubtful keeps the materialised path
// (a slab of identical NaNs would count as constant; the test for NaN is made on the reference words).  Different slabs
// may hold different matrices.  Library independent: D is a run-time argument (1..4).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace symode {

constexpr int JCONST_BLOCK = 256;
constexpr int JCONST_MAX_DD = 16;        // D <= 4

__global__ void jconst_flag_init_kernel(int* flag) { *flag = 1; }

// grid = (slabs, blocks per slab); slab = (problem, group element), `words` = N * D * D words each.
// vec: every slab starts on a 16-byte boundary and holds a whole number of 16-byte vectors.
__global__ __launch_bounds__(JCONST_BLOCK) void jconst_kernel(const unsigned* __restrict__ jgx, long words, int dd, bool vec,
                                                              unsigned* __restrict__ table, int* __restrict__ flag) {
    __shared__ unsigned ref[JCONST_MAX_DD];
    __shared__ int any_bad;
    const long slab = blockIdx.x;
    const unsigned* base = jgx + slab * words;
    if (threadIdx.x < dd) ref[threadIdx.x] = base[threadIdx.x];
    if (threadIdx.x == 0) any_bad = 0;
    __syncthreads();
    int bad = 0;
    if (blockIdx.y == 0 && threadIdx.x < dd) {
        const unsigned r = ref[threadIdx.x];
        table[slab * dd + threadIdx.x] = r;
        bad |= ((r & 0x7fffffffu) > 0x7f800000u);          // NaN in the reference matrix: never "constant"
    }
    const long tid = (long)blockIdx.y * JCONST_BLOCK + threadIdx.x, nthreads = (long)gridDim.y * JCONST_BLOCK;
    if (vec) {
        const uint4* q = reinterpret_cast<const uint4*>(base);
        const long nvec = words / 4;
        for (long i = tid; i < nvec; i += nthreads) {
            const uint4 v = q[i];
            const int e = (int)((4 * i) % dd);
            int e1 = e + 1, e2 = e + 2, e3 = e + 3;
            e1 -= e1 >= dd ? dd : 0;
            e2 -= e2 >= dd ? dd : 0;
            e2 -= e2 >= dd ? dd : 0;
            e3 -= e3 >= dd ? dd : 0;
            e3 -= e3 >= dd ? dd : 0;
            e3 -= e3 >= dd ? dd : 0;
            bad |= (v.x != ref[e]) | (v.y != ref[e1]) | (v.z != ref[e2]) | (v.w != ref[e3]);
        }
    } else {
        for (long i = tid; i < words; i += nthreads) bad |= (base[i] != ref[(int)(i % dd)]);
    }
    if (bad) any_bad = 1;                                    // (benign race: every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && any_bad) atomicAnd(flag, 0);
}

inline hipError_t launch_jacobian_constant(const float* jgx, long slabs, long n, int d, float* table, int* flag, hipStream_t st) {
    const int dd = d * d;
    const long words = n * dd;
    const bool vec = ((uintptr_t)jgx % 16 == 0) && (words % 4 == 0);
    long gy = (words + (long)JCONST_BLOCK * 16 - 1) / ((long)JCONST_BLOCK * 16);      // >= 16 words (4 vectors) per thread
    // ~8 K workgroups in all keep the chip streaming; a slab never needs more than 64
    const long want = slabs >= 8192 ? 1 : (8192 + slabs - 1) / slabs;
    if (gy > want) gy = want;
    if (gy > 64) gy = 64;
    if (gy < 1) gy = 1;
    jconst_flag_init_kernel<<<dim3(1), dim3(1), 0, st>>>(flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    jconst_kernel<<<dim3((unsigned)slabs, (unsigned)gy), dim3(JCONST_BLOCK), 0, st>>>(reinterpret_cast<const unsigned*>(jgx), words, dd,
                                                                                     vec, reinterpret_cast<unsigned*>(table), flag);
    return hipGetLastError();
}

}  // namespace symode
