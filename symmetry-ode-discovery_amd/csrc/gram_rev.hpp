// Gram matrix of the reversed symmetry regulariser (model_utils.py:160-168 of the reference with g(x), J_g(x) fixed).
//
// For one point x_n and one group element g the regulariser's residual is linear in v = vec(Xi * M) (Xi's (d, p) row-major
// order):  u = B v,  B (d, d p),  B[i, (j, a)] = J_g(x_n)[i, j] theta_a(x_n) - delta_ij theta_a(g x_n).  So
//     sum_g sum_n |u|^2 = v^T R v,   R = sum_g sum_n B^T B = sum over the d rows b_i of B of b_i b_i^T   (d p, d p),
// and a fit on fixed data needs R once (raw sums: shards and chunks add).  Work per point and group element: d rows times the
// d p (d p + 1) / 2 distinct entries.
//
// Shape.  The triangle (210 entries at d = 2 order 3, 903 at order 5, 3081 at d = 3 order 3 with sine + exp) is cut into
// T (T + 1) / 2 upper 4x4 tiles, T = ceil(d p / 4); a thread owns ONE tile (16 fp64 sums, ~40 VGPRs at every library), so no
// library spills.  A workgroup walks stages of SP (point, group element) items: the SP * d threads (item, row i) evaluate the
// fp32 library at x and at g(x), form their row b_i in fp64 (J theta exact, minus theta(g x): one rounding per entry) and park
// it in LDS; then the threads, PG = BLOCK / NT groups of NT tiles each, take the items of the stage in turn and add the 4x4
// outer products of their row / column slices (two 32-byte LDS reads per 16 FMAs and row).  Libraries with more than BLOCK
// tiles (d p > 88: nothing in the reference domain) are not instantiated.
// Per-workgroup partials (NT * 16 doubles) are added in fixed order by a second launch and scattered into both triangles.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace symode {

template <class Lib>
struct RevGramShape {
    static constexpr int D = Lib::D, P = Lib::P, DP = D * P;
    static constexpr int T = (DP + 3) / 4;                 // 4-wide tiles per side
    static constexpr int NT = T * (T + 1) / 2;             // upper-triangular tiles (ti <= tj)
    static constexpr bool OK = NT <= BLOCK;
    static constexpr int PG = OK ? BLOCK / NT : 1;         // point groups of one workgroup
    static constexpr int ROW = 4 * T;                      // one row b_i in LDS, zero padded to whole tiles
    static constexpr int PARTIAL = NT * 16;                // doubles per workgroup partial
    // items per stage: the largest power of two <= 64 whose rows fit 48 KB of LDS
    static constexpr int sp() {
        int s = 64;
        while (s > 1 && s * D * ROW * 8 > 48 * 1024) s /= 2;
        return s;
    }
    static constexpr int SP = sp();
};

// Workgroups per problem: at least 64 items each, about 1024 workgroups in all, at most 1024 per problem.  A function of the
// sizes alone (not of the library), so the workspace query and the launch agree.
inline int rev_gram_grid(long n, long S, int n_g) {
    const long items = n * (long)n_g;
    long g = (items + 63) / 64;
    const long cap = S >= 1024 ? 1 : 1024 / S;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

inline size_t rev_gram_workspace_doubles(int dp, long S, long n, int n_g) {
    const long T = (dp + 3) / 4, NT = T * (T + 1) / 2;
    return (size_t)S * rev_gram_grid(n, S, n_g) * NT * 16;
}

// Row sources of the item loads.  Item m = g N + k of problem s (N points per problem) reads row xr of x and row gr of
// (g(x), J_g(x)) (D and D * D floats per row).
// Dense: x (S, N, d), gx (S, n_g, N, d), jgx (S, n_g, N, d, d), every problem its own copies.
struct RevRowsDense {
    __device__ static void rows(const int*, long, long s, long N, int n_g, long m, long& xr, long& gr) {
        xr = s * N + m % N;
        gr = s * N * n_g + m;
    }
};
// Gathered: x (n_src, d), gx (n_g, n_src, d), jgx (n_g, n_src, d, d) shared by all problems; point k of problem s is row
// idx[s N + k] (one 4-byte load per item; the caller guarantees 0 <= idx < n_src).
struct RevRowsGather {
    __device__ static void rows(const int* idx, long n_src, long s, long N, int, long m, long& xr, long& gr) {
        const long g = m / N, r = idx[s * N + (m - g * N)];
        xr = r;
        gr = g * n_src + r;
    }
};

// grid = (GX, S).  part: (S, GX, NT * 16) fp64; tile t (ti <= tj) element e = 4 r + c is sum b[4 ti + r] b[4 tj + c].
template <class Lib, class Rows>
__global__ __launch_bounds__(BLOCK) void rev_gram_kernel(const float* __restrict__ x, const float* __restrict__ gx,
                                                         const float* __restrict__ jgx, int n_g, long N,
                                                         const int* __restrict__ idx, long n_src,
                                                         double* __restrict__ part) {
    using G = RevGramShape<Lib>;
    constexpr int D = Lib::D, P = Lib::P, DP = G::DP, NT = G::NT, PG = G::PG, ROW = G::ROW, SP = G::SP;
    constexpr int STAGE = SP * D * ROW, COMB = PG * NT * 16;
    __shared__ double lds[STAGE > COMB ? STAGE : COMB];
    const long s = blockIdx.y;
    const long M = N * n_g;                                  // items m = g N + k: g(x) and J_g(x) are contiguous in m
    const int tid = threadIdx.x, tile = tid % NT, grp = tid / NT;
    int ti = 0, rem = tile;                                  // tile -> (ti, tj), row-major over the upper triangle
    while (rem >= G::T - ti) {
        rem -= G::T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;

    const long nstage = (M + SP - 1) / SP;
    for (long c = blockIdx.x; c < nstage; c += gridDim.x) {
        __syncthreads();                                     // the previous stage's rows have been read
        for (int w = tid; w < SP * D; w += BLOCK) {
            const int k = w % SP, i = w / SP;
            const long m = c * SP + k;
            double* row = lds + (k * D + i) * ROW;
            if (m < M) {
                long xr, gr;
                Rows::rows(idx, n_src, s, N, n_g, m, xr, gr);
                float xp[D], gp[D], J[D], th[P], thg[P];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    xp[j] = x[xr * D + j];
                    gp[j] = gx[gr * D + j];
                    J[j] = jgx[(gr * D + i) * D + j];
                }
                Lib::eval(xp, th);
                Lib::eval(gp, thg);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double Jd = (double)J[j];
#pragma unroll
                    for (int a = 0; a < P; ++a)
                        row[j * P + a] = (j == i) ? fma(Jd, (double)th[a], -(double)thg[a]) : Jd * (double)th[a];
                }
#pragma unroll
                for (int q = DP; q < ROW; ++q) row[q] = 0.0;
            } else {
                for (int q = 0; q < ROW; ++q) row[q] = 0.0;
            }
        }
        __syncthreads();
        if (grp < PG) {
            for (int k = grp; k < SP; k += PG) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const double* row = lds + (k * D + i) * ROW;
                    const double2 r01 = *reinterpret_cast<const double2*>(row + 4 * ti);
                    const double2 r23 = *reinterpret_cast<const double2*>(row + 4 * ti + 2);
                    const double2 c01 = *reinterpret_cast<const double2*>(row + 4 * tj);
                    const double2 c23 = *reinterpret_cast<const double2*>(row + 4 * tj + 2);
                    const double rv[4] = {r01.x, r01.y, r23.x, r23.y}, cv[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[4 * a + b] = fma(rv[a], cv[b], acc[4 * a + b]);
                }
            }
        }
    }
    // the PG groups' tiles added in fixed order through LDS
    __syncthreads();
    if (grp < PG) {
#pragma unroll
        for (int e = 0; e < 16; ++e) lds[(grp * NT + tile) * 16 + e] = acc[e];
    }
    __syncthreads();
    double* dst = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * G::PARTIAL;
    for (int e = tid; e < G::PARTIAL; e += BLOCK) {
        double v = lds[e];
        for (int g = 1; g < PG; ++g) v += lds[g * G::PARTIAL + e];
        dst[e] = v;
    }
}

// grid = (ceil(NT * 16 / 64), S): 64 elements per workgroup, SL slices of the GX partials each, added in fixed order.
template <int SL = BLOCK / WAVE>
__global__ __launch_bounds__(BLOCK) void rev_gram_finalize_kernel(const double* __restrict__ part, int GX, int dp,
                                                                  double* __restrict__ gram) {
    __shared__ double comb[SL][WAVE];
    const int T = (dp + 3) / 4, NT = T * (T + 1) / 2, PARTIAL = NT * 16;
    const long s = blockIdx.y;
    const int el = threadIdx.x % WAVE, slice = threadIdx.x / WAVE;
    const int e = blockIdx.x * WAVE + el;
    double v = 0.0;
    if (e < PARTIAL) {
        const double* src = part + s * (long)GX * PARTIAL + e;
        int g = slice;
        for (; g + 7 * SL < GX; g += 8 * SL) {               // 8 independent loads in flight, added in fixed order
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = src[(long)(g + u * SL) * PARTIAL];
#pragma unroll
            for (int u = 0; u < 8; ++u) v += t[u];
        }
        for (; g < GX; g += SL) v += src[(long)g * PARTIAL];
    }
    comb[slice][el] = v;
    __syncthreads();
    if (slice == 0 && e < PARTIAL) {
        double t = comb[0][el];
#pragma unroll
        for (int u = 1; u < SL; ++u) t += comb[u][el];
        int ti = 0, rem = e / 16;
        while (rem >= T - ti) {
            rem -= T - ti;
            ++ti;
        }
        const int tj = ti + rem;
        const int r = 4 * ti + (e & 15) / 4, c = 4 * tj + (e & 3);
        if (r < dp && c < dp) {
            double* out = gram + s * (long)dp * dp;
            out[(long)r * dp + c] = t;
            out[(long)c * dp + r] = t;
        }
    }
}

// idx == nullptr: dense per-problem copies; else S index rows of n points each into shared (x, gx, jgx) of n_src rows.  The
// grid and the finalize depend on (n, S, n_g) alone, so a gathered launch adds in the order of the dense one on copies.
template <class Lib>
hipError_t launch_symreg_reversed_gram(const float* x, const float* gx, const float* jgx, int n_g, long S, long n,
                                       const int* idx, long n_src, double* gram, double* ws, hipStream_t st) {
    using G = RevGramShape<Lib>;
    const int GX = rev_gram_grid(n, S, n_g);
    if (idx)
        rev_gram_kernel<Lib, RevRowsGather><<<dim3(GX, (unsigned)S), dim3(BLOCK), 0, st>>>(x, gx, jgx, n_g, n, idx, n_src, ws);
    else
        rev_gram_kernel<Lib, RevRowsDense><<<dim3(GX, (unsigned)S), dim3(BLOCK), 0, st>>>(x, gx, jgx, n_g, n, nullptr, 0, ws);
    SYMODE_LAUNCH_CHECK();
    rev_gram_finalize_kernel<><<<dim3((G::PARTIAL + WAVE - 1) / WAVE, (unsigned)S), dim3(BLOCK), 0, st>>>(ws, GX, G::DP, gram);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

// The launcher for the ops table, or nullptr (SYMODE_E_UNSUPPORTED) where the tiles would not fit one workgroup.
using RevGramFn = hipError_t (*)(const float*, const float*, const float*, int, long, long, const int*, long, double*, double*,
                                  hipStream_t);
template <class Lib>
constexpr RevGramFn rev_gram_launcher() {
    if constexpr (RevGramShape<Lib>::OK)
        return &launch_symreg_reversed_gram<Lib>;
    else
        return nullptr;
}

}  // namespace symode
