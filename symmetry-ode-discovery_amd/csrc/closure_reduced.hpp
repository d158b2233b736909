// The closure without a point loop, reduced to a quadratic form in the fit's own variables (symode_quad_reduce, symode_quad_step;
// only capi.hip includes this header).  For fixed tables (aug, M, J), map Q, w_sym, column set and mask, closure_quad_kernel's
// loss is an exact quadratic in z = (beta, const), K = r + d_c numbers per problem: with W = P z the masked coefficients
// (P z = view(Q beta) + const on column 0, dead columns 0) and g(W) the gradient by Xi that kernel forms,
//     column i of H = 1/2 P^T (g(P e_i) - g(0)),    h = -1/2 P^T g(0),    c0 = inv tr(Gyy),
//     B = [[H, -h], [-h^T, c0]]  (K+1, K+1),        loss = v^T B v,  d loss / d z = 2 (B v)[:K],   v = [z; 1].
// quad_reduce_kernel builds B once per data set: one wave per problem walks the K + 1 states e_0 .. e_{K-1}, 0 through the
// statements of closure_quad_kernel's gradient (fold_c, fold_gram_term, W Gtt - Gty^T; nothing is rounded to fp32) and stores
// 1/2 (B + B^T), so that a row read and a column read agree bit for bit.  quad_step_kernel is the step: a group of 16 lanes per
// problem, lane i sums column i of B against v over coalesced row segments; no LDS, no barrier, 8 (K+1)^2 bytes per problem.
#pragma once
#include <hip/hip_runtime.h>

#include "closure_quad.hpp"

namespace symode {

constexpr unsigned long long WS_BODY_FOLD_REDUCED = 256;   // + the step read the reduced form B alone (word WS_BODY_WORD)
constexpr int REDUCED_GROUP = 16;                           // lanes of one problem in the step: K + 1 <= REDUCED_GROUP
constexpr int REDUCED_PER_BLOCK = BLOCK / REDUCED_GROUP;    // problems of one workgroup of the step

template <class Lib>
__global__ __launch_bounds__(BLOCK) void quad_reduce_kernel(const double* __restrict__ aug, const double* __restrict__ mt,
                                                            const float* __restrict__ jt, long S, const float* __restrict__ q,
                                                            int r, int use_kron, int has_const,
                                                            const float* __restrict__ mask, unsigned long long live,
                                                            float w_sym, double inv, double* __restrict__ bout) {
    constexpr int D = Lib::D, P = Lib::P, DP = D * P, F = P + D, NACC = 2 + DP, NW = BLOCK / WAVE;
    static_assert(D == 2 && !Lib::SINE && !Lib::EXP, "the fold kernels' libraries");
    __shared__ double wsh[NW][DP], cd[NW][DP], ud[NW][DP], gd[NW][DP], row_add[NW][NACC];
    __shared__ double pt[NW][REDUCED_GROUP][REDUCED_GROUP];              // pt[i][t] = (P^T g(state i))[t]
    const int lane = threadIdx.x % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long s_own = (long)blockIdx.x * NW + wave;
    const bool act = s_own < S;
    const long s = act ? s_own : S - 1;                                  // a wave past the last problem repeats it and writes nothing
    const float* js = jt + s * D * D;
    const double* ms = mt + s * P * P;
    const double* gs = aug + s * (long)F * F;
    double* W = wsh[wave];
    const int K = r + (has_const ? D : 0), n = K + 1;
    const double two_inv = 2.0 * inv;

    for (int i = 0; i <= K; ++i) {                                       // the same trip count in every wave: the barriers are uniform
        // W = P e_i (i < K) or 0 (i == K), masked, dead columns 0
        for (int o = lane; o < DP; o += WAVE) {
            const int j = o / P, k = o % P;
            double v = 0.0;
            if (i < r) v = (double)q[(long)(use_kron ? o : k * D + j) * r + i];
            else if (i < K) v = (k == 0 && j == i - r) ? 1.0 : 0.0;
            if (mask != nullptr) v *= (double)mask[s * DP + o];
            W[o] = ((live >> k) & 1ull) != 0 ? v : 0.0;
        }
        __syncthreads();
        for (int t = lane; t < DP; t += WAVE)
            cd[wave][t] = fold_c<D, P>(t / P, t % P, js, ms, [&](int b, int l) -> double { return W[b * P + l]; });
        fold_gram_term<D, P, ~0ull, WAVE, F>(lane, lane == WAVE - 1, js, ms, gs, live, w_sym, cd[wave], ud[wave], row_add[wave],
                                             [] { __syncthreads(); });
        // g = 2 inv (W Gtt - Gty^T + w_sym T), masked, zero in the dead columns
        for (int o = lane; o < DP; o += WAVE) {
            const int j = o / P, a = o % P;
            double wg = 0.0;
            for (int b = 0; b < P; ++b) wg = __builtin_fma(W[j * P + b], gs[b * F + a], wg);
            double g = two_inv * ((wg - gs[(P + j) * F + a]) + row_add[wave][2 + o]);
            if (mask != nullptr) g *= (double)mask[s * DP + o];
            if (((live >> a) & 1ull) == 0) g = 0.0;
            gd[wave][o] = g;
        }
        __syncthreads();
        // P^T g: the map's transpose, then the constant column
        for (int t = lane; t < K; t += WAVE) {
            double gb = 0.0;
            if (t < r) {
                for (int o = 0; o < DP; ++o) {
                    const int row = use_kron ? o : (o % P) * D + o / P;
                    gb = __builtin_fma(gd[wave][o], (double)q[(long)row * r + t], gb);
                }
            } else {
                gb = gd[wave][(t - r) * P];
            }
            pt[wave][i][t] = gb;
        }
        __syncthreads();
    }

    if (!act) return;
    const double c0 = inv * (gs[P * F + P] + gs[(P + 1) * F + P + 1]);
    auto raw = [&](int a, int b) -> double {                             // entry (a, b) of [[H, -h], [-h^T, c0]]
        if (a < K && b < K) return 0.5 * (pt[wave][b][a] - pt[wave][K][a]);
        if (a < K) return 0.5 * pt[wave][K][a];
        if (b < K) return 0.5 * pt[wave][K][b];
        return c0;
    };
    double* bs = bout + s * (long)n * n;
    for (int e = lane; e < n * n; e += WAVE) {
        const int a = e / n, b = e % n;
        bs[e] = 0.5 * (raw(a, b) + raw(b, a));
    }
}

__global__ __launch_bounds__(BLOCK) void quad_step_kernel(const double* __restrict__ bt, long S, int K, int dc,
                                                          const float* __restrict__ beta, long ldb,
                                                          const float* __restrict__ cst, long ldc, float* __restrict__ loss,
                                                          float* __restrict__ g_beta, float* __restrict__ g_const,
                                                          unsigned long long* header, unsigned long long body) {
    const int i = threadIdx.x % REDUCED_GROUP;
    const long s_own = (long)blockIdx.x * REDUCED_PER_BLOCK + threadIdx.x / REDUCED_GROUP;
    if (blockIdx.x == 0 && threadIdx.x == 0 && header != nullptr && header[0] == WS_MAGIC) header[WS_BODY_WORD] = body;
    const bool act = s_own < S;
    const long s = act ? s_own : S - 1;                                  // a group past the last problem repeats it and writes nothing
    const int r = K - dc, n = K + 1;
    double v = 0.0;                                                      // v = [beta; const; 1], one entry per lane
    if (i < r) v = (double)beta[s * ldb + i];
    else if (i < K) v = (double)cst[s * ldc + (i - r)];
    else if (i == K) v = 1.0;
    const double* bs = bt + s * (long)n * n;
    double row[REDUCED_GROUP];
#pragma unroll
    for (int j = 0; j < REDUCED_GROUP; ++j) row[j] = (j < n && i < n) ? bs[j * n + i] : 0.0;
    double a = 0.0;                                                      // a_i = sum_j B[j][i] v_j
#pragma unroll
    for (int j = 0; j < REDUCED_GROUP; ++j) a = __builtin_fma(row[j], __shfl(v, j, REDUCED_GROUP), a);
    double l = v * a;
#pragma unroll
    for (int off = REDUCED_GROUP / 2; off > 0; off /= 2) l += __shfl_xor(l, off, REDUCED_GROUP);
    if (!act) return;
    if (i == 0) loss[s] = (float)l;
    if (i < r) g_beta[s * r + i] = (float)(2.0 * a);
    else if (i < K) g_const[s * dc + (i - r)] = (float)(2.0 * a);
}

// the d = 2 plain polynomial library of `order` (1-5, checked by the caller)
inline hipError_t launch_quad_reduce_order(int order, const double* aug, const double* mt, const float* jt, long S, const float* q,
                                           int r, int use_kron, int has_const, const float* mask, unsigned long long live,
                                           float w_sym, double inv, double* bout, hipStream_t st) {
    constexpr int NW = BLOCK / WAVE;
    const dim3 grid((unsigned)((S + NW - 1) / NW));
    switch (order) {
#define SYMODE_REDUCE_CASE(O)                                                                                                   \
    case O:                                                                                                                     \
        quad_reduce_kernel<Library<2, O, 0>><<<grid, dim3(BLOCK), 0, st>>>(aug, mt, jt, S, q, r, use_kron, has_const, mask, live, \
                                                                           w_sym, inv, bout);                                   \
        break;
        SYMODE_REDUCE_CASE(1) SYMODE_REDUCE_CASE(2) SYMODE_REDUCE_CASE(3) SYMODE_REDUCE_CASE(4) SYMODE_REDUCE_CASE(5)
#undef SYMODE_REDUCE_CASE
        default: return hipErrorInvalidValue;
    }
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

inline hipError_t launch_quad_step(int order, unsigned long long live, const double* bt, long S, int K, int dc, const float* beta,
                                   long ldb, const float* cst, long ldc, float* loss, float* g_beta, float* g_const, double* ws,
                                   hipStream_t st) {
    unsigned long long body = 0;                            // what closure_quad_kernel of the same library and column set leaves
    switch (order) {
#define SYMODE_STEP_CASE(O) case O: body = closure_quad_body<Library<2, O, 0>>(live); break;
        SYMODE_STEP_CASE(1) SYMODE_STEP_CASE(2) SYMODE_STEP_CASE(3) SYMODE_STEP_CASE(4) SYMODE_STEP_CASE(5)
#undef SYMODE_STEP_CASE
        default: return hipErrorInvalidValue;
    }
    quad_step_kernel<<<dim3((unsigned)((S + REDUCED_PER_BLOCK - 1) / REDUCED_PER_BLOCK)), dim3(BLOCK), 0, st>>>(
        bt, S, K, dc, beta, ldb, cst, ldc, loss, g_beta, g_const, (unsigned long long*)ws, body | WS_BODY_FOLD_REDUCED);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
