// The fused reversed closure under a linear action WITHOUT a point loop (symode_loss_grad_reversed_linear_quad; only capi.hip
// includes this header).  closure_fold.hpp's Gram form takes the regulariser from G = sum_n Theta Theta^T; the rows and columns
// of the augmented matrix [Gtt Gty; Gty^T Gyy] = sum_n [Theta | dx]^T [Theta | dx] (symode_aug_gram) that it leaves out are what
// the residual needs:
//   sum_n |Xi Theta_n - dx_n|^2 = tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy),      R = sum_n r_n Theta_n^T = W Gtt - Gty^T,
// so a closure call reads 8 KB of fp64 tables per problem (order 5) instead of 16 bytes per point.  The regulariser is
// fold_gram_term (closure_fold.hpp), the statements of symreg_fold_kernel<FoldGram<..>>; the fold kernels' restrictions hold:
// d = 2, plain polynomial library, orders 1-5, one group element.
//
// One wave per problem.  Xi (as W, masked, dead columns 0), C, U, the fp64 gradient and beta sit in the wave's own rows of LDS
// in fp64; the stages are separated by workgroup barriers that every wave passes -- a wave past the last problem works on the
// last problem again and writes nothing.  Every load of G and of M in the products is a row segment along the lanes (G is
// symmetric: Gty is read as rows p.. of the matrix).  The columns are a run-time set (`live`): one instantiation per library.
//
// The coefficient map in the same launch (q != null): flat = Q beta in fp64, Xi its (d, p) view (use_kron) or the transposed
// (p, d) one, + const on column 0, rounded ONCE to fp32 -- from there on the kernel sees the fp32 Xi a caller of
// CoefMap.xi would have passed (written to xi_out when given) -- and on the way out g_beta = vec(grad) Q, g_const = grad[:, :, 0]
// from the fp64 gradient, rounded once.
#pragma once
#include <hip/hip_runtime.h>

#include "closure_fold.hpp"

namespace symode {

constexpr unsigned long long WS_BODY_FOLD_QUAD = 128;   // + no point loop: the residual from the augmented Gram (word WS_BODY_WORD)

struct QuadMap {              // the coefficient map's operands; q null: Xi is read from xi
    const float* q;           // (d p, r) fp32, row-major, rows in the order `use_kron` names
    const float* beta;        // (S, r), rows ldb floats apart
    const float* cst;         // (S, d), rows ldc floats apart, or null: the constant the model reads, added to column 0
    long ldb, ldc;
    int r, use_kron;
    float* xi_out;            // (S, d, p) or null
    float* g_beta;            // (S, r)
    float* g_const;           // (S, d) or null
};

template <class Lib>
__global__ __launch_bounds__(BLOCK) void closure_quad_kernel(const double* __restrict__ aug, const double* __restrict__ mt,
                                                             const float* __restrict__ jt, long S, const float* __restrict__ xi,
                                                             QuadMap map, const float* __restrict__ mask, unsigned long long live,
                                                             float w_sym, double inv, float* __restrict__ loss2,
                                                             float* __restrict__ loss, float* __restrict__ grad,
                                                             unsigned long long* header, unsigned long long body) {
    constexpr int D = Lib::D, P = Lib::P, DP = D * P, F = P + D, NACC = 2 + DP, NW = BLOCK / WAVE;
    static_assert(D == 2 && !Lib::SINE && !Lib::EXP, "the fold kernels' libraries");
    __shared__ double wsh[NW][DP], cd[NW][DP], ud[NW][DP], gd[NW][DP], bsh[NW][DP], row_add[NW][NACC];
    const int lane = threadIdx.x % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long s_own = (long)blockIdx.x * NW + wave;
    const bool act = s_own < S;
    const long s = act ? s_own : S - 1;
    const float* js = jt + s * D * D;
    const double* ms = mt + s * P * P;
    const double* gs = aug + s * (long)F * F;
    double* W = wsh[wave];
    if (blockIdx.x == 0 && threadIdx.x == 0 && header != nullptr && header[0] == WS_MAGIC) header[WS_BODY_WORD] = body;

    // Xi, masked as the fold kernel's wv() reads it
    if (map.q != nullptr) {
        for (int i = lane; i < map.r; i += WAVE) bsh[wave][i] = (double)map.beta[s * map.ldb + i];
    }
    __syncthreads();
    for (int o = lane; o < DP; o += WAVE) {
        const int j = o / P, k = o % P;
        float v;
        if (map.q != nullptr) {
            const float* qr = map.q + (long)(map.use_kron ? o : k * D + j) * map.r;
            double f = 0.0;
            for (int i = 0; i < map.r; ++i) f = __builtin_fma((double)qr[i], bsh[wave][i], f);
            if (map.cst != nullptr && k == 0) f += (double)map.cst[s * map.ldc + j];
            v = (float)f;
            if (act && map.xi_out != nullptr) map.xi_out[s * DP + o] = v;
        } else {
            v = xi[s * DP + o];
        }
        if (mask != nullptr) v *= mask[s * DP + o];
        W[o] = ((live >> k) & 1ull) != 0 ? (double)v : 0.0;
    }
    __syncthreads();

    // the regulariser: C = J Xi - Xi M, then U = C G, the value and w_sym T (row_add), as in symreg_fold_kernel's Gram form
    for (int t = lane; t < DP; t += WAVE)
        cd[wave][t] = fold_c<D, P>(t / P, t % P, js, ms, [&](int b, int l) -> double { return W[b * P + l]; });
    fold_gram_term<D, P, ~0ull, WAVE, F>(lane, lane == WAVE - 1, js, ms, gs, live, w_sym, cd[wave], ud[wave], row_add[wave],
                                         [] { __syncthreads(); });

    // the residual: R = W Gtt - Gty^T and the three traces
    double lsum = 0.0;
    const double two_inv = 2.0 * inv;
    for (int o = lane; o < DP; o += WAVE) {
        const int j = o / P, a = o % P;
        double wg = 0.0;                                    // (W Gtt)[j, a]
        for (int b = 0; b < P; ++b) wg = __builtin_fma(W[j * P + b], gs[b * F + a], wg);
        const double gty = gs[(P + j) * F + a];
        lsum = __builtin_fma(W[o], wg - 2.0 * gty, lsum);
        double g = two_inv * ((wg - gty) + row_add[wave][2 + o]);
        if (mask != nullptr) g *= (double)mask[s * DP + o];
        if (((live >> a) & 1ull) == 0) g = 0.0;
        gd[wave][o] = g;
        if (act) grad[s * DP + o] = (float)g;
    }
    if (lane < D) lsum += gs[(P + lane) * F + P + lane];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off /= 2) lsum += __shfl_xor(lsum, off, WAVE);
    if (act && lane == 0) {
        const double mse = inv * lsum, reg = inv * row_add[wave][1];
        loss2[2 * s] = (float)mse;
        loss2[2 * s + 1] = (float)reg;
        if (loss != nullptr) loss[s] = (float)(mse + (double)w_sym * reg);
    }
    __syncthreads();

    // the map's transpose on the fp64 gradient
    if (map.q != nullptr && act) {
        for (int i = lane; i < map.r; i += WAVE) {
            double gb = 0.0;
            for (int o = 0; o < DP; ++o) {
                const int row = map.use_kron ? o : (o % P) * D + o / P;
                gb = __builtin_fma(gd[wave][o], (double)map.q[(long)row * map.r + i], gb);
            }
            map.g_beta[s * map.r + i] = (float)gb;
        }
        if (map.g_const != nullptr && lane < D) map.g_const[s * D + lane] = (float)gd[wave][lane * P];
    }
}

// the header word of the fold kernel of the same column set (closure_fold.hpp: launch_symreg_fold), Gram form, + the new bit
template <class Lib>
unsigned long long closure_quad_body(unsigned long long live) {
    bool sparse = false;
    if constexpr (closure_fold_live_pays<Lib>) {
        constexpr unsigned long long columns = Lib::P >= 64 ? ~0ull : (1ull << Lib::P) - 1;
        sparse = knobs().closure_live && (live & columns & ~odd_degree_columns<Lib>()) == 0;
    }
    return WS_BODY_FOLD | (sparse ? WS_BODY_LIVE : 0ull) | WS_BODY_FOLD_GRAM | WS_BODY_FOLD_QUAD;
}

template <class Lib>
hipError_t launch_closure_quad(const double* aug, const double* mt, const float* jt, long S, const float* xi, const QuadMap& map,
                               const float* mask, unsigned long long live, float w_sym, double inv, float* loss2, float* loss,
                               float* grad, double* ws, hipStream_t st) {
    constexpr int NW = BLOCK / WAVE;
    const unsigned long long body = closure_quad_body<Lib>(live);
    closure_quad_kernel<Lib><<<dim3((unsigned)((S + NW - 1) / NW)), dim3(BLOCK), 0, st>>>(
        aug, mt, jt, S, xi, map, mask, live, w_sym, inv, loss2, loss, grad, (unsigned long long*)ws, body);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

// the d = 2 plain polynomial library of `order` (1-5, checked by the caller)
inline hipError_t launch_closure_quad_order(int order, const double* aug, const double* mt, const float* jt, long S, const float* xi,
                                            const QuadMap& map, const float* mask, unsigned long long live, float w_sym, double inv,
                                            float* loss2, float* loss, float* grad, double* ws, hipStream_t st) {
    switch (order) {
#define SYMODE_QUAD_CASE(O) \
    case O: return launch_closure_quad<Library<2, O, 0>>(aug, mt, jt, S, xi, map, mask, live, w_sym, inv, loss2, loss, grad, ws, st);
        SYMODE_QUAD_CASE(1) SYMODE_QUAD_CASE(2) SYMODE_QUAD_CASE(3) SYMODE_QUAD_CASE(4) SYMODE_QUAD_CASE(5)
#undef SYMODE_QUAD_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace symode
