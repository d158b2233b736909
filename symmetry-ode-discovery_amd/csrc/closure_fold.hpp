// The fused reversed closure under a LINEAR group action: g(x) = J x with J constant over the points of a problem.
//
// For the plain polynomial libraries Theta(J x) = M Theta(x) with a p x p matrix M that depends on J alone and is block
// diagonal by degree (linear_action.hpp builds it, in fp64, once per data set).  Then, with h = Xi Theta,
//   h(g x) = (Xi M) Theta(x),      u = J h(x) - h(g x) = C Theta(x),   C = J Xi - Xi M   (d x p, once per problem and launch),
//   sum_n u_n Theta(g x_n)^T = (sum_n u_n Theta(x_n)^T) M^T = U M^T,
// so a point needs neither g(x) nor Theta(g x): the library is evaluated ONCE, the 2d x p block [Xi; C] is applied to it,
// and the residual's sums R = sum r Theta(x)^T and U are formed against the same Theta(x).  The gradient of
// mse + w_sym * regulariser is R + w_sym (J^T U - U M^T), formed once per thread before the partial rows go out -- as
// R + w_sym ((J - I)^T U - U (M - I)^T), with J - I and M - I rounded from fp64, so that a group element close to the
// identity costs no digits.  16 bytes per point (x, dx) instead of 24, one library evaluation instead of two.
// The partial rows keep the layout of symreg_reversed_kernel<.., MSE = true> (NACC = 2 + d p), emit_partials and finalise
// are its own.  The results are NOT bit-identical to the streamed kernels: g(x) is replaced by the exact image J x (the
// detector accepts a g(x) within 4 * 2^-24 of it, componentwise relative to sum |J| |x|) and u is formed from C, which is
// rounded once from fp64, instead of as the difference of two fp32 chains -- a smaller error where u is round-off.
#pragma once
#include "closure_rev.hpp"

namespace symode {

// degree block of column k of a d = 2 polynomial library: columns [fold_deg_lo(k), fold_deg_hi(k))
constexpr int fold_deg_hi(int k) {
    int g = 0;
    while (k >= (g + 1) * (g + 2) / 2) ++g;
    return (g + 1) * (g + 2) / 2;
}
constexpr int fold_deg_lo(int k) {
    int g = 0;
    while (k >= (g + 1) * (g + 2) / 2) ++g;
    return g * (g + 1) / 2;
}

// jt: the compact (S, 1, D, D) table of J; mt: (S, 1, P, P) fp64, M of each problem (row k: Theta_k(J x) in terms of Theta(x)).
// W_SGPR / C_SGPR: Xi / C in SGPRs.  LIVE, live: as in symreg_reversed_kernel -- the set is a union of whole degrees, so it is
// closed under M; a column of LIVE outside `live` has a zero coefficient and a zero gradient, its C is formed like any other.
template <class Lib, int RING, int MINW, unsigned long long LIVE, bool W_SGPR, bool C_SGPR>
__global__ __launch_bounds__(BLOCK, MINW) void symreg_fold_kernel(const float* __restrict__ x, const float* __restrict__ dx,
                                                                  const float* __restrict__ jt, const double* __restrict__ mt,
                                                                  long N, bool vec, const float* __restrict__ xi,
                                                                  const float* __restrict__ mask, float w_sym,
                                                                  double* __restrict__ ws, Finish fin, unsigned long long live) {
    constexpr int D = Lib::D, P = Lib::P, NACC = 2 + D * P, PPT = Chunk<D>::PPT, NV = Chunk<D>::NV;
    constexpr bool SPARSE = LIVE != ~0ull;
    static_assert(D == 2 && !Lib::SINE && !Lib::EXP, "Theta(J x) = M Theta(x) holds for the plain polynomial libraries; M is built for d = 2");
    __shared__ float cs[D * P], mm[P * P], jm[D * D];
    const long s = blockIdx.y;
    const float* xs = x + s * N * D;
    const float* ys = dx + s * N * D;
    const float* js = jt + s * D * D;
    const double* ms = mt + s * P * P;
    if (!SPARSE) live = ~0ull;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && fin.header[0] == WS_MAGIC)
        fin.header[WS_BODY_WORD] = WS_BODY_FOLD | (SPARSE ? WS_BODY_LIVE : 0ull);

    // C = J Xi - Xi M of this problem, fp64 products of the masked fp32 coefficients the streamed kernels read
    for (int t = threadIdx.x; t < D * P; t += BLOCK) {
        const int j = t / P, k = t % P;
        const auto wv = [&](int b, int l) -> double {
            if (!col_live<LIVE>(l) || ((live >> l) & 1ull) == 0) return 0.0;
            float v = xi[s * D * P + b * P + l];
            if (mask != nullptr) v *= mask[s * D * P + b * P + l];
            return (double)v;
        };
        double c = 0.0;
        for (int b = 0; b < D; ++b) c += (double)js[j * D + b] * wv(b, k);
        for (int l = fold_deg_lo(k); l < fold_deg_hi(k); ++l) c -= wv(j, l) * ms[l * P + k];
        cs[t] = (float)c;
    }
    for (int t = threadIdx.x; t < P * P; t += BLOCK) mm[t] = (float)(ms[t] - (t / P == t % P ? 1.0 : 0.0));
    if (threadIdx.x < D * D) jm[threadIdx.x] = (float)((double)js[threadIdx.x] - (threadIdx.x / D == threadIdx.x % D ? 1.0 : 0.0));
    __syncthreads();

    float w[D * P], c[D * P];
    load_xi<Lib, W_SGPR ? 1 : 1 << 20, 1 << 20, LIVE>(xi, mask, s, w, live);
#pragma unroll
    for (int i = 0; i < D * P; ++i) {
        c[i] = col_live<LIVE>(i % P) ? cs[i] : 0.0f;
        if constexpr (C_SGPR) {
            if (col_live<LIVE>(i % P)) c[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, c[i])));
        }
    }
    float sum_r = 0.0f, sum_u = 0.0f, R[D * P], U[D * P];
#pragma unroll
    for (int i = 0; i < D * P; ++i) R[i] = U[i] = 0.0f;

    auto one = [&](const float (&xp)[D], const float (&yp)[D]) {
        float th[P], h[D], u[D];
        Lib::eval(xp, th);
        apply_xi<Lib, LIVE>(w, th, h);
        apply_xi<Lib, LIVE>(c, th, u);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float r = h[j] - yp[j];
            sum_r = fmaf(r, r, sum_r);
            sum_u = fmaf(u[j], u[j], sum_u);
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (col_live<LIVE>(k)) {
                    R[j * P + k] = fmaf(r, th[k], R[j * P + k]);
                    U[j * P + k] = fmaf(u[j], th[k], U[j * P + k]);
                }
        }
    };
    auto point = [&](long n) {
        float xp[D], yp[D];
        load_point<D>(xs, n, xp);
        load_point<D>(ys, n, yp);
        one(xp, yp);
    };
    // the chunk-to-lane assignment of symreg_reversed_kernel: a grid-wide stride, the ragged tail point by point
    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nthreads = (long)gridDim.x * BLOCK;
    if (vec) {
        const long nchunks = N / PPT;
        chunk_ring<RING, 2 * NV>(
            nchunks, tid, nthreads,
            [&](long q, float4 (&slot)[2 * NV]) {
                float4 vx[NV], vy[NV];
                load_chunk_raw<D, true>(xs, q, vx);
                load_chunk_raw<D, true>(ys, q, vy);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    slot[i] = vx[i];
                    slot[NV + i] = vy[i];
                }
            },
            [&](long, const float4 (&slot)[2 * NV]) {
                float4 vx[NV], vy[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    vx[i] = slot[i];
                    vy[i] = slot[NV + i];
                }
                float xp[PPT][D], yp[PPT][D];
                unpack_chunk<D>(vx, xp);
                unpack_chunk<D>(vy, yp);
                each_point<PPT>([&](auto i) { one(xp[i], yp[i]); });
            });
        const long n = nchunks * PPT + tid;
        if (n < N) point(n);
    } else {
        for (long n = tid; n < N; n += nthreads) point(n);
    }

    // this thread's share of the gradient: R + w_sym ((J - I)^T U - U (M - I)^T)
    float acc[NACC];
    acc[0] = sum_r;
    acc[1] = sum_u;
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            float t = 0.0f;
            if (col_live<LIVE>(k)) {
#pragma unroll
                for (int a = 0; a < D; ++a) t = fmaf(jm[a * D + j], U[a * P + k], t);
#pragma unroll
                for (int l = fold_deg_lo(k); l < fold_deg_hi(k); ++l) t = fmaf(-mm[k * P + l], U[j * P + l], t);
                t = fmaf(w_sym, t, R[j * P + k]);
                if (SPARSE && ((live >> k) & 1ull) == 0) t = 0.0f;
            }
            acc[2 + j * P + k] = t;
        }
    emit_partials<NACC>(acc, ws, fin);
}

// Libraries with the fold kernels: the d = 2 plain polynomial ones, dense at every order and on odd_degree_columns where the
// streamed closure has its sparse instantiation (orders 4-5).
template <class Lib>
constexpr bool closure_fold_lib = Lib::D == 2 && !Lib::SINE && !Lib::EXP && Lib::ORDER >= 1 && Lib::ORDER <= 5;

// Where the launcher routes to them (SYMODE_CLOSURE_FOLD=0: nowhere), filled in from measurement as closure_pk_pays /
// closure_live_pays are.  tools/micro/closure_ab fold on the MI355X, three interleaved passes, fold / shipped streamed kernel,
// ms per launch at the bench shape (8192 x 125 000) and the ratio at 64 x 50 000 (profiles/closure_fold.txt):
//   orders 1-3 dense   streamed 3.93-3.99   fold 2.56-2.70   0.650-0.687   small 0.82-0.94
//   order 4 dense      streamed 4.31-4.33   fold 3.46-3.49   0.802-0.811   small 0.86-0.90
//   order 5 dense      streamed 5.36-5.40   fold 4.47-4.49   0.827-0.835   small 0.995-1.015 (25.8-26.1 against 25.4-26.1 us: inside the spread)
//   order 4 odd set    streamed 3.91        fold 2.59        0.662         small 0.90-0.95
//   order 5 odd set    streamed 4.25-4.29   fold 3.28-3.31   0.770-0.774   small 0.95-0.96
// Orders 1-3 and the odd set at order 4 sit on the 16-byte stream (6.3-6.4 TB/s); order 5 stays bound by vector issue.
// Four chunks in flight instead of two measured within 1 % either way (order 5 dense: 2.5 % slower): ring 2.
template <class Lib>
constexpr bool closure_fold_dense_pays = closure_fold_lib<Lib>;
template <class Lib>
constexpr bool closure_fold_live_pays = closure_fold_lib<Lib> && closure_live_pays<Lib>;

// The instantiations the launcher takes (tools/micro/closure_ab fold times the same ones): [Xi; C] in SGPRs from 2 d p = 32
// on, as the streamed closure keeps Xi; the register allocation is asked to leave room for three waves per SIMD, two for the
// dense kernel of order 5 (84 sums beside 84 coefficients: 167 VGPRs, 3 waves, no scratch, as it comes out).
template <class Lib>
constexpr bool fold_sgpr = 2 * Lib::D * Lib::P >= 32;
template <class Lib, bool SPARSE>
constexpr int fold_minw = (!SPARSE && Lib::D * Lib::P > 32) ? 2 : 3;

// does a call with this column set take a fold kernel?
template <class Lib>
bool fold_takes(unsigned long long live) {
    if (!knobs().closure_fold) return false;
    if constexpr (closure_fold_live_pays<Lib>) {
        constexpr unsigned long long columns = Lib::P >= 64 ? ~0ull : (1ull << Lib::P) - 1;
        if (knobs().closure_live && (live & columns & ~odd_degree_columns<Lib>()) == 0) return true;
    }
    return closure_fold_dense_pays<Lib>;
}

template <class Lib>
hipError_t launch_symreg_fold(const float* x, const float* dx, const float* jt, const double* mt, long S, long n, const float* xi,
                              const float* mask, unsigned long long live, float inv_count, float w_sym, float* loss, float* grad,
                              double* ws, int gx, hipStream_t st) {
    constexpr int D = Lib::D, DP = D * Lib::P;
    double* part = ws + WS_HEADER_DOUBLES;
    Finish fin = make_finish(ws, mask, inv_count, 2.0f * inv_count, loss, grad);
    fin.n_loss = 2;
    const bool vec = ((uintptr_t)x % 16 == 0) && ((uintptr_t)dx % 16 == 0) && (S == 1 || (n * D) % 4 == 0);
    const dim3 grid(gx, (unsigned)S), block(BLOCK);
    bool sparse = false;
    if constexpr (closure_fold_live_pays<Lib>) {
        constexpr unsigned long long columns = Lib::P >= 64 ? ~0ull : (1ull << Lib::P) - 1;
        sparse = knobs().closure_live && (live & columns & ~odd_degree_columns<Lib>()) == 0;
    }
    if (sparse) {
        if constexpr (closure_fold_live_pays<Lib>)
            symreg_fold_kernel<Lib, 2, fold_minw<Lib, true>, odd_degree_columns<Lib>(), fold_sgpr<Lib>, fold_sgpr<Lib>>
                <<<grid, block, 0, st>>>(x, dx, jt, mt, n, vec, xi, mask, w_sym, part, fin, live);
    } else {
        symreg_fold_kernel<Lib, 2, fold_minw<Lib, false>, ~0ull, fold_sgpr<Lib>, fold_sgpr<Lib>>
            <<<grid, block, 0, st>>>(x, dx, jt, mt, n, vec, xi, mask, w_sym, part, fin, live);
    }
    SYMODE_LAUNCH_CHECK();
    return launch_finalize(fin, part, S, gx, 2 + DP, st);
}

typedef hipError_t (*FoldFn)(const float*, const float*, const float*, const double*, long, long, const float*, const float*,
                             unsigned long long, float, float, float*, float*, double*, int, hipStream_t);
typedef bool (*FoldTakesFn)(unsigned long long);

template <class Lib>
constexpr FoldFn fold_launcher() {
    if constexpr (closure_fold_lib<Lib>)
        return &launch_symreg_fold<Lib>;
    else
        return nullptr;
}
template <class Lib>
constexpr FoldTakesFn fold_takes_fn() {
    if constexpr (closure_fold_lib<Lib>)
        return &fold_takes<Lib>;
    else
        return nullptr;
}

}  // namespace symode
