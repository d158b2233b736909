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

// The packed body's pairing of the live columns from 1 on, two to an aligned register pair in column order: the i-th of them,
// or -1 past the last (an odd count leaves the last pair half used).
template <unsigned long long LIVE, int P>
constexpr int fold_pair_col(int i) {
    int n = 0;
    for (int k = 1; k < P; ++k)
        if (col_live<LIVE>(k)) {
            if (n == i) return k;
            ++n;
        }
    return -1;
}
template <unsigned long long LIVE, int P>
constexpr int fold_pairs() {
    int n = 0;
    for (int k = 1; k < P; ++k) n += col_live<LIVE>(k) ? 1 : 0;
    return (n + 1) / 2;
}

// fma(t.SEL broadcast to both halves, b, c) in one v_pk_fma_f32 (pk_fma_bcast, closure_rev.hpp, with the broadcast operand a
// VGPR pair of two monomials): b a VGPR pair (the residual pair) or an SGPR pair (a coefficient pair).
// pk_fma_bcast_acc: in place, the result tied to the addend (a sum, a later link of a chain); pk_fma_bcast_first: a chain's
// first link, which reads the thread's constant first term and must not need a copy of it.
template <int SEL, bool SGPR>
__device__ __forceinline__ void pk_fma_bcast_acc(float2v t, float2v b, float2v& acc) {
    if constexpr (SGPR) {
        if constexpr (SEL == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(t), "s"(b));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(acc) : "v"(t), "s"(b));
    } else {
        if constexpr (SEL == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(t), "v"(b));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(acc) : "v"(t), "v"(b));
    }
}
template <bool SGPR>
__device__ __forceinline__ float2v pk_fma_bcast_first(float2v t, float2v b, float2v c) {
    float2v d;
    if constexpr (SGPR)
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "v"(t), "s"(b), "v"(c));
    else
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "v"(t), "v"(b), "v"(c));
    return d;
}

// The fold's ring with the chunk addressing off the vector pipe (SADDR): every lane of the launch takes chunk
// r * nthreads + tid in round r, so a round is ONE uniform offset -- advanced in SGPRs -- plus the lane's own constant 32-bit
// byte offset: the scalar and the vector offset of a buffer load.  The rounds in which every lane has a chunk are counted
// once, uniformly; the steady state refills without an index, a compare or a clamp per lane, and the last rounds -- the
// ragged one among them, where the lanes from `rem` on re-read the round's first chunk, in bounds, and use nothing -- are
// peeled.  The same chunks reach the same lanes in the same order as chunk_ring(nchunks, tid, nthreads, ..).
// load(q0, lc, slot): the loads of chunk q0 + lc, q0 uniform; use(slot).  Everything is counted in 32 bits: the launcher
// keeps chunk_ring where a problem does not fit (fold_saddr_fits).
template <int R, int NVTOT, typename Load, typename Use>
__device__ __forceinline__ void chunk_ring_uniform(unsigned nchunks, unsigned tid, unsigned nthreads, Load load, Use use) {
    if (nchunks == 0) return;
    const unsigned full = nchunks / nthreads, rem = nchunks - full * nthreads, rounds = full + (rem != 0 ? 1 : 0);
    const bool mine = tid < rem;
    float4 ring[R][NVTOT];
    auto fetch = [&](unsigned r, float4 (&slot)[NVTOT]) { load(r * nthreads, (r < full || mine) ? tid : 0u, slot); };
    each_point_static<0, R>([&](auto k) {
        if (k < rounds) fetch(k, ring[k]);
    });
    unsigned r = 0;
    for (; r + 2 * R <= full; r += R) {
        each_point_static<0, R>([&](auto k) {
            use(ring[k]);
            load((r + R + k) * nthreads, tid, ring[k]);
            __builtin_amdgcn_sched_barrier(0);           // as in chunk_ring: the refill stays behind its slot's use
        });
    }
    for (; r < rounds; r += R) {
        each_point_static<0, R>([&](auto k) {
            if (r + k < rounds) {
                if (r + k < full || mine) use(ring[k]);
                if (r + R + k < rounds) fetch(r + R + k, ring[k]);
            }
        });
    }
}

// jt: the compact (S, 1, D, D) table of J; mt: (S, 1, P, P) fp64, M of each problem (row k: Theta_k(J x) in terms of Theta(x)).
// W_SGPR / C_SGPR: Xi / C in SGPRs.  LIVE, live: as in symreg_reversed_kernel -- the set is a union of whole degrees, so it is
// closed under M; a column of LIVE outside `live` has a zero coefficient and a zero gradient, its C is formed like any other.
// PK: the packed-fp32 body over the two equation rows.  The monomials stay scalar, in Lib::eval's order, and sit two to an
// aligned register pair; the coefficients are the pairs (w[0][k], w[1][k]), (c[0][k], c[1][k]), the residual and the
// regulariser term the pairs (r_0, r_1), (u_0, u_1), the sums the pairs (R[0][k], R[1][k]), (U[0][k], U[1][k]).  Per live column
// four v_pk_fma_f32 with Theta_k broadcast to both halves by op_sel -- h2 += Theta_k w2_k, u2 += Theta_k c2_k,
// R2_k += Theta_k r2, U2_k += Theta_k u2 -- instead of eight v_fmac_f32; the constant column is a v_pk_add_f32 (fma(r, 1, R)
// = r + R).  Each half is the scalar body's fmaf on the same operands in the same order, sum r^2 and sum u^2 are the scalar
// body's: bit-identical to it on the same grid.  The pairs are unpacked once per thread before the recombination.
// SADDR: chunk_ring_uniform instead of chunk_ring, see there; the same chunk-to-lane assignment, bit-identical.
// The levers ride on the library type, so that a kernel without them keeps the name and the code it had:
// symreg_fold_kernel<FoldLevers<Lib, PK, SADDR>, ..> is the kernel of Lib with them, symreg_fold_kernel<Lib, ..> the one without.
template <class L, bool PK_, bool SADDR_>
struct FoldLevers : L {
    static constexpr bool FOLD_PK = PK_, FOLD_SADDR = SADDR_;
};
template <class L, class = void>
struct fold_levers {
    static constexpr bool pk = false, saddr = false;
};
template <class L>
struct fold_levers<L, std::void_t<decltype(L::FOLD_PK)>> {
    static constexpr bool pk = L::FOLD_PK, saddr = L::FOLD_SADDR;
};
//
// The Gram form (FoldGram<L>, GRAM below): the regulariser does not go through the points at all.  With G = sum_n Theta Theta^T
// of the problem (gt: the (S, 1, P, P) fp64 raw sums, a function of x alone, built once per data set),
//   sum_n |u_n|^2 = sum_j c_j G c_j^T,      U = sum_n u_n Theta^T = C G,
// so the point loop is the monomials, h = Xi Theta, r, sum r^2 and R += r Theta^T -- the statements above without every c, u
// and U: sum_r and R are the plain fold kernel's bits on the same grid.  Workgroup 0 of each problem forms C, U = C G, the
// value and T = (J - I)^T U - U (M - I)^T in fp64 (J - I, M - I not rounded to fp32) and adds value and w_sym T to ITS OWN
// partial row as the row is written, in double: once per problem whatever grid.x is, through whichever finalisation.  The
// other workgroups read neither M nor G; slot 1 of their rows is 0.  Same NACC, workspace layout and finalisation.
template <class L>
struct FoldGram : L {
    static constexpr bool FOLD_GRAM = true;
};
template <class L, class = void>
struct fold_gram {
    static constexpr bool value = false;
};
template <class L>
struct fold_gram<L, std::void_t<decltype(L::FOLD_GRAM)>> {
    static constexpr bool value = L::FOLD_GRAM;
};

// The regulariser's statements, stated once for symreg_fold_kernel and for the kernel without a point loop (closure_quad.hpp).
// fold_c: entry (j, k) of C = J Xi - Xi M in fp64; wv(b, l) is the masked coefficient as a double (0 in a dead column).
template <int D, int P, class WV>
__device__ __forceinline__ double fold_c(int j, int k, const float* js, const double* ms, const WV& wv) {
    double c = 0.0;
    for (int b = 0; b < D; ++b) c += (double)js[j * D + b] * wv(b, k);
    for (int l = fold_deg_lo(k); l < fold_deg_hi(k); ++l) c -= wv(j, l) * ms[l * P + k];
    return c;
}
// fold_gram_term: from cd = C (D x P, in LDS, written by the caller's threads before the call) the rows U = C G into ud, and
// into row_add slot 1 the value sum_j c_j G c_j^T and slots 2.. the share w_sym T of the gradient, T = (J - I)^T U - U (M - I)^T
// with J - I and M - I in fp64.  The caller's threads t0, t0 + STEP, .. share the D P entries, `last` names the one that adds
// the value up; gs: G of the problem, rows LDG doubles apart; sync(): the barrier between the stages (the first one makes cd
// visible, the last one row_add).
template <int D, int P, unsigned long long LIVE, int STEP, int LDG, class Sync>
__device__ __forceinline__ void fold_gram_term(int t0, bool last, const float* js, const double* ms,
                                               const double* gs, unsigned long long live, float w_sym,
                                               const double* cd, double* ud, double* row_add, Sync sync) {
    sync();
    // U = C G over the columns of LIVE, in column order
    for (int t = t0; t < D * P; t += STEP) {
        const int j = t / P, k = t % P;
        double u = 0.0;
        if (col_live<LIVE>(k))
            for (int l = 0; l < P; ++l)
                if (col_live<LIVE>(l)) u = __builtin_fma(cd[j * P + l], gs[l * LDG + k], u);
        ud[t] = u;
    }
    sync();
    // T = (J - I)^T U - U (M - I)^T over the degree block of the column, J - I and M - I in fp64; sum_j c_j G c_j^T
    for (int t = t0; t < D * P; t += STEP) {
        const int j = t / P, k = t % P;
        double v = 0.0;
        if (col_live<LIVE>(k) && ((live >> k) & 1ull) != 0) {
            for (int a = 0; a < D; ++a) v = __builtin_fma((double)js[a * D + j] - (a == j ? 1.0 : 0.0), ud[a * P + k], v);
            for (int l = fold_deg_lo(k); l < fold_deg_hi(k); ++l)
                v = __builtin_fma(-(ms[k * P + l] - (k == l ? 1.0 : 0.0)), ud[j * P + l], v);
            v *= (double)w_sym;
        }
        row_add[2 + t] = v;
    }
    if (last) {
        double v = 0.0;
        for (int t = 0; t < D * P; ++t) v = __builtin_fma(cd[t], ud[t], v);
        row_add[0] = 0.0;
        row_add[1] = v;
    }
    sync();
}

// One template for both forms: the plain kernel has the arguments (and so the name) it had, the Gram form takes gt, one more
// pointer, behind them -- the trailing pack is empty or that pointer.
template <class Lib, int RING, int MINW, unsigned long long LIVE, bool W_SGPR, bool C_SGPR, class... GT>
__global__ __launch_bounds__(BLOCK, MINW) void symreg_fold_kernel(const float* __restrict__ x, const float* __restrict__ dx,
                                                                  const float* __restrict__ jt, const double* __restrict__ mt,
                                                                  long N, bool vec, const float* __restrict__ xi,
                                                                  const float* __restrict__ mask, float w_sym,
                                                                  double* __restrict__ ws, Finish fin, unsigned long long live,
                                                                  GT... gtp) {
    constexpr bool PK = fold_levers<Lib>::pk, SADDR = fold_levers<Lib>::saddr, GRAM = fold_gram<Lib>::value;
    constexpr int D = Lib::D, P = Lib::P, NACC = 2 + D * P, PPT = Chunk<D>::PPT, NV = Chunk<D>::NV;
    constexpr bool SPARSE = LIVE != ~0ull;
    static_assert(sizeof...(GT) == (GRAM ? 1 : 0), "the Gram form, and it alone, takes the Gram table");
    static_assert(D == 2 && !Lib::SINE && !Lib::EXP, "Theta(J x) = M Theta(x) holds for the plain polynomial libraries; M is built for d = 2");
    __shared__ float cs[GRAM ? 1 : D * P], mm[GRAM ? 1 : P * P], jm[GRAM ? 1 : D * D];
    __shared__ double cd[GRAM ? D * P : 1], ud[GRAM ? D * P : 1], row_add[GRAM ? NACC : 1];
    const long s = blockIdx.y;
    const float* xs = x + s * N * D;
    const float* ys = dx + s * N * D;
    const float* js = jt + s * D * D;
    const double* ms = mt + s * P * P;
    if (!SPARSE) live = ~0ull;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && fin.header[0] == WS_MAGIC)
        fin.header[WS_BODY_WORD] = WS_BODY_FOLD | (SPARSE ? WS_BODY_LIVE : 0ull) | (PK ? WS_BODY_FOLD_PK : 0ull) |
                                   (SADDR ? WS_BODY_FOLD_SADDR : 0ull) | (GRAM ? WS_BODY_FOLD_GRAM : 0ull);

    // C = J Xi - Xi M of this problem, fp64 products of the masked fp32 coefficients the streamed kernels read; the Gram form
    // keeps it in fp64, and forms it in workgroup 0 of the problem alone (the condition is uniform over the workgroup)
    if (!GRAM || blockIdx.x == 0) {
        for (int t = threadIdx.x; t < D * P; t += BLOCK) {
            const int j = t / P, k = t % P;
            const auto wv = [&](int b, int l) -> double {
                if (!col_live<LIVE>(l) || ((live >> l) & 1ull) == 0) return 0.0;
                float v = xi[s * D * P + b * P + l];
                if (mask != nullptr) v *= mask[s * D * P + b * P + l];
                return (double)v;
            };
            const double c = fold_c<D, P>(j, k, js, ms, wv);
            if constexpr (GRAM)
                cd[t] = col_live<LIVE>(k) ? c : 0.0;
            else
                cs[t] = (float)c;
        }
    }
    if constexpr (GRAM) {
        // the regulariser of this problem: U = C G, sum_j c_j G c_j^T and T, left for this workgroup's partial row
        if (blockIdx.x == 0) {
            const double* gs = [](const double* g) { return g; }(gtp...) + s * P * P;
            fold_gram_term<D, P, LIVE, BLOCK, P>((int)threadIdx.x, threadIdx.x == BLOCK - 1, js, ms, gs, live, w_sym, cd, ud, row_add,
                                                 [] { __syncthreads(); });
        }
    } else {
        for (int t = threadIdx.x; t < P * P; t += BLOCK) mm[t] = (float)(ms[t] - (t / P == t % P ? 1.0 : 0.0));
        if (threadIdx.x < D * D) jm[threadIdx.x] = (float)((double)js[threadIdx.x] - (threadIdx.x / D == threadIdx.x % D ? 1.0 : 0.0));
        __syncthreads();
    }

    float w[D * P], c[D * P];
    load_xi<Lib, W_SGPR ? 1 : 1 << 20, 1 << 20, LIVE>(xi, mask, s, w, live);
#pragma unroll
    for (int i = 0; i < D * P; ++i) {
        c[i] = (!GRAM && col_live<LIVE>(i % P)) ? cs[GRAM ? 0 : i] : 0.0f;
        if constexpr (C_SGPR && !GRAM) {
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
        if constexpr (!GRAM) apply_xi<Lib, LIVE>(c, th, u);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float r = h[j] - yp[j];
            sum_r = fmaf(r, r, sum_r);
            if constexpr (!GRAM) sum_u = fmaf(u[j], u[j], sum_u);
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (col_live<LIVE>(k)) {
                    R[j * P + k] = fmaf(r, th[k], R[j * P + k]);
                    if constexpr (!GRAM) U[j * P + k] = fmaf(u[j], th[k], U[j * P + k]);
                }
        }
    };
    // PK: the same point on pairs over the two equation rows (see above); h0 / u0 are the chains' first links,
    // fma(w[j][0], Theta_0 = 1, 0), formed once
    constexpr int P2 = PK ? P : 1, NPAIR = fold_pairs<LIVE, P>();
    float2v R2[P2], U2[P2], w2[P2], c2[P2], h0 = float2v{0.0f, 0.0f}, u0 = h0;
#pragma unroll
    for (int k = 0; k < P2; ++k) {
        R2[k] = U2[k] = float2v{0.0f, 0.0f};
        w2[k] = PK ? float2v{w[k], w[(D - 1) * P + k]} : R2[k];
        c2[k] = PK ? float2v{c[k], c[(D - 1) * P + k]} : R2[k];
    }
    if constexpr (col_live<LIVE>(0)) {
        h0 = float2v{fmaf(w[0], 1.0f, 0.0f), fmaf(w[(D - 1) * P], 1.0f, 0.0f)};
        u0 = float2v{fmaf(c[0], 1.0f, 0.0f), fmaf(c[(D - 1) * P], 1.0f, 0.0f)};
    }
    auto one_pk = [&](const float (&xp)[D], float2v y2) {
        if constexpr (PK) {   // (the pair arrays have one slot in the scalar kernels)
            float th[P];
            Lib::eval(xp, th);
            // pair m of the monomials and the columns in its halves (b < 0: the last pair of an odd count, half used)
            auto pair = [&](auto m) {
                constexpr int a = fold_pair_col<LIVE, P>(2 * decltype(m)::value), b = fold_pair_col<LIVE, P>(2 * decltype(m)::value + 1);
                return float2v{th[a], th[b < 0 ? a : b]};
            };
            float2v h2 = h0, u2 = u0;
            each_point_static<0, NPAIR>([&](auto m) {
                constexpr int a = fold_pair_col<LIVE, P>(2 * decltype(m)::value), b = fold_pair_col<LIVE, P>(2 * decltype(m)::value + 1);
                const float2v t = pair(m);
                if constexpr (decltype(m)::value == 0) {
                    h2 = pk_fma_bcast_first<W_SGPR>(t, w2[a], h0);
                    if constexpr (!GRAM) u2 = pk_fma_bcast_first<C_SGPR>(t, c2[a], u0);
                } else {
                    pk_fma_bcast_acc<0, W_SGPR>(t, w2[a], h2);
                    if constexpr (!GRAM) pk_fma_bcast_acc<0, C_SGPR>(t, c2[a], u2);
                }
                if constexpr (b >= 0) {
                    pk_fma_bcast_acc<1, W_SGPR>(t, w2[b], h2);
                    if constexpr (!GRAM) pk_fma_bcast_acc<1, C_SGPR>(t, c2[b], u2);
                }
            });
            const float2v r2 = h2 - y2;
            sum_r = fmaf(r2.x, r2.x, sum_r);
            if constexpr (!GRAM) sum_u = fmaf(u2.x, u2.x, sum_u);
            sum_r = fmaf(r2.y, r2.y, sum_r);
            if constexpr (!GRAM) sum_u = fmaf(u2.y, u2.y, sum_u);
            if constexpr (col_live<LIVE>(0)) {
                R2[0] += r2;
                if constexpr (!GRAM) U2[0] += u2;
            }
            each_point_static<0, NPAIR>([&](auto m) {
                constexpr int a = fold_pair_col<LIVE, P>(2 * decltype(m)::value), b = fold_pair_col<LIVE, P>(2 * decltype(m)::value + 1);
                const float2v t = pair(m);
                pk_fma_bcast_acc<0, false>(t, r2, R2[a]);
                if constexpr (!GRAM) pk_fma_bcast_acc<0, false>(t, u2, U2[a]);
                if constexpr (b >= 0) {
                    pk_fma_bcast_acc<1, false>(t, r2, R2[b]);
                    if constexpr (!GRAM) pk_fma_bcast_acc<1, false>(t, u2, U2[b]);
                }
            });
        }
    };
    auto point = [&](long n) {
        float xp[D], yp[D];
        load_point<D>(xs, n, xp);
        load_point<D>(ys, n, yp);
        if constexpr (PK)
            one_pk(xp, float2v{yp[0], yp[D - 1]});
        else
            one(xp, yp);
    };
    // the chunk-to-lane assignment of symreg_reversed_kernel: a grid-wide stride, the ragged tail point by point
    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nthreads = (long)gridDim.x * BLOCK;
    if (vec) {
        const long nchunks = N / PPT;
        const auto use = [&](const float4 (&slot)[2 * NV]) {
            float4 vx[NV], vy[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                vx[i] = slot[i];
                vy[i] = slot[NV + i];
            }
            float xp[PPT][D], yp[PPT][D];
            unpack_chunk<D>(vx, xp);
            unpack_chunk<D>(vy, yp);
            each_point<PPT>([&](auto i) {
                if constexpr (PK)
                    one_pk(xp[i], float2v{yp[i][0], yp[i][D - 1]});
                else
                    one(xp[i], yp[i]);
            });
        };
        if constexpr (SADDR) {
            static_assert(NV == 1, "one 16-byte vector of x and one of dx per chunk");
            // one buffer descriptor per stream, over the problem's whole chunks (built from the kernel's arguments and
            // blockIdx.y alone: wave-uniform); the round's base is the scalar offset of the load, the lane's the vector one
            typedef float f4v __attribute__((ext_vector_type(4)));
            constexpr int NT_AUX = 2;
            const int bytes = (int)((unsigned)nchunks * 16u);
            const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xs), 0, bytes, 0x00020000);
            const auto ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ys), 0, bytes, 0x00020000);
            chunk_ring_uniform<RING, 2 * NV>(
                (unsigned)nchunks, (unsigned)tid, (unsigned)nthreads,
                [&](unsigned q0, unsigned lc, float4 (&slot)[2 * NV]) {
                    // (the whole vector is cast: a bit_cast of one element of the builtin's vector reads element 0 for each)
                    const f4v vx = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(lc * 16u), (int)(q0 * 16u), NT_AUX));
                    const f4v vy = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(ry, (int)(lc * 16u), (int)(q0 * 16u), NT_AUX));
                    slot[0] = make_float4(vx.x, vx.y, vx.z, vx.w);
                    slot[1] = make_float4(vy.x, vy.y, vy.z, vy.w);
                },
                use);
        } else {
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
                [&](long, const float4 (&slot)[2 * NV]) { use(slot); });
        }
        const long n = nchunks * PPT + tid;
        if (n < N) point(n);
    } else {
        for (long n = tid; n < N; n += nthreads) point(n);
    }

    if constexpr (PK) {
#pragma unroll
        for (int k = 0; k < P; ++k) {
            R[k] = R2[k].x;
            R[(D - 1) * P + k] = R2[k].y;
            U[k] = U2[k].x;
            U[(D - 1) * P + k] = U2[k].y;
        }
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
                if constexpr (GRAM) {
                    t = R[j * P + k];                    // (the regulariser's share is workgroup 0's, in double: row_add)
                } else {
#pragma unroll
                    for (int a = 0; a < D; ++a) t = fmaf(jm[GRAM ? 0 : a * D + j], U[a * P + k], t);
#pragma unroll
                    for (int l = fold_deg_lo(k); l < fold_deg_hi(k); ++l) t = fmaf(-mm[GRAM ? 0 : k * P + l], U[j * P + l], t);
                    t = fmaf(w_sym, t, R[j * P + k]);
                }
                if (SPARSE && ((live >> k) & 1ull) == 0) t = 0.0f;
            }
            acc[2 + j * P + k] = t;
        }
    if constexpr (GRAM) {
        const bool first = blockIdx.x == 0;
        emit_partials<NACC>(acc, ws, fin, [&](int k, double v) { return (first && k >= 1) ? v + row_add[k] : v; });
    } else {
        emit_partials<NACC>(acc, ws, fin);
    }
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

// The two levers on the fold body, per instantiation (SPARSE: the odd set), filled in from measurement: taken only where the
// arm wins in all three passes of tools/micro/closure_ab fold at the bench shape by more than the arms' own spread, and is not
// slower at 64 x 50 000 by more than the parent arm's spread there (2.8 % at order 5 on the odd set, 21.3-21.9 us; 3.6 % at
// order 4 dense, 19.6-20.3 us).
// SYMODE_FOLD_PK=0 keeps the parent's body and addressing everywhere, bit for bit (both levers are bit-identical to it anyway).
// What a launch took is left in word 1 of the workspace header (WS_BODY_FOLD_PK, WS_BODY_FOLD_SADDR beside WS_BODY_FOLD).
//   closure_fold_pk_pays     the packed body over the two equation rows (PK)
//   closure_fold_saddr_pays  the uniform ring, chunk addressing in SGPRs (SADDR)
// MI355X, ms per launch at the bench shape (8192 x 125 000), parent body | + SADDR | + PK | both, and the ratios to the parent
// body there and at 64 x 50 000 (profiles/closure_fold_pk.txt):
//   order 5 odd set   3.307-3.335 | 3.163-3.205 | 3.253-3.291 | 3.199-3.222   0.948-0.969 | 0.975-0.994 | 0.966-0.973   small 1.00-1.02 | 0.97-0.99 | 0.98-1.03
//   order 5 dense     4.480-4.492 | 4.421-4.447 | 4.331-4.360 | 4.255-4.291   0.987-0.993 | 0.964-0.973 | 0.950-0.958   small 0.98-0.99 | 0.93-0.94 | 0.93-0.95
//   order 4 dense     3.437-3.462 | 3.319-3.340 | 3.396-3.406 | 3.313-3.328   0.959-0.969 | 0.981-0.989 | 0.961-0.967   small 1.04-1.07 | 0.98-1.01 | 1.01-1.03
//   orders 1-3 dense, order 4 odd set: 0.995-1.037 in every arm, they sit on the 16-byte stream: nothing taken
// Order 5 on the odd set (the flagship's) takes the uniform ring alone: the packed body, 313 instead of 517 instructions in the
// steady-state block, is inside the parent arm's 0.85 % spread in two passes of three and adds nothing on top of the ring.  At
// 64 x 50 000 the ring is 0-2.3 % slower there (21.7-21.9 against 21.3-21.9 us), inside that arm's 2.8 % spread: taken.
// Order 5 dense takes both (each wins alone, together 4.2-5.0 %).  Order 4 dense takes neither: the ring's 3-4 % at the bench
// shape are 4.2-6.7 % lost at 64 x 50 000 (its prologue), beyond the 3.6 % spread; the packed body alone is 1.1-1.9 % against a
// spread of 0.7 %, too little to carry a kernel of its own.
template <class Lib, bool SPARSE>
constexpr bool closure_fold_pk_pays = closure_fold_lib<Lib> && Lib::ORDER == 5 && !SPARSE;
template <class Lib, bool SPARSE>
constexpr bool closure_fold_saddr_pays = closure_fold_lib<Lib> && Lib::ORDER == 5;
// The uniform ring addresses a problem's stream through a buffer descriptor with 32-bit byte offsets: the bytes of one
// problem's x (n * d * 4) must stay below 2^31, that is n < 2^28 points at d = 2 (and the lane's own offset, grid.x * BLOCK * 16,
// with them).  Beyond that the launch keeps chunk_ring's 64-bit per-lane indices -- the parent's kernel, the same bits.
template <int D>
inline bool fold_saddr_fits(long n, int gx) {
    return n * D * 4 < (1L << 31) && (long)gx * BLOCK * 16 < (1L << 31);
}

// The Gram form (FoldGram), per instantiation, by the same rule.  SYMODE_FOLD_GRAM=0: nowhere -- the call that brings a Gram
// table is the call without one, bit for bit; 2: every fold library (the tests reach the instantiations the table leaves out).
// tools/micro/closure_ab foldgram on the MI355X, three interleaved passes, ms per launch at the bench shape (8192 x 125 000):
// the fold kernel shipped for the instantiation | Gram form, plain | + SADDR | + PK | both, the ratio of the plain Gram form to
// the shipped kernel there and at 64 x 50 000 (profiles/closure_fold_gram.txt); the order-3 dense fold kernel of the same
// passes, the 16-byte floor so far, took 2.684-2.700:
//   order 5 odd set   3.173-3.195 | 2.591-2.597 | 2.588-2.593 | 2.620-2.631 | 2.612-2.622   0.812-0.817   small 0.83-0.86
//   order 5 dense     4.310-4.332 | 2.903-2.917 | 2.783-2.821 | 2.934-2.961 | 2.857-2.881   0.670-0.674   small 0.76-0.78
//   order 4 dense     3.477-3.500 | 2.571-2.573 | 2.571-2.577 | 2.584-2.590 | 2.584-2.593   0.735-0.740   small 0.79-0.80
//   order 3 dense     2.681-2.696 | 2.579-2.583 | 2.588-2.592 | 2.579-2.588 | 2.587-2.597   0.958-0.962   small 0.87-0.91
//   order 4 odd set   2.565-2.574 | 2.583-2.585 |     every arm 1.004-1.010 of the shipped kernel: not taken
// Taken where the issue expected it and, by the same rule, at order 3 dense: 3.8-4.2 % in every pass against spreads of 0.6 %
// (shipped) and 0.2 % (Gram), 9-13 % at 64 x 50 000.  Every taken form is at 2.57-2.60 ms, 6.3-6.4 TB/s of its 16 B/point,
// but the dense one of order 5 (5.6 TB/s).  Orders 1-2: not measured, the plain kernels stay.
// No lever: on the Gram form the uniform ring is inside 0.2 % at the bench shape except at order 5 dense (3-4 %), and there it
// is 5-6 % slower at 64 x 50 000 (21.1-21.2 against 19.8-20.0 us, a spread of 1 %); the packed body loses everywhere; four
// chunks in flight are within 0.5 % of two.  So the Gram form has ONE instantiation per library and column set.
template <class Lib, bool SPARSE>
constexpr bool closure_fold_gram_pays = closure_fold_lib<Lib> && (Lib::ORDER == 5 || (Lib::ORDER >= 3 && !SPARSE));
// half the sums and no C: three waves per SIMD asked for every instantiation
constexpr int fold_gram_minw = 3;
template <class Lib>
bool fold_gram_takes(bool sparse) {
    const int knob = knobs().fold_gram;
    if (knob == 0) return false;
    if (knob == 2) return true;
    return sparse ? closure_fold_gram_pays<Lib, true> : closure_fold_gram_pays<Lib, false>;
}

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

// gt: the (S, 1, P, P) fp64 Gram table of the library on x, or null; with it the launch takes the Gram form where
// fold_gram_takes says so (one kernel per library and column set, without the levers), the plain kernel otherwise.
template <class Lib>
hipError_t launch_symreg_fold(const float* x, const float* dx, const float* jt, const double* mt, const double* gt, long S, long n,
                              const float* xi, const float* mask, unsigned long long live, float inv_count, float w_sym, float* loss,
                              float* grad, double* ws, int gx, hipStream_t st) {
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
    // the column set as a compile-time constant; the levers of the table where SYMODE_FOLD_PK allows them and the uniform ring's
    // bounds hold (fold_saddr_fits), the parent's kernel -- the same bits -- otherwise
    const auto launch = [&](auto sp) {
        constexpr bool SPARSE = decltype(sp)::value, PKB = closure_fold_pk_pays<Lib, SPARSE>, SA = closure_fold_saddr_pays<Lib, SPARSE>;
        constexpr unsigned long long LIVE = SPARSE ? odd_degree_columns<Lib>() : ~0ull;
        if (gt != nullptr && fold_gram_takes<Lib>(SPARSE)) {
            symreg_fold_kernel<FoldGram<Lib>, 2, fold_gram_minw, LIVE, fold_sgpr<Lib>, fold_sgpr<Lib>>
                <<<grid, block, 0, st>>>(x, dx, jt, mt, n, vec, xi, mask, w_sym, part, fin, live, gt);
            return;
        }
        if constexpr (PKB || SA) {
            if (knobs().fold_pk && (!SA || fold_saddr_fits<D>(n, gx))) {
                symreg_fold_kernel<FoldLevers<Lib, PKB, SA>, 2, fold_minw<Lib, SPARSE>, LIVE, fold_sgpr<Lib>, fold_sgpr<Lib>>
                    <<<grid, block, 0, st>>>(x, dx, jt, mt, n, vec, xi, mask, w_sym, part, fin, live);
                return;
            }
        }
        symreg_fold_kernel<Lib, 2, fold_minw<Lib, SPARSE>, LIVE, fold_sgpr<Lib>, fold_sgpr<Lib>>
            <<<grid, block, 0, st>>>(x, dx, jt, mt, n, vec, xi, mask, w_sym, part, fin, live);
    };
    if (sparse) {
        if constexpr (closure_fold_live_pays<Lib>) launch(std::true_type{});
    } else {
        launch(std::false_type{});
    }
    SYMODE_LAUNCH_CHECK();
    return launch_finalize(fin, part, S, gx, 2 + DP, st);
}

typedef hipError_t (*FoldFn)(const float*, const float*, const float*, const double*, const double*, long, long, const float*, const float*,
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
