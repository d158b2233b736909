// S4: reversed symmetry regulariser with precomputed (g(x), J_g(x))
//   u = J_g(x) h(x) - h(g(x));  loss = sum_g mean(u^2);
//   dloss/dXi[j,k] = (2/(N D)) sum ( (J_g^T u)_j th_k(x) - u_j th_k(g x) ).
// Batched like K1: problem s = blockIdx.y owns x[s] (N, D), gx[s] (n_g, N, D), jgx[s] (n_g, N, D, D), xi[s], mask[s].
// A pure stream (8 + n_g * 24 bytes per point at D = 2, each read once): every operand arrives as non-temporal
// 16-byte vectors -- a chunk of PPT points is one vector of x, one of g(x) and PPT*D*D/4 consecutive vectors of J_g --
// and a step issues the loads of two chunks before the arithmetic of either.
#pragma once
#include "kernels.hpp"

namespace symode {

template <int D>
struct JChunk {
    static constexpr int NV = Chunk<D>::PPT * D * D / 4;              // dwordx4 per chunk of Jacobians
    static_assert(Chunk<D>::PPT * D * D == NV * 4, "Jacobian chunk must be whole 16-byte vectors");
};

// a chunk of J_g as it was streamed -> the matrix of each of its points
template <int D>
__device__ __forceinline__ void unpack_j(const float4 (&vj)[JChunk<D>::NV], float (&J)[Chunk<D>::PPT][D * D]) {
    constexpr int NVJ = JChunk<D>::NV;
    float jf[NVJ * 4];
#pragma unroll
    for (int i = 0; i < NVJ; ++i) {
        jf[4 * i + 0] = vj[i].x;
        jf[4 * i + 1] = vj[i].y;
        jf[4 * i + 2] = vj[i].z;
        jf[4 * i + 3] = vj[i].w;
    }
#pragma unroll
    for (int e = 0; e < Chunk<D>::PPT * D * D; ++e) J[e / (D * D)][e % (D * D)] = jf[e];
}

// d = fma(w.SEL broadcast to both halves, t, c) in one v_pk_fma_f32: op_sel / op_sel_hi pick half SEL of the first operand
// for the low / the high result.  Written out because the compiler, given the same thing as a shuffle of a uniform pair,
// makes a pair (w, w) of its own for every coefficient -- twice the SGPRs the kernel has.
template <int SEL, bool SGPR>
__device__ __forceinline__ float2v pk_fma_bcast(float2v w, float2v t, float2v c) {
    float2v d;
    if constexpr (SGPR) {
        if constexpr (SEL == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "s"(w), "v"(t), "v"(c));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0]" : "=v"(d) : "s"(w), "v"(t), "v"(c));
    } else {
        if constexpr (SEL == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "v"(w), "v"(t), "v"(c));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0]" : "=v"(d) : "v"(w), "v"(t), "v"(c));
    }
    return d;
}

// One point of the reversed closure between its group elements: x, the residual's target y (MSE form) and -- where the
// visitor keeps them, see symreg_reversed_kernel -- Theta(x), h(x) and the residual r.  References: the arrays themselves stay
// separate locals of the chunk or the point (one aggregate for all of them schedules differently).
template <int D, int P>
struct ClosurePoint {
    const float (&x)[D];
    const float (&y)[D];
    float (&th)[P];
    float (&h)[D];
    float (&r)[D];
};

// The symmetric part of one point against one group element, stated once for both bodies of symreg_reversed_kernel:
// u = J h(x) - h(g x), sum += u^2, jtu = J^T u -- in the MSE form w_sym J^T u + r, where r is the point's residual on the group
// element that carries it and zero on the others: the residual's gradient rides on the same Theta(x) products.
template <int D, bool MSE>
__device__ __forceinline__ void sym_uv(const float (&J)[D * D], const float (&h)[D], const float (&hg)[D], const float (&r)[D],
                                       float w_sym, float& sum, float (&u)[D], float (&jtu)[D]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        float t = -hg[a];
#pragma unroll
        for (int b = 0; b < D; ++b) t = fmaf(J[a * D + b], h[b], t);
        u[a] = t;
        sum = fmaf(t, t, sum);
    }
#pragma unroll
    for (int b = 0; b < D; ++b) {
        float t = 0.0f;
#pragma unroll
        for (int a = 0; a < D; ++a) t = fmaf(J[a * D + b], u[a], t);
        jtu[b] = MSE ? fmaf(w_sym, t, r[b]) : t;
    }
}

// MSE = true: the whole closure of the reversed-regulariser runs in ONE pass -- the residual r = h(x) - dx shares
// Theta(x) and h(x) with the regulariser, x is read once (40 instead of 16 + 32 bytes per point at D = 2, n_g = 1):
//   sums[0] = sum r^2, sums[1] = sum_g sum u^2,  grad = d( sums[0] + w_sym sums[1] ) / dXi  (both under the same 1/(N D)).
// CJ = true: J_g is the same matrix at every point of a (problem, group element) -- a linear or affine action, a frozen
// linear autoencoder -- and jgx is the compact (S, n_g, D, D) table: the D*D values are wave-uniform and live in SGPRs,
// nothing of J_g is streamed (24 instead of 40 bytes per point at D = 2, n_g = 1).  Same arithmetic in the same order on
// the same chunk-to-lane assignment as the materialised form: the results are bit-identical to it.
// MINW: waves per SIMD the register allocation has to leave room for (the launcher asks for 3 in the CJ form of the
// d = 2 polynomial libraries: left alone, the order-5 closure comes out at 169 VGPRs -- one over the 3-wave limit of 168 --
// although its ring slot is two vectors shorter; asked, it fits in 148 without scratch).
// PK (CJ form, D = 2): the packed-fp32 body.  The point's two library evaluations run as ONE on the pairs
// t[k] = (Theta_k(x), Theta_k(g x)): v_pk_mul_f32 for the monomials, one v_pk_fma_f32 per (j, k) for (h_j(x), h_j(g x)) with
// the pair (w[0][k], w[1][k]) as the coefficient operand and op_sel choosing j, and the gradient sums as pairs over the two
// equation rows, acc2[k] = fma((jtu_0, jtu_1), t[k].xx, fma(-(u_0, u_1), t[k].yy, acc2[k])) -- the halves of a full pair
// picked by op_sel, so no register is half used.  Every product and every sum is the one the scalar body forms, in its
// order: the results are bit-identical to it (and so to the materialised form).  Per point 19 + 42 + 42 packed
// instructions instead of 36 + 84 + 84 scalar ones; where that pays is in the launcher's table (launch_symreg_reversed).
// LIVE (CJ form): the library columns that may hold a coefficient, a compile-time set (col_live).  A column outside it costs
// nothing per point: its coefficients are not read, its two links of the h(x) / h(g x) chains, its gradient sums and its
// slots of acc2 / w2 are not formed -- the monomials stay, an even degree feeds the next odd one, and the compiler drops
// those nothing reads.  What a dead column contributes with a zero coefficient is fma(0, t, s) = s, so on coefficients
// that ARE zero there every live sum is the one the dense kernel forms, in its order, on its chunk-to-lane assignment:
// bit-identical.  The dead slots of acc stay zero; partial rows and finalise keep their layout.  `live` is the caller's
// own set, a subset of LIVE: the columns of LIVE outside it are read as zero and their gradient sums cleared, once per
// thread, so that the result depends on the caller's set alone and not on which instantiation served it.
template <class Lib, bool MSE, int RING = 2, int XI_SGPR_FROM = 32, bool CJ = false, int MINW = 1, bool PK = false,
          unsigned long long LIVE = ~0ull>
__global__ __launch_bounds__(BLOCK, MINW) void symreg_reversed_kernel(const float* __restrict__ x, const float* __restrict__ dx,
                                                                const float* __restrict__ gx,
                                                                const float* __restrict__ jgx, int n_g, long N, bool vec,
                                                                const float* __restrict__ xi,
                                                                const float* __restrict__ mask, float w_sym,
                                                                double* __restrict__ ws, Finish fin,
                                                                unsigned long long live = ~0ull) {
    vec = vec && chunked_stream<Lib>;            // (D = 3 sine / exp libraries: point by point, see chunked_stream)
    constexpr int D = Lib::D, P = Lib::P, NL = MSE ? 2 : 1, NACC = NL + D * P, PPT = Chunk<D>::PPT, NV = Chunk<D>::NV,
                  NVJ = JChunk<D>::NV, SYM0 = NL - 1;
    constexpr bool SPARSE = LIVE != ~0ull;
    static_assert(!PK || (CJ && D == 2), "the packed body pairs the two library evaluations of the constant-J form at d = 2");
    static_assert(!SPARSE || (CJ && P <= 64), "a column set is honoured in the constant-J forms, for libraries of up to 64 columns");
    const long s = blockIdx.y;
    const float* xs = x + s * N * D;
    const float* ys = MSE ? dx + s * N * D : nullptr;
    const float* gs = gx + s * (long)n_g * N * D;
    const float* js = jgx + s * (long)n_g * (CJ ? 1 : N) * D * D;
    float w[D * P];
    // two libraries per point live here: Xi in SGPRs from d*p = 32 (3 waves/SIMD at order 5) -- and up to 80, the d = 3
    // order-3 libraries with sine / exp columns (69-78 coefficients would otherwise sit in VGPRs beside 70-79 sums)
    load_xi<Lib, XI_SGPR_FROM, 80, LIVE>(xi, mask, s, w, SPARSE ? live : ~0ull);
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;
    const float ws_ = MSE ? w_sym : 1.0f;
    // (an initialised workspace only: one that never saw symode_workspace_init is left as it was found)
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && fin.header[0] == WS_MAGIC)
        fin.header[WS_BODY_WORD] = (PK ? WS_BODY_PACKED : WS_BODY_SCALAR) | (SPARSE ? WS_BODY_LIVE : 0ull);
    // CJ: the matrix of group element g, wave-uniform (scalar loads; readfirstlane pins the values to SGPRs)
    auto load_cj = [&](int g, float (&J)[D * D]) {
#pragma unroll
        for (int e = 0; e < D * D; ++e)
            J[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, js[(long)g * D * D + e])));
    };
    float J0[D * D];                                 // (CJ) group element 0, loaded once per workgroup
#pragma unroll
    for (int e = 0; e < D * D; ++e) J0[e] = 0.0f;
    if constexpr (CJ) {
        if (n_g > 0) load_cj(0, J0);
    }

    // one point against one group element: th, h belong to x (shared by all group elements of the point);
    // `extra` (MSE form, first group element only) is the residual r
    auto one = [&](const float (&th)[P], const float (&h)[D], const float (&gp)[D], const float (&J)[D * D], const float (&extra)[D]) {
        float thg[P], hg[D], u[D], jtu[D];
        Lib::eval(gp, thg);
        apply_xi<Lib, LIVE>(w, thg, hg);
        sym_uv<D, MSE>(J, h, hg, extra, ws_, acc[SYM0], u, jtu);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float uj = MSE ? ws_ * u[j] : u[j];
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (col_live<LIVE>(k)) acc[NL + j * P + k] = fmaf(jtu[j], th[k], fmaf(-uj, thg[k], acc[NL + j * P + k]));
        }
    };
    // residual of one point (MSE form): r = h - dx, sums[0] += r^2; returned for the first group element's `extra`
    auto resid = [&](const float (&h)[D], const float (&yp)[D], float (&r)[D]) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            r[j] = h[j] - yp[j];
            acc[0] = fmaf(r[j], r[j], acc[0]);
        }
    };
    // PK: one point against one group element, everything of the point formed here (a further group element forms
    // Theta(x), h(x) again in the low halves: the same bits); `first`: the group element that carries the residual.
    // The gradient sums live in acc2 (pair k = rows 0 and 1 of column k) and are unpacked into acc before emit_partials.
    // The coefficient pair w2[k] = (w[0][k], w[1][k]) is ONE operand (an SGPR pair where load_xi keeps Xi in SGPRs) and the
    // row is chosen by op_sel (pk_fma_bcast); h0 is the chain's first link, fma(w[j][0], Theta_0 = 1, 0), formed once.
    constexpr int P2 = PK ? P : 1;
    constexpr bool W_SGPR = D * P >= XI_SGPR_FROM && D * P <= 80;
    float2v acc2[P2], w2[P2], h0[D];
#pragma unroll
    for (int k = 0; k < P2; ++k) {
        acc2[k] = float2v{0.0f, 0.0f};
        w2[k] = PK ? float2v{w[k], w[(D - 1) * P + k]} : acc2[k];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const float s0 = fmaf(w[j * P], 1.0f, 0.0f);
        h0[j] = float2v{s0, s0};
    }
    auto one_pk = [&](const float (&xp)[D], const float (&gp)[D], const float (&J)[D * D], const float (&yp)[D], bool first) {
        float2v xx[D], t[P], hh[D];
#pragma unroll
        for (int a = 0; a < D; ++a) xx[a] = float2v{xp[a], gp[a]};
        Lib::eval_pair(xx, t);
        hh[0] = h0[0];
        hh[D - 1] = h0[D - 1];
#pragma unroll
        for (int k = 1; k < P; ++k)
            if (col_live<LIVE>(k)) {
                hh[0] = pk_fma_bcast<0, W_SGPR>(w2[k], t[k], hh[0]);
                hh[D - 1] = pk_fma_bcast<1, W_SGPR>(w2[k], t[k], hh[D - 1]);
            }
        float h[D], hg[D], r[D], u[D], jtu[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            h[j] = hh[j].x;
            hg[j] = hh[j].y;
            r[j] = 0.0f;
        }
        if constexpr (MSE) {
            if (first) resid(h, yp, r);
        }
        sym_uv<D, MSE>(J, h, hg, r, ws_, acc[SYM0], u, jtu);
        const float2v ja = float2v{jtu[0], jtu[D - 1]};
        const float2v ub = MSE ? float2v{-(ws_ * u[0]), -(ws_ * u[D - 1])} : float2v{-u[0], -u[D - 1]};
#pragma unroll
        for (int k = 0; k < P2; ++k)
            if (col_live<LIVE>(k))
                acc2[k] = __builtin_elementwise_fma(ja, __builtin_shufflevector(t[k], t[k], 0, 0),
                                                    __builtin_elementwise_fma(ub, __builtin_shufflevector(t[k], t[k], 1, 1), acc2[k]));
    };
    // A point against its group elements.  What is kept of the point from one group element to the next is the visitor's form,
    // fixed at compile time:
    //   CACHED  scalar body; Theta(x), h(x) and the residual r are formed once (prep) and shared by all group elements;
    //   REEVAL  scalar body; they are formed again for every group element (same values, same order of every sum): the
    //           chunks at D = 3, see chunk_all;
    //   PACKED  one_pk, which forms them in the low halves of its pairs.
    // `first`: this group element carries the residual (MSE form), a bool or a std::bool_constant; y is read in the MSE form
    // only.  r is zero until `aim` has formed a residual.
    enum Keep { CACHED, REEVAL, PACKED };
    using Pt = ClosurePoint<D, P>;
    auto prep = [&](auto keep, const Pt& p) {
        if constexpr (decltype(keep)::value == CACHED) {
            Lib::eval(p.x, p.th);
            apply_xi<Lib, LIVE>(w, p.th, p.h);
        }
    };
    // (MSE form) the residual's target y: consumed at once where r is kept, kept itself where r is formed per group element
    auto aim = [&](auto keep, const Pt& p) {
        if constexpr (decltype(keep)::value == CACHED) resid(p.h, p.y, p.r);
    };
    auto visit = [&](auto keep, const Pt& p, const float (&gp)[D], const float (&J)[D * D], auto first) {
        if constexpr (decltype(keep)::value == PACKED) {
            one_pk(p.x, gp, J, p.y, first);
        } else if constexpr (decltype(keep)::value == CACHED) {
            const float zero[D] = {};
            if (first)
                one(p.th, p.h, gp, J, p.r);
            else
                one(p.th, p.h, gp, J, zero);
        } else {
            float th[P], h[D], r[D];
            Lib::eval(p.x, th);
            apply_xi<Lib, LIVE>(w, th, h);
#pragma unroll
            for (int j = 0; j < D; ++j) r[j] = 0.0f;
            if constexpr (MSE) {
                if (first) resid(h, p.y, r);
            }
            one(th, h, gp, J, r);
        }
    };
    auto load_j = [&](const float* base, long c, float4 (&v)[NVJ]) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v* q = reinterpret_cast<const f4v*>(base) + c * NVJ;
#pragma unroll
        for (int i = 0; i < NVJ; ++i) {
            const f4v t = __builtin_nontemporal_load(q + i);
            v[i] = make_float4(t.x, t.y, t.z, t.w);
        }
    };
    // the per-point path: every operand of every group element by per-lane loads
    auto point = [&](long n) {
        constexpr std::integral_constant<Keep, PK ? PACKED : CACHED> keep{};
        float xp[D], yp[D], th[P], h[D], r[D];
        const Pt p{xp, yp, th, h, r};
        load_point<D>(xs, n, xp);
        prep(keep, p);
#pragma unroll
        for (int j = 0; j < D; ++j) r[j] = 0.0f;
        if constexpr (MSE) {
            load_point<D>(ys, n, yp);
            aim(keep, p);
        }
        for (int g = 0; g < n_g; ++g) {
            float gp[D], J[D * D];
            load_point<D>(gs + (long)g * N * D, n, gp);
            if constexpr (CJ) {
                load_cj(g, J);
            } else {
                const float* Jp = js + ((long)g * N + n) * D * D;
#pragma unroll
                for (int e = 0; e < D * D; ++e) J[e] = Jp[e];
            }
            if constexpr (PK) {
                visit(keep, p, gp, J, g == 0);
            } else {                                 // the cached body: the residual rides on the first group element
                const float zero[D] = {};
                if (g == 0)
                    one(th, h, gp, J, r);
                else
                    one(th, h, gp, J, zero);
            }
        }
    };

    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nthreads = (long)gridDim.x * BLOCK;
    // one chunk against every group element: the first one's operands came with the chunk (ring slot or tile), the later ones
    // are fetched here.  Theta(x), h(x) of the chunk's points are formed once and live only while its group elements are
    // visited -- except at D = 3, four points per chunk: Theta(x), h(x) of ALL of them (4 P + 12 registers) do not fit beside
    // the sums -- point by point instead, Theta(x) re-evaluated for every further group element (same values, same order of
    // every sum)
    auto chunk_all = [&](long c, const float4 (&vx)[NV], const float4 (&vy)[NV], const float4 (&vg)[NV], const float4 (&vj)[NVJ]) {
        constexpr std::integral_constant<Keep, PK ? PACKED : D == 3 ? REEVAL : CACHED> keep{};
        float xp[PPT][D], yp[PPT][D], th[PPT][P], h[PPT][D], r[PPT][D];
        auto pt = [&](auto i) { return Pt{xp[i], yp[i], th[i], h[i], r[i]}; };
        unpack_chunk<D>(vx, xp);
        each_point<PPT>([&](auto i) { prep(keep, pt(i)); });
#pragma unroll
        for (int i = 0; i < PPT; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) r[i][j] = 0.0f;
        if constexpr (MSE) {
            unpack_chunk<D>(vy, yp);
            each_point<PPT>([&](auto i) { aim(keep, pt(i)); });
        }
        // (`first` reaches the cached and the packed visitor as a compile-time constant -- `group` is instantiated per value --
        //  and the re-evaluating one as a flag of one `group`: the forms in which each body was generated before)
        auto flag = [&](auto b) {
            if constexpr (decltype(keep)::value == REEVAL)
                return bool(b);
            else
                return b;
        };
        auto group = [&](const float4 (&ug)[NV], const float4 (&uj)[NVJ], const float (&Jc)[D * D], auto first) {
            float gp[PPT][D], J[PPT][D * D];
            unpack_chunk<D>(ug, gp);
            if constexpr (!CJ) unpack_j<D>(uj, J);
            each_point<PPT>([&](auto i) {
                if constexpr (CJ)
                    visit(keep, pt(i), gp[i], Jc, first);
                else
                    visit(keep, pt(i), gp[i], J[i], first);
            });
        };
        group(vg, vj, J0, flag(std::true_type{}));
        for (int g = 1; g < n_g; ++g) {
            float4 ng[NV], nj[NVJ];
            float Jg[D * D];
            load_chunk_raw<D, true>(gs + (long)g * N * D, c, ng);
            if constexpr (CJ) {
                load_cj(g, Jg);
                group(ng, nj, Jg, flag(std::false_type{}));
            } else {
                load_j(js + (long)g * N * D * D, c, nj);
                group(ng, nj, J0, flag(std::false_type{}));
            }
        }
    };
    if constexpr (D == 3) {
        // 12-byte points and 36-byte Jacobians: whole waves fetch their tiles coalesced and redistribute through a
        // wave-private LDS slab (points.hpp, exchange_tile); ragged waves and the tail keep the per-lane loads
        if (vec && n_g > 0) {
            __shared__ float4 slab3[BLOCK / WAVE][(CJ ? NV : NVJ) * WAVE];
            const int lane = threadIdx.x & (WAVE - 1);
            float4* slab = slab3[threadIdx.x / WAVE];
            const long nchunks = N / PPT;
            for (long c = tid;; c += nthreads) {
                const bool in = c < nchunks;
                const unsigned long long live = __builtin_amdgcn_ballot_w64(in);
                if (live == 0ull) break;
                float4 ax[NV], ay[NV], ag[NV], aj[NVJ];
                if (live == ~0ull) {
                    const long c0 = c - lane;
                    float4 tx[NV], ty[NV], tg[NV], tj[NVJ];
                    load_tile_raw<NV, true>(xs, c0, lane, tx);
                    if constexpr (MSE) load_tile_raw<NV, true>(ys, c0, lane, ty);
                    load_tile_raw<NV, true>(gs, c0, lane, tg);
                    if constexpr (!CJ) load_tile_raw<NVJ, true>(js, c0, lane, tj);
                    exchange_tile<NV>(tx, ax, slab, lane);
                    if constexpr (MSE) exchange_tile<NV>(ty, ay, slab, lane);
                    exchange_tile<NV>(tg, ag, slab, lane);
                    if constexpr (!CJ) exchange_tile<NVJ>(tj, aj, slab, lane);
                } else if (in) {
                    load_chunk_raw<D, true>(xs, c, ax);
                    if constexpr (MSE) load_chunk_raw<D, true>(ys, c, ay);
                    load_chunk_raw<D, true>(gs, c, ag);
                    if constexpr (!CJ) load_j(js, c, aj);
                }
                if (in) chunk_all(c, ax, ay, ag, aj);
            }
            const long n = nchunks * PPT + tid;
            if (n < N) point(n);
        } else {
            for (long n = tid; n < N; n += nthreads) point(n);
        }
    } else if (vec && n_g > 0) {
        // register ring: RING chunks of x, (dx,) g(x), J_g of the first group element in flight per lane, a slot refilled
        // as soon as its chunk has been consumed (closure_ab: one 2^26-point problem 334 -> 325 us at order 3, the fused
        // closure at order 5 470 -> 442 us; the batched bench shape is VALU / HBM co-limited either way)
        constexpr int NVT = (MSE ? 3 : 2) * NV + (CJ ? 0 : NVJ), OY = NV, OG = (MSE ? 2 : 1) * NV, OJ = OG + NV;
        const long nchunks = N / PPT;
        chunk_ring<RING, NVT>(
            nchunks, tid, nthreads,
            [&](long q, float4 (&slot)[NVT]) {
                float4 tx[NV], tg[NV], tj[NVJ];
                load_chunk_raw<D, true>(xs, q, tx);
                load_chunk_raw<D, true>(gs, q, tg);
                if constexpr (!CJ) load_j(js, q, tj);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    slot[i] = tx[i];
                    slot[OG + i] = tg[i];
                }
                if constexpr (!CJ) {
#pragma unroll
                    for (int i = 0; i < NVJ; ++i) slot[OJ + i] = tj[i];
                }
                if constexpr (MSE) {
                    float4 ty[NV];
                    load_chunk_raw<D, true>(ys, q, ty);
#pragma unroll
                    for (int i = 0; i < NV; ++i) slot[OY + i] = ty[i];
                }
            },
            [&](long c, const float4 (&slot)[NVT]) {
                float4 ax[NV], ay[NV], ag[NV], aj[NVJ];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    ax[i] = slot[i];
                    ay[i] = MSE ? slot[OY + i] : slot[i];
                    ag[i] = slot[OG + i];
                }
                if constexpr (!CJ) {
#pragma unroll
                    for (int i = 0; i < NVJ; ++i) aj[i] = slot[OJ + i];
                }
                chunk_all(c, ax, ay, ag, aj);
            });
        const long n = nchunks * PPT + tid;
        if (n < N) point(n);
    } else {
        for (long n = tid; n < N; n += nthreads) point(n);
    }
    if constexpr (PK) {
#pragma unroll
        for (int k = 0; k < P; ++k) {
            acc[NL + k] = acc2[k].x;
            acc[NL + (D - 1) * P + k] = acc2[k].y;
        }
    }
    if constexpr (SPARSE) {
#pragma unroll
        for (int i = 0; i < D * P; ++i)
            if (col_live<LIVE>(i % P) && ((live >> (i % P)) & 1ull) == 0) acc[NL + i] = 0.0f;
    }
    emit_partials<NACC>(acc, ws, fin);
}

// Libraries whose constant-J closure takes the packed body (symreg_reversed_kernel, PK): where it measured faster on the
// MI355X at the bench shape (8192 x 125 000) in every pass, by more than the arms' own spread, and no slower at 64 x 50 000
// (tools/micro/closure_ab pk, three interleaved passes, packed / scalar time; profiles/closure_packed.txt has all twenty
// d = 2 libraries):
//   order 5           plain 0.980-0.981 / 0.98-1.00   sine 1.012-1.018 / 0.97-0.98   exp 0.897-0.900 / 0.88-0.89   both 0.937-0.944 / 0.90-0.91
//   order 4           plain 1.03-1.04 / 1.06-1.09     sine 1.05 / 1.05-1.06          exp 0.932-0.944 / 0.92-0.94   both 0.987-0.994 / 0.92-0.93
//   orders 1-3        0.95-1.14 at the bench shape (plain: 0.99-1.02, they stream at the HBM rate either way), 0.98-1.17 at the small
//                     one; the two that gain at the bench shape, exp alone at orders 2-3 (0.95-0.96), lose up to 8 % at the small one
// Sine columns alone lose or stay inside the spread at the bench shape at every order (the two sinf of a pair do not
// pack and the pair layout only costs); sine + exp at order 4 is inside the arms' 0.85 % spread there: all scalar.
// The order-5 plain library is the flagship's: its kernel falls from 5.40-5.44 to 5.29-5.33 ms, 2 %, although the
// vector instructions per point fall from 225 to 128 (counters): a packed instruction costs 4.6-4.8 cycles against 2.85-3.1,
// both bodies fill the vector pipe, and of the 8 % fewer cycles the kernel then takes 2 % arrive as time.  Below order 4
// the coefficients sit in VGPRs and the kernels are not issue-bound.
template <class Lib>
constexpr bool closure_pk_pays = Lib::D == 2 && ((Lib::ORDER == 5 && (Lib::EXP || !Lib::SINE)) || (Lib::ORDER == 4 && Lib::EXP && !Lib::SINE));

// The column set the sparse closures are instantiated for: the constant column and the whole odd degrees.  A planar field
// that commutes with the rotations has odd degrees only, so the constraint's Q holds nothing but SVD round-off (1e-7 against
// 0.2-0.4 in the live rows) in the even ones: degree 2 (columns 3-5), degree 4 (10-14) -- at order 5 the set is
// {0, 1, 2, 6-9, 15-20}, 13 of 21 columns.  A closed family, picked by the launcher: a run-time branch per column would put
// every two to four FMAs into a basic block of their own.
template <class Lib>
constexpr unsigned long long odd_degree_columns() {
    unsigned long long m = 1ull;
    for (int deg = 1; deg <= Lib::ORDER; deg += 2)
        for (int k = poly_terms(Lib::D, deg - 1); k < poly_terms(Lib::D, deg); ++k) m |= 1ull << k;
    return m;
}
// Libraries with a sparse instantiation: the d = 2 plain polynomial ones where the dense closure is bound by vector issue and
// not by the stream.  tools/micro/closure_ab live on the MI355X, fused closure, three interleaved passes, ms per launch at the
// bench shape (8192 x 125 000), and sparse / dense at 64 x 50 000 (profiles/closure_live.txt):
//   order 5   dense packed 5.37-5.39, dense scalar 5.48-5.52   sparse scalar 4.30-4.32   sparse packed 4.37-4.43   small 0.87-0.93
//   order 4   dense scalar 4.34-4.35, dense packed 4.50-4.52   sparse scalar 3.87-3.88   sparse packed 3.88-3.89   small 0.79-0.85
//   orders 1-3  dense 3.88-3.94, sparse 3.86-3.95: the stream floor either way -- no instantiation
// With the even degrees gone the SCALAR body is the faster one at order 5 in every pass (fewer instructions left to pack,
// and it needs no SGPR pairs), and no slower at order 4: the sparse launch always takes it.  Order 4 then sits on the
// stream floor of the orders 1-3; order 5 stays 10 % above it.
template <class Lib>
constexpr bool closure_live_pays = Lib::D == 2 && !Lib::SINE && !Lib::EXP && (Lib::ORDER == 4 || Lib::ORDER == 5);

// constj: jgx is the compact (S, n_g, D, D) table of a point-constant Jacobian (the CJ kernels, see symreg_reversed_kernel)
// live: the library columns that may hold a coefficient (bit k = column k, all ones: nothing known).  Where the set lies
// inside odd_degree_columns and the library has the instantiation, the constant-J launch takes the kernel that leaves the
// other columns out: their coefficients count as zero, their gradient comes back zero.  Any other set runs the dense kernel.
// SYMODE_CLOSURE_PK=0 keeps the scalar body everywhere, SYMODE_CLOSURE_LIVE=0 the dense kernels.  What a launch took is left
// in word 1 of the workspace header (WS_BODY_SCALAR / WS_BODY_PACKED, + WS_BODY_LIVE): the bodies are bit-identical, so
// nothing else tells them apart.
template <class Lib>
hipError_t launch_symreg_reversed(const float* x, const float* dx, const float* gxp, const float* jgx, bool constj, int n_g, long S,
                                  long n, const float* xi, const float* mask, unsigned long long live, float inv_count,
                                  float w_sym, float* loss, float* grad, double* ws, int gx, hipStream_t st) {
    constexpr int D = Lib::D;
    const bool mse = dx != nullptr;
    const int nacc = (mse ? 2 : 1) + D * Lib::P;
    double* part = ws + WS_HEADER_DOUBLES;
    Finish fin = make_finish(ws, mask, inv_count, 2.0f * inv_count, loss, grad);
    fin.n_loss = mse ? 2 : 1;
    // 16-byte vectors need every slab (problem, group element) to start on a 16-byte boundary
    // (the compact table of the CJ form is read by scalar loads: it takes no part in this)
    const bool multi = S > 1 || n_g > 1;
    const bool vec = ((uintptr_t)x % 16 == 0) && ((uintptr_t)gxp % 16 == 0) && (constj || (uintptr_t)jgx % 16 == 0) &&
                     (!mse || (uintptr_t)dx % 16 == 0) && (!multi || ((n * D) % 4 == 0 && (constj || (n * D * D) % 4 == 0)));
    const dim3 grid(gx, (unsigned)S), block(BLOCK);
    // the kernel family: CJ, the body and the column set as compile-time constants
    const auto launch = [&](auto cj, auto pk, auto sparse) {
        constexpr bool CJ = decltype(cj)::value, PK = decltype(pk)::value;
        constexpr int MINW = (CJ && D == 2 && !Lib::SINE && !Lib::EXP) ? 3 : 1;
        constexpr unsigned long long LIVE = decltype(sparse)::value ? odd_degree_columns<Lib>() : ~0ull;
        if (mse)
            symreg_reversed_kernel<Lib, true, 2, 32, CJ, MINW, PK, LIVE><<<grid, block, 0, st>>>(x, dx, gxp, jgx, n_g, n, vec, xi, mask,
                                                                                               w_sym, part, fin, live);
        else
            symreg_reversed_kernel<Lib, false, 2, 32, CJ, MINW, PK, LIVE><<<grid, block, 0, st>>>(x, nullptr, gxp, jgx, n_g, n, vec, xi,
                                                                                                mask, 1.0f, part, fin, live);
    };
    const bool pk = closure_pk_pays<Lib> && constj && knobs().closure_pk;
    bool sparse = false;
    if constexpr (closure_live_pays<Lib>) {
        constexpr unsigned long long columns = Lib::P >= 64 ? ~0ull : (1ull << Lib::P) - 1;
        sparse = constj && knobs().closure_live && (live & columns & ~odd_degree_columns<Lib>()) == 0;
    }
    if (sparse) {
        if constexpr (closure_live_pays<Lib>) launch(std::true_type{}, std::false_type{}, std::true_type{});
    } else if (pk) {
        if constexpr (closure_pk_pays<Lib>) launch(std::true_type{}, std::true_type{}, std::false_type{});
    } else if (constj) {
        launch(std::true_type{}, std::false_type{}, std::false_type{});
    } else {
        launch(std::false_type{}, std::false_type{}, std::false_type{});
    }
    SYMODE_LAUNCH_CHECK();
    return launch_finalize(fin, part, S, gx, nacc, st);
}

}  // namespace symode
