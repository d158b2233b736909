// The closure of the latent L-BFGS fit (train.py:647-661 + 689) as one streaming pass.
//
// With the autoencoder frozen, z = enc(x), dz = J_enc(x) dx and A_n = J_dec(z_n) are data; a thin QR A_n = Q_n B_n leaves
//   |A_n h - dx_n|^2 = |B_n h - y_n|^2 + const,   y_n = Q_n^T dx_n,
// so per point the closure is Theta(z) once, h = Theta(z)(Xi*mask)^T and two residuals
//   r_z = h - dz,   r_x = B h - y:
//   sums[0] = sum r_z^2,  sums[1] = sum r_x^2,  grad = d( sums[0] + w_pair sums[1] ) / dXi  (both under the same 1/(N D)),
//   dsums/dXi[j,k] = 2 sum_n ( r_z + w_pair B^T r_x )_j th_k(z_n).
// The same shape of work as the J_g(x) h(x) half of symreg_reversed_kernel (closure_rev.hpp) with one library evaluation per
// point instead of two, and the same traffic at D = 2: z 8, dz 8, B 16, y 8 bytes per point, each read once.
#pragma once
#include "closure_rev.hpp"
#include "kernels.hpp"

namespace symode {

// Batched like the reversed closure: problem s = blockIdx.y owns z[s], dz[s], y[s] (N, D), B[s] (N, D, D) row-major,
// xi[s], mask[s].  Every operand arrives as non-temporal 16-byte vectors -- a chunk of PPT points is one vector each of
// z, dz, y and PPT*D*D/4 consecutive vectors of B -- through the register ring (points.hpp, chunk_ring); D = 3 goes
// through the wave's coalesced-tile exchange.  Every lane visits its chunks in a fixed order and the partial rows are
// added in a fixed order (emit_partials): two launches on the same inputs give the same bits.
template <class Lib, int RING = 2, int MINW = 1>
__global__ __launch_bounds__(BLOCK, MINW) void latent_closure_kernel(const float* __restrict__ z, const float* __restrict__ dz,
                                                                    const float* __restrict__ B, const float* __restrict__ y,
                                                                    long N, bool vec, const float* __restrict__ xi,
                                                                    const float* __restrict__ mask, float w_pair,
                                                                    double* __restrict__ ws, Finish fin) {
    vec = vec && chunked_stream<Lib>;            // (D = 3 sine / exp libraries: point by point, see chunked_stream)
    constexpr int D = Lib::D, P = Lib::P, NACC = 2 + D * P, PPT = Chunk<D>::PPT, NV = Chunk<D>::NV, NVB = JChunk<D>::NV;
    const long s = blockIdx.y;
    const float* zs = z + s * N * D;
    const float* ds = dz + s * N * D;
    const float* ys = y + s * N * D;
    const float* bs = B + s * N * D * D;
    float w[D * P];
    // one library per point lives here (the reversed closure holds two): Xi stays in VGPRs up to VGPR_XI_MAX, beyond
    // that -- up to 80, the d = 3 order-3 libraries with sine / exp columns -- it goes to the scalar file
    load_xi<Lib, VGPR_XI_MAX + 1, 80>(xi, mask, s, w);
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;

    auto one = [&](const float (&zp)[D], const float (&dp)[D], const float (&yp)[D], const float (&Bp)[D * D]) {
        float th[P], h[D], rx[D], c[D];
        Lib::eval(zp, th);
        apply_xi<Lib>(w, th, h);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            c[j] = h[j] - dp[j];
            acc[0] = fmaf(c[j], c[j], acc[0]);
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            float t = -yp[a];
#pragma unroll
            for (int b = 0; b < D; ++b) t = fmaf(Bp[a * D + b], h[b], t);
            rx[a] = t;
            acc[1] = fmaf(t, t, acc[1]);
        }
#pragma unroll
        for (int b = 0; b < D; ++b) {
            float t = 0.0f;
#pragma unroll
            for (int a = 0; a < D; ++a) t = fmaf(Bp[a * D + b], rx[a], t);
            c[b] = fmaf(w_pair, t, c[b]);
        }
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int k = 0; k < P; ++k) acc[2 + j * P + k] = fmaf(c[j], th[k], acc[2 + j * P + k]);
    };
    auto point = [&](long n) {
        float zp[D], dp[D], yp[D], Bp[D * D];
        load_point<D>(zs, n, zp);
        load_point<D>(ds, n, dp);
        load_point<D>(ys, n, yp);
        load_point<D * D>(bs, n, Bp);
        one(zp, dp, yp, Bp);
    };
    auto load_b = [&](long c, float4 (&v)[NVB]) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v* q = reinterpret_cast<const f4v*>(bs) + c * NVB;
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const f4v t = __builtin_nontemporal_load(q + i);
            v[i] = make_float4(t.x, t.y, t.z, t.w);
        }
    };
    // the chunk's points, operands already in registers
    auto chunk = [&](const float4 (&vz)[NV], const float4 (&vd)[NV], const float4 (&vy)[NV], const float4 (&vb)[NVB]) {
        float zp[PPT][D], dp[PPT][D], yp[PPT][D], bf[NVB * 4], Bp[PPT][D * D];
        unpack_chunk<D>(vz, zp);
        unpack_chunk<D>(vd, dp);
        unpack_chunk<D>(vy, yp);
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            bf[4 * i + 0] = vb[i].x;
            bf[4 * i + 1] = vb[i].y;
            bf[4 * i + 2] = vb[i].z;
            bf[4 * i + 3] = vb[i].w;
        }
#pragma unroll
        for (int e = 0; e < PPT * D * D; ++e) Bp[e / (D * D)][e % (D * D)] = bf[e];
        each_point<PPT>([&](auto i) { one(zp[i], dp[i], yp[i], Bp[i]); });
    };

    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nthreads = (long)gridDim.x * BLOCK;
    if constexpr (D == 3) {
        // 12-byte points and 36-byte matrices: whole waves fetch their tiles coalesced and redistribute through a
        // wave-private LDS slab (points.hpp, exchange_tile); ragged waves and the tail keep the per-lane loads
        if (vec) {
            __shared__ float4 slab3[BLOCK / WAVE][NVB * WAVE];
            const int lane = threadIdx.x & (WAVE - 1);
            float4* slab = slab3[threadIdx.x / WAVE];
            const long nchunks = N / PPT;
            for (long c = tid;; c += nthreads) {
                const bool in = c < nchunks;
                const unsigned long long live = __builtin_amdgcn_ballot_w64(in);
                if (live == 0ull) break;
                float4 az[NV], ad[NV], ay[NV], ab[NVB];
                if (live == ~0ull) {
                    const long c0 = c - lane;
                    float4 tz[NV], td[NV], ty[NV], tb[NVB];
                    load_tile_raw<NV, true>(zs, c0, lane, tz);
                    load_tile_raw<NV, true>(ds, c0, lane, td);
                    load_tile_raw<NV, true>(ys, c0, lane, ty);
                    load_tile_raw<NVB, true>(bs, c0, lane, tb);
                    exchange_tile<NV>(tz, az, slab, lane);
                    exchange_tile<NV>(td, ad, slab, lane);
                    exchange_tile<NV>(ty, ay, slab, lane);
                    exchange_tile<NVB>(tb, ab, slab, lane);
                } else if (in) {
                    load_chunk_raw<D, true>(zs, c, az);
                    load_chunk_raw<D, true>(ds, c, ad);
                    load_chunk_raw<D, true>(ys, c, ay);
                    load_b(c, ab);
                }
                if (in) chunk(az, ad, ay, ab);
            }
            const long n = nchunks * PPT + tid;
            if (n < N) point(n);
        } else {
            for (long n = tid; n < N; n += nthreads) point(n);
        }
    } else if (vec) {
        // register ring: RING chunks of z, dz, y, B in flight per lane, a slot refilled as soon as its chunk has been consumed
        constexpr int NVT = 3 * NV + NVB, OD = NV, OY = 2 * NV, OB = 3 * NV;
        const long nchunks = N / PPT;
        chunk_ring<RING, NVT>(
            nchunks, tid, nthreads,
            [&](long q, float4 (&slot)[NVT]) {
                float4 tz[NV], td[NV], ty[NV], tb[NVB];
                load_chunk_raw<D, true>(zs, q, tz);
                load_chunk_raw<D, true>(ds, q, td);
                load_chunk_raw<D, true>(ys, q, ty);
                load_b(q, tb);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    slot[i] = tz[i];
                    slot[OD + i] = td[i];
                    slot[OY + i] = ty[i];
                }
#pragma unroll
                for (int i = 0; i < NVB; ++i) slot[OB + i] = tb[i];
            },
            [&](long, const float4 (&slot)[NVT]) {
                float4 az[NV], ad[NV], ay[NV], ab[NVB];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    az[i] = slot[i];
                    ad[i] = slot[OD + i];
                    ay[i] = slot[OY + i];
                }
#pragma unroll
                for (int i = 0; i < NVB; ++i) ab[i] = slot[OB + i];
                chunk(az, ad, ay, ab);
            });
        const long n = nchunks * PPT + tid;
        if (n < N) point(n);
    } else {
        for (long n = tid; n < N; n += nthreads) point(n);
    }
    emit_partials<NACC>(acc, ws, fin);
}

template <class Lib>
hipError_t launch_latent_closure(const float* z, const float* dz, const float* B, const float* y, long S, long n, const float* xi,
                                 const float* mask, float inv_count, float w_pair, float* loss2, float* grad, double* ws, int gx,
                                 hipStream_t st) {
    constexpr int D = Lib::D, NACC = 2 + D * Lib::P;
    double* part = ws + WS_HEADER_DOUBLES;
    Finish fin = make_finish(ws, mask, inv_count, 2.0f * inv_count, loss2, grad);
    fin.n_loss = 2;
    // 16-byte vectors need every problem's slab to start on a 16-byte boundary
    const bool vec = ((uintptr_t)z % 16 == 0) && ((uintptr_t)dz % 16 == 0) && ((uintptr_t)B % 16 == 0) && ((uintptr_t)y % 16 == 0) &&
                     (S == 1 || ((n * D) % 4 == 0 && (n * D * D) % 4 == 0));
    latent_closure_kernel<Lib><<<dim3(gx, (unsigned)S), dim3(BLOCK), 0, st>>>(z, dz, B, y, n, vec, xi, mask, w_pair, part, fin);
    SYMODE_LAUNCH_CHECK();
    return launch_finalize(fin, part, S, gx, NACC, st);
}

}  // namespace symode
