// A/B harness for the closure kernels (tuning runs, not product code): loss_grad and the fused residual + reversed
// regulariser closure straight from csrc/kernels.hpp and csrc/closure_rev.hpp, one big problem (S = 1, 2^26 points) and the
// bench's batched shape (8192 x 125 000 points), over launch widths and ring depths -- one process, so variants see the same box.  (The run
// kept as profiles/r03_closure_ab.txt also held the two-chunk form the ring replaced: ring=0 there; the problem-walking
// form of the closure measured in profiles/r03_closure_walk.txt lives in commit becc803 only.)
// `closure_ab constj`: only the ring-depth A/B of the constant-Jacobian form of the fused closure (24 B/point) at the
// bench's batched shape, beside the materialised form (40 B/point), three interleaved passes.
// `closure_ab pk`: scalar body against the packed-fp32 body (PK) of the constant-Jacobian fused closure for the d = 2
// libraries, at the bench's batched shape and at 64 x 50 000, on the launcher's grids, three interleaved passes.  The
// launcher's table (closure_rev.hpp, closure_pk_pays) is read off this run.
// `closure_ab live`: every column against the constant + odd-degree column set (LIVE) of the constant-Jacobian fused closure
// for the d = 2 plain libraries, both bodies at orders 4-5, same shapes and passes.  closure_live_pays is read off this run.
// `closure_ab fold`: the fold kernel of a linear action (closure_fold.hpp: x and dx alone, 16 B/point, one library evaluation)
// against the kernel the launcher ships for the same call, d = 2 plain orders 1-5 on every column and on the constant +
// odd-degree set at orders 4-5, same shapes and passes; beside the parent fold body its two levers alone and together (the
// uniform ring with the chunk addressing in SGPRs, the packed body over the two equation rows) and grid.x = 1 beside the
// launcher's width.  closure_fold_dense_pays / closure_fold_live_pays / closure_fold_pk_pays / closure_fold_saddr_pays are read
// off this run.
// `closure_ab foldcheck`: no timing -- the partial rows of every lever arm of every fold instantiation against the parent body's,
// bit for bit, on grids with full and ragged rounds (the arms the launcher does not route to are compiled only here).
// `closure_ab foldgram`: the Gram form of the fold kernel (the regulariser from the library Gram, nothing of it in the point
// loop) beside the shipped fold kernel, its lever arms and ring depth 4, against the order-3 dense fold kernel as the 16-byte
// floor; before the timing, sum_r and R of every arm's partial rows against the parent body's, bit for bit.
// closure_fold_gram_pays is read off this run.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -I symmetry-ode-discovery_amd/csrc
//              -o tools/micro/closure_ab tools/micro/closure_ab.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "closure_fold.hpp"
#include "closure_rev.hpp"
#include "kernels.hpp"
using namespace symode;
using L3 = Library<2, 3, 0>;
using L5 = Library<2, 5, 0>;

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

__global__ void fill(float* a, long n, unsigned seed, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        a[i] = scale * ((float)(h & 0xffffff) / 8388608.0f - 1.0f);
    }
}

// The fused closure's memory side alone: the same four streams (x, dx, g(x) 8 B/point each, J_g 16 B/point), the same
// 16-byte non-temporal chunk loads in the same two-slot ring on the same (grid.x, problems) launch -- and six adds per
// chunk instead of ~880 vector instructions.  What this reaches is the HBM ceiling of the closure's access pattern.
__global__ __launch_bounds__(BLOCK) void stream_only_kernel(const float* __restrict__ x, const float* __restrict__ dx,
                                                            const float* __restrict__ gx, const float* __restrict__ jgx, long N,
                                                            float* __restrict__ out) {
    const long s = blockIdx.y;
    const float* xs = x + s * N * 2;
    const float* ys = dx + s * N * 2;
    const float* gs = gx + s * N * 2;
    const float* js = jgx + s * N * 4;
    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nthreads = (long)gridDim.x * BLOCK;
    float acc = 0.0f;
    chunk_ring<2, 5>(
        N / 2, tid, nthreads,
        [&](long q, float4 (&slot)[5]) {
            float4 a[1], b[1], c[1];
            load_chunk_raw<2, true>(xs, q, a);
            load_chunk_raw<2, true>(ys, q, b);
            load_chunk_raw<2, true>(gs, q, c);
            typedef float f4v __attribute__((ext_vector_type(4)));
            const f4v* jq = reinterpret_cast<const f4v*>(js) + q * 2;
            const f4v j0 = __builtin_nontemporal_load(jq), j1 = __builtin_nontemporal_load(jq + 1);
            slot[0] = a[0];
            slot[1] = b[0];
            slot[2] = c[0];
            slot[3] = make_float4(j0.x, j0.y, j0.z, j0.w);
            slot[4] = make_float4(j1.x, j1.y, j1.z, j1.w);
        },
        [&](long, const float4 (&slot)[5]) {
#pragma unroll
            for (int i = 0; i < 5; ++i) acc += slot[i].x + slot[i].y + slot[i].z + slot[i].w;
        });
    if (acc == 123456.789f) out[s * gridDim.x + blockIdx.x] = acc;      // (never true: keeps the loads alive without a store stream)
}

// ... and the same bytes as ONE flat stream over all problems (they are contiguous): G long-lived workgroups, ring depth R,
// SLAB = true: every workgroup walks its own contiguous slab instead of striding through the whole array.
template <int R, bool SLAB>
__global__ __launch_bounds__(BLOCK) void stream_flat_kernel(const float* __restrict__ x, const float* __restrict__ dx,
                                                            const float* __restrict__ gx, const float* __restrict__ jgx, long NT_,
                                                            float* __restrict__ out) {
    const long nchunks_all = NT_ / 2;
    long nchunks = nchunks_all, c0 = (long)blockIdx.x * BLOCK + threadIdx.x, stride = (long)gridDim.x * BLOCK;
    if (SLAB) {
        const long per = (nchunks_all + gridDim.x - 1) / gridDim.x, lo = (long)blockIdx.x * per;
        nchunks = lo + per < nchunks_all ? lo + per : nchunks_all;
        c0 = lo + threadIdx.x;
        stride = BLOCK;
    }
    float acc = 0.0f;
    chunk_ring<R, 5>(
        nchunks, c0, stride,
        [&](long q, float4 (&slot)[5]) {
            float4 a[1], b[1], c[1];
            load_chunk_raw<2, true>(x, q, a);
            load_chunk_raw<2, true>(dx, q, b);
            load_chunk_raw<2, true>(gx, q, c);
            typedef float f4v __attribute__((ext_vector_type(4)));
            const f4v* jq = reinterpret_cast<const f4v*>(jgx) + q * 2;
            const f4v j0 = __builtin_nontemporal_load(jq), j1 = __builtin_nontemporal_load(jq + 1);
            slot[0] = a[0];
            slot[1] = b[0];
            slot[2] = c[0];
            slot[3] = make_float4(j0.x, j0.y, j0.z, j0.w);
            slot[4] = make_float4(j1.x, j1.y, j1.z, j1.w);
        },
        [&](long, const float4 (&slot)[5]) {
#pragma unroll
            for (int i = 0; i < 5; ++i) acc += slot[i].x + slot[i].y + slot[i].z + slot[i].w;
        });
    if (acc == 123456.789f) out[blockIdx.x] = acc;
}

template <typename F>
static double time_us(F launch, int reps, int rounds = 3) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<double> t;
    for (int r = 0; r < rounds; ++r) {
        launch();
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(a));
        for (int i = 0; i < reps; ++i) launch();
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        t.push_back(ms * 1e3 / reps);
    }
    return *std::min_element(t.begin(), t.end());
}

int main(int argc, char** argv) {
    const long S = 8192, NB = 125000, N1 = 1L << 26;
    const long NT = S * NB;                       // 1.024e9 points >= 2^26
    constexpr int D = 2;
    float *x, *dx, *gx, *jgx, *xi3, *xi5, *loss, *grad;
    double* ws;
    CK(hipMalloc(&x, NT * D * 4));
    CK(hipMalloc(&dx, NT * D * 4));
    CK(hipMalloc(&gx, NT * D * 4));
    CK(hipMalloc(&jgx, NT * D * D * 4));
    CK(hipMalloc(&xi3, S * D * L3::P * 4));
    CK(hipMalloc(&xi5, S * D * L5::P * 4));
    CK(hipMalloc(&loss, S * 2 * 4));
    constexpr int PW = Library<2, 5, 3>::P;       // the widest library any arm launches (`pk`: order 5 with sine and exp columns)
    CK(hipMalloc(&grad, S * D * PW * 4));
    const long max_rows = 4 * S;                  // partial rows of the widest launch
    CK(hipMalloc(&ws, (WS_HEADER_DOUBLES + max_rows * (2 + D * PW)) * 8));
    fill<<<4096, 256>>>(x, NT * D, 1u, 0.7f);
    fill<<<4096, 256>>>(dx, NT * D, 2u, 0.5f);
    fill<<<4096, 256>>>(gx, NT * D, 3u, 0.7f);
    fill<<<4096, 256>>>(jgx, NT * D * D, 4u, 1.0f);
    fill<<<64, 256>>>(xi3, S * D * L3::P, 5u, 0.3f);
    fill<<<64, 256>>>(xi5, S * D * L5::P, 6u, 0.3f);
    workspace_init_kernel<0><<<dim3((WS_HEADER_DOUBLES + BLOCK - 1) / BLOCK), dim3(BLOCK)>>>((unsigned long long*)ws, WS_HEADER_DOUBLES);
    CK(hipDeviceSynchronize());
    double* part = ws + WS_HEADER_DOUBLES;
    Finish fin{(unsigned long long*)ws, nullptr, 1.0f, 2.0f, loss, grad, 1, 1};
    Finish fin2 = fin;
    fin2.n_loss = 2;

    if (argc > 1 && strcmp(argv[1], "constj") == 0) {
        // the compact table: the first 4 floats per problem of the (random) Jacobian buffer
        printf("# fused closure, order 5, %ld problems x %ld points, grid.x = 2: us per launch (min of 3 rounds of 5), three passes\n", S, NB);
#define CJRUN(LABEL, BPP, ...)                                                                                                   \
    {                                                                                                                            \
        const double us = time_us([&] { symreg_reversed_kernel<L5, true, __VA_ARGS__><<<dim3(2, (unsigned)S), dim3(BLOCK)>>>(     \
                                            x, dx, gx, jgx, 1, NB, true, xi5, nullptr, 0.1f, part, fin2); }, 5);                 \
        printf("pass %d  %-44s %8.1f us  %5.0f GB/s of its own %2.0f B/point\n", pass, LABEL, us, NT * BPP / us * 1e-3, BPP);     \
    }
        for (int pass = 0; pass < 3; ++pass) {
            CJRUN("materialised J, ring 2", 40.0, 2, 32, false, 1)
            CJRUN("constant J, ring 2, 3 waves/SIMD asked", 24.0, 2, 32, true, 3)
            CJRUN("constant J, ring 3, 3 waves/SIMD asked", 24.0, 3, 32, true, 3)
            CJRUN("constant J, ring 2, allocator left alone", 24.0, 2, 32, true, 1)
        }
        CK(hipDeviceSynchronize());
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "pk") == 0) {
        float* xiw;                                   // coefficients of the widest library; every library reads a prefix
        CK(hipMalloc(&xiw, S * D * PW * 4));
        fill<<<64, 256>>>(xiw, S * D * PW, 6u, 0.3f);
        CK(hipDeviceSynchronize());
        printf("# fused closure, constant J (24 B/point), scalar body | packed body: us per launch (min of 3 rounds of 5), three passes\n");
        const long shapes[2][2] = {{S, NB}, {64, 50000}};
#define PKRUN(ORDER, FLAGS)                                                                                                        \
    {                                                                                                                              \
        using LB = Library<2, ORDER, FLAGS>;                                                                                       \
        static_assert(LB::P <= PW, "grad, ws and xiw are sized for PW columns");                                                   \
        constexpr int MW = FLAGS == 0 ? 3 : 1;                                                                                     \
        const double a_ = time_us([&] { symreg_reversed_kernel<LB, true, 2, 32, true, MW, false><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>( \
                                            x, dx, gx, jgx, 1, Nx, true, xiw, nullptr, 0.1f, part, fin2); }, 5);                   \
        const double b_ = time_us([&] { symreg_reversed_kernel<LB, true, 2, 32, true, MW, true><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>(  \
                                            x, dx, gx, jgx, 1, Nx, true, xiw, nullptr, 0.1f, part, fin2); }, 5);                   \
        printf("pass %d  %5ld x %6ld  order %d flags %d (p = %2d)  scalar %8.1f us  packed %8.1f us  packed/scalar %.3f\n", pass, Sx, Nx, \
               ORDER, FLAGS, LB::P, a_, b_, b_ / a_);                                                                              \
    }
        for (int pass = 0; pass < 3; ++pass)
            for (const auto& sh : shapes) {
                const long Sx = sh[0], Nx = sh[1];
                const int gxw = grid_x_for(Nx, Sx, 2, 512);
                if ((long)gxw * Sx > max_rows) {
                    fprintf(stderr, "grid %d x %ld needs more partial rows than the workspace holds\n", gxw, Sx);
                    return 1;
                }
                PKRUN(1, 0) PKRUN(2, 0) PKRUN(3, 0) PKRUN(4, 0) PKRUN(5, 0)
                PKRUN(1, 1) PKRUN(2, 1) PKRUN(3, 1) PKRUN(4, 1) PKRUN(5, 1)
                PKRUN(1, 2) PKRUN(2, 2) PKRUN(3, 2) PKRUN(4, 2) PKRUN(5, 2)
                PKRUN(1, 3) PKRUN(2, 3) PKRUN(3, 3) PKRUN(4, 3) PKRUN(5, 3)
                {   // the packed body with three chunks in flight (161 VGPRs, still 3 waves/SIMD): does the freed issue time want a deeper ring?
                    const double r3 = time_us([&] { symreg_reversed_kernel<L5, true, 3, 32, true, 3, true><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>(
                                                        x, dx, gx, jgx, 1, Nx, true, xiw, nullptr, 0.1f, part, fin2); }, 5);
                    printf("pass %d  %5ld x %6ld  order 5 flags 0 (p = 21)  packed, ring 3 %8.1f us\n", pass, Sx, Nx, r3);
                }
            }
        CK(hipDeviceSynchronize());
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "live") == 0) {
        printf("# fused closure, constant J (24 B/point), every column | constant + odd degrees only: us per launch (min of 3 rounds of 5), three passes\n");
        const long shapes[2][2] = {{S, NB}, {64, 50000}};
#define LVRUN(ORDER, PKB)                                                                                                          \
    {                                                                                                                              \
        using LB = Library<2, ORDER, 0>;                                                                                           \
        constexpr unsigned long long LV = odd_degree_columns<LB>();                                                                \
        const double a_ = time_us([&] { symreg_reversed_kernel<LB, true, 2, 32, true, 3, PKB><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>( \
                                            x, dx, gx, jgx, 1, Nx, true, xi5, nullptr, 0.1f, part, fin2); }, 5);                   \
        const double b_ = time_us([&] { symreg_reversed_kernel<LB, true, 2, 32, true, 3, PKB, LV><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>( \
                                            x, dx, gx, jgx, 1, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV); }, 5);               \
        printf("pass %d  %5ld x %6ld  order %d (p = %2d) %s  dense %8.1f us  sparse %8.1f us  sparse/dense %.3f\n", pass, Sx, Nx,   \
               ORDER, LB::P, PKB ? "packed" : "scalar", a_, b_, b_ / a_);                                                          \
    }
        for (int pass = 0; pass < 3; ++pass)
            for (const auto& sh : shapes) {
                const long Sx = sh[0], Nx = sh[1];
                const int gxw = grid_x_for(Nx, Sx, 2, 512);
                if ((long)gxw * Sx > max_rows) {
                    fprintf(stderr, "grid %d x %ld needs more partial rows than the workspace holds\n", gxw, Sx);
                    return 1;
                }
                LVRUN(1, false) LVRUN(2, false) LVRUN(3, false) LVRUN(4, false) LVRUN(5, false)
                LVRUN(4, true) LVRUN(5, true)
            }
        CK(hipDeviceSynchronize());
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "foldcheck") == 0) {
        // every lever arm of every fold instantiation against the parent body on the same grid: the partial rows, bit for bit
        // (the arms the launcher does not route to are compiled nowhere else).  64 problems, three workgroups each; 50 000
        // points: 32 full rounds and a ragged one; 12 288: 8 full rounds, none ragged.  Exit status 1 on any difference.
        double* mt;
        CK(hipMalloc(&mt, S * L5::P * L5::P * 8));
        CK(hipMemset(mt, 0, S * L5::P * L5::P * 8));
        const long Sx = 64, GX = 3, rows = GX * Sx;
        std::vector<double> want(rows * (2 + D * L5::P)), got(want.size());
        int bad = 0;
#define FCLAUNCH(LIBT) symreg_fold_kernel<LIBT, 2, fold_minw<LB, SP>, LV, fold_sgpr<LB>, fold_sgpr<LB>><<<dim3(GX, (unsigned)Sx), dim3(BLOCK)>>>( \
        x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV)
#define FCARM(PKB_, SA_)                                                                                                           \
    {                                                                                                                              \
        CK(hipMemset(part, 0, nb));                                                                                                \
        FCLAUNCH(FoldLevers<LB COMMA PKB_ COMMA SA_>);                                                                              \
        CK(hipDeviceSynchronize());                                                                                                \
        CK(hipMemcpy(got.data(), part, nb, hipMemcpyDeviceToHost));                                                                \
        const bool same = memcmp(got.data(), want.data(), nb) == 0;                                                                \
        bad += same ? 0 : 1;                                                                                                       \
        printf("%6ld points  order %d (p = %2d) %s  packed %d  saddr %d: %s\n", Nx, LB::ORDER, LB::P, SP ? "odd set" : "dense  ", \
               (int)PKB_, (int)SA_, same ? "same bits" : "DIFFERENT");                                                             \
    }
#define COMMA ,
#define FCRUN(ORDER, SPARSE)                                                                                                       \
    {                                                                                                                              \
        using LB = Library<2, ORDER, 0>;                                                                                           \
        constexpr unsigned long long LV = SPARSE ? odd_degree_columns<LB>() : ~0ull;                                               \
        constexpr bool SP = SPARSE;                                                                                                \
        const size_t nb = rows * (2 + D * LB::P) * sizeof(double);                                                                 \
        CK(hipMemset(part, 0, nb));                                                                                                \
        FCLAUNCH(LB);                                                                                                              \
        CK(hipDeviceSynchronize());                                                                                                \
        CK(hipMemcpy(want.data(), part, nb, hipMemcpyDeviceToHost));                                                               \
        double sum = 0.0;                                                                                                          \
        for (size_t i = 0; i < nb / sizeof(double); ++i) sum += want[i] * want[i];                                                 \
        if (!(sum > 0.0)) { printf("order %d: the parent body left no partial rows\n", ORDER); bad += 1; }                         \
        FCARM(false, true) FCARM(true, false) FCARM(true, true)                                                                    \
    }
        for (const long Nx : {50000L, 12288L}) {
            FCRUN(1, false) FCRUN(2, false) FCRUN(3, false) FCRUN(4, false) FCRUN(5, false)
            FCRUN(4, true) FCRUN(5, true)
        }
        printf("# %d arm(s) differ\n", bad);
        return bad ? 1 : 0;
    }
    if (argc > 1 && strcmp(argv[1], "foldgram") == 0) {
        // The Gram form of the fold kernel (FoldGram: no c, u, U in the point loop) beside the fold kernel the launcher ships for
        // the same instantiation: plain | + uniform ring | + packed | both, same shapes and passes as `fold`; the order-3 dense fold
        // kernel of the same pass is the 16-byte floor.  First, no timing: sum_r and the R slots of every partial row of every
        // Gram arm against the parent body's at w_sym = 0 (where its rows hold R alone), bit for bit, 64 problems x 3 workgroups.
        double *mt, *gt;
        CK(hipMalloc(&mt, S * L5::P * L5::P * 8));
        CK(hipMemset(mt, 0, S * L5::P * L5::P * 8));
        CK(hipMalloc(&gt, S * L5::P * L5::P * 8));
        CK(hipMemset(gt, 0, S * L5::P * L5::P * 8));
        int bad = 0;
#define COMMA ,
#define FGK(LIBT, MW) symreg_fold_kernel<LIBT, 2, MW, LV, fold_sgpr<LB>, fold_sgpr<LB>>
#define FGCHECK(PKB_, SA_)                                                                                                         \
    {                                                                                                                              \
        CK(hipMemset(part, 0, nb));                                                                                                \
        FGK(FoldGram<FoldLevers<LB COMMA PKB_ COMMA SA_>>, fold_gram_minw)<<<dim3(GX, (unsigned)Sc), dim3(BLOCK)>>>(                \
            x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.0f, part, fin2, LV, gt);                                                     \
        CK(hipDeviceSynchronize());                                                                                                \
        CK(hipMemcpy(got.data(), part, nb, hipMemcpyDeviceToHost));                                                                \
        long diff = 0;                                                                                                             \
        for (long r_ = 0; r_ < rows; ++r_)                                                                                         \
            for (int k_ = 0; k_ < NA; ++k_)                                                                                        \
                if (k_ != 1 && memcmp(&got[r_ * NA + k_], &want[r_ * NA + k_], 8) != 0) ++diff;                                    \
        bad += diff ? 1 : 0;                                                                                                       \
        printf("%6ld points  order %d (p = %2d) %s  gram, packed %d  saddr %d: %s\n", Nx, LB::ORDER, LB::P, SP ? "odd set" : "dense  ", \
               (int)PKB_, (int)SA_, diff ? "DIFFERENT" : "same sum_r and R");                                                      \
    }
#define FGCRUN(ORDER, SPARSE)                                                                                                      \
    {                                                                                                                              \
        using LB = Library<2, ORDER, 0>;                                                                                           \
        constexpr unsigned long long LV = SPARSE ? odd_degree_columns<LB>() : ~0ull;                                               \
        constexpr bool SP = SPARSE;                                                                                                \
        constexpr int NA = 2 + D * LB::P;                                                                                          \
        const size_t nb = rows * NA * sizeof(double);                                                                              \
        CK(hipMemset(part, 0, nb));                                                                                                \
        FGK(LB, fold_minw<LB COMMA SP>)<<<dim3(GX, (unsigned)Sc), dim3(BLOCK)>>>(x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.0f, part, fin2, LV); \
        CK(hipDeviceSynchronize());                                                                                                \
        CK(hipMemcpy(want.data(), part, nb, hipMemcpyDeviceToHost));                                                               \
        FGCHECK(false, false) FGCHECK(false, true) FGCHECK(true, false) FGCHECK(true, true)                                        \
    }
        {
            const long Sc = 64, GX = 3, rows = GX * Sc;
            std::vector<double> want(rows * (2 + D * L5::P)), got(want.size());
            for (const long Nx : {50000L, 12288L}) {
                FGCRUN(1, false) FGCRUN(2, false) FGCRUN(3, false) FGCRUN(4, false) FGCRUN(5, false)
                FGCRUN(4, true) FGCRUN(5, true)
            }
            printf("# %d arm(s) differ\n", bad);
            if (bad) return 1;
        }
        printf("# fold kernel shipped for the instantiation | Gram form: plain | + scalar addressing | + packed | both | both, ring 4: "
               "us per launch (min of 3 rounds of 5), three passes; floor = the order-3 dense fold kernel of the pass\n");
        const long shapes[2][2] = {{S, NB}, {64, 50000}};
#define FGARM(PKB_, SA_, RG_)                                                                                                      \
    time_us([&] { symreg_fold_kernel<FoldGram<FoldLevers<LB, PKB_, SA_>>, RG_, fold_gram_minw, LV, fold_sgpr<LB>, fold_sgpr<LB>>   \
                      <<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>(x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV, gt); }, 5)
#define FGRUN(ORDER, SPARSE)                                                                                                       \
    {                                                                                                                              \
        using LB = Library<2, ORDER, 0>;                                                                                           \
        constexpr unsigned long long LV = SPARSE ? odd_degree_columns<LB>() : ~0ull;                                               \
        constexpr bool SP = SPARSE, PKS = closure_fold_pk_pays<LB, SP>, SAS = closure_fold_saddr_pays<LB, SP>;                      \
        const double a_ = time_us([&] { symreg_fold_kernel<FoldLevers<LB, PKS, SAS>, 2, fold_minw<LB, SP>, LV, fold_sgpr<LB>, fold_sgpr<LB>> \
                                            <<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>(x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV); }, 5); \
        const double b_ = FGARM(false, false, 2), c_ = FGARM(false, true, 2), d_ = FGARM(true, false, 2), e_ = FGARM(true, true, 2), \
                     f_ = FGARM(true, true, 4);                                                                                    \
        printf("pass %d  %5ld x %6ld  order %d (p = %2d) %s  shipped %8.1f us  gram %8.1f  +saddr %8.1f  +packed %8.1f  both %8.1f  both ring4 %8.1f"   \
               "  | /shipped %.3f %.3f %.3f %.3f %.3f  | /floor %.3f %.3f %.3f %.3f %.3f\n",                                       \
               pass, Sx, Nx, ORDER, LB::P, SPARSE ? "odd set" : "dense  ", a_, b_, c_, d_, e_, f_, b_ / a_, c_ / a_, d_ / a_, e_ / a_, f_ / a_, \
               b_ / floor_, c_ / floor_, d_ / floor_, e_ / floor_, f_ / floor_);                                                   \
    }
        for (int pass = 0; pass < 3; ++pass)
            for (const auto& sh : shapes) {
                const long Sx = sh[0], Nx = sh[1];
                const int gxw = grid_x_for(Nx, Sx, 2, 512);
                if ((long)gxw * Sx > max_rows) {
                    fprintf(stderr, "grid %d x %ld needs more partial rows than the workspace holds\n", gxw, Sx);
                    return 1;
                }
                const double floor_ = time_us([&] { symreg_fold_kernel<L3, 2, 3, ~0ull, fold_sgpr<L3>, fold_sgpr<L3>>
                                                        <<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>(x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, ~0ull); }, 5);
                printf("pass %d  %5ld x %6ld  floor: order 3 dense fold kernel %8.1f us\n", pass, Sx, Nx, floor_);
                FGRUN(4, false) FGRUN(5, false) FGRUN(4, true) FGRUN(5, true) FGRUN(3, false) FGRUN(2, false) FGRUN(1, false)
            }
        CK(hipDeviceSynchronize());
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "fold") == 0) {
        double* mt;                                 // (S, p, p) substitution matrices: the identity (the timing does not read their values)
        CK(hipMalloc(&mt, S * L5::P * L5::P * 8));
        CK(hipMemset(mt, 0, S * L5::P * L5::P * 8));
        printf("# fused closure, constant J: shipped streamed kernel (24 B/point) | fold (16 B/point): parent body | + scalar addressing | + packed | both; "
               "parent body and both at grid.x = 1: us per launch (min of 3 rounds of 5), three passes\n");
        const long shapes[2][2] = {{S, NB}, {64, 50000}};
#define FDPARENT(GX_)                                                                                                              \
    time_us([&] { symreg_fold_kernel<LB, 2, fold_minw<LB, SP>, LV, fold_sgpr<LB>, fold_sgpr<LB>><<<dim3(GX_, (unsigned)Sx), dim3(BLOCK)>>>( \
                      x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV); }, 5)
#define FDARM(PKB_, SA_, GX_)                                                                                                      \
    time_us([&] { symreg_fold_kernel<FoldLevers<LB, PKB_, SA_>, 2, fold_minw<LB, SP>, LV, fold_sgpr<LB>, fold_sgpr<LB>><<<dim3(GX_, (unsigned)Sx), dim3(BLOCK)>>>( \
                      x, dx, jgx, mt, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV); }, 5)
#define FDRUN(ORDER, SPARSE)                                                                                                       \
    {                                                                                                                              \
        using LB = Library<2, ORDER, 0>;                                                                                           \
        constexpr unsigned long long LV = SPARSE ? odd_degree_columns<LB>() : ~0ull;                                               \
        constexpr bool SP = SPARSE, PKB = !SPARSE && closure_pk_pays<LB>;                                                          \
        const double a_ = time_us([&] { symreg_reversed_kernel<LB, true, 2, 32, true, 3, PKB, LV><<<dim3(gxw, (unsigned)Sx), dim3(BLOCK)>>>( \
                                            x, dx, gx, jgx, 1, Nx, true, xi5, nullptr, 0.1f, part, fin2, LV); }, 5);               \
        const double b_ = FDPARENT(gxw), c_ = FDARM(false, true, gxw), d_ = FDARM(true, false, gxw), e_ = FDARM(true, true, gxw); \
        const double f_ = FDPARENT(1), g_ = FDARM(true, true, 1);                                                       \
        printf("pass %d  %5ld x %6ld  order %d (p = %2d) %s  streamed %8.1f us  fold %8.1f us  +saddr %8.1f  +packed %8.1f  both %8.1f  "   \
               "grid.x=1: fold %8.1f  both %8.1f  | fold/streamed %.3f  saddr/fold %.3f  packed/fold %.3f  both/fold %.3f\n",       \
               pass, Sx, Nx, ORDER, LB::P, SPARSE ? "odd set" : "dense  ", a_, b_, c_, d_, e_, f_, g_, b_ / a_, c_ / b_, d_ / b_, e_ / b_); \
    }
        for (int pass = 0; pass < 3; ++pass)
            for (const auto& sh : shapes) {
                const long Sx = sh[0], Nx = sh[1];
                const int gxw = grid_x_for(Nx, Sx, 2, 512);
                if ((long)gxw * Sx > max_rows) {
                    fprintf(stderr, "grid %d x %ld needs more partial rows than the workspace holds\n", gxw, Sx);
                    return 1;
                }
                FDRUN(1, false) FDRUN(2, false) FDRUN(3, false) FDRUN(4, false) FDRUN(5, false)
                FDRUN(4, true) FDRUN(5, true)
            }
        CK(hipDeviceSynchronize());
        return 0;
    }
    printf("# one problem, N = %ld points (d = 2)\n", N1);
    const int grids[] = {128, 256, 512, 768, 1024, 2048};
    for (int g : grids) {
        double us = time_us([&] { loss_grad_kernel<L3, true><<<dim3(g, 1), dim3(BLOCK)>>>(x, dx, N1, true, xi3, nullptr, part, fin, true); }, 10);
        printf("loss_grad o3 ring4 seg grid=%d: %.1f us %.0f GB/s\n", g, us, N1 * 16.0 / us * 1e-3);
        us = time_us([&] { loss_grad_kernel<L5, true><<<dim3(g, 1), dim3(BLOCK)>>>(x, dx, N1, true, xi5, nullptr, part, fin, true); }, 10);
        printf("loss_grad o5 ring4 seg grid=%d: %.1f us %.0f GB/s\n", g, us, N1 * 16.0 / us * 1e-3);
    }
#define REV1(LIB, MSEF, RG, BPP)                                                                                               \
    for (int g : grids) {                                                                                                      \
        const double us = time_us([&] {                                                                                        \
            symreg_reversed_kernel<LIB, MSEF, RG><<<dim3(g, 1), dim3(BLOCK)>>>(x, MSEF ? dx : nullptr, gx, jgx, 1, N1, true,    \
                                                                                (LIB::P == 10 ? xi3 : xi5), nullptr, 0.1f, part, \
                                                                                MSEF ? fin2 : fin);                              \
        }, 10);                                                                                                                 \
        printf("symreg_reversed p=%d mse=%d ring=%d grid=%d: %.1f us %.0f GB/s\n", LIB::P, (int)MSEF, RG, g, us, N1 * BPP / us * 1e-3); \
    }
    REV1(L3, false, 2, 32.0)
    REV1(L3, false, 3, 32.0)
    REV1(L5, true, 2, 40.0)
    REV1(L5, true, 3, 40.0)

    printf("# batched: %ld problems x %ld points\n", S, NB);
    const int gxs[] = {1, 2, 4};
#define REVB(RG)                                                                                                                \
    for (int g : gxs) {                                                                                                         \
        const double us = time_us([&] {                                                                                         \
            symreg_reversed_kernel<L5, true, RG><<<dim3(g, (unsigned)S), dim3(BLOCK)>>>(x, dx, gx, jgx, 1, NB, true, xi5, nullptr, \
                                                                                       0.1f, part, fin2);                         \
        }, 5);                                                                                                                   \
        printf("closure o5 batched ring=%d grid.x=%d: %.1f us %.0f GB/s (%.3f of 8 TB/s)\n", RG, g, us, NT * 40.0 / us * 1e-3,   \
               NT * 40.0 / us * 1e-3 / 8000);                                                                                   \
    }
    REVB(2)
    REVB(3)
    // Xi of the order-5 closure in VGPRs instead of SGPRs (42 more registers: 2 waves per SIMD instead of 3)
    for (int g : gxs) {
        const double us = time_us([&] {
            symreg_reversed_kernel<L5, true, 2, 1000><<<dim3(g, (unsigned)S), dim3(BLOCK)>>>(x, dx, gx, jgx, 1, NB, true, xi5, nullptr,
                                                                                          0.1f, part, fin2);
        }, 5);
        printf("closure o5 batched ring=2 Xi in VGPRs grid.x=%d: %.1f us %.0f GB/s (%.3f of 8 TB/s)\n", g, us, NT * 40.0 / us * 1e-3,
               NT * 40.0 / us * 1e-3 / 8000);
    }
    for (int g : gxs) {
        const double us = time_us([&] { stream_only_kernel<<<dim3(g, (unsigned)S), dim3(BLOCK)>>>(x, dx, gx, jgx, NB, loss); }, 5);
        printf("the closure's four streams alone (ring=2, six adds per chunk) grid.x=%d: %.1f us %.0f GB/s (%.3f of 8 TB/s)\n", g, us,
               NT * 40.0 / us * 1e-3, NT * 40.0 / us * 1e-3 / 8000);
    }
    const int flat_grids[] = {256, 512, 768, 1024, 2048, 4096};
#define FLAT(RR, SL)                                                                                                              \
    for (int g : flat_grids) {                                                                                                    \
        const double us = time_us([&] { stream_flat_kernel<RR, SL><<<dim3(g), dim3(BLOCK)>>>(x, dx, gx, jgx, NT, loss); }, 5);     \
        printf("four streams, ONE flat pass, %s, ring=%d, %d workgroups: %.1f us %.0f GB/s (%.3f of 8 TB/s)\n",                      \
               SL ? "slab per workgroup" : "grid-stride", RR, g, us, NT * 40.0 / us * 1e-3, NT * 40.0 / us * 1e-3 / 8000);            \
    }
    FLAT(2, false)
    FLAT(4, false)
    FLAT(2, true)
    FLAT(4, true)
    // the same with the closure's residency: 52 KB of (unused) LDS per workgroup = 3 workgroups per CU = 3 waves per SIMD
    {
        const int grids2[] = {768, 1024, 4096, 8192, 16384};
        CK(hipFuncSetAttribute((const void*)stream_flat_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 53248));
        CK(hipFuncSetAttribute((const void*)stream_flat_kernel<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 53248));
        for (int g : grids2) {
            double us = time_us([&] { stream_flat_kernel<2, true><<<dim3(g), dim3(BLOCK), 53248>>>(x, dx, gx, jgx, NT, loss); }, 5);
            printf("four streams, flat, slab, 3 waves/SIMD, ring=2, %d workgroups: %.1f us %.0f GB/s (%.3f)\n", g, us, NT * 40.0 / us * 1e-3,
                   NT * 40.0 / us * 1e-3 / 8000);
            us = time_us([&] { stream_flat_kernel<4, true><<<dim3(g), dim3(BLOCK), 53248>>>(x, dx, gx, jgx, NT, loss); }, 5);
            printf("four streams, flat, slab, 3 waves/SIMD, ring=4, %d workgroups: %.1f us %.0f GB/s (%.3f)\n", g, us, NT * 40.0 / us * 1e-3,
                   NT * 40.0 / us * 1e-3 / 8000);
            us = time_us([&] { stream_flat_kernel<2, true><<<dim3(g), dim3(BLOCK)>>>(x, dx, gx, jgx, NT, loss); }, 5);
            printf("four streams, flat, slab, 8 waves/SIMD, ring=2, %d workgroups: %.1f us %.0f GB/s (%.3f)\n", g, us, NT * 40.0 / us * 1e-3,
                   NT * 40.0 / us * 1e-3 / 8000);
        }
    }
    for (int g : gxs) {
        const double us = time_us([&] { loss_grad_kernel<L5, true><<<dim3(g, (unsigned)S), dim3(BLOCK)>>>(x, dx, NB, true, xi5, nullptr, part, fin, false); }, 5);
        printf("loss_grad o5 batched ring4 grid.x=%d: %.1f us %.0f GB/s\n", g, us, NT * 16.0 / us * 1e-3);
    }
    CK(hipDeviceSynchronize());
    float hl;
    CK(hipMemcpy(&hl, grad, 4, hipMemcpyDeviceToHost));
    printf("# done (grad[0] = %g)\n", hl);
    return 0;
}
