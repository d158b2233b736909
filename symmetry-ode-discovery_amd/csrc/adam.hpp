// Device-resident minibatch Adam trainer (symode_adam_epochs): the plain branch of train_SIGED -- train.py:491-547 of the
// reference, per minibatch MSELoss()(regressor(x), dx) + w_reg |params|_1, backward, torch.optim.Adam.step, and
// set_threshold every st_freq epochs -- as ONE launch for n_epochs whole epochs of n_problems independent problems.
// symode_adam_epochs_reversed is the same launch with the reversed symmetry regulariser (model_utils.py:160-168 of the
// reference, the JVP as the explicit matvec on precomputed g(x), J_g(x)) added to every minibatch loss.
// symode_adam_epochs_latent is the use_latent branch of the same loop (train.py:491-508, 522-547) under a frozen autoencoder:
// mse_z, mse_x and the linear-latent regulariser on per-row operands z, dz, B, y, e computed once per fit.
#pragma once
#include <cfloat>

#include "adam_order.hpp"
#include "kernels.hpp"

namespace symode {

constexpr int ADAM_BLOCK = 256;       // four wave64: thread j owns parameter j and coefficient j, row b of a batch goes to thread b % 256
constexpr int ADAM_LOG = 8;           // floats per (epoch, problem) log row, see include/symode.h
constexpr int ADAM_LOG_LATENT = 10;   // the latent entry's row (SYMODE_ADAM_LOG_LATENT)
constexpr int ADAM_HYPER = 4;         // columns of a problem's hyper-parameter row (SYMODE_ADAM_HYPER)

// the three forms of the epoch kernel: they share the cursor, the step and the epoch end
enum AdamKind { ADAM_PLAIN = 0, ADAM_REVERSED = 1, ADAM_LATENT = 2 };
constexpr int ADAM_PER_PROBLEM = 4;   // or-ed to a kind: the instantiation that reads a.hyper

struct AdamArgs {
    const float* x;
    const float* dx;
    long n_src;
    const int* idx;                   // (n_epochs, n_idx_problems, n_steps, batch), or nullptr: the keyed entries, rows from order_seeds
    long n_idx_problems;
    int n_epochs, n_steps, batch;
    long n_problems;
    const float* q;                   // (d p, r) row-major in Xi's order, or nullptr (the parameters are Xi)
    int r, allow_const, n_params;
    float lr, beta1, beta2, eps, w_x, w_reg;
    int l1;
    float threshold;
    int st_freq, epoch0;
    float near_band;
    float *params, *m, *v;
    int* step;
    float *mask, *xi_out, *log;
    // the reversed variant alone (adam_epochs_kernel<Lib, ADAM_REVERSED>); the plain kernel reads none of these
    const float* gx;                  // (n_g, n_src, d)
    const float* jgx;                 // (n_g, n_src, d, d)
    int n_g;
    float w_ratio;                    // w_sym / w_x (0 with n_g == 0): the C entry refuses w_x <= 0 with n_g > 0
    // the latent variant alone (adam_epochs_kernel<Lib, ADAM_LATENT>): x, dx are z, dz, w_x is w_z and w_ratio is w_sym / w_z
    const float* lat_b;               // (n_src, d, d)
    const float* lat_y;               // (n_src, d)
    const float* lat_e;               // (n_src) or nullptr (D_obs == d: every e_b is 0)
    const float* gen_l;               // (n_gen, d, d)
    int n_gen, d_obs;
    float w_obs, w_sym;               // the weights of mse_x and sym in the value the freezing rule tests
    // the keyed entries alone (idx == nullptr): no table, n_steps = ceil(n_src / batch)
    const long long* order_seeds;     // (n_order_seeds): 1 (every problem walks the same order) or n_problems
    long n_order_seeds;
    int shuffle;                      // 0: position pos is row pos (the loader with shuffle=False)
    // symode_adam_run alone: (n_problems, ADAM_HYPER) rows [lr, w_reg, threshold, w_sym], or nullptr (the scalars above apply)
    const float* hyper;
};

// b^n for an integer n >= 0 by squaring: a function of (b, n) alone, so a fit cut into several launches meets the same
// bias corrections bit for bit
__device__ __forceinline__ double adam_ipow(double b, int n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

// One workgroup = one problem; everything between two minibatch steps stays on chip:
//   w_s      Xi * mask, read (broadcast) by every row's residual
//   part     the four waves' sums of the d p gradient entries, sum r^2 and the valid-row count
// A step is: rows of the batch through the index table (entries outside [0, n_src) are padding: not read, not counted),
// Theta(x) and the residual per row, per-thread accumulation over the thread's rows b = tid, tid + 256, ... in that order,
// wave sums (permlane / DPP butterfly), the four wave partials added in wave order -- no atomics, the order of every sum is
// fixed by (thread, row) -- then the parameter gradient, the Adam update of parameter j by thread j and, under the
// constraint, Xi = reshape(Q beta) + const.  Two barriers per step (four under the constraint).
// The gathers do not depend on the parameters, so they run ahead of the chain of steps: the index of chunk c + 2 and the
// rows of chunk c + 1 are in flight while chunk c is evaluated, across step and epoch boundaries of the launch.
// Without a table (a.idx == nullptr, the keyed entries) that index is COMPUTED in the same slot, two chunks ahead: batch
// slot b of step s in epoch e is position pos = s batch + b, its row adam_order_row(key(order seed, epoch0 + e), n_src, pos)
// for pos < n_src and the pad -1 beyond (adam_order.hpp).  The branch is uniform over the launch; everything downstream of
// the index is the same code.  The slot keeps the rows' latency where it was, but with one wave per SIMD the integer
// arithmetic itself is on the step's path: 0.2-0.3 us per chunk at 125 000 rows (profiles/adam_device_shuffle.txt).
//
// REV adds  w_sym * sum_g sum_b |r|^2 / (valid rows * d),  r = J_g(x_b) h(x_b) - h(g x_b),  h = Theta(.) (Xi * mask)^T,  to the
// loss of every batch.  A valid row gathers gx[g, i, :] and jgx[g, i, :, :] with the row number i of x and dx (padding reads
// none of the four arrays); these gathers run ONE group element ahead of the evaluation -- element g + 1 of the row while
// element g is evaluated, element 0 of the next chunk's row during the last one, hence across the optimiser step -- so n_g
// is a run-time number at a fixed register cost.  The gradient
//   (2 w_sym / (rows d)) sum_g sum_b [ (J_g^T r)_i theta_k(x_b) - r_i theta_k(g x_b) ]
// lands in the SAME d p accumulators as the residual's: r is scaled by w_sym / w_x before it is accumulated, and the
// optimiser multiplies the sum by w_x as before.  The MSE sums are untouched, so with n_g == 0 every value of the plain
// kernel is reproduced bit for bit.  sum |r|^2 (unscaled) is one more reduced value; a batch is non-finite when
// MSE + regulariser is.
//
// LAT is the --use_latent branch (symode_adam_epochs_latent): x, dx are z, dz, and a valid row also gathers B_b (d x d), y_b
// and e_b by its row number, one chunk ahead like z and dz.  The residual above is r_z; r_x = B_b h - y_b adds |r_x|^2 + e_b to
// a sum of its own (logged, no gradient).  The generators L_g are read uniformly inside the row, as symreg_linear_kernel
// reads them: u = W J_Theta(z)(L_g z) - L_g h, sum |u|^2 NOT divided by the rows, and  u dth^T - (L_g^T u) th^T  goes into a
// SECOND set of d p accumulators, because its divisor (none) differs from r_z's (rows d) and rows is known only after the
// reduction: there the two meet as  tot_z + (w_sym / w_z) rows d tot_s,  and the optimiser multiplies by 2 w_z / (rows d)
// as before.  With n_gen == 0 the second set is neither reduced nor added, so params, m, v and mask are those of the plain
// kernel on (z, dz) with w_x = w_z bit for bit.  A batch is non-finite when w_z mse_z + w_x mse_x + w_sym sym is.
//
// a.hyper (symode_adam_run) gives every problem its own lr, w_reg, threshold and w_sym: workgroup s reads row s ONCE, before
// the step loop, and uses it wherever the launch-wide scalars stand otherwise -- the step size, the L1 term, the thresholding
// event with its near count, w_ratio = w_sym / w_x (REV, LAT; one fp32 division, rounded as the host's) and w_sym in LAT's
// tested value.  PLAIN does not read column 3.  The row is uniform over the workgroup (the address depends on blockIdx
// alone), so it costs no memory traffic and no barrier per step.  The table is a bit of the template parameter
// (KIND | ADAM_PER_PROBLEM), not a test of the pointer: the kernel is bound by its scalar registers (the compiler already
// spills some into vector lanes), and the launches without a table keep the instantiations -- name and code -- they had
// before the table existed.
template <class Lib, int KIND = ADAM_PLAIN>
__global__ __launch_bounds__(ADAM_BLOCK) void adam_epochs_kernel(const AdamArgs a) {
    constexpr bool HYPER = (KIND & ADAM_PER_PROBLEM) != 0;
    constexpr bool REV = (KIND & ~ADAM_PER_PROBLEM) == ADAM_REVERSED, LAT = (KIND & ~ADAM_PER_PROBLEM) == ADAM_LATENT;
    // reduced values: [0, DP) the gradient sums, DP sum r^2, DP + 1 the valid rows, DP + 2 sum |r|^2 (REV) / sum |u|^2 (LAT),
    // LAT: DP + 3 sum (|r_x|^2 + e), then the regulariser's DP gradient sums
    constexpr int D = Lib::D, P = Lib::P, DP = D * P, NV1 = DP + 2 + (REV ? 1 : 0) + (LAT ? 2 : 0), NV = NV1 + (LAT ? DP : 0),
                  NW = ADAM_BLOCK / WAVE, SLOTS = (NV + WAVE - 1) / WAVE, LOGW = LAT ? ADAM_LOG_LATENT : ADAM_LOG;
    static_assert(DP <= ADAM_BLOCK, "thread j owns coefficient j");
    __shared__ float w_s[DP];
    __shared__ float part[NW][NV];
    __shared__ float gxi_s[DP];
    __shared__ float par_s[ADAM_BLOCK];
    __shared__ float l1_s[NW];
    __shared__ int near_s[NW];

    const long s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int np = a.n_params, r = a.r;
    const bool con = a.q != nullptr;

    float lr = a.lr, w_reg = a.w_reg, threshold = a.threshold, w_ratio = a.w_ratio, w_sym = a.w_sym;
    if constexpr (HYPER) {
        const float* row = a.hyper + s * ADAM_HYPER;
        lr = row[0];
        w_reg = row[1];
        threshold = row[2];
        if constexpr (REV) w_ratio = a.n_g > 0 ? row[3] / a.w_x : 0.0f;
        if constexpr (LAT) {
            w_sym = row[3];
            w_ratio = a.n_gen > 0 ? row[3] / a.w_x : 0.0f;
        }
    }
    (void)w_sym;

    float p = 0.0f, m = 0.0f, v = 0.0f, mk = 0.0f, xi = 0.0f;
    if (tid < np) {
        p = a.params[s * np + tid];
        m = a.m[s * np + tid];
        v = a.v[s * np + tid];
    }
    if (tid < DP) mk = a.mask[s * DP + tid];
    int t = a.step[s];                                        // < 0: frozen after a non-finite loss, at step -t - 1
    bool frozen = t < 0;
    if (frozen) t = -t - 1;

    // Xi[tid] at the current parameters (sindy.py:169-176); the constrained form reads every parameter through par_s
    auto coefficient = [&]() __attribute__((always_inline)) {
        if (con) {
            par_s[tid] = p;
            __syncthreads();
            if (tid < DP) {
                float f = 0.0f;
                for (int c = 0; c < r; ++c) f = fmaf(a.q[(long)tid * r + c], par_s[c], f);
                if (a.allow_const && tid % P == 0) f += par_s[r + tid / P];
                xi = f;
            }
        } else {
            xi = p;
        }
        if (tid < DP) w_s[tid] = xi * mk;
    };
    coefficient();
    __syncthreads();

    const int n_chunks = (a.batch + ADAM_BLOCK - 1) / ADAM_BLOCK;
    const long sp = a.n_idx_problems == 1 ? 0 : s;
    const bool keyed = a.idx == nullptr;
    unsigned long long seed_w = 0;
    if (keyed && a.shuffle) seed_w = seed_words((unsigned long long)a.order_seeds[a.n_order_seeds == 1 ? 0 : s]);
    AdamOrderKey okey{};                                      // the round keys of epoch okey_e: derived once per epoch, not per chunk
    int okey_e = -1;
    struct Cursor { int e, s, k; };
    auto advance = [&](Cursor& c) __attribute__((always_inline)) {
        if (++c.k == n_chunks) {
            c.k = 0;
            if (++c.s == a.n_steps) {
                c.s = 0;
                ++c.e;
            }
        }
    };
    auto fetch_idx = [&](const Cursor& c) __attribute__((always_inline)) {
        const int b = c.k * ADAM_BLOCK + tid;
        int i = -1;
        if (c.e < a.n_epochs && b < a.batch) {
            if (!keyed) {
                i = a.idx[(((long)c.e * a.n_idx_problems + sp) * a.n_steps + c.s) * a.batch + b];
            } else {
                const long pos = (long)c.s * a.batch + b;    // n_src < 2^31: a position that is a row fits an int
                if (a.shuffle && c.e != okey_e) {             // uniform over the workgroup
                    okey = adam_order_key(seed_w, a.epoch0 + c.e);
                    okey_e = c.e;
                }
                if (pos < a.n_src) i = a.shuffle ? adam_order_row(okey, (int)a.n_src, (int)pos) : (int)pos;
            }
        }
        return i;
    };
    auto fetch_row = [&](int i, float (&xr)[D], float (&dr)[D]) __attribute__((always_inline)) {
        const bool ok = i >= 0 && (long)i < a.n_src;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            float u = 0.0f, w = 0.0f;
            if (ok) {
                u = a.x[(long)i * D + c];
                w = a.dx[(long)i * D + c];
            }
            xr[c] = u;
            dr[c] = w;
        }
        return ok;
    };
    // g(x), J_g(x) of group element g at row i: the validity predicate of fetch_row, and nothing at all without elements
    auto fetch_sym = [&](int g, int i, float (&gr)[D], float (&jr)[D * D]) __attribute__((always_inline)) {
        const bool ok = g < a.n_g && i >= 0 && (long)i < a.n_src;
        const long at = (long)g * a.n_src + i;
#pragma unroll
        for (int c = 0; c < D; ++c) gr[c] = ok ? a.gx[at * D + c] : 0.0f;
#pragma unroll
        for (int c = 0; c < D * D; ++c) jr[c] = ok ? a.jgx[at * (D * D) + c] : 0.0f;
    };

    // B_b, y_b, e_b of row i: the validity predicate of fetch_row
    auto fetch_lat = [&](int i, float (&br)[D * D], float (&yr)[D], float& er) __attribute__((always_inline)) {
        const bool ok = i >= 0 && (long)i < a.n_src;
#pragma unroll
        for (int c = 0; c < D * D; ++c) br[c] = ok ? a.lat_b[(long)i * (D * D) + c] : 0.0f;
#pragma unroll
        for (int c = 0; c < D; ++c) yr[c] = ok ? a.lat_y[(long)i * D + c] : 0.0f;
        er = (ok && a.lat_e) ? a.lat_e[i] : 0.0f;
    };

    Cursor c{0, 0, 0}, c2{0, 0, 0};
    float cx[D], cdx[D];
    int cidx = fetch_idx(c2);
    bool cok = fetch_row(cidx, cx, cdx);
    float cg[D], cj[D * D];
    if constexpr (REV) fetch_sym(0, cidx, cg, cj);
    float cb[D * D], cy[D], ce = 0.0f;
    if constexpr (LAT) fetch_lat(cidx, cb, cy, ce);
    advance(c2);
    int nidx = fetch_idx(c2);
    advance(c2);

    float acc[DP], ss = 0.0f, cnt = 0.0f, sr = 0.0f;
#pragma unroll
    for (int j = 0; j < DP; ++j) acc[j] = 0.0f;
    float accs[LAT ? DP : 1], sx = 0.0f;                      // LAT: the regulariser's gradient sums, sum (|r_x|^2 + e)
#pragma unroll
    for (int j = 0; j < (LAT ? DP : 1); ++j) accs[j] = 0.0f;
    double loss_sum = 0.0, l1_sum = 0.0, sym_sum = 0.0;       // the epoch's running sums (train.py:541-543), uniform over the block
    double msez_sum = 0.0;                                    // LAT: loss_sum holds mse_x, this one mse_z
    int steps = 0;
    const float om1 = (float)(1.0 - (double)a.beta1), om2 = (float)(1.0 - (double)a.beta2);

    while (c.e < a.n_epochs) {
        float nx[D], ndx[D];
        const bool nok = fetch_row(nidx, nx, ndx);
        float nb[D * D], ny[D], ne = 0.0f;
        if constexpr (LAT) fetch_lat(nidx, nb, ny, ne);
        const int nnidx = fetch_idx(c2);

        const bool eval = cok && !frozen;
        float th[P], hx[D];
        if (eval) {
            Lib::eval(cx, th);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                float f = 0.0f;
#pragma unroll
                for (int k = 0; k < P; ++k) f = fmaf(th[k], w_s[i * P + k], f);
                hx[i] = f;
                const float res = f - cdx[i];
                ss = fmaf(res, res, ss);
#pragma unroll
                for (int k = 0; k < P; ++k) acc[i * P + k] = fmaf(res, th[k], acc[i * P + k]);
            }
            cnt += 1.0f;
        }
        if constexpr (REV) {
            for (int g = 0; g < a.n_g; ++g) {
                float ng[D], nj[D * D];
                const bool last = g + 1 == a.n_g;
                fetch_sym(last ? 0 : g + 1, last ? nidx : cidx, ng, nj);
                if (eval) {
                    float tg[P], rs[D];
                    Lib::eval(cg, tg);
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        float hg = 0.0f, jh = 0.0f;
#pragma unroll
                        for (int k = 0; k < P; ++k) hg = fmaf(tg[k], w_s[i * P + k], hg);
#pragma unroll
                        for (int j = 0; j < D; ++j) jh = fmaf(cj[i * D + j], hx[j], jh);
                        const float rr = jh - hg;
                        sr = fmaf(rr, rr, sr);
                        rs[i] = w_ratio * rr;
                    }
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        float u = 0.0f;                       // (J_g^T r)_i
#pragma unroll
                        for (int j = 0; j < D; ++j) u = fmaf(cj[j * D + i], rs[j], u);
#pragma unroll
                        for (int k = 0; k < P; ++k) acc[i * P + k] = fmaf(u, th[k], fmaf(-rs[i], tg[k], acc[i * P + k]));
                    }
                }
#pragma unroll
                for (int i = 0; i < D; ++i) cg[i] = ng[i];
#pragma unroll
                for (int i = 0; i < D * D; ++i) cj[i] = nj[i];
            }
        }
        if constexpr (LAT) {
            if (eval) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    float f = -cy[i];                         // r_x = B h - y
#pragma unroll
                    for (int j = 0; j < D; ++j) f = fmaf(cb[i * D + j], hx[j], f);
                    sx = fmaf(f, f, sx);
                }
                sx += ce;
                for (int g = 0; g < a.n_gen; ++g) {
                    float L[D][D], lz[D];
#pragma unroll
                    for (int i = 0; i < D; ++i)
#pragma unroll
                        for (int j = 0; j < D; ++j) L[i][j] = a.gen_l[(g * D + i) * D + j];
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        float f = 0.0f;
#pragma unroll
                        for (int j = 0; j < D; ++j) f = fmaf(L[i][j], cx[j], f);
                        lz[i] = f;
                    }
                    float tz[P], dth[P], u[D];
                    Lib::eval_jvp(cx, lz, tz, dth);           // tz = th again
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        float f = 0.0f;                       // u = W dth - L h
#pragma unroll
                        for (int k = 0; k < P; ++k) f = fmaf(dth[k], w_s[i * P + k], f);
#pragma unroll
                        for (int j = 0; j < D; ++j) f = fmaf(-L[i][j], hx[j], f);
                        u[i] = f;
                        sr = fmaf(f, f, sr);
                    }
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        float ltu = 0.0f;                     // (L^T u)_i
#pragma unroll
                        for (int j = 0; j < D; ++j) ltu = fmaf(L[j][i], u[j], ltu);
#pragma unroll
                        for (int k = 0; k < P; ++k) accs[i * P + k] = fmaf(u[i], dth[k], fmaf(-ltu, th[k], accs[i * P + k]));
                    }
                }
            }
        }

        if (c.k == n_chunks - 1) {                            // the batch is complete: one optimiser step
            float keep[SLOTS];
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) keep[q] = 0.0f;
#pragma unroll
            for (int j = 0; j < NV1; ++j) {
                const float tot = wave_sum_dpp(j < DP ? acc[j < DP ? j : 0] : (j == DP ? ss : (j == DP + 1 ? cnt : (j == DP + 2 ? sr : sx))));
                if (lane == (j & (WAVE - 1))) keep[j / WAVE] = tot;
            }
            if constexpr (LAT) {
                if (a.n_gen > 0) {
#pragma unroll
                    for (int j = NV1; j < NV; ++j) {
                        const float tot = wave_sum_dpp(accs[j - NV1]);
                        if (lane == (j & (WAVE - 1))) keep[j / WAVE] = tot;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < SLOTS; ++q)
                if (q * WAVE + lane < NV) part[wave][q * WAVE + lane] = keep[q];
            const float l1w = wave_sum_dpp(tid < np ? fabsf(p) : 0.0f);       // |params|_1 BEFORE the update, as the loss sees it
            if (lane == 0) l1_s[wave] = l1w;
            __syncthreads();

            float ss_t = part[0][DP], cnt_t = part[0][DP + 1];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                ss_t += part[w][DP];
                cnt_t += part[w][DP + 1];
            }
            const bool live = !frozen && cnt_t > 0.0f;       // a batch of padding alone is no step
            const float loss = ss_t / (cnt_t * (float)D);
            float reg = 0.0f;
            if constexpr (REV) {
                float sr_t = part[0][DP + 2];
#pragma unroll
                for (int w = 1; w < NW; ++w) sr_t += part[w][DP + 2];
                reg = sr_t / (cnt_t * (float)D);
            }
            float loss_x = 0.0f;
            if constexpr (LAT) {
                float sr_t = part[0][DP + 2], sx_t = part[0][DP + 3];
#pragma unroll
                for (int w = 1; w < NW; ++w) {
                    sr_t += part[w][DP + 2];
                    sx_t += part[w][DP + 3];
                }
                reg = sr_t;                                   // torch.norm(..)**2 over the batch: no divisor
                loss_x = sx_t / (cnt_t * (float)a.d_obs);
            }
            const float tested = LAT ? fmaf(a.w_x, loss, fmaf(a.w_obs, loss_x, w_sym * reg)) : (REV ? loss + reg : loss);
            const bool bad = live && !(fabsf(tested) <= FLT_MAX);
            if (bad) frozen = true;                           // NaN / inf: the problem keeps its state from here on
            const bool upd = live && !bad;
            const float scale = 2.0f / (cnt_t * (float)D);
            float g_xi = 0.0f;
            if (upd && tid < DP) {
                float tot = part[0][tid];
#pragma unroll
                for (int w = 1; w < NW; ++w) tot += part[w][tid];
                if constexpr (LAT) {
                    if (a.n_gen > 0) {
                        float tot_s = part[0][NV1 + tid];
#pragma unroll
                        for (int w = 1; w < NW; ++w) tot_s += part[w][NV1 + tid];
                        tot = fmaf(w_ratio * (cnt_t * (float)D), tot_s, tot);
                    }
                }
                g_xi = scale * tot * mk;                      // d mse / d Xi: the model reads Xi * mask
            }
            float g_data = g_xi;
            if (con) {
                if (tid < DP) gxi_s[tid] = g_xi;
                __syncthreads();
                g_data = 0.0f;
                if (upd && tid < r) {
                    for (int e = 0; e < DP; ++e) g_data = fmaf(a.q[(long)e * r + tid], gxi_s[e], g_data);
                } else if (upd && tid < np && a.allow_const) {
                    g_data = gxi_s[(tid - r) * P];            // column 0 of row tid - r
                }
            }
            if (upd) {
                ++t;
                if (tid < np) {
                    const float sgn = (float)(p > 0.0f) - (float)(p < 0.0f);
                    const float g = a.l1 ? fmaf(w_reg, sgn, a.w_x * g_data) : a.w_x * g_data;
                    // torch's lerp_(g, 1 - b1): from the nearer end, so that a weight of 1 (b1 = 0) gives g itself, not m + (g - m)
                    m = om1 < 0.5f ? fmaf(om1, g - m, m) : fmaf(-(g - m), a.beta1, g);
                    v = fmaf(om2, g * g, a.beta2 * v);
                    const double bc1 = 1.0 - adam_ipow((double)a.beta1, t), bc2 = 1.0 - adam_ipow((double)a.beta2, t);
                    const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
                    p -= step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
                }
                float l1_t = l1_s[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) l1_t += l1_s[w];
                loss_sum += (double)(LAT ? loss_x : loss);
                l1_sum += (double)l1_t;
                if constexpr (REV || LAT) sym_sum += (double)reg;
                if constexpr (LAT) msez_sum += (double)loss;
                ++steps;
                coefficient();
            }
#pragma unroll
            for (int j = 0; j < DP; ++j) acc[j] = 0.0f;
            ss = 0.0f;
            cnt = 0.0f;
            sr = 0.0f;
            if constexpr (LAT) {
#pragma unroll
                for (int j = 0; j < DP; ++j) accs[j] = 0.0f;
                sx = 0.0f;
            }
            __syncthreads();

            if (c.s == a.n_steps - 1) {                       // the epoch is complete (train.py:545-546, sindy.py:192-194)
                const int epoch = a.epoch0 + c.e;
                const bool ev = !frozen && a.st_freq > 0 && (epoch + 1) % a.st_freq == 0;
                bool near = false;
                if (ev && tid < DP) {
                    const float av = fabsf(xi);
                    near = fabsf(av - threshold) < a.near_band && mk > 0.0f;
                    mk = (av > threshold && mk > 0.0f) ? 1.0f : 0.0f;       // strict >, monotone
                    w_s[tid] = xi * mk;
                }
                const int near_w = __popcll(__ballot(near));
                if (lane == 0) near_s[wave] = near_w;
                __syncthreads();
                if (tid == 0) {
                    int near_t = 0;
                    for (int w = 0; w < NW; ++w) near_t += near_s[w];
                    float* rec = a.log + ((long)c.e * a.n_problems + s) * LOGW;
                    rec[0] = (float)(loss_sum / (double)steps);               // 0 / 0 = NaN: an epoch without a step
                    rec[1] = (float)(l1_sum / (double)steps);
                    rec[2] = (float)steps;
                    rec[3] = (float)near_t;
                    rec[4] = frozen ? 1.0f : 0.0f;
                    rec[5] = ev ? 1.0f : 0.0f;
                    rec[6] = (float)epoch;
                    if constexpr (LAT) {
                        rec[7] = (float)(sym_sum / (double)steps);            // 0 with n_gen == 0, NaN for an epoch without a step
                        rec[8] = (float)(msez_sum / (double)steps);
                        rec[9] = 0.0f;
                    } else {
                        rec[7] = (REV && a.n_g > 0) ? (float)(sym_sum / (double)steps) : 0.0f;   // no elements: 0 as the plain entry, stepless epochs too
                    }
                }
                msez_sum = 0.0;
                loss_sum = 0.0;
                l1_sum = 0.0;
                sym_sum = 0.0;
                steps = 0;
            }
        }

        cok = nok;
        cidx = nidx;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            cx[i] = nx[i];
            cdx[i] = ndx[i];
        }
        if constexpr (LAT) {
#pragma unroll
            for (int i = 0; i < D * D; ++i) cb[i] = nb[i];
#pragma unroll
            for (int i = 0; i < D; ++i) cy[i] = ny[i];
            ce = ne;
        }
        nidx = nnidx;
        advance(c);
        advance(c2);
    }

    if (tid < np) {
        a.params[s * np + tid] = p;
        a.m[s * np + tid] = m;
        a.v[s * np + tid] = v;
    }
    if (tid < DP) {
        a.mask[s * DP + tid] = mk;
        a.xi_out[s * DP + tid] = xi;
    }
    if (tid == 0) a.step[s] = frozen ? -t - 1 : t;
}

// a.hyper picks the instantiation that reads the per-problem rows
template <class Lib, int KIND>
hipError_t launch_adam_kind(const AdamArgs& a, hipStream_t st) {
    if (a.n_problems == 0 || a.n_epochs == 0) return hipSuccess;
    if (a.hyper)
        adam_epochs_kernel<Lib, KIND | ADAM_PER_PROBLEM><<<dim3((unsigned)a.n_problems), dim3(ADAM_BLOCK), 0, st>>>(a);
    else
        adam_epochs_kernel<Lib, KIND><<<dim3((unsigned)a.n_problems), dim3(ADAM_BLOCK), 0, st>>>(a);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

template <class Lib>
hipError_t launch_adam_epochs(const AdamArgs& a, hipStream_t st) {
    return launch_adam_kind<Lib, ADAM_PLAIN>(a, st);
}

template <class Lib>
hipError_t launch_adam_epochs_reversed(const AdamArgs& a, hipStream_t st) {
    return launch_adam_kind<Lib, ADAM_REVERSED>(a, st);
}

template <class Lib>
hipError_t launch_adam_epochs_latent(const AdamArgs& a, hipStream_t st) {
    return launch_adam_kind<Lib, ADAM_LATENT>(a, st);
}

}  // namespace symode
