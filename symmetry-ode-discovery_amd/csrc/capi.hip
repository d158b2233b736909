// C ABI of libsymode_hip.so (declarations and per-entry reference citations: include/symode.h).
// Argument validation happens here, on the host, before anything is launched: a call that
// returns a negative code has touched no device memory.
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "../../include/symode.h"
#include "closure_quad.hpp"
#include "closure_reduced.hpp"
#include "gram_resample.hpp"
#include "jconst.hpp"
#include "linear_action.hpp"
#include "ops_table.hpp"
#include "quad_closure.hpp"
#include "stlsq.hpp"
#include "stlsq_bag.hpp"
#include "stlsq_constrained.hpp"
#include "stlsq_path.hpp"
#include "stlsq_symreg.hpp"
#include "stlsq_path_symreg.hpp"
#include "weak_normal.hpp"

using namespace symode;

namespace {

const LibOps* find_ops(int d, int order, int flags) {
    if (order < 1 || order > MAX_ORDER || flags < 0 || flags > 3) return nullptr;
#define SYMODE_CASE(D, O) case D * 10 + O: return ops_d##D##_o##O(flags);
    switch (d * 10 + order) {
        SYMODE_CASE(1, 1) SYMODE_CASE(1, 2) SYMODE_CASE(1, 3) SYMODE_CASE(1, 4) SYMODE_CASE(1, 5)
        SYMODE_CASE(2, 1) SYMODE_CASE(2, 2) SYMODE_CASE(2, 3) SYMODE_CASE(2, 4) SYMODE_CASE(2, 5)
        SYMODE_CASE(3, 1) SYMODE_CASE(3, 2) SYMODE_CASE(3, 3) SYMODE_CASE(3, 4)
#ifdef SYMODE_WITH_D4                                 // `make ALL=1`: no task of the reference has four state variables
        SYMODE_CASE(4, 1) SYMODE_CASE(4, 2) SYMODE_CASE(4, 3)
#endif
        default: return nullptr;                      // (d, order) outside the compiled set
    }
#undef SYMODE_CASE
}

inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p % a) != 0; }
template <class... P> inline bool any_null(const P*... p) { return (... || (p == nullptr)); }
template <class... P> inline bool any_misaligned(size_t a, const P*... p) { return (... || misaligned(p, a)); }

// ---- the size rules the symode_stlsq_* entries share, each stated once (host only; true = SYMODE_E_BADSIZE) ----
inline bool stlsq_bad_library(int d, int p) { return d < 1 || d > STLSQ_MAX_D || p < 1 || p > STLSQ_MAX_P; }
// problem s reads set s % n_sets; ``grid``: more problems than sets are allowed (the sweeps: only behind a hyper table)
inline bool stlsq_bad_problems(long n_sets, long n_problems, bool grid) {
    return n_sets < 1 || n_problems < n_sets || n_problems > 2147483647L || (!grid && n_problems != n_sets);
}
inline bool stlsq_bad_val_sets(long n_val_sets, long n_problems) { return n_val_sets < 1 || n_val_sets > n_problems; }
// r' = r + (d if allow_constant): beta and, where the model reads it, const
inline bool stlsq_bad_free(int d, int p, int r, int allow_constant) {
    const long rr = (long)r + (allow_constant ? d : 0);
    return r < 1 || rr > STLSQC_MAX_R || rr > (long)d * p;
}
inline bool all_finite_nonneg(std::initializer_list<double> values) {
    for (const double v : values)
        if (!(v >= 0.0) || !std::isfinite(v)) return false;
    return true;
}

// Gram passes are MFMA-bound, not latency-bound: a bounded number of workgroups per launch (default 1024 = 4 per CU:
// one wave per SIMD cannot cover the LDS round trip between MFMAs; SYMODE_GRAM_GRID for tuning runs) keeps the
// number of partials the single finalize block has to add small.
inline int gram_grid(long n, long S) {
    const long total = knobs().gram_grid < 0 ? 1024 : (knobs().gram_grid < 2 ? 2 : knobs().gram_grid);
    const long g = grid_x_by_points(n, 1);
    long cap = S >= total / 2 ? 2 : total / S;
    // one problem: the single finalize block adds every partial (6 KB each at two tiles): 125 000 points cost 84 us on
    // 1024 workgroups, 34 us on 128; 1 M points 178 vs 83 us on 256; 16 M 596 vs 564 us on 512 (r02_single_grid.txt)
    if (S == 1 && knobs().gram_grid < 0) cap = n <= 300000 ? 128 : n <= 2000000 ? 256 : n <= 32000000 ? 512 : total;
    return (int)(g > cap ? cap : g);
}

// Workgroups of ONE closure problem (the last of them adds the partial rows alone; all of them stream one moving window
// of memory): measured best counts (profiles/r02_single_grid.txt, us per launch at cap 128 / 256 / 512 / round-2 default):
//   Theta + residual + grad, 16 B/point:   1 M points 10.5 / 11.4 / 15.7 / 10.3    4 M  19.0 / 16.5 / 20.5 / 30.0
//                                          16 M       58.8 / 44.9 / 48.3 / 51.6    64 M  211 / 169.5 / 175 / 195.5
//   fused with the regulariser, 40 B/point: 1 M       24.5 / 17.1 / 17.8 / 24.7    4 M  80.7 / 47.0 / 36.9 / 43.5
//                                          16 M        308 /  170 /  113 /  118    64 M 1195 /  645 /  432 /  447
// SYMODE_SMALL_GRID fixes the cap for tuning runs (0 = none).
inline int small_grid_cap(long n, bool with_regulariser) {
    if (knobs().small_grid >= 0) return (int)knobs().small_grid;
    if (with_regulariser) return n <= 300000 ? 128 : (n <= 1500000 ? 256 : 512);
    return n <= 1500000 ? 128 : 256;
}

// The vector-pipe Gram (gram_valu.hpp) holds two workgroups per CU (register-bound): one balanced round of them for a
// single large problem, the streaming grid for batches; its partial rows are 78 doubles, so many workgroups are cheap.
inline int gram_valu_grid(long n, long S, int d) {
    const long total = knobs().gram_valu_grid < 0 ? 1024 : (knobs().gram_valu_grid < 2 ? 2 : knobs().gram_valu_grid);
    // at least 32 points per thread: the epilogue transposes 78 fp64 sums per thread through LDS (ten rounds), which a
    // thread must amortise over its own 78-fma-per-point work; beyond that, enough workgroups to fill the chip
    long g = (n + 256L * 32 - 1) / (256L * 32);
    long want = (total + S - 1) / S;                       // ~`total` workgroups in all
    if (S == 1 && want > 512 && knobs().gram_valu_grid < 0) want = 512;   // one problem: 16 M points 84 vs 97 us, 64 M equal
    if (g > want) g = want;
    if (g < 1) g = 1;
    return (int)g;
}

// The 4x4-tile matrix-core Gram (gram_m4.hpp): a wave takes 64 points per pass and wants >= 8 passes to pay for its
// epilogue (21 tiles across lanes and waves); ~1024 workgroups in all (3-4 resident per CU), its partials are 336 doubles.
inline int gram_m4_grid(long n, long S) {
    const long total = knobs().gram_m4_grid < 0 ? 1024 : (knobs().gram_m4_grid < 1 ? 1 : knobs().gram_m4_grid);
    long g = (n + 256L * 8 - 1) / (256L * 8);
    // one problem: exactly one resident round (3 workgroups per CU at 134 registers): 16 M points 286 us on 1024, where the
    // last 256 workgroups run on a third of the chip
    const long cap = S >= total / 2 ? 2 : (S == 1 && knobs().gram_m4_grid < 0 ? 768 : total / S);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// One problem through a reduction kernel: the workgroups loop over the data with a grid-wide stride, so all of them read
// one moving window of memory -- fewer, longer-lived workgroups keep that window (and the DRAM pages under it) tighter,
// and the last workgroup has fewer partial rows to add.  The best count grows with the problem
// (profiles/r02_single_grid.txt, us per launch at 64 / 128 / 256 / 512 / 1024 workgroups, d = 2, order 3):
//   125 000 points  vjp 7.8 / 8.2 / 13.3 / 13.2 / 13.2      jvp_vjp 8.5 / 8.4 / 13.8 / 13.3 / 13.3
//   1 M             vjp 18.2 / 13.8 / 13.2 / 16.8 / 16.7    jvp_vjp 31.5 / 21.0 / 17.2 / 21.3 / 21.5
//   8 M             vjp 181 / 103 / 61 / 45.8 / 48.8        jvp_vjp 205 / 112 / 70.2 / 79.3 / 118
//   64 M            vjp 1461 / 780 / 436 / 310 / 289        jvp_vjp 1605 / 841 / 495 / 572 / 561
// (round 3: with the register-ring pipelines the optimum moved to ONE workgroup per CU from 4 M points up --
//  profiles/r03_stream_ab.txt, 64 .. 1024 workgroups at 125 000 .. 64 M points)
// hence a cap per size class: <= 300 K points, <= 2 M, <= 16 M, beyond.  SYMODE_REDUCE_GRID overrides it for tuning runs.
inline int single_problem_grid(int gx, long n, int c_small, int c_mid, int c_large, int c_huge) {
    const int env = (int)knobs().reduce_grid;
    const int c = env > 0 ? env : (n <= 300000 ? c_small : n <= 2000000 ? c_mid : n <= 16000000 ? c_large : c_huge);
    return gx > c ? c : gx;
}

// points per 16-byte chunk step (points.hpp, Chunk<D>::PPT)
inline int ppt_for(int d) { return d == 2 ? 2 : d == 4 ? 1 : 4; }

// scratch (in doubles) of the widest reduction for this library at (S, n)
size_t workspace_doubles(const LibOps* ops, long S, long n) {
    const int F = ops->p + ops->d;
    const int T = (F + 15) / 16;
    const size_t gram_partial = (size_t)(T * (T + 1) / 2) * 256;
    const size_t nacc = 2 + (size_t)ops->d * ops->p;          // widest row: the fused closure keeps two scalar sums
    size_t g_red = (size_t)grid_x_for(n, S, 1, 512);    // widest grid any reduction uses
    if ((size_t)gram_grid(n, S) > g_red) g_red = (size_t)gram_grid(n, S);
    if ((size_t)gram_valu_grid(n, S, ops->d) + 8 > g_red) g_red = (size_t)gram_valu_grid(n, S, ops->d) + 8;   // (+8: the split form rounds up)
    const size_t a = (size_t)S * g_red * nacc;
    size_t b = (size_t)S * g_red * gram_partial;
    const size_t T4 = (size_t)(F + 3) / 4, m4 = (size_t)S * (size_t)gram_m4_grid(n, S) * (T4 * (T4 + 1) / 2 * 16);
    if (m4 > b) b = m4;
    return (size_t)WS_HEADER_DOUBLES + (a > b ? a : b);      // [magic + tickets | partial rows]
}

// the time slabs of a weak-form contraction over n_t points: a workgroup = 4 waves x 64 time points per step
inline long weak_slabs(long n_t) {
    const long gx = (n_t + 255) / 256;
    return gx > 64 ? 64 : gx;
}

#define SYMODE_GET_OPS()                              \
    const LibOps* ops = find_ops(d, order, flags);    \
    if (!ops) return SYMODE_E_UNSUPPORTED;

#define SYMODE_CHECK_WS(S_, n_)                                                              \
    if (!workspace || misaligned(workspace, 8)) return SYMODE_E_WORKSPACE;                   \
    if (workspace_bytes < workspace_doubles(ops, (S_), (n_)) * sizeof(double)) return SYMODE_E_WORKSPACE;

// Workgroups per problem of a reversed-closure launch (the streamed forms and the fold kernel of a linear action alike).
int reversed_closure_grid(bool fused, const LibOps* ops, long n_problems, long n, int d) {
    int gx = grid_x_for(n, n_problems, ppt_for(d), 512);
    if (n_problems == 1) {
        int cap = small_grid_cap(n, true);
        // the regulariser alone, 32 B/point: the small libraries stream best from ONE workgroup per CU like the other
        //  reductions -- order 3 at 2^26 points 314 us = 0.855 of HBM on 256 workgroups against 338 on 512; order 4-5 want the
        //  second one: 340 against 374 us.  The fused closure (40 B/point) keeps the cap of small_grid_cap.
        if (!fused && cap > 256 && ops->d * ops->p <= 24 && knobs().small_grid < 0) cap = 256;
        if (cap > 0 && gx > cap) gx = cap;
    }
    return gx;
}

// The reversed-symmetry closure: the one path from its seven C entries to LibOps::symreg_reversed.
//   fused   MSE + w_sym * regulariser on (x, dx), loss (S, 2); else the regulariser alone, loss (S) (dx, w_sym unused)
//   constj  jgx is the compact (S, n_g, d, d) table of a point-constant Jacobian (symode_jacobian_constant), not the
//           materialised (S, n_g, n, d, d) tensor: the same grids and workspace, the same partial rows summed in the same order
//   live    the library columns that may hold a coefficient (the _live entries; all ones from every other entry): handed to the
//           launcher, which owns the choice of kernel
// The forms differ in the three places marked (1)-(3), and nowhere else.
int reversed_closure(bool fused, bool constj, const float* x, const float* dx, const float* gx_, const float* jgx, int n_g,
                     long n_problems, long n, int d, int order, int flags, const float* xi, const float* mask, float inv_count,
                     float w_sym, float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream,
                     unsigned long long live = ~0ull) {
    SYMODE_GET_OPS();
    // (1) no group element at all (the regulariser is 0) is a call only the materialised regulariser accepts
    const int min_n_g = (fused || constj) ? 1 : 0;
    if (n < 1 || n_g < min_n_g || n_problems < 1 || n_problems > 65535) return SYMODE_E_BADSIZE;
    if (!x || (fused && !dx) || !xi || !loss_out || !grad_out || (n_g > 0 && (!gx_ || !jgx))) return SYMODE_E_NULLPTR;
    if (!fused) dx = nullptr;                               // (the launcher takes "dx given" for "fused")
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(gx_, 4) || misaligned(jgx, 4) || misaligned(xi, 4) || misaligned(mask, 4) ||
        misaligned(loss_out, 4) || misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, n);
    const int gx = reversed_closure_grid(fused, ops, n_problems, n, d);   // (2) the regulariser alone has a grid rule of its own
    // (3) without dx there is no second term to weigh the regulariser against: its weight is 1
    return (int)ops->symreg_reversed(x, dx, gx_, jgx, constj, n_g, n_problems, n, xi, mask, live, inv_count,
                                     fused ? w_sym : 1.0f, loss_out, grad_out, (double*)workspace, gx, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int symode_abi_version(void) { return 8; }

void symode_reload_env(void) { knobs() = read_knobs(); }

const char* symode_error_string(int code) {
    switch (code) {
        case SYMODE_OK: return "ok";
        case SYMODE_E_UNSUPPORTED: return "library (d, order, flags) not compiled into libsymode_hip";
        case SYMODE_E_NULLPTR: return "null pointer argument";
        case SYMODE_E_BADSIZE: return "bad size argument";
        case SYMODE_E_WORKSPACE: return "workspace missing or too small";
        case SYMODE_E_ALIGN: return "misaligned pointer";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown symode error";
    }
}

int symode_lib_size(int d, int order, int flags) {
    const LibOps* ops = find_ops(d, order, flags);
    return ops ? ops->p : SYMODE_E_UNSUPPORTED;
}

size_t symode_workspace_bytes(int d, int order, int flags, long n_problems, long n) {
    const LibOps* ops = find_ops(d, order, flags);
    if (!ops || n_problems < 1 || n < 0) return 0;
    return workspace_doubles(ops, n_problems, n) * sizeof(double);
}

int symode_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace) return SYMODE_E_NULLPTR;
    if (misaligned(workspace, 8)) return SYMODE_E_ALIGN;
    if (workspace_bytes < (size_t)WS_HEADER_DOUBLES * sizeof(double)) return SYMODE_E_WORKSPACE;
    const long words = WS_HEADER_DOUBLES;
    workspace_init_kernel<0><<<dim3((unsigned)((words + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream>>>(
        (unsigned long long*)workspace, words);
    return (int)hipGetLastError();
}

int symode_theta(const float* x, long n, int d, int order, int flags, float* theta_out, void* stream) {
    SYMODE_GET_OPS();
    if (n < 0) return SYMODE_E_BADSIZE;
    if (n == 0) return SYMODE_OK;
    if (!x || !theta_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(theta_out, 4)) return SYMODE_E_ALIGN;
    return (int)ops->theta(x, n, theta_out, (hipStream_t)stream);
}

int symode_forward(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask, float* out,
                   void* stream) {
    SYMODE_GET_OPS();
    if (n < 0) return SYMODE_E_BADSIZE;
    if (n == 0) return SYMODE_OK;
    if (!x || !xi || !out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(out, 4) || misaligned(xi, 4) || misaligned(mask, 4)) return SYMODE_E_ALIGN;
    return (int)ops->forward(x, n, xi, mask, out, (hipStream_t)stream);
}

int symode_odeint(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask, int n_steps,
                  float dt, int method, float* out, void* stream) {
    SYMODE_GET_OPS();
    if (n < 0 || n_steps < 0 || (method != 0 && method != 1)) return SYMODE_E_BADSIZE;
    if (n == 0) return SYMODE_OK;
    if (!x || !xi || !out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(out, 4) || misaligned(xi, 4) || misaligned(mask, 4)) return SYMODE_E_ALIGN;
    return (int)ops->odeint(x, n, xi, mask, n_steps, dt, method, out, (hipStream_t)stream);
}

int symode_odeint_traj(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask, int n_steps,
                       float dt, int method, float* traj, void* stream) {
    SYMODE_GET_OPS();
    if (n < 0 || n_steps < 0 || (method != 0 && method != 1)) return SYMODE_E_BADSIZE;
    if (n == 0 || n_steps == 0) return SYMODE_OK;
    if (!x || !xi || !traj) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(traj, 4) || misaligned(xi, 4) || misaligned(mask, 4)) return SYMODE_E_ALIGN;
    return (int)ops->odeint_traj(x, n, xi, mask, n_steps, dt, method, traj, (hipStream_t)stream);
}

int symode_rollout_error(const float* x_true, long n_ics, int n_steps, int d, int order, int flags, const float* xi,
                         const float* mask, long n_models, float dt, int method, float bound, float* err_out,
                         double* mean_err_out, int* horizon_out, void* stream) {
    SYMODE_GET_OPS();
    if (n_ics < 0 || n_models < 0 || n_steps <= 0 || (method != 0 && method != 1)) return SYMODE_E_BADSIZE;
    if (n_ics == 0 || n_models == 0) return SYMODE_OK;
    if (n_ics > 2147483647L / n_models) return SYMODE_E_BADSIZE;            // one lane per (model, trajectory)
    if (!x_true || !xi || !mean_err_out || !horizon_out) return SYMODE_E_NULLPTR;
    if (misaligned(x_true, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(err_out, 4) ||
        misaligned(mean_err_out, 8) || misaligned(horizon_out, 4))
        return SYMODE_E_ALIGN;
    return (int)ops->rollout_error(x_true, n_ics, n_models, xi, mask, n_steps, dt, method, bound, err_out, mean_err_out,
                                   horizon_out, (hipStream_t)stream);
}

int symode_loss_grad(const float* x, const float* dx, long n_problems, long n, int d, int order, int flags,
                     const float* xi, const float* mask, float inv_count, float* loss_out, float* grad_out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n_problems < 1 || n_problems > 65535 || n < 1) return SYMODE_E_BADSIZE;
    if (!x || !dx || !xi || !loss_out || !grad_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(loss_out, 4) ||
        misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, n);
    int gx = grid_x_for(n, n_problems, ppt_for(d));
    // a single latency-bound problem: the last workgroup adds gx partial rows alone, so fewer, longer workgroups win
    // (SYMODE_SMALL_GRID overrides the cap for tuning runs; 0 = no cap)
    if (n_problems == 1) {
        // (order 4-5 libraries are as arithmetic-heavy as the regulariser closures: 64 M points at order 5, 240 us at 256
        //  workgroups, 184 at 512 -- profiles/r03_closure_ab.txt; order 4 (d p = 30): 191 against 176 us; order 3 (20) is
        //  best at 256: 161 against 169)
        const int cap = small_grid_cap(n, ops->d * ops->p > 24);
        if (cap > 0 && gx > cap) gx = cap;
    }
    return (int)ops->loss_grad(x, dx, n_problems, n, xi, mask, inv_count, loss_out, grad_out, (double*)workspace, gx,
                               (hipStream_t)stream);
}

int symode_aug_gram(const float* x, const float* dx, long n_problems, long n, int d, int order, int flags,
                    double* gram_out, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n_problems < 1 || n_problems > 65535 || n < 1) return SYMODE_E_BADSIZE;
    if (!x || !dx || !gram_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(gram_out, 8)) return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, n);
    return (int)ops->aug_gram(x, dx, n_problems, n, nullptr, gram_out, (double*)workspace, gram_grid(n, n_problems),
                              gram_valu_grid(n, n_problems, d), gram_m4_grid(n, n_problems), (hipStream_t)stream);
}

int symode_aug_gram_gather(const float* x, const float* dx, long n_src, const int* idx, long n_problems, long m, int d,
                           int order, int flags, double* gram_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
    SYMODE_GET_OPS();
    if (n_problems < 1 || n_problems > 65535 || m < 1 || n_src < 1 || n_src > 2147483647L) return SYMODE_E_BADSIZE;
    if (!x || !dx || !idx || !gram_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(idx, 4) || misaligned(gram_out, 8)) return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, m);
    return (int)ops->aug_gram(x, dx, n_problems, m, idx, gram_out, (double*)workspace, gram_grid(m, n_problems),
                              gram_valu_grid(m, n_problems, d), gram_m4_grid(m, n_problems), (hipStream_t)stream);
}

int symode_symreg_linear(const float* z, long n, int d, int order, int flags, const float* xi, const float* mask,
                         const float* L, int n_gen, float* loss_out, float* grad_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n < 1 || n_gen < 0) return SYMODE_E_BADSIZE;
    if (!z || !xi || !loss_out || !grad_out || (n_gen > 0 && !L)) return SYMODE_E_NULLPTR;
    if (misaligned(z, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(L, 4)) return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(1, n);
    const int gx = single_problem_grid(grid_x_for(n, 1, ppt_for(d)), n, 128, 256, 512, 512);      // r03_stream_ab.txt
    return (int)ops->symreg_linear(z, n, xi, mask, L, n_gen, loss_out, grad_out, (double*)workspace, gx,
                                   (hipStream_t)stream);
}

// The seven entries of the reversed-symmetry closure are forwards to reversed_closure() above: batched or not, with or
// without dx, jgx materialised or the compact (S, n_g, d, d) table (_constj), the latter with a set of live columns (_live).
int symode_symreg_reversed_batched(const float* x, const float* gx_, const float* jgx, int n_g, long n_problems, long n, int d,
                                   int order, int flags, const float* xi, const float* mask, float inv_count,
                                   float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    return reversed_closure(false, false, x, nullptr, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, 1.0f,
                            loss_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_loss_grad_reversed(const float* x, const float* dx, const float* gx_, const float* jgx, int n_g, long n_problems, long n,
                              int d, int order, int flags, const float* xi, const float* mask, float inv_count, float w_sym,
                              float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    return reversed_closure(true, false, x, dx, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, w_sym,
                            loss2_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_loss_grad_latent(const float* z, const float* dz, const float* B, const float* y, long n_problems, long n, int d, int order,
                            int flags, const float* xi, const float* mask, float inv_count, float w_pair, float* loss2_out,
                            float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n < 1 || n_problems < 1 || n_problems > 65535) return SYMODE_E_BADSIZE;
    if (!z || !dz || !B || !y || !xi || !loss2_out || !grad_out) return SYMODE_E_NULLPTR;
    if (misaligned(z, 4) || misaligned(dz, 4) || misaligned(B, 4) || misaligned(y, 4) || misaligned(xi, 4) || misaligned(mask, 4) ||
        misaligned(loss2_out, 4) || misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, n);
    // the grid rule of the fused reversed closure: the same 40 bytes per point at d = 2, the same partial rows
    int gx = grid_x_for(n, n_problems, ppt_for(d), 512);
    if (n_problems == 1) {
        const int cap = small_grid_cap(n, true);
        if (cap > 0 && gx > cap) gx = cap;
    }
    return (int)ops->latent_closure(z, dz, B, y, n_problems, n, xi, mask, inv_count, w_pair, loss2_out, grad_out, (double*)workspace,
                                    gx, (hipStream_t)stream);
}

int symode_symreg_reversed_batched_constj(const float* x, const float* gx_, const float* jgx, int n_g, long n_problems, long n,
                                          int d, int order, int flags, const float* xi, const float* mask, float inv_count,
                                          float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    return reversed_closure(false, true, x, nullptr, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, 1.0f,
                            loss_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_loss_grad_reversed_constj(const float* x, const float* dx, const float* gx_, const float* jgx, int n_g, long n_problems,
                                     long n, int d, int order, int flags, const float* xi, const float* mask, float inv_count,
                                     float w_sym, float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return reversed_closure(true, true, x, dx, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, w_sym,
                            loss2_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_symreg_reversed_batched_constj_live(const float* x, const float* gx_, const float* jgx, int n_g, long n_problems,
                                               long n, int d, int order, int flags, const float* xi, const float* mask,
                                               unsigned long long live_columns, float inv_count, float* loss_out,
                                               float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    return reversed_closure(false, true, x, nullptr, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, 1.0f,
                            loss_out, grad_out, workspace, workspace_bytes, stream, live_columns);
}

int symode_loss_grad_reversed_constj_live(const float* x, const float* dx, const float* gx_, const float* jgx, int n_g,
                                          long n_problems, long n, int d, int order, int flags, const float* xi,
                                          const float* mask, unsigned long long live_columns, float inv_count, float w_sym,
                                          float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    return reversed_closure(true, true, x, dx, gx_, jgx, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, w_sym,
                            loss2_out, grad_out, workspace, workspace_bytes, stream, live_columns);
}

int symode_jacobian_constant(const float* jgx, int n_g, long n_problems, long n, int d, float* table_out, int* flag_out,
                             void* stream) {
    if (d < 1 || d > 4) return SYMODE_E_UNSUPPORTED;
    if (n < 1 || n_g < 1 || n_problems < 1 || n_problems > 65535 || n_problems * (long)n_g > 2147483647L) return SYMODE_E_BADSIZE;
    if (!jgx || !table_out || !flag_out) return SYMODE_E_NULLPTR;
    if (misaligned(jgx, 4) || misaligned(table_out, 4) || misaligned(flag_out, 4)) return SYMODE_E_ALIGN;
    return (int)launch_jacobian_constant(jgx, n_problems * (long)n_g, n, d, table_out, flag_out, (hipStream_t)stream);
}

int symode_linear_action(const float* x, const float* gx_, const float* table, int n_g, long n_problems, long n, int d, int order,
                         int flags, double* m_out, int* flag_out, void* stream) {
    if (d != 2 || flags != 0 || order < 1 || order > MAX_ORDER) return SYMODE_E_UNSUPPORTED;
    if (n < 1 || n_g < 1 || n_problems < 1 || n_problems > 65535) return SYMODE_E_BADSIZE;
    if (n_g != 1) return SYMODE_E_UNSUPPORTED;
    if (!x || !gx_ || !table || !m_out || !flag_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(gx_, 4) || misaligned(table, 4) || misaligned(m_out, 8) || misaligned(flag_out, 4))
        return SYMODE_E_ALIGN;
    return (int)launch_linear_action(x, gx_, table, n_problems, n, order, m_out, flag_out, (hipStream_t)stream);
}

// The two entries of the folded linear action: g_table null is the plain one.
static int fold_closure(const float* x, const float* dx, const float* gx_, const float* table, const double* m_table,
                        const double* g_table, int n_g, long n_problems, long n, int d, int order, int flags, const float* xi,
                        const float* mask, unsigned long long live_columns, float inv_count, float w_sym, float* loss2_out,
                        float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    // where the launcher's table (or SYMODE_CLOSURE_FOLD=0) keeps the streamed kernels, this IS the _constj_live entry
    if (!ops->symreg_fold || !ops->fold_takes(live_columns))
        return reversed_closure(true, true, x, dx, gx_, table, n_g, n_problems, n, d, order, flags, xi, mask, inv_count, w_sym,
                                loss2_out, grad_out, workspace, workspace_bytes, stream, live_columns);
    if (n < 1 || n_problems < 1 || n_problems > 65535) return SYMODE_E_BADSIZE;
    if (!x || !dx || !gx_ || !table || !xi || !loss2_out || !grad_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(gx_, 4) || misaligned(table, 4) || misaligned(xi, 4) || misaligned(mask, 4) ||
        misaligned(loss2_out, 4) || misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(n_problems, n);
    return (int)ops->symreg_fold(x, dx, table, m_table, g_table, n_problems, n, xi, mask, live_columns, inv_count, w_sym, loss2_out,
                                 grad_out, (double*)workspace, reversed_closure_grid(true, ops, n_problems, n, d), (hipStream_t)stream);
}

int symode_loss_grad_reversed_linear(const float* x, const float* dx, const float* gx_, const float* table, const double* m_table,
                                     int n_g, long n_problems, long n, int d, int order, int flags, const float* xi,
                                     const float* mask, unsigned long long live_columns, float inv_count, float w_sym,
                                     float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (d != 2 || flags != 0 || order < 1 || order > MAX_ORDER) return SYMODE_E_UNSUPPORTED;
    if (n_g < 1) return SYMODE_E_BADSIZE;
    if (n_g != 1) return SYMODE_E_UNSUPPORTED;
    if (!m_table) return SYMODE_E_NULLPTR;
    if (misaligned(m_table, 8)) return SYMODE_E_ALIGN;
    return fold_closure(x, dx, gx_, table, m_table, nullptr, n_g, n_problems, n, d, order, flags, xi, mask, live_columns, inv_count,
                        w_sym, loss2_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_loss_grad_reversed_linear_gram(const float* x, const float* dx, const float* gx_, const float* table,
                                          const double* m_table, const double* g_table, int n_g, long n_problems, long n, int d,
                                          int order, int flags, const float* xi, const float* mask,
                                          unsigned long long live_columns, float inv_count, float w_sym, float* loss2_out,
                                          float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (d != 2 || flags != 0 || order < 1 || order > MAX_ORDER) return SYMODE_E_UNSUPPORTED;
    if (n_g < 1) return SYMODE_E_BADSIZE;
    if (n_g != 1) return SYMODE_E_UNSUPPORTED;
    if (!m_table || !g_table) return SYMODE_E_NULLPTR;
    if (misaligned(m_table, 8) || misaligned(g_table, 8)) return SYMODE_E_ALIGN;
    // SYMODE_FOLD_GRAM=0: the entry without the table (the launcher's own table is asked per column set, in the launch)
    return fold_closure(x, dx, gx_, table, m_table, knobs().fold_gram ? g_table : nullptr, n_g, n_problems, n, d, order, flags, xi,
                        mask, live_columns, inv_count, w_sym, loss2_out, grad_out, workspace, workspace_bytes, stream);
}

// The fold closure without a point loop (closure_quad.hpp): one kernel per library, the column set is a run-time argument.
int symode_loss_grad_reversed_linear_quad(const double* aug_table, const double* m_table, const float* table, int n_g, long n_problems,
                                          int d, int order, int flags, const float* xi, const float* q, const float* beta,
                                          long beta_stride, const float* const_, long const_stride, int r, int use_kron,
                                          const float* mask,
                                          unsigned long long live_columns, double inv_count, float w_sym, float* loss2_out,
                                          float* loss_out, float* grad_out, float* xi_out, float* g_beta_out, float* g_const_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (d != 2 || flags != 0 || order < 1 || order > 5) return SYMODE_E_UNSUPPORTED;
    if (n_g < 1 || n_problems < 1 || n_problems > 2147483647L) return SYMODE_E_BADSIZE;
    if (n_g != 1) return SYMODE_E_UNSUPPORTED;
    // the switches that keep the point-loop kernels: the caller goes to the _linear / _linear_gram entries then
    if (!knobs().closure_fold || !knobs().fold_gram || !knobs().fold_resid_gram) return SYMODE_E_UNSUPPORTED;
    const bool mapped = q != nullptr;
    if (!aug_table || !m_table || !table || !loss2_out || !grad_out) return SYMODE_E_NULLPTR;
    if (mapped ? (!beta || !g_beta_out || xi) : (!xi || beta || const_ || xi_out || g_beta_out || g_const_out)) return SYMODE_E_NULLPTR;
    if (mapped && (r < 1 || r > 2 * symode_lib_size(2, order, 0) || beta_stride < r || (const_ && const_stride < 2))) return SYMODE_E_BADSIZE;
    if (misaligned(aug_table, 8) || misaligned(m_table, 8) || misaligned(table, 4) || misaligned(xi, 4) || misaligned(q, 4) ||
        misaligned(beta, 4) || misaligned(const_, 4) || misaligned(mask, 4) || misaligned(loss2_out, 4) || misaligned(loss_out, 4) ||
        misaligned(grad_out, 4) || misaligned(xi_out, 4) || misaligned(g_beta_out, 4) || misaligned(g_const_out, 4))
        return SYMODE_E_ALIGN;
    if (!workspace || misaligned(workspace, 8) || workspace_bytes < (size_t)WS_HEADER_DOUBLES * sizeof(double)) return SYMODE_E_WORKSPACE;
    const QuadMap map{q, beta, const_, beta_stride, const_stride, r, use_kron != 0 ? 1 : 0, xi_out, g_beta_out, g_const_out};
    return (int)launch_closure_quad_order(order, aug_table, m_table, table, n_problems, xi, map, mask, live_columns, w_sym, inv_count,
                                          loss2_out, loss_out, grad_out, (double*)workspace, (hipStream_t)stream);
}

// The closure without a point loop as a quadratic form in (beta, const) (closure_reduced.hpp): the set-up and the step.
static bool quad_reduced_on() {
    return knobs().closure_fold && knobs().fold_gram && knobs().fold_resid_gram && knobs().quad_reduced;
}

int symode_quad_reduce(const double* aug_table, const double* m_table, const float* table, long n_problems, int order,
                       const float* q, int r, int use_kron, int has_const, unsigned long long live_columns, double inv_count,
                       float w_sym, const float* mask, double* b_out, void* stream) {
    if (order < 1 || order > 5 || !quad_reduced_on()) return SYMODE_E_UNSUPPORTED;
    if (n_problems < 1 || n_problems > 2147483647L) return SYMODE_E_BADSIZE;
    if (r < 1 || r > 2 * symode_lib_size(2, order, 0) || r + (has_const ? 2 : 0) + 1 > REDUCED_GROUP) return SYMODE_E_BADSIZE;
    if (!aug_table || !m_table || !table || !q || !b_out) return SYMODE_E_NULLPTR;
    if (misaligned(aug_table, 8) || misaligned(m_table, 8) || misaligned(table, 4) || misaligned(q, 4) || misaligned(mask, 4) ||
        misaligned(b_out, 8))
        return SYMODE_E_ALIGN;
    return (int)launch_quad_reduce_order(order, aug_table, m_table, table, n_problems, q, r, use_kron != 0 ? 1 : 0,
                                         has_const != 0 ? 1 : 0, mask, live_columns, w_sym, inv_count, b_out, (hipStream_t)stream);
}

int symode_quad_step(const double* b, long n_problems, int k, int d_c, int order, unsigned long long live_columns,
                     const float* beta, long beta_stride, const float* const_, long const_stride, float* loss_out,
                     float* g_beta_out, float* g_const_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (order < 1 || order > 5 || !quad_reduced_on()) return SYMODE_E_UNSUPPORTED;
    if (n_problems < 1 || n_problems > 2147483647L) return SYMODE_E_BADSIZE;
    if (k < 1 || k + 1 > REDUCED_GROUP || d_c < 0 || d_c >= k) return SYMODE_E_BADSIZE;
    if (!b || !beta || !loss_out || !g_beta_out) return SYMODE_E_NULLPTR;
    if (d_c > 0 ? (!const_ || !g_const_out) : (const_ || g_const_out)) return SYMODE_E_NULLPTR;
    if (beta_stride < k - d_c || (d_c > 0 && const_stride < d_c)) return SYMODE_E_BADSIZE;
    if (misaligned(b, 8) || misaligned(beta, 4) || misaligned(const_, 4) || misaligned(loss_out, 4) || misaligned(g_beta_out, 4) ||
        misaligned(g_const_out, 4))
        return SYMODE_E_ALIGN;
    if (!workspace || misaligned(workspace, 8) || workspace_bytes < (size_t)WS_HEADER_DOUBLES * sizeof(double)) return SYMODE_E_WORKSPACE;
    return (int)launch_quad_step(order, live_columns, b, n_problems, k, d_c, beta, beta_stride, const_, const_stride, loss_out,
                                 g_beta_out, g_const_out, (double*)workspace, (hipStream_t)stream);
}

size_t symode_symreg_reversed_gram_workspace_bytes(int d, int order, int flags, int n_g, long n_problems, long n) {
    const LibOps* ops = find_ops(d, order, flags);
    if (!ops || !ops->symreg_reversed_gram || n_g < 1 || n_problems < 1 || n < 1) return 0;
    return rev_gram_workspace_doubles(ops->d * ops->p, n_problems, n, n_g) * sizeof(double);
}

int symode_symreg_reversed_gram(const float* x, const float* gx_, const float* jgx, int n_g, long n_problems, long n, int d,
                                int order, int flags, double* gram_out, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (!ops->symreg_reversed_gram) return SYMODE_E_UNSUPPORTED;
    if (n < 1 || n_g < 1 || n_problems < 1 || n_problems > 65535) return SYMODE_E_BADSIZE;
    if (!x || !gx_ || !jgx || !gram_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(gx_, 4) || misaligned(jgx, 4) || misaligned(gram_out, 8)) return SYMODE_E_ALIGN;
    if (!workspace || misaligned(workspace, 8)) return SYMODE_E_WORKSPACE;
    if (workspace_bytes < rev_gram_workspace_doubles(ops->d * ops->p, n_problems, n, n_g) * sizeof(double)) return SYMODE_E_WORKSPACE;
    return (int)ops->symreg_reversed_gram(x, gx_, jgx, n_g, n_problems, n, nullptr, 0, gram_out, (double*)workspace,
                                          (hipStream_t)stream);
}

size_t symode_symreg_reversed_gram_gather_workspace_bytes(int d, int order, int flags, int n_g, long n_problems, long m) {
    return symode_symreg_reversed_gram_workspace_bytes(d, order, flags, n_g, n_problems, m);   // same grid, same partials
}

int symode_symreg_reversed_gram_gather(const float* x, const float* gx_, const float* jgx, int n_g, long n_src, const int* idx,
                                       long n_problems, long m, int d, int order, int flags, double* gram_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (!ops->symreg_reversed_gram) return SYMODE_E_UNSUPPORTED;
    if (m < 1 || n_g < 1 || n_problems < 1 || n_problems > 65535 || n_src < 1 || n_src > 2147483647L) return SYMODE_E_BADSIZE;
    if (!x || !gx_ || !jgx || !idx || !gram_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(gx_, 4) || misaligned(jgx, 4) || misaligned(idx, 4) || misaligned(gram_out, 8))
        return SYMODE_E_ALIGN;
    if (!workspace || misaligned(workspace, 8)) return SYMODE_E_WORKSPACE;
    if (workspace_bytes < rev_gram_workspace_doubles(ops->d * ops->p, n_problems, m, n_g) * sizeof(double)) return SYMODE_E_WORKSPACE;
    return (int)ops->symreg_reversed_gram(x, gx_, jgx, n_g, n_problems, m, idx, n_src, gram_out, (double*)workspace,
                                          (hipStream_t)stream);
}

int symode_quad_closure(const double* aug_gram, const double* rev_gram, long n_problems, int d, int p, const float* xi,
                        const float* mask, double inv_count, float w_sym, float* loss_out, float* grad_out, void* stream) {
    if (n_problems < 1 || d < 1 || p < 1 || d * p > QUAD_MAX_DP) return SYMODE_E_BADSIZE;
    if (!aug_gram || !xi || !loss_out || !grad_out) return SYMODE_E_NULLPTR;
    if (misaligned(aug_gram, 8) || misaligned(rev_gram, 8) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(loss_out, 4) ||
        misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    return (int)launch_quad_closure(aug_gram, rev_gram, n_problems, d, p, xi, mask, inv_count, w_sym, loss_out, grad_out,
                                    (hipStream_t)stream);
}

int symode_quad_closure_grid(const double* aug_gram, const double* rev_gram, long n_sets, long n_problems, int d, int p,
                             const float* xi, const float* mask, double inv_count, const float* hyper, float* loss_out,
                             float* grad_out, void* stream) {
    if (n_problems < 1 || n_problems > 2147483647L || d < 1 || p < 1 || d * p > QUAD_MAX_DP) return SYMODE_E_BADSIZE;
    if (n_sets < 1 || n_problems % n_sets != 0) return SYMODE_E_BADSIZE;
    if (!aug_gram || !xi || !hyper || !loss_out || !grad_out) return SYMODE_E_NULLPTR;
    if (misaligned(aug_gram, 8) || misaligned(rev_gram, 8) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(hyper, 4) ||
        misaligned(loss_out, 4) || misaligned(grad_out, 4))
        return SYMODE_E_ALIGN;
    return (int)launch_quad_closure_grid(aug_gram, rev_gram, (int)n_sets, n_problems, d, p, xi, mask, inv_count, hyper, loss_out,
                                         grad_out, (hipStream_t)stream);
}

int symode_stlsq_sweep(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points, const float* hyper,
                       double gamma, double threshold, int max_iter, double near_band, float* xi_out, unsigned char* mask_out,
                       int* passes_out, int* near_out, int* fell_out, void* stream) {
    (void)n_points;                     // the rows behind a matrix: gelsy's rank rule reads them, the full-rank driver does not
    if (stlsq_bad_library(d, p) || max_iter < 1 || stlsq_bad_problems(n_sets, n_problems, hyper != nullptr)) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, xi_out, mask_out, passes_out, near_out, fell_out)) return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram) || any_misaligned(4, hyper, xi_out, passes_out, near_out, fell_out)) return SYMODE_E_ALIGN;
    return (int)launch_stlsq_sweep(aug_gram, n_sets, n_problems, d, p, hyper, gamma, threshold, max_iter, near_band, xi_out,
                                   mask_out, passes_out, near_out, fell_out, (hipStream_t)stream);
}

int symode_stlsq_path(const double* aug_gram, const double* val_gram, long n_sets, long n_val_sets, long n_problems, int d, int p,
                      long n_points, double gamma, double tol, double floor_rel, double near_band, float* path_xi, int* order,
                      double* rss_train, double* rss_val, int* best, float* xi_out, unsigned char* mask_out, int* near_out,
                      int* fell_out, void* stream) {
    (void)n_points;                     // as symode_stlsq_sweep: only gelsy's rank rule would read it
    if (stlsq_bad_library(d, p) || stlsq_bad_problems(n_sets, n_problems, true) || stlsq_bad_val_sets(n_val_sets, n_problems))
        return SYMODE_E_BADSIZE;
    if (!all_finite_nonneg({gamma, tol, floor_rel, near_band})) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, val_gram, path_xi, order, rss_train, rss_val, best, xi_out, mask_out, near_out, fell_out))
        return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, val_gram, rss_train, rss_val) || any_misaligned(4, path_xi, order, best, xi_out, near_out, fell_out))
        return SYMODE_E_ALIGN;
    return (int)launch_stlsq_path(aug_gram, val_gram, n_sets, n_val_sets, n_problems, d, p, gamma, tol, floor_rel, near_band, path_xi,
                                  order, rss_train, rss_val, best, xi_out, mask_out, near_out, fell_out, (hipStream_t)stream);
}

int symode_gram_resample(const double* chunk, const long long* seeds, long n_seeds, int n_chunks, int n, int n_replicas, double* out,
                         int* counts_out, void* stream) {
    if (n_chunks < 1 || n_chunks > RESAMPLE_MAX_CHUNKS || n < 1 || n > RESAMPLE_MAX_N || n_replicas < 1 || n_seeds < 1 ||
        n_seeds > 2147483647L)
        return SYMODE_E_BADSIZE;
    if (stlsq_bad_problems(n_seeds, n_seeds * n_replicas, true)) return SYMODE_E_BADSIZE;   // the replicas are the sweep's problems
    if (any_null(chunk, seeds, out)) return SYMODE_E_NULLPTR;
    if (any_misaligned(8, chunk, seeds, out) || any_misaligned(4, counts_out)) return SYMODE_E_ALIGN;
    return (int)launch_gram_resample(chunk, seeds, n_seeds, n_chunks, n, n_replicas, out, counts_out, (hipStream_t)stream);
}

int symode_stlsq_bag(const double* aug_gram, long n_seeds, long n_problems, int d, int p, int n_replicas, const float* rep_xi,
                     const unsigned char* rep_mask, const int* rep_fell, const int* tau_table, int tau_milli, double gamma,
                     float* xi_out, unsigned char* mask_out, int* fell_out, int* count_out, int* valid_out, double* mean_out,
                     double* std_out, void* stream) {
    if (stlsq_bad_library(d, p) || stlsq_bad_problems(n_seeds, n_problems, true) || n_problems % n_seeds != 0) return SYMODE_E_BADSIZE;
    if (n_replicas < 1 || stlsq_bad_problems(n_seeds, n_seeds * n_replicas, true)) return SYMODE_E_BADSIZE;
    if (!tau_table && (tau_milli < 0 || tau_milli > STLSQ_BAG_TAU_MAX)) return SYMODE_E_BADSIZE;
    if (!all_finite_nonneg({gamma})) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, rep_xi, rep_mask, rep_fell, xi_out, mask_out, fell_out, count_out, valid_out, mean_out, std_out))
        return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, mean_out, std_out) || any_misaligned(4, rep_xi, rep_fell, tau_table, xi_out, fell_out, count_out, valid_out))
        return SYMODE_E_ALIGN;
    return (int)launch_stlsq_bag(aug_gram, n_seeds, n_problems, d, p, n_replicas, rep_xi, rep_mask, rep_fell, tau_table, tau_milli, gamma,
                                 xi_out, mask_out, fell_out, count_out, valid_out, mean_out, std_out, (hipStream_t)stream);
}

int symode_stlsq_sweep_constrained(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points,
                                   const double* q_solve, const float* q_xi, int r, int allow_constant, const float* hyper,
                                   double gamma, double threshold, int max_iter, double near_band, double pivot_floor, float* xi_out,
                                   float* var_out, unsigned char* mask_out, int* passes_out, int* near_out, int* fell_out,
                                   void* stream) {
    (void)n_points;                     // as symode_stlsq_sweep: only gelsy's rank rule would read it
    if (stlsq_bad_library(d, p) || max_iter < 1 || stlsq_bad_free(d, p, r, allow_constant)) return SYMODE_E_BADSIZE;
    if (stlsq_bad_problems(n_sets, n_problems, hyper != nullptr) || !all_finite_nonneg({pivot_floor})) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, q_solve, q_xi, xi_out, var_out, mask_out, passes_out, near_out, fell_out)) return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, q_solve) || any_misaligned(4, q_xi, hyper, xi_out, var_out, passes_out, near_out, fell_out))
        return SYMODE_E_ALIGN;
    return (int)launch_stlsq_constrained(aug_gram, n_sets, n_problems, d, p, q_solve, q_xi, r, allow_constant ? 1 : 0, hyper, gamma,
                                         threshold, max_iter, near_band, pivot_floor, xi_out, var_out, mask_out, passes_out,
                                         near_out, fell_out, (hipStream_t)stream);
}

int symode_stlsq_sweep_minnorm(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points,
                               const double* q_solve, const float* q_xi, int r, int allow_constant, const float* hyper, double gamma,
                               double threshold, int max_iter, double near_band, double rcond, float* xi_out, float* var_out,
                               unsigned char* mask_out, int* passes_out, int* near_out, int* fell_out, int* trunc_out, int* rank_out,
                               void* stream) {
    (void)n_points;                     // as symode_stlsq_sweep: only gelsy's DEFAULT rank rule would read it
    if (stlsq_bad_library(d, p) || max_iter < 1 || stlsq_bad_free(d, p, r, allow_constant)) return SYMODE_E_BADSIZE;
    if (stlsq_bad_problems(n_sets, n_problems, hyper != nullptr)) return SYMODE_E_BADSIZE;
    if (!std::isfinite(rcond) || !(rcond > 0.0) || !(rcond < 1.0)) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, q_solve, q_xi, xi_out, var_out, mask_out, passes_out, near_out, fell_out, trunc_out, rank_out))
        return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, q_solve) ||
        any_misaligned(4, q_xi, hyper, xi_out, var_out, passes_out, near_out, fell_out, trunc_out, rank_out))
        return SYMODE_E_ALIGN;
    return (int)launch_stlsq_minnorm(aug_gram, n_sets, n_problems, d, p, q_solve, q_xi, r, allow_constant ? 1 : 0, hyper, gamma,
                                     threshold, max_iter, near_band, rcond, xi_out, var_out, mask_out, passes_out, near_out, fell_out,
                                     trunc_out, rank_out, (hipStream_t)stream);
}

int symode_stlsq_sweep_symreg(const double* aug_gram, const double* rev_gram, long n_sets, long n_problems, int d, int p,
                              long n_points, const float* hyper, double gamma, double threshold, double w_sym, int max_iter,
                              double near_band, double pivot_floor, float* xi_out, unsigned char* mask_out, int* passes_out,
                              int* near_out, int* fell_out, void* stream) {
    (void)n_points;                     // as symode_stlsq_sweep: only gelsy's rank rule would read it
    if (stlsq_bad_library(d, p) || (long)d * p > STLSQS_MAX_DP || max_iter < 1) return SYMODE_E_BADSIZE;
    if (stlsq_bad_problems(n_sets, n_problems, hyper != nullptr)) return SYMODE_E_BADSIZE;
    // gamma, threshold and w_sym as the launch holds them
    if (!all_finite_nonneg({(double)(float)gamma, (double)(float)threshold, (double)(float)w_sym, pivot_floor})) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, rev_gram, xi_out, mask_out, passes_out, near_out, fell_out)) return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, rev_gram) || any_misaligned(4, hyper, xi_out, passes_out, near_out, fell_out)) return SYMODE_E_ALIGN;
    // the three values in fp32, as a row of the table holds them
    return (int)launch_stlsq_symreg(aug_gram, rev_gram, n_sets, n_problems, d, p, hyper, (float)gamma, (float)threshold, (float)w_sym,
                                    max_iter, near_band, pivot_floor, xi_out, mask_out, passes_out, near_out, fell_out,
                                    (hipStream_t)stream);
}

int symode_stlsq_path_symreg(const double* aug_gram, const double* rev_gram, const double* val_gram, long n_sets, long n_val_sets,
                             long n_problems, int d, int p, long n_points, const float* hyper, double gamma, double w_sym, double tol,
                             double floor_rel, double near_band, double pivot_floor, float* path_xi, int* order, double* mse_train,
                             double* reg_train, double* mse_val, int* best, float* xi_out, unsigned char* mask_out, int* near_out,
                             int* fell_out, void* stream) {
    (void)n_points;                     // as symode_stlsq_sweep: only gelsy's rank rule would read it
    if (stlsq_bad_library(d, p) || (long)d * p > STLSQS_MAX_DP) return SYMODE_E_BADSIZE;
    if (stlsq_bad_problems(n_sets, n_problems, true) || stlsq_bad_val_sets(n_val_sets, n_problems)) return SYMODE_E_BADSIZE;
    // gamma and w_sym as the launch holds them
    if (!all_finite_nonneg({(double)(float)gamma, (double)(float)w_sym, tol, floor_rel, near_band, pivot_floor})) return SYMODE_E_BADSIZE;
    if (any_null(aug_gram, rev_gram, val_gram, path_xi, order, mse_train, reg_train, mse_val, best, xi_out, mask_out, near_out, fell_out))
        return SYMODE_E_NULLPTR;
    if (any_misaligned(8, aug_gram, rev_gram, val_gram, mse_train, reg_train, mse_val) ||
        any_misaligned(4, hyper, path_xi, order, best, xi_out, near_out, fell_out))
        return SYMODE_E_ALIGN;
    // the two values in fp32, as a row of the table holds them
    return (int)launch_stlsq_path_symreg(aug_gram, rev_gram, val_gram, n_sets, n_val_sets, n_problems, d, p, hyper, (float)gamma,
                                         (float)w_sym, tol, floor_rel, near_band, pivot_floor, path_xi, order, mse_train, reg_train,
                                         mse_val, best, xi_out, mask_out, near_out, fell_out, (hipStream_t)stream);
}

int symode_symreg_reversed(const float* x, const float* gx_, const float* jgx, int n_g, long n, int d, int order,
                           int flags, const float* xi, const float* mask, float* loss_out, float* grad_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1 || d < 1) return SYMODE_E_BADSIZE;
    return reversed_closure(false, false, x, nullptr, gx_, jgx, n_g, 1, n, d, order, flags, xi, mask, 1.0f / ((float)n * (float)d),
                            1.0f, loss_out, grad_out, workspace, workspace_bytes, stream);
}

int symode_weak_gram(const float* x, long n_t, int d, int order, int flags, const float* V, const float* V_drv, int n_test,
                     double* out, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n_t < 1 || n_test < 1 || n_test > 128) return SYMODE_E_BADSIZE;
    if (!x || !V || !V_drv || !out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(V, 4) || misaligned(V_drv, 4) || misaligned(out, 8)) return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(1, n_t);
    const int RT = (2 * n_test + 15) / 16, CT = (ops->p + ops->d + 15) / 16;
    long gx = weak_slabs(n_t);
    const size_t avail = workspace_bytes / sizeof(double) - (size_t)WS_HEADER_DOUBLES;
    while (gx > 1 && (size_t)gx * RT * CT * 256 > avail) gx /= 2;
    if ((size_t)gx * RT * CT * 256 > avail) return SYMODE_E_WORKSPACE;
    return (int)ops->weak_gram(x, n_t, V, V_drv, n_test, out, (double*)workspace, (int)gx, (hipStream_t)stream);
}

int symode_weak_normal_windows(const float* x, long n_ics, long n_steps, int d, int order, int flags, const int* windows,
                               long n_windows, long n_t, const float* V, const float* V_drv, int n_test, const double* M,
                               double* aug_out, double* z_out, int* bad_out, void* workspace, size_t workspace_bytes,
                               void* stream) {
    SYMODE_GET_OPS();
    if (n_t < 1 || n_t > n_steps || n_ics < 1 || n_windows < 1 || n_windows > 65535 || n_test < 1 || n_test > WEAK_NORMAL_MAX_K)
        return SYMODE_E_BADSIZE;
    if (ops->p > STLSQ_MAX_P || d > STLSQ_MAX_D) return SYMODE_E_BADSIZE;          // what symode_stlsq_sweep takes
    if (!x || !windows || !V || !V_drv || !M || !aug_out || !bad_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(windows, 4) || misaligned(V, 4) || misaligned(V_drv, 4) || misaligned(M, 8) ||
        misaligned(aug_out, 8) || misaligned(z_out, 8) || misaligned(bad_out, 4))
        return SYMODE_E_ALIGN;
    if (!workspace || misaligned(workspace, 8)) return SYMODE_E_WORKSPACE;
    // symode_weak_gram's slab count for n_t, never halved: window s's partials are then that entry's, addition by addition
    const long gx = weak_slabs(n_t);
    const size_t RT = (size_t)(2 * n_test + 15) / 16, CT = (size_t)(ops->p + ops->d + 15) / 16;
    const size_t need = (size_t)WS_HEADER_DOUBLES + (size_t)n_windows * RT * (size_t)gx * CT * 256;
    if (workspace_bytes / sizeof(double) < need) return SYMODE_E_WORKSPACE;
    double* part = (double*)workspace + WS_HEADER_DOUBLES;
    const hipError_t e = ops->weak_windows(x, n_ics, n_steps, windows, n_windows, n_t, V, V_drv, n_test, part, (int)gx, bad_out,
                                           (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return (int)launch_weak_normal(part, (int)gx, n_windows, n_test, ops->p, ops->d, M, aug_out, z_out, (hipStream_t)stream);
}

int symode_vjp(const float* x, const float* g, long n, int d, int order, int flags, const float* xi, const float* mask,
               float* grad_x, float* grad_xi, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n < 1) return SYMODE_E_BADSIZE;
    if (!x || !g || !xi || !grad_xi) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(g, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(grad_x, 4) ||
        misaligned(grad_xi, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(1, n);
    // register ring of 3 chunks per lane: one workgroup per CU streams best from 4 M points up (round 3,
    // profiles/r03_stream_ab.txt: 64 M points 262 us at 256 workgroups against 321 at 1024; without grad_x 152 against 188)
    // (order 5, d p = 42: the second workgroup per CU pays from 8 M points -- 2^26 points 316 -> 295 us; orders 3-4 lose 8-11 % on it)
    const bool heavy = ops->d * ops->p > 32 && grad_x != nullptr;        // (without grad_x one per CU stays best: 163 against 175 us)
    const int gx = single_problem_grid(grid_x_for(n, 1, ppt_for(d)), n, 64, 128, heavy ? 512 : 256, heavy ? 512 : 256);
    return (int)ops->vjp(x, g, n, xi, mask, grad_x, grad_xi, (double*)workspace, gx, (hipStream_t)stream);
}

int symode_forward_jvp(const float* x, const float* v, long n, int d, int order, int flags, const float* xi,
                       const float* mask, float* out, float* jv, void* stream) {
    SYMODE_GET_OPS();
    if (n < 0) return SYMODE_E_BADSIZE;
    if (n == 0) return SYMODE_OK;
    if (!x || !v || !xi || !jv) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(v, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(out, 4) ||
        misaligned(jv, 4))
        return SYMODE_E_ALIGN;
    return (int)ops->forward_jvp(x, v, n, xi, mask, out, jv, (hipStream_t)stream);
}

int symode_jvp_vjp(const float* x, const float* v, const float* g_out, const float* g_jv, long n, int d, int order,
                   int flags, const float* xi, const float* mask, float* grad_x, float* grad_v, float* grad_xi,
                   void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n < 1) return SYMODE_E_BADSIZE;
    if (!x || !v || !g_jv || !xi || !grad_x || !grad_v || !grad_xi) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(v, 4) || misaligned(g_out, 4) || misaligned(g_jv, 4) || misaligned(xi, 4) ||
        misaligned(mask, 4) || misaligned(grad_x, 4) || misaligned(grad_v, 4) || misaligned(grad_xi, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(1, n);
    // ring of 3: r03_stream_ab.txt.  Order 5 (d p = 42) wants more than one workgroup per CU: 2^26 points, us at 256 / 512 /
    // 768 workgroups 693 / 652 / 646 on one box, 727 / - / 672-694 on another; 8 M points 94 -> 82 us at 512.  Orders 3-4
    // stay at one per CU (768 won on one box, 531 against 546 us, and lost on the next, 586-602 against 545-567)
    const bool heavy = ops->d * ops->p > 32;
    const int gx = single_problem_grid(grid_x_for(n, 1, ppt_for(d)), n, 128, 256, heavy ? 512 : 256, heavy ? 768 : 256);
    return (int)ops->jvp_vjp(x, v, g_out, g_jv, n, xi, mask, grad_x, grad_v, grad_xi, (double*)workspace, gx,
                             (hipStream_t)stream);
}

int symode_rk4_traj(const double* x0, long n_traj, int d, int order, int flags, const double* xi, int n_steps, double dt,
                    int subsample, float* x_out, float* dx_out, void* stream) {
    SYMODE_GET_OPS();
    if (n_traj < 0 || n_steps < 1 || subsample < 1) return SYMODE_E_BADSIZE;
    if (n_traj == 0) return SYMODE_OK;
    if (!x0 || !xi || !x_out || !dx_out) return SYMODE_E_NULLPTR;
    if (misaligned(x0, 8) || misaligned(xi, 8) || misaligned(x_out, 4) || misaligned(dx_out, 4)) return SYMODE_E_ALIGN;
    return (int)ops->rk4_traj(x0, n_traj, xi, n_steps, dt, subsample, x_out, dx_out, (hipStream_t)stream);
}

int symode_euler_jvp(const float* x, const float* v, long n, int d, int order, int flags, const float* xi,
                     const float* mask, int n_steps, float dt, float* x_out, float* t_out, void* stream) {
    SYMODE_GET_OPS();
    if (n < 0 || n_steps < 0) return SYMODE_E_BADSIZE;
    if (n == 0) return SYMODE_OK;
    if (!x || !v || !xi || !x_out || !t_out) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(v, 4) || misaligned(xi, 4) || misaligned(mask, 4) || misaligned(x_out, 4) ||
        misaligned(t_out, 4))
        return SYMODE_E_ALIGN;
    return (int)ops->euler_jvp(x, v, n, xi, mask, n_steps, dt, x_out, t_out, (hipStream_t)stream);
}

int symode_euler_jvp_vjp(const float* x, const float* v, const float* g_x, const float* g_t, long n, int d, int order,
                         int flags, const float* xi, const float* mask, int n_steps, float dt, float* grad_x,
                         float* grad_v, float* grad_xi, void* workspace, size_t workspace_bytes, void* stream) {
    SYMODE_GET_OPS();
    if (n < 1 || n_steps < 0) return SYMODE_E_BADSIZE;
    if (!x || !v || !g_x || !g_t || !xi || !grad_x || !grad_v || !grad_xi) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(v, 4) || misaligned(g_x, 4) || misaligned(g_t, 4) || misaligned(xi, 4) ||
        misaligned(mask, 4) || misaligned(grad_x, 4) || misaligned(grad_v, 4) || misaligned(grad_xi, 4))
        return SYMODE_E_ALIGN;
    SYMODE_CHECK_WS(1, n);
    const int gx = grid_x_for(n, 1, ppt_for(d));
    return (int)ops->euler_jvp_vjp(x, v, g_x, g_t, n, xi, mask, n_steps, dt, grad_x, grad_v, grad_xi,
                                   (double*)workspace, gx, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// symode_adam_order_table: the (n_epochs, n_seeds, per) rows the keyed epoch kernels compute in their index slot, per =
// n_steps * batch positions of which those from n_src on are the pad.  blockIdx.y strides over the (epoch, seed) tables,
// blockIdx.x over the positions of one.
__global__ __launch_bounds__(ADAM_BLOCK) void adam_order_table_kernel(int n_src, long per, const long long* __restrict__ seeds,
                                                                      long n_seeds, int shuffle, int epoch0, long tables,
                                                                      int* __restrict__ out) {
    for (long t = blockIdx.y; t < tables; t += gridDim.y) {
        const long e = t / n_seeds, sp = t % n_seeds;
        const AdamOrderKey key = adam_order_key(seed_words((unsigned long long)seeds[sp]), epoch0 + (int)e);
        for (long pos = (long)blockIdx.x * ADAM_BLOCK + threadIdx.x; pos < per; pos += (long)gridDim.x * ADAM_BLOCK) {
            int i = -1;
            if (pos < n_src) i = shuffle ? adam_order_row(key, n_src, (int)pos) : (int)pos;
            out[t * per + pos] = i;
        }
    }
}

// the operands symode_adam_epochs_latent has beyond z, dz
struct AdamLatent {
    const float *B, *y, *e, *L;
    int d_obs, n_gen;
    float w_obs, w_sym;
};

// what the keyed entries take in place of (idx, n_idx_problems, n_steps)
struct AdamOrder {
    const long long* seeds;
    long n_seeds;
    int shuffle;
};

// symode_adam_epochs (gx_, jgx null, n_g 0, kind ADAM_PLAIN), symode_adam_epochs_reversed and symode_adam_epochs_latent (lat
// set; x, dx are z, dz and w_x is w_z): one set of argument checks.  The keyed entries pass ord (idx null, n_idx_problems and
// n_steps unused: the order seeds take the table's place and n_steps is ceil(n_src / batch)).  symode_adam_run alone passes
// hyper, the per-problem (n_problems, 4) table that takes the place of lr, w_reg, threshold and w_sym (adam.hpp).
int adam_epochs(AdamKind kind, const AdamLatent* lat, const AdamOrder* ord, const float* x, const float* dx, const float* gx_, const float* jgx, int n_g,
                long n_src, const int* idx, long n_idx_problems, int n_epochs, int n_steps, int batch, long n_problems, int d,
                int order, int flags, const float* q_eff, int r, int allow_constant, int n_params, float lr, float beta1,
                float beta2, float eps, float w_x, float w_reg, float w_sym, int l1, float threshold, int st_freq, int epoch0,
                float near_band, float* params, float* m, float* v, int* step, float* mask, float* xi_out, float* log,
                const float* hyper, void* stream) {
    SYMODE_GET_OPS();
    if (n_epochs < 0 || n_problems < 0 || n_g < 0 || (lat && lat->n_gen < 0)) return SYMODE_E_BADSIZE;
    if (n_epochs == 0 || n_problems == 0) return SYMODE_OK;
    // the regulariser's gradient is accumulated at weight w_sym / w_x next to the residual's (adam.hpp): it needs w_x > 0
    if (n_g > 0 && !(w_x > 0.0f)) return SYMODE_E_BADSIZE;
    // latent: the same for w_sym / w_z, and without w_z no data term reaches the coefficients at all (mse_x has no gradient)
    if (lat && (!(w_x > 0.0f) || lat->d_obs < d || (!lat->e && lat->d_obs > d) || (!lat->L && lat->n_gen > 0)))
        return SYMODE_E_BADSIZE;
    if (ord) {
        if (n_src < 1 || n_src > 2147483647L || batch < 1) return SYMODE_E_BADSIZE;
        n_idx_problems = ord->n_seeds;
        n_steps = (int)((n_src + batch - 1) / batch);
    }
    if (n_problems > 2147483647L || n_src < 1 || n_src > 2147483647L || n_steps < 1 || batch < 1 || epoch0 < 0)
        return SYMODE_E_BADSIZE;
    if (n_idx_problems != 1 && n_idx_problems != n_problems) return SYMODE_E_BADSIZE;
    // thread j of the problem's workgroup owns parameter j: [beta | const] under the constraint, Xi without
    if (q_eff ? (r < 1 || n_params != r + d) : (n_params != d * ops->p)) return SYMODE_E_BADSIZE;
    if (n_params > ADAM_BLOCK || d * ops->p > ADAM_BLOCK) return SYMODE_E_BADSIZE;
    if (!x || !dx || (ord ? !ord->seeds : !idx) || !params || !m || !v || !step || !mask || !xi_out || !log) return SYMODE_E_NULLPTR;
    if (n_g > 0 && (!gx_ || !jgx)) return SYMODE_E_NULLPTR;
    if (lat && (!lat->B || !lat->y)) return SYMODE_E_NULLPTR;
    if (misaligned(x, 4) || misaligned(dx, 4) || misaligned(idx, 4) || misaligned(q_eff, 4) || misaligned(params, 4) ||
        misaligned(m, 4) || misaligned(v, 4) || misaligned(step, 4) || misaligned(mask, 4) || misaligned(xi_out, 4) ||
        misaligned(log, 4) || (n_g > 0 && (misaligned(gx_, 4) || misaligned(jgx, 4))))
        return SYMODE_E_ALIGN;
    if (lat && (misaligned(lat->B, 4) || misaligned(lat->y, 4) || (lat->d_obs > d && misaligned(lat->e, 4)) ||
                (lat->n_gen > 0 && misaligned(lat->L, 4))))
        return SYMODE_E_ALIGN;
    if (ord && misaligned(ord->seeds, 8)) return SYMODE_E_ALIGN;
    if (misaligned(hyper, 4)) return SYMODE_E_ALIGN;
    AdamArgs a{x, dx, n_src, ord ? nullptr : idx, n_idx_problems, n_epochs, n_steps, batch, n_problems, q_eff, q_eff ? r : 0,
               allow_constant != 0, n_params, lr, beta1, beta2, eps, w_x, w_reg, l1, threshold, st_freq, epoch0,
               near_band, params, m, v, step, mask, xi_out, log, n_g > 0 ? gx_ : nullptr, n_g > 0 ? jgx : nullptr, n_g,
               n_g > 0 ? w_sym / w_x : 0.0f};
    a.hyper = hyper;
    if (ord) {
        a.order_seeds = ord->seeds;
        a.n_order_seeds = ord->n_seeds;
        a.shuffle = ord->shuffle != 0;
    }
    if (lat) {
        a.lat_b = lat->B;
        a.lat_y = lat->y;
        a.lat_e = lat->d_obs > d ? lat->e : nullptr;          // D_obs == d: every e_b is 0, the array is not read
        a.gen_l = lat->n_gen > 0 ? lat->L : nullptr;
        a.n_gen = lat->n_gen;
        a.d_obs = lat->d_obs;
        a.w_obs = lat->w_obs;
        a.w_sym = lat->w_sym;
        a.w_ratio = lat->n_gen > 0 ? lat->w_sym / w_x : 0.0f;
        return (int)ops->adam_epochs_latent(a, (hipStream_t)stream);
    }
    return (int)(kind == ADAM_REVERSED ? ops->adam_epochs_reversed(a, (hipStream_t)stream) : ops->adam_epochs(a, (hipStream_t)stream));
}

}  // namespace

extern "C" {

int symode_adam_epochs(const float* x, const float* dx, long n_src, const int* idx, long n_idx_problems, int n_epochs,
                       int n_steps, int batch, long n_problems, int d, int order, int flags, const float* q_eff, int r,
                       int allow_constant, int n_params, float lr, float beta1, float beta2, float eps, float w_x, float w_reg,
                       int l1, float threshold, int st_freq, int epoch0, float near_band, float* params, float* m, float* v,
                       int* step, float* mask, float* xi_out, float* log, void* stream) {
    return adam_epochs(ADAM_PLAIN, nullptr, nullptr, x, dx, nullptr, nullptr, 0, n_src, idx, n_idx_problems, n_epochs, n_steps, batch, n_problems, d,
                       order, flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_x, w_reg, 0.0f, l1, threshold,
                       st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_epochs_reversed(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_src,
                                const int* idx, long n_idx_problems, int n_epochs, int n_steps, int batch, long n_problems,
                                int d, int order, int flags, const float* q_eff, int r, int allow_constant, int n_params,
                                float lr, float beta1, float beta2, float eps, float w_x, float w_reg, float w_sym, int l1,
                                float threshold, int st_freq, int epoch0, float near_band, float* params, float* m, float* v,
                                int* step, float* mask, float* xi_out, float* log, void* stream) {
    return adam_epochs(ADAM_REVERSED, nullptr, nullptr, x, dx, gx, jgx, n_g, n_src, idx, n_idx_problems, n_epochs, n_steps, batch, n_problems, d, order,
                       flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_x, w_reg, w_sym, l1, threshold,
                       st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_epochs_latent(const float* z, const float* dz, const float* B, const float* y, const float* e, int D_obs,
                              const float* L, int n_gen, long n_src, const int* idx, long n_idx_problems, int n_epochs,
                              int n_steps, int batch, long n_problems, int d, int order, int flags, const float* q_eff, int r,
                              int allow_constant, int n_params, float lr, float beta1, float beta2, float eps, float w_z,
                              float w_x, float w_reg, float w_sym, int l1, float threshold, int st_freq, int epoch0,
                              float near_band, float* params, float* m, float* v, int* step, float* mask, float* xi_out,
                              float* log, void* stream) {
    const AdamLatent lat{B, y, e, L, D_obs, n_gen, w_x, w_sym};
    return adam_epochs(ADAM_LATENT, &lat, nullptr, z, dz, nullptr, nullptr, 0, n_src, idx, n_idx_problems, n_epochs, n_steps, batch,
                       n_problems, d, order, flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_z, w_reg, 0.0f, l1,
                       threshold, st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_epochs_keyed(const float* x, const float* dx, long n_src, const long long* order_seeds, long n_order_seeds,
                             int shuffle, int n_epochs, int batch, long n_problems, int d, int order, int flags,
                             const float* q_eff, int r, int allow_constant, int n_params, float lr, float beta1, float beta2,
                             float eps, float w_x, float w_reg, int l1, float threshold, int st_freq, int epoch0,
                             float near_band, float* params, float* m, float* v, int* step, float* mask, float* xi_out,
                             float* log, void* stream) {
    const AdamOrder ord{order_seeds, n_order_seeds, shuffle};
    return adam_epochs(ADAM_PLAIN, nullptr, &ord, x, dx, nullptr, nullptr, 0, n_src, nullptr, 0, n_epochs, 0, batch, n_problems, d,
                       order, flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_x, w_reg, 0.0f, l1, threshold,
                       st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_epochs_reversed_keyed(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_src,
                                      const long long* order_seeds, long n_order_seeds, int shuffle, int n_epochs, int batch,
                                      long n_problems, int d, int order, int flags, const float* q_eff, int r,
                                      int allow_constant, int n_params, float lr, float beta1, float beta2, float eps,
                                      float w_x, float w_reg, float w_sym, int l1, float threshold, int st_freq, int epoch0,
                                      float near_band, float* params, float* m, float* v, int* step, float* mask,
                                      float* xi_out, float* log, void* stream) {
    const AdamOrder ord{order_seeds, n_order_seeds, shuffle};
    return adam_epochs(ADAM_REVERSED, nullptr, &ord, x, dx, gx, jgx, n_g, n_src, nullptr, 0, n_epochs, 0, batch, n_problems, d, order,
                       flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_x, w_reg, w_sym, l1, threshold,
                       st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_epochs_latent_keyed(const float* z, const float* dz, const float* B, const float* y, const float* e, int D_obs,
                                    const float* L, int n_gen, long n_src, const long long* order_seeds, long n_order_seeds,
                                    int shuffle, int n_epochs, int batch, long n_problems, int d, int order, int flags,
                                    const float* q_eff, int r, int allow_constant, int n_params, float lr, float beta1,
                                    float beta2, float eps, float w_z, float w_x, float w_reg, float w_sym, int l1,
                                    float threshold, int st_freq, int epoch0, float near_band, float* params, float* m,
                                    float* v, int* step, float* mask, float* xi_out, float* log, void* stream) {
    const AdamLatent lat{B, y, e, L, D_obs, n_gen, w_x, w_sym};
    const AdamOrder ord{order_seeds, n_order_seeds, shuffle};
    return adam_epochs(ADAM_LATENT, &lat, &ord, z, dz, nullptr, nullptr, 0, n_src, nullptr, 0, n_epochs, 0, batch, n_problems, d,
                       order, flags, q_eff, r, allow_constant, n_params, lr, beta1, beta2, eps, w_z, w_reg, 0.0f, l1, threshold,
                       st_freq, epoch0, near_band, params, m, v, step, mask, xi_out, log, nullptr, stream);
}

int symode_adam_run(const symode_adam_job* J, void* stream) {
    if (!J) return SYMODE_E_NULLPTR;
    if (J->kind != SYMODE_ADAM_PLAIN && J->kind != SYMODE_ADAM_REVERSED && J->kind != SYMODE_ADAM_LATENT) return SYMODE_E_BADSIZE;
    if ((J->idx != nullptr) == (J->order_seeds != nullptr)) return SYMODE_E_BADSIZE;      // the table or the order seeds: one of them
    const bool rev = J->kind == SYMODE_ADAM_REVERSED, latent = J->kind == SYMODE_ADAM_LATENT, per_problem = J->hyper != nullptr;
    // pointers and counts of another kind are never read; with the table the four scalars it replaces are not either
    const AdamLatent lat{J->lat_B, J->lat_y, J->lat_e, J->lat_L, J->D_obs, J->n_gen, J->w_obs, per_problem ? 0.0f : J->w_sym};
    const AdamOrder ord{J->order_seeds, J->n_order_seeds, J->shuffle};
    return adam_epochs((AdamKind)J->kind, latent ? &lat : nullptr, J->order_seeds ? &ord : nullptr, J->x, J->dx, rev ? J->gx : nullptr,
                       rev ? J->jgx : nullptr, rev ? J->n_g : 0, J->n_src, J->idx, J->n_idx_problems, J->n_epochs, J->n_steps, J->batch,
                       J->n_problems, J->d, J->order, J->flags, J->q_eff, J->r, J->allow_constant, J->n_params,
                       per_problem ? 0.0f : J->lr, J->beta1, J->beta2, J->eps, J->w_x, per_problem ? 0.0f : J->w_reg,
                       rev && !per_problem ? J->w_sym : 0.0f, J->l1, per_problem ? 0.0f : J->threshold, J->st_freq, J->epoch0, J->near_band,
                       J->params, J->m, J->v, J->step, J->mask, J->xi_out, J->log, J->hyper, stream);
}

int symode_adam_order_table(long n_src, int batch, const long long* order_seeds, long n_order_seeds, int shuffle, int epoch0,
                            int n_epochs, int* idx_out, void* stream) {
    if (n_src < 1 || n_src > 2147483647L || batch < 1 || n_order_seeds < 1 || n_order_seeds > 2147483647L || n_epochs < 0 ||
        epoch0 < 0)
        return SYMODE_E_BADSIZE;
    if (n_epochs == 0) return SYMODE_OK;
    if (!order_seeds || !idx_out) return SYMODE_E_NULLPTR;
    if (misaligned(order_seeds, 8) || misaligned(idx_out, 4)) return SYMODE_E_ALIGN;
    const long per = (n_src + batch - 1) / batch * (long)batch, tables = (long)n_epochs * n_order_seeds;
    const long bx = (per + ADAM_BLOCK - 1) / ADAM_BLOCK;
    adam_order_table_kernel<<<dim3((unsigned)(bx < 65535 ? bx : 65535), (unsigned)(tables < 65535 ? tables : 65535)),
                              dim3(ADAM_BLOCK), 0, (hipStream_t)stream>>>((int)n_src, per, order_seeds, n_order_seeds,
                                                                          shuffle != 0, epoch0, tables, idx_out);
    return (int)hipGetLastError();
}

}  // extern "C"
