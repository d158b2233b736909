// Roll-out error of S models on n_ics held-out trajectories in ONE launch (symode_rollout_error): what
// evaluation/eval_ltp.py:31-43 does for one regressor -- RK4 roll-out from x[:, 0] (odeint(..., full_traj=True),
// model_utils.py:241-254), squared error per step -- for every model of a seed sweep at once, the predicted
// trajectories never written to memory.
#pragma once
#include <cfloat>

#include "kernels.hpp"

namespace symode {

// One lane = one (model s, trajectory i) pair, lanes numbered s * n_ics + i: n_ics is 5-20 in the validation recipes, so a
// wave spans several models and every lane carries ITS model's masked coefficients in VGPRs (d p <= 42 for the shipped
// libraries, 80 at d = 3 order 3 with sine and exp).  The launch is a serial chain of n_steps RK4 steps per lane and a few
// hundred to a few thousand lanes in all: one wave per workgroup spreads them over as many CUs as there are waves.
constexpr int ROLLOUT_BLOCK = WAVE;

// The step is integrate_steps<Lib> -- the arithmetic of odeint_traj_kernel.  After step k (state at time point k + 1):
//     e = mean_j (x_true[i, k+1, j] - x_pred[j])^2       fp32, differences and products rounded one by one (no FMA), summed
//                                                        over j in index order, times 1/d: torch's ((x - xp) ** 2).mean(-1)
//                                                        bit for bit at d <= 2; at d = 3 torch adds the three squares in
//                                                        another order, a last-place difference
//     err[s, i, k] = e;   mean_err[s, i] = (sum_k (double)e) / n_steps;   horizon[s, i] = number of leading steps with e <= bound
// A lane reads its own truth row and writes its own err row -- 64 different lines per wave and step -- so both move as
// 16-byte vectors where the row allows: truth in groups of four TIME POINTS from the row base (x0 comes out of the first
// group; the next group is requested four steps before its first use), four e values staged for one store.  A row whose
// base is not 16-byte aligned, and the ragged last group of either, take the scalar path of the same loop.
// No early exit: inf / NaN propagate as in the per-model path; the comparison with the bound is false for NaN, and a bound
// of +inf counts the finite steps (e = +inf ends the count).  No workspace, no atomics, no cross-lane traffic.
template <class Lib>
__global__ __launch_bounds__(ROLLOUT_BLOCK) void rollout_error_kernel(const float* __restrict__ x_true, long n_ics, long n_lanes,
                                                                      const float* __restrict__ xi,
                                                                      const float* __restrict__ mask, int n_steps, float dt,
                                                                      int method, float bound, float* __restrict__ err,
                                                                      double* __restrict__ mean_err, int* __restrict__ horizon) {
    constexpr int D = Lib::D, G = 4;
    typedef float f4v __attribute__((ext_vector_type(4)));
    const long lane = (long)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x;
    if (lane >= n_lanes) return;
    const long s = lane / n_ics, i = lane - s * n_ics;
    float w[D * Lib::P];
    load_xi<Lib, 1, 0>(xi, mask, s, w);                       // (1, 0): never the SGPR form, s differs across the wave

    const long T = (long)n_steps + 1;                         // time points of a truth row
    const float* row = x_true + i * T * D;
    const bool tr_vec = ((uintptr_t)row % 16) == 0;
    // time points t0 .. t0+3 of the row (zeros beyond its end)
    auto fetch = [&](long t0, float (&v)[G * D]) __attribute__((always_inline)) {
        const float* q = row + t0 * D;
        if (tr_vec && t0 + G <= T) {
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const f4v u = reinterpret_cast<const f4v*>(q)[a];
                v[4 * a + 0] = u.x;
                v[4 * a + 1] = u.y;
                v[4 * a + 2] = u.z;
                v[4 * a + 3] = u.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const bool in = t0 + j < T;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    float t = 0.0f;
                    if (in) t = q[j * D + c];
                    v[j * D + c] = t;
                }
            }
        }
    };
    // `cur`: a shift register, the next unused time point in front; `nxt`: the group after it, in flight
    float cur[G * D], nxt[G * D], x[D];
    fetch(0, cur);
    fetch(G, nxt);
    auto pop = [&](float (&p)[D]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < D; ++c) p[c] = cur[c];
#pragma unroll
        for (int c = 0; c < (G - 1) * D; ++c) cur[c] = cur[c + D];
    };
    pop(x);                                                   // x0 = x_true[i, 0]

    float* erow = err != nullptr ? err + lane * (long)n_steps : nullptr;
    const bool er_vec = ((uintptr_t)erow % 16) == 0;
    const float b = bound > FLT_MAX ? FLT_MAX : bound;
    float est[G] = {0.0f, 0.0f, 0.0f, 0.0f};
    double sum = 0.0;
    int h = 0;
    bool alive = true;
    integrate_steps<Lib>(w, x, n_steps, dt, method, [&](int k, const float (&xp)[D]) __attribute__((always_inline)) {
        const int t = k + 1;
        if ((t & (G - 1)) == 0) {
#pragma unroll
            for (int c = 0; c < G * D; ++c) cur[c] = nxt[c];
            fetch((long)t + G, nxt);
        }
        float xt[D];
        pop(xt);
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float df = __fsub_rn(xt[c], xp[c]);
            const float sq = __fmul_rn(df, df);
            acc = c == 0 ? sq : __fadd_rn(acc, sq);
        }
        const float e = __fmul_rn(acc, 1.0f / D);
        sum += (double)e;
        alive = alive && (e <= b);
        h += alive ? 1 : 0;
        const int j = k & (G - 1);
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (j == jj) est[jj] = e;
        if (j == G - 1 && erow != nullptr) {
            float* q = erow + (k - (G - 1));
            if (er_vec) {
                __builtin_nontemporal_store(f4v{est[0], est[1], est[2], est[3]}, reinterpret_cast<f4v*>(q));
            } else {
#pragma unroll
                for (int jj = 0; jj < G; ++jj) q[jj] = est[jj];
            }
        }
    });
    const int rem = n_steps & (G - 1);
    if (erow != nullptr) {
#pragma unroll
        for (int jj = 0; jj < G - 1; ++jj)
            if (jj < rem) erow[n_steps - rem + jj] = est[jj];
    }
    mean_err[lane] = sum / (double)n_steps;
    horizon[lane] = h;
}

template <class Lib>
hipError_t launch_rollout_error(const float* x_true, long n_ics, long S, const float* xi, const float* mask, int n_steps,
                                float dt, int method, float bound, float* err, double* mean_err, int* horizon,
                                hipStream_t st) {
    const long n_lanes = S * n_ics;
    if (n_lanes == 0) return hipSuccess;
    const long g = (n_lanes + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK;
    rollout_error_kernel<Lib><<<dim3((unsigned)g), dim3(ROLLOUT_BLOCK), 0, st>>>(x_true, n_ics, n_lanes, xi, mask, n_steps, dt, method,
                                                                               bound, err, mean_err, horizon);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
