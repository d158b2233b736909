// Sequential-threshold least squares under the equivariance constraint Xi = Q beta (+ const) on the device
// (symode_stlsq_sweep_constrained): the constrained branch of sindy.solve_SINDy_one_step (reference sindy.py:250-315),
// restated from a Gram matrix for one launch over all problems.  Library independent, so only capi.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "laic1.hpp"
#include "stlsq.hpp"
#include "stlsq_joint.hpp"

namespace symode {

constexpr int STLSQC_MAX_R = WAVE;     // free parameters r' = r + (allow_constant ? d : 0): one lane per position of the pivot order

// LDS of a workgroup: Gq (r' x r' fp64, rows of stride r'), the support masks of the STLSQ_MAX_D rows (64-bit words), the
// list of effective columns (r' ints) and the fp32 variables [beta | const] (r' floats).  33.3 KiB at r' = 64.
inline size_t stlsqc_lds_bytes(int R) {
    return (size_t)R * R * sizeof(double) + STLSQ_MAX_D * sizeof(unsigned long long) + (size_t)R * (sizeof(int) + sizeof(float));
}

// ... of the rank-revealing mode (MINNORM): a second r' x r' fp64 array behind Gq, for Wm Wm^T and its factor.  64.5 KiB at
// r' = 64 -- above the 64 KiB a launch gets by default, so the launcher raises the kernel's limit.
inline size_t stlsqc_minnorm_lds_bytes(int R) { return stlsqc_lds_bytes(R) + (size_t)R * R * sizeof(double); }

// One workgroup of ONE wave per problem.  The constraint couples the equation rows into one joint system of n <= r' <= 64
// unknowns, so the factorisation -- one lane per position of the pivot order -- is a single wave's work whatever d is, and
// the build of Gq in front of it is at most d p (p + n) steps per lane.  d waves would build d partial sums that then have
// to meet in a fixed order through LDS and barriers, to then idle through the solve; with one wave the documented order of
// the sums (ascending j, k, l) is simply the loop order, and no __syncthreads is needed at all.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): 70 VGPRs (69 without the table), 0 AGPRs, 106 SGPRs
// of which 9 are kept in VGPR lanes, scratch 0 bytes per lane, no VGPR spill; LDS is dynamic, stlsqc_lds_bytes(r'): 33.3 KiB at
// r' = 64, 0.4 KiB at r' = 6.
//
// Per pass, with the (d, p) mask M held as d 64-bit words in LDS (the same in every lane), lane b the owner of column b:
//   columns   column c of q_solve (d p, r') is effective when one of its rows with M set is != 0 (the host's test on
//             Q[mask], sindy.py:284); the effective columns in ascending order are col[0 .. n);
//   system    Gq = Qe^T Gm Qe and cq = Qe^T cm in fp64, Gm = blockdiag(Gtt + gamma^2 I)[M, M] never formed: for j, then
//             active k ascending, lane b forms u_b = sum over active l ascending of (Gtt[k, l] + gamma^2 [k == l]) Qe[(j,l), b]
//             and adds Qe[(j,k), a] u_b into Gq[a, b] for a <= b, Qe[(j,k), b] Gty[k, j] into cq[b].  The lower triangle is
//             the mirror of the upper one, so Gq is exactly symmetric;
//   solve     stlsq_sweep_kernel's pivoted Cholesky and substitutions (stated for joint systems in stlsq_joint.hpp, which
//             stlsq_symreg_kernel shares), except that a pivot which is not
//             > pivot_floor * (first pivot) (or not > 0) flags the problem (fell) and ends it;
//   Xi        beta32 = (float) of the solution in its r' slots (0 elsewhere); lane k forms Xi[j, k] = sum over c < r ascending
//             of q_xi[(j p + k), c] beta32[c] in fp32, plus const32[j] at k = 0 when allow_constant;
//   threshold the host's rule on the still-active entries, near counted on them; stop when the mask repeats.
// No multiply-add is contracted (-ffp-contract=off).  Every LDS and global index is bounded by d, p, r': no address
// depends on data.  HYPER, n_sets: as stlsq_sweep_kernel.
//
// MINNORM (symode_stlsq_sweep_minnorm; a template bit, so the two instantiations above keep their code): the solve of a
// pass is symode_host_lstsq_normal's driver 0 with the launch's rcond (`cut`), i.e. what the host replay of a flagged problem
// performs (lstsq_normal(Gq, cq, m, 'gelsy', SINGULAR_RCOND)), so a problem with collinear columns ends inside the launch:
//   factor    as above without the pivot floor: a pivot that is not > 0 ends the factorisation at fact = kk, the remaining
//             rows of R are zero (host_lstsq.cpp:55);
//   rank      xGELSY's loop over xLAIC1 estimates (host_lstsq.cpp:67-84, laic1.hpp): xmin and xmax hold one element per
//             lane, indexed by position in the pivot order; alpha is summed in ascending position order through stlsq_lane,
//             so it is the host's sum; sest, s, c and every branch are wave-uniform (the decision goes through an SGPR);
//             position `rank` is accepted while smaxpr * cut <= sminpr;
//   rank == n today's back substitution; rank == 0: Y = 0;
//   else      Y = Wm^T (Wm Wm^T)^-1 q, Wm = R[:rank, :], q the first `rank` entries of the forward substitution, in the
//             host's order (host_lstsq.cpp:102-132): M[a, b] = sum over positions t ascending of R(a, t) R(b, t) (from
//             t = a: the terms before it are exact zeros), lane b the owner of column b; the Cholesky factor of M column
//             by column, lane a the owner of row a, per entry the subtractions in ascending t; the two substitutions with
//             the products formed across the lanes and subtracted in the host's order; Y[t] = sum over a ascending of
//             R(a, t) z[a].  A diagonal of M's factor that is not > 0 sets fell and ends the problem: it stays the host's.
// trunc_out: the passes solved with rank < n; rank_out: the rank of the last pass's system (0 on an empty support).  Both are
// read by MINNORM only (NULL otherwise).  Resources of the two MINNORM instantiations: profiles/stlsq_minnorm.txt.
template <bool HYPER, bool MINNORM = false>
__global__ __launch_bounds__(WAVE) void stlsq_constrained_kernel(const double* __restrict__ aug, int n_sets, int d, int p,
                                                                 const double* __restrict__ q_solve,
                                                                 const float* __restrict__ q_xi, int r, int allow_constant,
                                                                 const float* __restrict__ hyper, double gamma, double threshold,
                                                                 int max_iter, double near_band, double pivot_floor,
                                                                 float* __restrict__ xi_out, float* __restrict__ var_out,
                                                                 unsigned char* __restrict__ mask_out,
                                                                 int* __restrict__ passes_out, int* __restrict__ near_out,
                                                                 int* __restrict__ fell_out, int* __restrict__ trunc_out,
                                                                 int* __restrict__ rank_out) {
    extern __shared__ double stlsqc_smem[];
    const int lane = threadIdx.x;
    const long s = blockIdx.x;
    const int F = p + d;
    const int R = r + (allow_constant ? d : 0);
    double* A = stlsqc_smem;
    double* W = A + (size_t)R * R;                     // MINNORM: Wm Wm^T, then its factor
    unsigned long long* M = (unsigned long long*)(A + (size_t)(MINNORM ? 2 : 1) * R * R);
    const double cut = pivot_floor;                    // MINNORM: the launch's rcond travels in this argument
    int* col = (int*)(M + STLSQ_MAX_D);
    float* var = (float*)(col + R);
    if constexpr (HYPER) {
        gamma = (double)hyper[s * STLSQ_HYPER];
        threshold = (double)hyper[s * STLSQ_HYPER + 1];
    }
    const double* G = aug + (s % n_sets) * (long)F * F;
    const double g2 = gamma * gamma;
    const float thr32 = (float)threshold;
    if (lane < STLSQ_MAX_D) M[lane] = lane < d ? (p == 64 ? ~0ull : (1ull << p) - 1ull) : 0ull;
    stlsq_wave_sync();
    int near = 0, passes = 0, fell = 0;
    int trunc = 0, rank = 0;
    for (int it = 0; it < max_iter; ++it) {
        // ---- effective columns
        bool eff = false;
        if (lane < R) {
            for (int j = 0; j < d; ++j) {
                const unsigned long long mj = M[j];
                for (int k = 0; k < p; ++k)
                    if ((mj >> k) & 1ull) eff = eff || q_solve[((long)j * p + k) * R + lane] != 0.0;
            }
        }
        const unsigned long long support = __ballot(eff);
        const int n = __popcll(support);
        if (eff) col[__popcll(support & ((1ull << lane) - 1ull))] = lane;
        if (lane < R) var[lane] = 0.0f;
        stlsq_wave_sync();
        bool bad = false;
        if constexpr (MINNORM) rank = 0;
        if (n > 0) {
            const bool on = lane < n;
            const int cb = on ? col[lane] : 0;
            // ---- system
            for (int a = 0; a < n; ++a)
                if (on) A[a * R + lane] = 0.0;
            double c = 0.0;
            for (int j = 0; j < d; ++j) {
                const unsigned long long mj = M[j];
                for (int k = 0; k < p; ++k) {
                    if (!((mj >> k) & 1ull)) continue;
                    double u = 0.0;
                    for (int l = 0; l < p; ++l) {
                        if (!((mj >> l) & 1ull)) continue;
                        const double g = G[(long)k * F + l] + (k == l ? g2 : 0.0);
                        u += g * q_solve[((long)j * p + l) * R + cb];
                    }
                    const double qk = on ? q_solve[((long)j * p + k) * R + cb] : 0.0;
                    c += qk * G[(long)k * F + p + j];
                    for (int a = 0; a < n; ++a) {
                        const double qa = stlsq_lane(qk, a);
                        if (on && a <= lane) A[a * R + lane] += qa * u;
                    }
                }
            }
            stlsq_wave_sync();
            for (int a = 0; a < n; ++a)
                if (on && a < lane) A[lane * R + a] = A[a * R + lane];
            stlsq_wave_sync();
            // ---- factor and solve (stlsq_joint.hpp: stlsq_sweep_kernel's, rows of stride R, and the pivot floor)
            int orig, fact;
            bad = stlsq_joint_factor<MINNORM>(A, R, n, lane, orig, c, pivot_floor, fact);
            if constexpr (MINNORM) {
                // ---- rank: lane i holds element i of the two approximate singular vectors
                stlsq_wave_sync();
                if (fact > 0) {
                    const int o0 = __builtin_amdgcn_readlane(orig, 0);
                    double smax = fabs(A[o0 * R + o0]), smin = smax;
                    double xmin = lane == 0 ? 1.0 : 0.0, xmax = xmin;
                    rank = 1;
                    while (rank < n) {
                        const int jr = __builtin_amdgcn_readlane(orig, rank);
                        const double w = lane < rank ? A[orig * R + jr] : 0.0;
                        const double gam = rank < fact ? A[jr * R + jr] : 0.0;
                        const double pmin = xmin * w, pmax = xmax * w;
                        double amin = 0.0, amax = 0.0;
                        for (int i = 0; i < rank; ++i) {
                            amin += stlsq_lane(pmin, i);
                            amax += stlsq_lane(pmax, i);
                        }
                        double sminpr, s1, c1, smaxpr, s2, c2;
                        laic1(2, amin, smin, gam, sminpr, s1, c1);
                        laic1(1, amax, smax, gam, smaxpr, s2, c2);
                        if (!__builtin_amdgcn_readfirstlane((int)(smaxpr * cut <= sminpr))) break;
                        if (lane < rank) {
                            xmin *= s1;
                            xmax *= s2;
                        }
                        if (lane == rank) {
                            xmin = c1;
                            xmax = c2;
                        }
                        smin = sminpr;
                        smax = smaxpr;
                        ++rank;
                    }
                }
                if (rank < n) ++trunc;
                if (rank > 0 && rank < n) {
                    // ---- minimum norm: M = Wm Wm^T, lane b the owner of column b
                    const bool in = lane < rank;
                    for (int a = 0; a < rank; ++a) {
                        const int oa = __builtin_amdgcn_readlane(orig, a);
                        double acc = 0.0;
                        for (int t = a; t < n; ++t) {
                            const int ot = __builtin_amdgcn_readlane(orig, t);
                            const double rb = (in && lane <= t) ? A[orig * R + ot] : 0.0;
                            acc += A[oa * R + ot] * rb;
                        }
                        if (in) W[a * R + lane] = acc;
                    }
                    stlsq_wave_sync();
                    // ---- its factor in place, column by column, lane a the owner of row a
                    for (int b = 0; b < rank; ++b) {
                        double acc = 0.0;
                        if (in && lane >= b) {
                            acc = W[lane * R + b];
                            for (int t = 0; t < b; ++t) acc -= W[lane * R + t] * W[b * R + t];
                        }
                        const double dbb = stlsq_lane(acc, b);
                        if (!(dbb > 0.0)) {
                            bad = true;
                            break;
                        }
                        const double lbb = sqrt(dbb);
                        if (in && lane >= b) W[lane * R + b] = lane == b ? lbb : acc / lbb;
                        stlsq_wave_sync();
                    }
                    if (!bad) {
                        for (int i = 0; i < rank; ++i) {                  // Lc z' = q
                            const double prod = lane < i ? W[i * R + lane] * c : 0.0;
                            double acc = stlsq_lane(c, i);
                            for (int t = 0; t < i; ++t) acc -= stlsq_lane(prod, t);
                            const double y = acc / W[i * R + i];
                            if (lane == i) c = y;
                        }
                        for (int i = rank - 1; i >= 0; --i) {             // Lc^T z = z'
                            const double prod = (lane > i && in) ? W[lane * R + i] * c : 0.0;
                            double acc = stlsq_lane(c, i);
                            for (int t = i + 1; t < rank; ++t) acc -= stlsq_lane(prod, t);
                            const double y = acc / W[i * R + i];
                            if (lane == i) c = y;
                        }
                        double y = 0.0;                                   // Y = Wm^T z
                        for (int a = 0; a < rank; ++a) {
                            const int oa = __builtin_amdgcn_readlane(orig, a);
                            const double ra = (on && a <= lane) ? A[oa * R + orig] : 0.0;
                            y += ra * stlsq_lane(c, a);
                        }
                        c = y;
                    }
                } else if (rank == 0) {
                    c = 0.0;
                }
            }
            if (!bad) {
                if (!MINNORM || rank == n) stlsq_joint_back(A, R, n, lane, orig, c);
                if (on) var[col[orig]] = (float)c;
            }
        }
        passes = it + 1;
        if (bad) {
            fell = 1;
            break;
        }
        stlsq_wave_sync();
        // ---- coefficients and threshold
        if (lane < R) var_out[s * R + lane] = var[lane];
        int changed = 0;
        for (int j = 0; j < d; ++j) {
            const unsigned long long mj = M[j];
            float v = 0.0f;
            if (lane < p) {
                const float* qrow = q_xi + ((long)j * p + lane) * r;
                for (int cc = 0; cc < r; ++cc) v += qrow[cc] * var[cc];
                if (allow_constant && lane == 0) v += var[r + j];
                xi_out[(s * d + j) * p + lane] = v;
            }
            const bool m = (mj >> lane) & 1ull;
            const float av = fabsf(v);
            near += __popcll(__ballot(m && fabs((double)av - threshold) < near_band));
            const unsigned long long nm = __ballot(m && av > thr32);
            changed |= nm != mj;
            stlsq_wave_sync();                      // every lane has read M[j]
            if (lane == 0) M[j] = nm;
        }
        stlsq_wave_sync();
        if (!changed) break;
    }
    for (int j = 0; j < d; ++j)
        if (lane < p) mask_out[(s * d + j) * p + lane] = (M[j] >> lane) & 1ull ? 1 : 0;
    if (lane == 0) {
        passes_out[s] = passes;
        near_out[s] = near;
        fell_out[s] = fell;
        if constexpr (MINNORM) {
            trunc_out[s] = trunc;
            rank_out[s] = rank;
        }
    }
}

inline hipError_t launch_stlsq_constrained(const double* aug, long n_sets, long n_problems, int d, int p, const double* q_solve,
                                           const float* q_xi, int r, int allow_constant, const float* hyper, double gamma,
                                           double threshold, int max_iter, double near_band, double pivot_floor, float* xi_out,
                                           float* var_out, unsigned char* mask_out, int* passes_out, int* near_out, int* fell_out,
                                           hipStream_t st) {
    const int R = r + (allow_constant ? d : 0);
    auto kernel = hyper ? stlsq_constrained_kernel<true> : stlsq_constrained_kernel<false>;
    kernel<<<dim3((unsigned)n_problems), dim3(WAVE), stlsqc_lds_bytes(R), st>>>(aug, (int)n_sets, d, p, q_solve, q_xi, r,
                                                                                allow_constant, hyper, gamma, threshold, max_iter,
                                                                                near_band, pivot_floor, xi_out, var_out, mask_out,
                                                                                passes_out, near_out, fell_out, nullptr, nullptr);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

// The rank-revealing mode: rcond in place of the pivot floor, two more outputs per problem.
inline hipError_t launch_stlsq_minnorm(const double* aug, long n_sets, long n_problems, int d, int p, const double* q_solve,
                                       const float* q_xi, int r, int allow_constant, const float* hyper, double gamma,
                                       double threshold, int max_iter, double near_band, double rcond, float* xi_out, float* var_out,
                                       unsigned char* mask_out, int* passes_out, int* near_out, int* fell_out, int* trunc_out,
                                       int* rank_out, hipStream_t st) {
    const int R = r + (allow_constant ? d : 0);
    const size_t lds = stlsqc_minnorm_lds_bytes(R);
    auto kernel = hyper ? stlsq_constrained_kernel<true, true> : stlsq_constrained_kernel<false, true>;
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch: gfx950 has 160 KB per workgroup
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    kernel<<<dim3((unsigned)n_problems), dim3(WAVE), lds, st>>>(aug, (int)n_sets, d, p, q_solve, q_xi, r, allow_constant, hyper,
                                                                gamma, threshold, max_iter, near_band, rcond, xi_out, var_out,
                                                                mask_out, passes_out, near_out, fell_out, trunc_out, rank_out);
    SYMODE_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace symode
