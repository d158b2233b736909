// The solve of ONE joint symmetric positive definite system of n <= 64 unknowns by a single wave, stated once for the device
// STLSQ kernels whose equation rows couple: stlsq_constrained_kernel (the rows meet in Q) and stlsq_symreg_kernel (the rows
// meet in the regulariser's R).  It is stlsq_sweep_kernel's per-row arithmetic (stlsq.hpp) on rows of stride `ld`, with the
// pivot floor; no multiply-add is contracted (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "stlsq.hpp"

namespace symode {

// Pivoted Cholesky with fused forward substitution.  A (n x n, rows of stride ld, LDS) holds the full symmetric system, lane t
// POSITION t of the pivot order: `orig` the index of its row / column of A (lane on entry), `c` its entry of the right-hand
// side.  Largest remaining diagonal first, the lowest position of equals; the row of the factor takes the place of the
// pivot's row of A; q_kk as soon as row kk exists, subtracted from the positions behind it.  On return A holds the factor,
// c = R^-T (right-hand side) by position.
//   !MINNORM  a pivot that is not > pivot_floor * (first pivot) (or not > 0) ends the factorisation: returns true;
//   MINNORM   a pivot that is not > 0 ends it at fact = kk (the remaining rows of the factor are zero); returns false.
// Every branch is wave-uniform (pivot position and pivot value come through readfirstlane / readlane).
template <bool MINNORM>
__device__ __forceinline__ bool stlsq_joint_factor(double* A, int ld, int n, int lane, int& orig, double& c, double pivot_floor,
                                                   int& fact) {
    const bool on = lane < n;
    orig = lane;
    double dg = on ? A[lane * ld + lane] : 0.0;
    double first = 0.0;
    fact = n;
    for (int kk = 0; kk < n; ++kk) {
        double bv = dg;
        int bi = (lane >= kk && lane < n) ? lane : WAVE;
#pragma unroll
        for (int off = WAVE / 2; off > 0; off /= 2) {
            const double ov = __shfl_xor(bv, off, WAVE);
            const int oi = __shfl_xor(bi, off, WAVE);
            if (oi < WAVE && (bi == WAVE || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        const int jp = __builtin_amdgcn_readfirstlane(bi);
        if (jp != kk) {
            const int src = lane == kk ? jp : (lane == jp ? kk : lane);
            orig = __shfl(orig, src, WAVE);
            dg = __shfl(dg, src, WAVE);
            c = __shfl(c, src, WAVE);
        }
        const double dkk = stlsq_lane(dg, kk);
        if constexpr (MINNORM) {
            if (!(dkk > 0.0)) {
                fact = kk;
                return false;
            }
        } else {
            if (kk == 0) first = dkk;
            if (!(dkk > pivot_floor * first) || !(dkk > 0.0)) return true;
        }
        const double rr = sqrt(dkk);
        const int jo = __builtin_amdgcn_readlane(orig, kk);
        const bool rest = lane > kk && lane < n;
        double Rt = 0.0;
        if (rest) {
            Rt = A[jo * ld + orig] / rr;
            A[jo * ld + orig] = Rt;
        }
        if (lane == kk) A[jo * ld + jo] = rr;
        for (int a = kk + 1; a < n; ++a) {
            const double Ra = stlsq_lane(Rt, a);
            const int oa = __builtin_amdgcn_readlane(orig, a);
            if (rest) A[oa * ld + orig] -= Ra * Rt;
        }
        const double q = stlsq_lane(c, kk) / rr;
        if (rest) {
            c -= Rt * q;
            dg -= Rt * Rt;
        }
        if (lane == kk) c = q;
        stlsq_wave_sync();
    }
    return false;
}

// Back substitution on the factor stlsq_joint_factor left: row by row from the last, the products formed across the lanes
// and subtracted in the order t = i + 1 .. n - 1.  On return c is the solution by position (lane t: unknown orig).
__device__ __forceinline__ void stlsq_joint_back(const double* A, int ld, int n, int lane, int orig, double& c) {
    for (int i = n - 1; i >= 0; --i) {
        const int jo = __builtin_amdgcn_readlane(orig, i);
        const double prod = (lane > i && lane < n) ? A[jo * ld + orig] * c : 0.0;
        double acc = stlsq_lane(c, i);
        for (int t = i + 1; t < n; ++t) acc -= stlsq_lane(prod, t);
        const double y = acc / A[jo * ld + jo];
        if (lane == i) c = y;
    }
}

}  // namespace symode
