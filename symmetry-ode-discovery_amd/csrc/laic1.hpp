// One step of incremental condition estimation (LAPACK xLAIC1, real case), stated ONCE for the host solver
// (host_lstsq.cpp, compiled as plain C++) and for the rank-revealing device sweep (stlsq_constrained.hpp, compiled as HIP).
// The caller forms alpha = x^T w -- the only part that depends on where x and w live -- in ascending index order; what is
// below is scalar arithmetic in the order and with the tests of the Fortran routine, so host and device take the same
// branch and round the same way (no multiply-add is contracted on the device: -ffp-contract=off).
#pragma once
#include <cmath>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SYMODE_HD __host__ __device__ __forceinline__
#else
#define SYMODE_HD inline
#endif

namespace symode {

constexpr double LAIC1_EPS = 2.220446049250313e-16;       // DBL_EPSILON = std::numeric_limits<double>::epsilon()

SYMODE_HD double laic1_sgn(double a) { return a >= 0 ? 1.0 : -1.0; }
SYMODE_HD double laic1_max(double a, double b) { return a < b ? b : a; }     // std::max's definition

// job 1: largest, job 2: smallest singular value of [[L, 0], [w^T, gamma]] given the estimate sest of L's with approximate
// singular vector x, alpha = x^T w.  sestpr: the new estimate; (s, c): the new vector is [s x, c].
SYMODE_HD void laic1(int job, double alpha, double sest, double gamma, double& sestpr, double& s, double& c) {
    const double EPS = LAIC1_EPS;
    const double absalp = std::fabs(alpha), absgam = std::fabs(gamma), absest = std::fabs(sest);
    if (job == 1) {
        if (sest == 0.0) {
            const double s1 = laic1_max(absgam, absalp);
            if (s1 == 0.0) { s = 0; c = 1; sestpr = 0; return; }
            s = alpha / s1; c = gamma / s1;
            const double t = std::sqrt(s * s + c * c);
            s /= t; c /= t; sestpr = s1 * t; return;
        }
        if (absgam <= EPS * absest) {
            const double t = laic1_max(absest, absalp), s1 = absest / t, s2 = absalp / t;
            s = 1; c = 0; sestpr = t * std::sqrt(s1 * s1 + s2 * s2); return;
        }
        if (absalp <= EPS * absest) {
            if (absgam <= absest) { s = 1; c = 0; sestpr = absest; } else { s = 0; c = 1; sestpr = absgam; }
            return;
        }
        if (absest <= EPS * absalp || absest <= EPS * absgam) {
            const double s1 = absgam, s2 = absalp;
            if (s1 <= s2) { const double t = s1 / s2; const double q = std::sqrt(1 + t * t); sestpr = s2 * q; c = (gamma / s2) / q; s = laic1_sgn(alpha) / q; }
            else { const double t = s2 / s1; const double q = std::sqrt(1 + t * t); sestpr = s1 * q; s = (alpha / s1) / q; c = laic1_sgn(gamma) / q; }
            return;
        }
        const double z1 = alpha / absest, z2 = gamma / absest;
        const double b = (1.0 - z1 * z1 - z2 * z2) * 0.5, cc = z1 * z1;
        const double t = b > 0 ? cc / (b + std::sqrt(b * b + cc)) : std::sqrt(b * b + cc) - b;
        const double sine = -z1 / t, cosine = -z2 / (1.0 + t), nrm = std::sqrt(sine * sine + cosine * cosine);
        s = sine / nrm; c = cosine / nrm; sestpr = std::sqrt(t + 1.0) * absest; return;
    }
    if (sest == 0.0) {
        sestpr = 0;
        double sine, cosine;
        if (laic1_max(absgam, absalp) == 0.0) { sine = 1; cosine = 0; } else { sine = -gamma; cosine = alpha; }
        const double s1 = laic1_max(std::fabs(sine), std::fabs(cosine));
        s = sine / s1; c = cosine / s1;
        const double t = std::sqrt(s * s + c * c);
        s /= t; c /= t; return;
    }
    if (absgam <= EPS * absest) { s = 0; c = 1; sestpr = absgam; return; }
    if (absalp <= EPS * absest) {
        if (absgam <= absest) { s = 0; c = 1; sestpr = absgam; } else { s = 1; c = 0; sestpr = absest; }
        return;
    }
    if (absest <= EPS * absalp || absest <= EPS * absgam) {
        const double s1 = absgam, s2 = absalp;
        if (s1 <= s2) { const double t = s1 / s2; const double q = std::sqrt(1 + t * t); sestpr = absest * (t / q); s = -(gamma / s2) / q; c = laic1_sgn(alpha) / q; }
        else { const double t = s2 / s1; const double q = std::sqrt(1 + t * t); sestpr = absest / q; c = (alpha / s1) / q; s = -laic1_sgn(gamma) / q; }
        return;
    }
    const double z1 = alpha / absest, z2 = gamma / absest;
    const double norma = laic1_max(1.0 + z1 * z1 + std::fabs(z1 * z2), std::fabs(z1 * z2) + z2 * z2);
    const double test = 1.0 + 2.0 * (z1 - z2) * (z1 + z2);
    double sine, cosine;
    if (test >= 0) {
        const double b = (z1 * z1 + z2 * z2 + 1.0) * 0.5, cc = z2 * z2;
        const double t = cc / (b + std::sqrt(std::fabs(b * b - cc)));
        sine = z1 / (1.0 - t); cosine = -z2 / t;
        sestpr = std::sqrt(t + 4.0 * EPS * EPS * norma) * absest;
    } else {
        const double b = (z2 * z2 + z1 * z1 - 1.0) * 0.5, cc = z1 * z1;
        const double t = b >= 0 ? -cc / (b + std::sqrt(b * b + cc)) : b - std::sqrt(b * b + cc);
        sine = -z1 / t; cosine = -z2 / (1.0 + t);
        sestpr = std::sqrt(1.0 + t + 4.0 * EPS * EPS * norma) * absest;
    }
    const double nrm = std::sqrt(sine * sine + cosine * cosine);
    s = sine / nrm; c = cosine / nrm;
}

}  // namespace symode
