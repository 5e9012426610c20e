// device_math.hpp -- per-element FP64 math of the ADMM local step for gfx950 (one lane = one element).
//
// Reference behaviour restated (file:line relative to the reference repo):
//   signed SVD                     src/FastSVD.hpp:43-68
//   linear tet prox                src/TetEnergyTerm.cpp:73-92
//   hyperelastic prox (NH, StVK)   src/TetEnergyTerm.cpp:114-136, :173-237
//   triangle prox + strain limit   src/TriEnergyTerm.cpp:73-101
//
// Design notes (MI355X): everything lives in VGPRs (arrays are fully unrolled -> SROA); the SVD is a
// cyclic Jacobi eigen-solve of the symmetric 3x3 F^T F (cheap rotations: 1 rcp + 1 sqrt + 1 rsqrt each)
// followed by a Gram-Schmidt reconstruction of U from F V, which (a) returns U,V in SO(3) by
// construction, (b) recovers the *signed* smallest stretch as u2 . F v2 directly from F, so inverted
// and flat elements need no special-casing.  The principal-stretch minimisation is a safeguarded
// Newton with the analytic diag + rank-one Hessian (Sherman-Morrison solve, no 3x3 factorisation),
// iterated to the exact minimiser -- the reference's L-BFGS (absent mcloptlib) stops at
// |g|<1e-6 or |dx|<1e-6 of the same objective (src/TetEnergyTerm.hpp:93-95).
#pragma once
#include <hip/hip_runtime.h>

namespace admm_dev {

#define ADMM_M3(A, r, c) ((A)[(c) * 3 + (r)])
#ifndef ADMM_COUNT
#define ADMM_COUNT(slot)      // experiments/hostmath counts sweeps / rotations through this; nothing on the device
#endif
#ifndef ADMM_RECORD
#define ADMM_RECORD(slot, value)
#endif

__device__ __forceinline__ double dot3(const double *a, const double *b) {
    return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2]));
}
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- fast FP64 reciprocal / rsqrt: hardware seed + two Newton steps (no IEEE div/sqrt sequences) ----
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0); r = fma(r, e, r);
    e = fma(-x, r, 1.0); r = fma(r, e, r);
    return r;
}
__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    double e = fma(-h * y, y, 0.5); y = fma(y, e, y);
    e = fma(-h * y, y, 0.5); y = fma(y, e, y);
    return y;
}

// FP32 rotation used only to SEED the eigenvectors (quarter-rate hardware rcp/sqrt/rsq).  Unconditional: with b = 0 it is
// the identity (t = 0, c = 1), so there is no branch whose two sides the compiler would have to merge with register copies.
__device__ __forceinline__ void jacobi_rotate_f32(float &app, float &aqq, float &apq, float &arp, float &arq,
                                                  float *vp, float *vq) {
    const float a = aqq - app, b = apq + apq;
    const float h = __builtin_amdgcn_sqrtf(fmaxf(fmaf(a, a, b * b), 1e-36f));
    const float t = b * __builtin_amdgcn_rcpf(a + copysignf(h, a));      // sgn(a) b / (|a| + h)
    const float c = __builtin_amdgcn_rsqf(fmaf(t, t, 1.0f));
    const float s = t * c;
    app = fmaf(-t, apq, app);
    aqq = fmaf(t, apq, aqq);
    apq = 0.0f;
    const float rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = fmaf(s, rp, c * rq);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float x = vp[i], y = vq[i];
        vp[i] = c * x - s * y;
        vq[i] = fmaf(s, x, c * y);
    }
}

// One-sided (Hestenes) Jacobi rotation in FP64: rotates columns p, q of B = F V (and of V) so that b_p . b_q = 0.
// al = |b_p|^2, be = |b_q|^2, ga = b_p . b_q.  Same angle as the two-sided rotation of F^T F: t = sgn(a) b / (|a| + sqrt(a^2 + b^2)).
// t only steers the convergence (one Newton step on the 2^-24 hardware seeds); c decides the orthogonality of V (two steps).
__device__ __forceinline__ void hestenes_rotate(double *bp, double *bq, double *vp, double *vq, double al, double be, double ga) {
    ADMM_COUNT(2);
    const double a = be - al, b = ga + ga;
    const double h2 = fmax(fma(a, a, b * b), 1e-300);
    double y = __builtin_amdgcn_rsq(h2);
    y = fma(y, fma(-0.5 * h2 * y, y, 0.5), y);
    const double den = fma(h2, y, fabs(a));
    double r = __builtin_amdgcn_rcp(den);
    r = fma(r, fma(-den, r, 1.0), r);
    const double t = copysign(b, a * b) * r;        // sgn(a) b / den   (a = 0: the sign of b, i.e. a 45 degree rotation)
    const double c = fast_rsqrt(fma(t, t, 1.0));
    const double s = t * c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = bp[i], z = bq[i];
        bp[i] = c * x - s * z;
        bq[i] = fma(s, x, c * z);
        const double vx = vp[i], vz = vq[i];
        vp[i] = c * vx - s * vz;
        vq[i] = fma(s, vx, c * vz);
    }
}

// Signed SVD  F = U diag(S) V^T with U, V in SO(3).  S is NOT sorted (every energy of the library is a symmetric function of
// the stretches; the reference sorts, src/FastSVD.hpp:43-68); at most one entry is negative, and then it is the one of
// smallest magnitude (the reference's convention: the sign of det F goes to the smallest stretch).
// F, U, V column-major.  Mixed precision, FP64 result:
//  (1) FP32 cyclic Jacobi on the DEVIATORIC part of F^T F, scaled to unit norm: the eigenvectors are those of F^T F, and an
//      element at strain 1e-6 is resolved as well as one at strain 1 (on the trace-normalised matrix the FP32 phase stalled at
//      1e-7 / strain and the FP64 phase paid for it with extra sweeps).  Three sweeps, a fourth if some lane of the wave is not
//      at the FP32 floor yet (wave-uniform decisions: straight-line code, no merges).
//  (2) V is re-orthonormalised in FP64, B = F V.
//  (3) ONE one-sided (Hestenes) FP64 Jacobi sweep on the columns of B -- Jacobi converges quadratically, so the 1e-7 of the seed
//      becomes round-off; further sweeps only while some pair of columns of some lane is not orthogonal to 3e-14 (cosine).
//  (4) U by Gram-Schmidt on B: U in SO(3) by construction, the last stretch u2 . b2 carries the sign of det F; if it is negative
//      and not the smallest, the sign is moved by flipping two columns of U (no sorting, no special case for flat elements).
// tol2 = the cos^2 at which the FP64 sweeps of (3) stop.  kSvdTol2: F = U diag(S) V^T to 5e-14 |F| (measured <= 3e-14), what every
// hyperelastic prox needs.  The LINEAR tet passes kSvdTolLinear2: its z = U diag((1 + S) / 2) V^T implies the rotation P = 2 z - F
// = U V^T + (U diag(S) V^T - F), so the factorisation error is P's distance from SO(3); with 1e-30 (cos <= 1e-15, a decade above
// the round-off of the dot products) P^T P = I to 1e-14 for |F| of a few units (tests/test_local_step_edges.py, check D).
constexpr double kSvdTol2 = 1e-27, kSvdTolLinear2 = 1e-30;
__device__ __forceinline__ void signed_svd3(const double *Fin, double *U, double *S, double *V, const double tol2 = kSvdTol2) {
    // (0) F is scaled by an EVEN power of two that brings its largest entry into [1, 4): exact, and every quantity below scales
    // by an exact power of two with it (the v_rsq seeds see the same mantissa), so the factors of an element of ordinary size do
    // not change by a bit -- but the squares of the Gram entries (nd2, the rotations' a^2 + b^2) no longer leave the double range
    // for |F| beyond 1e+-75: unscaled, 1e100 came back as NaN and 1e-100 as a wrong factorisation (tests/test_local_step_edges.py).
    double F[9];
    int ev;
    {
        double fmx = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) fmx = fmax(fmx, fabs(Fin[i]));
        int he = (__double2hiint(fmx) >> 20) & 0x7ff;
        he = he < 3 ? 3 : (he > 2043 ? 2043 : he);      // zero / denormal / next to overflow: the scale stays a normal number
        ev = (he - 1023) & ~1;
        const double sc = __hiloint2double((1023 - ev) << 20, 0);
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = Fin[i] * sc;
    }
    double v0[3], v1[3], v2[3];
    const double c00 = dot3(F + 0, F + 0), c01 = dot3(F + 0, F + 3), c02 = dot3(F + 0, F + 6);
    const double c11 = dot3(F + 3, F + 3), c12 = dot3(F + 3, F + 6), c22 = dot3(F + 6, F + 6);
    const double m = (c00 + c11 + c22) * (1.0 / 3.0);
    const double d0 = c00 - m, d1 = c11 - m, d2 = c22 - m;
    const double o2 = fma(c01, c01, fma(c02, c02, c12 * c12));
    const double nd2 = fma(d0, d0, fma(d1, d1, fma(d2, d2, o2 + o2)));
    const bool seeded = nd2 > 1e-30 * m * m && nd2 > 1e-280;     // else: a multiple of the identity to round-off, V = I
    {
        const double inv = seeded ? __builtin_amdgcn_rsq(nd2) : 0.0;
        float a00 = (float)(d0 * inv), a01 = (float)(c01 * inv), a02 = (float)(c02 * inv);
        float a11 = (float)(d1 * inv), a12 = (float)(c12 * inv), a22 = (float)(d2 * inv);
        float w0[3] = {1.f, 0.f, 0.f}, w1[3] = {0.f, 1.f, 0.f}, w2[3] = {0.f, 0.f, 1.f};
        constexpr float kF32Off2 = 2e-13f;      // off-diagonal mass below which the three sweeps suffice
#define ADMM_F32_SWEEP() { ADMM_COUNT(0); jacobi_rotate_f32(a00, a11, a01, a02, a12, w0, w1); jacobi_rotate_f32(a00, a22, a02, a01, a12, w0, w2); \
                           jacobi_rotate_f32(a11, a22, a12, a01, a02, w1, w2); }
        ADMM_F32_SWEEP(); ADMM_F32_SWEEP(); ADMM_F32_SWEEP();
        if (__any(fmaf(a01, a01, fmaf(a02, a02, a12 * a12)) > kF32Off2)) ADMM_F32_SWEEP();
#undef ADMM_F32_SWEEP
        // (2) orthonormalise in FP64 (Gram-Schmidt; the columns are unit vectors to 1e-7: 1/sqrt(1 + e) by its series)
#pragma unroll
        for (int i = 0; i < 3; ++i) { v0[i] = (double)w0[i]; v1[i] = (double)w1[i]; }
        double e = dot3(v0, v0) - 1.0;
        double n = fma(e, fma(e, 0.375, -0.5), 1.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) v0[i] *= n;
        const double pr01 = dot3(v0, v1);
#pragma unroll
        for (int i = 0; i < 3; ++i) v1[i] = fma(-pr01, v0[i], v1[i]);
        e = dot3(v1, v1) - 1.0;
        n = fma(e, fma(e, 0.375, -0.5), 1.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) v1[i] *= n;
        cross3(v0, v1, v2);
    }
    // B = F V
    double b0[3], b1[3], b2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        b0[r] = fma(F[r], v0[0], fma(F[3 + r], v0[1], F[6 + r] * v0[2]));
        b1[r] = fma(F[r], v1[0], fma(F[3 + r], v1[1], F[6 + r] * v1[2]));
        b2[r] = fma(F[r], v2[0], fma(F[3 + r], v2[1], F[6 + r] * v2[2]));
    }
    // (3) FP64 one-sided sweeps until every pair of columns is orthogonal: cos^2 <= tol2 (kSvdTol2).  Then F = U diag(S) V^T to
    // ~3e-14 |F| whatever the order of the columns in the Gram-Schmidt below.
    double n0, n1, n2;
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {
        hestenes_rotate(b0, b1, v0, v1, dot3(b0, b0), dot3(b1, b1), dot3(b0, b1));
        hestenes_rotate(b0, b2, v0, v2, dot3(b0, b0), dot3(b2, b2), dot3(b0, b2));
        hestenes_rotate(b1, b2, v1, v2, dot3(b1, b1), dot3(b2, b2), dot3(b1, b2));
        ADMM_COUNT(1);
        n0 = dot3(b0, b0); n1 = dot3(b1, b1); n2 = dot3(b2, b2);
        const double g01 = dot3(b0, b1), g02 = dot3(b0, b2), g12 = dot3(b1, b2);
        ADMM_RECORD(8 + sweep, fmax(g01 * g01 / fmax(n0 * n1, 1e-300), fmax(g02 * g02 / fmax(n0 * n2, 1e-300), g12 * g12 / fmax(n1 * n2, 1e-300))));
        const bool open = g01 * g01 > tol2 * n0 * n1 || g02 * g02 > tol2 * n0 * n2 || g12 * g12 > tol2 * n1 * n2;
        if (!__any(open)) break;
    }
    // (4) U by Gram-Schmidt on b0, b1; u2 = u0 x u1.  A column that is round-off (flat or collapsed element) must not be one
    // of the two the basis is built from: only then (rare, whole waves skip it) sort the columns by norm.  Every swap is a
    // rotation (the moved column changes sign), so V stays in SO(3) and F = B V^T.
    if (fmin(n0, fmin(n1, n2)) <= 1e-28 * fmax(n0, fmax(n1, n2))) {
#define ADMM_SWAPNEG3(x, y) { _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) { const double t_ = x[i_]; x[i_] = y[i_]; y[i_] = -t_; } }
        if (n0 < n1) { ADMM_SWAPNEG3(b0, b1); ADMM_SWAPNEG3(v0, v1); const double t = n0; n0 = n1; n1 = t; }
        if (n0 < n2) { ADMM_SWAPNEG3(b0, b2); ADMM_SWAPNEG3(v0, v2); const double t = n0; n0 = n2; n2 = t; }
        if (n1 < n2) { ADMM_SWAPNEG3(b1, b2); ADMM_SWAPNEG3(v1, v2); const double t = n1; n1 = n2; n2 = t; }
#undef ADMM_SWAPNEG3
    }
    double u0[3], u1[3], u2[3];
    double s0 = 0.0;
    if (n0 > 1e-300) {
        const double inv = fast_rsqrt(n0);
        s0 = n0 * inv;
#pragma unroll
        for (int i = 0; i < 3; ++i) u0[i] = b0[i] * inv;
    } else { u0[0] = 1.0; u0[1] = 0.0; u0[2] = 0.0; }
    const double pr = dot3(u0, b1);
    double w[3] = {fma(-pr, u0[0], b1[0]), fma(-pr, u0[1], b1[1]), fma(-pr, u0[2], b1[2])};
    double wn = dot3(w, w);
    if (!(wn > 1e-30 * n0) || !(wn > 1e-300)) {
        // rank <= 1: any unit vector orthogonal to u0
        double ee[3] = {0.0, 0.0, 0.0};
        const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
        if (a0 <= a1 && a0 <= a2) ee[0] = 1.0; else if (a1 <= a2) ee[1] = 1.0; else ee[2] = 1.0;
        cross3(u0, ee, w);
        wn = dot3(w, w);
    }
    {
        const double inv = fast_rsqrt(wn);
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] = w[i] * inv;
    }
    cross3(u0, u1, u2);
    double s1 = dot3(u1, b1), s2 = dot3(u2, b2);
    // the sign of det F sits on s2; the convention wants it on the smallest stretch: flip u2 and that column of U
    const bool f0 = s2 < 0.0 && s0 < -s2 && s0 <= s1, f1 = s2 < 0.0 && s1 < -s2 && !f0;
    const double g0 = f0 ? -1.0 : 1.0, g1 = f1 ? -1.0 : 1.0, g2 = (f0 || f1) ? -1.0 : 1.0;
    const double isc = __hiloint2double((1023 + ev) << 20, 0);      // back to the scale of F
    S[0] = s0 * g0 * isc; S[1] = s1 * g1 * isc; S[2] = s2 * g2 * isc;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        U[i] = u0[i] * g0; U[3 + i] = u1[i] * g1; U[6 + i] = u2[i] * g2;
        V[i] = v0[i]; V[3 + i] = v1[i]; V[6 + i] = v2[i];
    }
}

// out = U diag(s) V^T
__device__ __forceinline__ void usvt(const double *U, const double *s, const double *V, double *out) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            ADMM_M3(out, r, c) = fma(U[r] * s[0], V[c], fma(U[3 + r] * s[1], V[3 + c], U[6 + r] * s[2] * V[6 + c]));
}

// ---- principal-stretch objectives --------------------------------------------------------------
// KIND 1: Neo-Hookean  Psi = mu/2 (I1 - ln I3 - 3) + lambda/8 ln^2 I3     (TetEnergyTerm.cpp:173-182)
// KIND 2: StVK         Psi = mu |E|^2 + lambda/2 tr(E)^2, E_i=(s_i^2-1)/2  (TetEnergyTerm.cpp:220-226)
// KIND 3: co-rotated   Psi = mu sum (s_i-1)^2 + lambda/2 (sum s_i - 3)^2   (SplineTet with xu::CoRotated, kappa = 0)
// objective = Psi(s) + k/2 |s - x0|^2                                      (:184-192, :210-218)
// The model is templated on the scalar type: the same Newton runs first in FP32 (cheap iterations that
// get within ~1e-6 of the minimiser) and then in FP64 (one or two polishing iterations).  Newton is
// self-correcting, so the FP64 result does not depend on the FP32 phase beyond its starting point.
__device__ __forceinline__ float t_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double t_rcp(double x) { return fast_rcp(x); }
__device__ __forceinline__ float t_log(float x) { return __logf(x); }
// ln(x) for finite normal x > 0 (the callers pass J = s0 s1 s2 with every s >= 1e-12).  x = m 2^e with
// m in [sqrt(1/2), sqrt(2)); ln m = 2 atanh(z), z = (m - 1)/(m + 1), |z| <= 0.1716: ten odd-series terms give
// < 1 ulp of truncation error.  ~30 instructions against ~120 for the library log (the NH polish is VALU-bound).
__device__ __forceinline__ double fast_log(double x) {
    const int hi = __double2hiint(x), lo = __double2loint(x);
    int e = ((hi >> 20) & 0x7ff) - 1023;
    double m = __hiloint2double((hi & 0x000fffff) | 0x3ff00000, lo);   // [1, 2)
    if (m > 1.4142135623730951) { m *= 0.5; e += 1; }
    const double z = (m - 1.0) * fast_rcp(m + 1.0);
    const double z2 = z * z;
    double p = 1.0 / 21.0;
    p = fma(p, z2, 1.0 / 19.0); p = fma(p, z2, 1.0 / 17.0); p = fma(p, z2, 1.0 / 15.0); p = fma(p, z2, 1.0 / 13.0);
    p = fma(p, z2, 1.0 / 11.0); p = fma(p, z2, 1.0 / 9.0); p = fma(p, z2, 1.0 / 7.0); p = fma(p, z2, 1.0 / 5.0);
    p = fma(p, z2, 1.0 / 3.0);
    const double lm = fma(z * z2, 2.0 * p, 2.0 * z);                  // 2 z (1 + z^2 p)
    return fma((double)e, 0.6931471805599453, lm);
}
#ifdef ADMM_LIBM_LOG
__device__ __forceinline__ double t_log(double x) { return log(x); }
#else
__device__ __forceinline__ double t_log(double x) { return fast_log(x); }
#endif
__device__ __forceinline__ float t_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double t_fma(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float t_abs(float a) { return fabsf(a); }
__device__ __forceinline__ double t_abs(double a) { return fabs(a); }
__device__ __forceinline__ float t_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double t_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float t_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double t_min(double a, double b) { return fmin(a, b); }

template <int KIND, typename T>
struct StretchModel {
    T mu, la, k;
    T x0[3];

    // value, gradient and the Hessian split H = diag(D) + la * w w^T
    __device__ __forceinline__ T eval(const T *s, T *g, T *D, T *w) const {
        if (KIND == 1) {
            const T J = s[0] * s[1] * s[2];
            const T lJ = t_log(J);
            T f = T(0), q = T(0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const T si = t_rcp(s[i]);
                const T d = s[i] - x0[i];
                w[i] = si;
                g[i] = t_fma(mu, s[i] - si, t_fma(la * lJ, si, k * d));
                D[i] = t_fma(mu, t_fma(si, si, T(1)), t_fma(-la * lJ, si * si, k));
                f = t_fma(s[i], s[i], f);
                q = t_fma(d, d, q);
            }
            return T(0.5) * mu * (f - T(3)) - mu * lJ + T(0.5) * la * lJ * lJ + T(0.5) * k * q;
        } else if (KIND == 3) {
            // co-rotated linear: Psi = mu sum (s_i - 1)^2 + la/2 (sum s_i - 3)^2  (xu::CoRotated, XuSpline.hpp:84-96,
            // with kappa = 0: sum f(s_i) + sum g(s_i s_j) collapses to this); quadratic, H = (2 mu + k) I + la 1 1^T
            const T tr = s[0] + s[1] + s[2] - T(3);
            T ee = T(0), q = T(0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const T e = s[i] - T(1);
                const T d = s[i] - x0[i];
                w[i] = T(1);
                g[i] = t_fma(T(2) * mu, e, t_fma(la, tr, k * d));
                D[i] = t_fma(T(2), mu, k);
                ee = t_fma(e, e, ee);
                q = t_fma(d, d, q);
            }
            return mu * ee + T(0.5) * la * tr * tr + T(0.5) * k * q;
        } else {
            const T ss = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
            const T trE = T(0.5) * (ss - T(3));
            T ee = T(0), q = T(0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const T E = T(0.5) * (s[i] * s[i] - T(1));
                const T d = s[i] - x0[i];
                w[i] = s[i];
                g[i] = t_fma(mu * s[i], s[i] * s[i] - T(1), t_fma(la * trE, s[i], k * d));
                D[i] = t_fma(mu, T(3) * s[i] * s[i] - T(1), t_fma(la, trE, k));
                ee = t_fma(E, E, ee);
                q = t_fma(d, d, q);
            }
            return mu * ee + T(0.5) * la * trE * trE + T(0.5) * k * q;
        }
    }
    // NH needs s > 0 (log barrier); StVK / co-rotated accept s >= 0 (value() returns FLT_MAX only for s < 0)
    __device__ __forceinline__ bool feasible(const T *s) const {
        if (KIND == 1) return s[0] > T(0) && s[1] > T(0) && s[2] > T(0);
        return s[0] >= T(0) && s[1] >= T(0) && s[2] >= T(0);
    }
};

// Newton direction at (s, g, D, w): Sherman-Morrison solve with |D| floored, frozen components on the s = 0 boundary (StVK),
// scaled steepest descent if the rank-one part makes it no descent direction.  Returns false at a zero (reduced) gradient.
// pure = the exact Newton step (no floored / flipped curvature, no frozen component).
template <int KIND, typename T>
__device__ __forceinline__ bool newton_direction(const StretchModel<KIND, T> &m, const T *s, const T *g, const T *D, const T *w,
                                                 T *d, T &gd, bool &pure) {
    const T floorD = T(1e-8) * (t_abs(m.k) + t_abs(m.mu)) + T(1e-30);
    // H = diag(D) + la w w^T.  Every D_i > 0: positive definite.  Exactly ONE D_i < 0: still positive definite iff
    // 1 + la sum w_i^2 / D_i < 0 (det H = prod D_i (1 + la sum w_i^2 / D_i); Cauchy interlacing settles the other minors) --
    // the case of a strongly compressed stretch next to strongly extended ones (NH: log J > 0 turns a diagonal entry negative
    // while the rank-one barrier term keeps the Hessian convex).  In both cases the Sherman-Morrison solve with the SIGNED
    // diagonal is the exact Newton step.  Otherwise |D| is floored: a convexified model, linear convergence (it used to
    // serve the second case too, and elements at stretches like (4.9, 2.9, 2.4) then stopped at the iteration cap 5e-5 short
    // of the minimiser).
    T a[3], y[3];
    int nneg = 0;
    bool okD = true, act[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        act[i] = (KIND >= 2) && (s[i] <= T(0)) && (g[i] > T(0));
        okD = okD && !act[i] && (t_abs(D[i]) >= floorD);
        nneg += (D[i] < T(0)) ? 1 : 0;
    }
    T wDw = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = t_rcp(okD ? D[i] : T(1));
        wDw = t_fma(w[i] * w[i], a[i], wDw);
    }
    T den = t_fma(m.la, wDw, T(1));
    pure = okD && (nneg == 0 ? den > T(1e-6) : (nneg == 1 && den < T(-1e-6)));
    if (!pure) {
        wDw = T(0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i] = act[i] ? T(0) : t_rcp(t_max(t_abs(D[i]), floorD));
            wDw = t_fma(w[i] * w[i], a[i], wDw);
        }
        den = t_fma(m.la, wDw, T(1));
    }
    T wDg = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        y[i] = g[i] * a[i];
        wDg = t_fma(w[i], y[i], wDg);
    }
    const T coef = (pure || den > T(1e-6)) ? m.la * wDg * t_rcp(den) : T(0);
    gd = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = -(y[i] - coef * w[i] * a[i]);
        gd = t_fma(g[i], d[i], gd);
    }
    if (!(gd < T(0))) { // not a descent direction (indefinite rank-one part): scaled steepest descent
        gd = T(0); pure = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) { d[i] = -y[i]; gd = t_fma(g[i], d[i], gd); }
        if (!(gd < T(0))) return false;
    }
    return true;
}
// The lean version for the common case: the EXACT Newton step, or false if the Hessian is not positive definite by the test
// above / a bound is active / the step is no descent direction -- the caller then leaves the element to the general loop.
template <int KIND, typename T>
__device__ __forceinline__ bool newton_direction_exact(const StretchModel<KIND, T> &m, const T *s, const T *g, const T *D, const T *w, T *d) {
    const T floorD = T(1e-8) * (t_abs(m.k) + t_abs(m.mu)) + T(1e-30);
    T a[3];
    int nneg = 0;
    bool okD = true;
    T wDw = T(0), wDg = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        okD = okD && !((KIND >= 2) && (s[i] <= T(0)) && (g[i] > T(0))) && (t_abs(D[i]) >= floorD);
        nneg += (D[i] < T(0)) ? 1 : 0;
        a[i] = t_rcp(D[i]);
        wDw = t_fma(w[i] * w[i], a[i], wDw);
        wDg = t_fma(w[i], g[i] * a[i], wDg);
    }
    const T den = t_fma(m.la, wDw, T(1));
    const bool pd = okD && (nneg == 0 ? den > T(1e-6) : (nneg == 1 && den < T(-1e-6)));
    const T coef = m.la * wDg * t_rcp(den);
    T gd = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = -(g[i] - coef * w[i]) * a[i];
        gd = t_fma(g[i], d[i], gd);
    }
    return pd && gd < T(0);
}
// Is the step d small enough to be applied without re-evaluation (quadratic convergence: the remaining error is ~ step^2)?
// That error is ~ step^2 times (third / second derivative) ~ step^2 / s_min near the barrier / the s = 0 boundary: the
// threshold scales with min(1, s_min)^2, never below the 1e-9 the FP64 callers tolerate; and the estimate only holds for
// an exact Newton step.
template <typename T>
__device__ __forceinline__ bool newton_step_is_final(const T *s, const T *d, bool pure, T tol_final) {
    T dmax = T(0), mag = T(1);
#pragma unroll
    for (int i = 0; i < 3; ++i) { dmax = t_max(dmax, t_abs(d[i])); mag = t_max(mag, t_abs(s[i])); }
    const T smin = t_max(T(0), t_min(T(1), t_min(s[0], t_min(s[1], s[2]))));
    const T tol_floor = sizeof(T) == 4 ? tol_final * T(0.03) : T(1e-9);
    return dmax <= (pure ? t_max(tol_final * smin * smin, tol_floor) : tol_floor) * mag;
}

// (everything by value: an array whose address is passed to a real call lives in scratch memory for its whole life)
template <typename T> struct NewtonIO { T s[3], g[3], D[3], w[3], f; int it; };
template <int KIND, typename T>
__device__ __attribute__((noinline)) NewtonIO<T> newton_stretch_general(StretchModel<KIND, T> m, NewtonIO<T> io, int max_it, T tol_final, T noise, int max_ls);
// Safeguarded Newton for argmin_s Psi(s) + k/2 |s - x0|^2, started from s (in/out); returns iterations.
//  - Hessian = diag(D) + la w w^T  -> Sherman-Morrison solve, |D| floored to stay positive definite
//  - NH: the log barrier keeps iterates strictly positive.  StVK: the feasible set is s >= 0 and for
//    inverted elements the minimiser sits ON that boundary -> projected Newton (components at the bound
//    with an outward gradient are frozen, trial points are projected back)
//  - Armijo backtracking on the objective, evaluated once per trial point (value+gradient+Hessian)
//  - a predicted step below tol_final is applied without re-evaluation and ends the iteration
//  - the common case -- the FIRST step is already that final step in every lane of the wave (the callers start close) --
//    is straight-line code under a wave-uniform branch; the general loop follows only for waves that need it
template <int KIND, typename T>
__device__ __forceinline__ int newton_stretch(const StretchModel<KIND, T> &m, T *s, int max_it, T tol_final, T noise, int max_ls) {
    T g[3], D[3], w[3];
    T f = m.eval(s, g, D, w);
    {
        T d[3], sn[3];
        const bool exact = newton_direction_exact<KIND, T>(m, s, g, D, w, d);
        bool fin = exact && newton_step_is_final<T>(s, d, true, tol_final);
#pragma unroll
        for (int i = 0; i < 3; ++i) { sn[i] = s[i] + d[i]; if (KIND >= 2) sn[i] = t_max(sn[i], T(0)); }
        fin = fin && m.feasible(sn);
        if (__all(fin)) {
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] = sn[i];
            return 1;
        }
    }
    NewtonIO<T> io;
#pragma unroll
    for (int i = 0; i < 3; ++i) { io.s[i] = s[i]; io.g[i] = g[i]; io.D[i] = D[i]; io.w[i] = w[i]; }
    io.f = f; io.it = 0;
    io = newton_stretch_general<KIND, T>(m, io, max_it, tol_final, noise, max_ls);
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] = io.s[i];
    return io.it;
}
// the general loop, OUTLINED (noinline): it is the rare path (waves whose first step is not final in every lane) but it is the
// part with the most values alive -- inlined, it dictated the register allocation of the whole local-step kernel
template <int KIND, typename T>
__device__ __attribute__((noinline)) NewtonIO<T> newton_stretch_general(StretchModel<KIND, T> m, NewtonIO<T> io, int max_it, T tol_final, T noise, int max_ls) {
    T s[3], g[3], D[3], w[3], f = io.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { s[i] = io.s[i]; g[i] = io.g[i]; D[i] = io.D[i]; w[i] = io.w[i]; }
    const T fscale = T(4) * (t_abs(m.mu) + t_abs(m.la) + t_abs(m.k));
    int it = 0;
#pragma unroll 1
    for (; it < max_it; ++it) {
        T d[3], gd;
        bool pure;
        if (!newton_direction<KIND, T>(m, s, g, D, w, d, gd, pure)) break;
        if (newton_step_is_final<T>(s, d, pure, tol_final)) { // final correction: apply and stop
            T sn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { sn[i] = s[i] + d[i]; if (KIND >= 2) sn[i] = t_max(sn[i], T(0)); }
            if (m.feasible(sn)) {
#pragma unroll
                for (int i = 0; i < 3; ++i) s[i] = sn[i];
            }
            ++it;
            break;
        }
        T t = T(1), sn[3], gn[3], Dn[3], wn[3], fn = f;
        bool ok = false;
#pragma unroll 1
        for (int ls = 0; ls < max_ls; ++ls) {
            T gs = T(0); // g . (sn - s) along the projected path
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sn[i] = t_fma(t, d[i], s[i]);
                if (KIND >= 2) sn[i] = t_max(sn[i], T(0));
                gs = t_fma(g[i], sn[i] - s[i], gs);
            }
            if (m.feasible(sn)) {
                fn = m.eval(sn, gn, Dn, wn);
                // round-off in f is absolute (O(1) terms cancel to O(strain^2)): scale the allowance by the
                // magnitude of the terms, not by |f|
                if (fn <= f + T(1e-4) * gs + noise * (t_abs(f) + fscale)) { ok = true; break; }
            }
            t *= T(0.5);
        }
        if (!ok) break;
        f = fn;
#pragma unroll
        for (int i = 0; i < 3; ++i) { s[i] = sn[i]; g[i] = gn[i]; D[i] = Dn[i]; w[i] = wn[i]; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) io.s[i] = s[i];
    io.it = it;
    return io;
}

// mixed-precision driver: FP32 iterations, then FP64 polish.  Parameters are normalised by k so the
// FP32 phase works with O(1) coefficients.
//  - Start: for moderate strains (|x0 - 1| < 1/4) the exact Newton step from the REST state, whose gradient
//    and Hessian are known in closed form for both models (g = k (1 - x0), H = (2 mu + k) I + la 1 1^T), so
//    the first objective evaluation is saved and the start is O(strain^2) from the minimiser instead of
//    O(strain).  Larger strains start from the caller's s as before.
//  - FP32 Newton to a step of 3e-5, then FP64 Newton: its first step is ~1e-7 (FP32 rounding), below the
//    2e-6 threshold under which a step is applied without re-evaluation (remaining error ~ step^2).
template <int KIND>
__device__ __forceinline__ int minimize_stretch(double mu, double la, double k, const double *x0, double *s) {
    const double ik = fast_rcp(k);
    StretchModel<KIND, float> mf;
    mf.mu = (float)(mu * ik); mf.la = (float)(la * ik); mf.k = 1.0f;
    float sf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { mf.x0[i] = (float)x0[i]; sf[i] = (float)s[i]; }
    {
        const float v0 = mf.x0[0] - 1.0f, v1 = mf.x0[1] - 1.0f, v2 = mf.x0[2] - 1.0f;
        if (fmaxf(fabsf(v0), fmaxf(fabsf(v1), fabsf(v2))) < 0.25f) {
            const float D = fmaf(2.0f, mf.mu, 1.0f);
            const float iD = __frcp_rn(D);
            const float c = mf.la * (v0 + v1 + v2) * iD * __frcp_rn(fmaf(3.0f, mf.la, D));
            sf[0] = 1.0f + fmaf(v0, iD, -c); sf[1] = 1.0f + fmaf(v1, iD, -c); sf[2] = 1.0f + fmaf(v2, iD, -c);
        }
    }
    if (KIND == 1) { sf[0] = fmaxf(sf[0], 1e-12f); sf[1] = fmaxf(sf[1], 1e-12f); sf[2] = fmaxf(sf[2], 1e-12f); }
    int it = newton_stretch<KIND, float>(mf, sf, 10, 3e-5f, 1e-6f, 12);
    StretchModel<KIND, double> md;
    md.mu = mu * ik; md.la = la * ik; md.k = 1.0;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) { md.x0[i] = x0[i]; fin = fin && (sf[i] == sf[i]) && (fabsf(sf[i]) < 1e30f); }
    if (fin && mf.feasible(sf)) {
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = (double)sf[i];
    }
    it += newton_stretch<KIND, double>(md, s, 60, 2e-6, 4e-16, 50);
    return it;
}

// Prox in principal stretches.  S (in) = signed stretches of q = D_i x + u_i; S (out) = stretches of z.
// KIND 0, linear tet (src/TetEnergyTerm.cpp:73-92): z = (P + q)/2 with P = U V^T (signed factors)
//         == U diag((1 + S)/2) V^T.
// KIND 1/2/3, hyperelastic (src/TetEnergyTerm.cpp:114-136): minimise over the stretches.
// ---- xu:: splines WITH their compression term (SplineTet with a spline constructed with kappa != 0) --------------------
// Psi(s) = Psi_spline(s) + c(J),  J = s0 s1 s2,  c(J) = kappa/12 ((1 - J)/6)^3      (src/XuSpline.hpp:43-45, Eq. 16 of Xu et al.)
// c' = -kappa/24 ((1 - J)/6)^2 as the reference writes it; c'' = kappa/72 (1 - J)/6.  The Hessian of c(J) is
// c'' dJ dJ^T + c' d2J (d2J_ij = s_k off the diagonal): not diagonal-plus-rank-one next to the StVK / co-rotated terms, so
// this (rare) model runs a Newton with the dense 3 x 3 Hessian, FP64 only.  type: 0 xu::NeoHookean, 1 xu::StVK, 2 xu::CoRotated.
struct SplineKappaModel {
    int type;
    double mu, la, k, kappa, x0[3];
    __device__ __forceinline__ double lower() const { return 0.0; }
    __device__ __forceinline__ bool feasible(const double *s) const {
        if (type == 0) return s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0;
        return s[0] >= 0.0 && s[1] >= 0.0 && s[2] >= 0.0;
    }
    // value, gradient, Hessian H = {h00, h01, h02, h11, h12, h22}
    __device__ __forceinline__ double eval(const double *s, double *g, double *H) const {
        double D[3], w[3], f;
        if (type == 0) { StretchModel<1, double> m; m.mu = mu; m.la = la; m.k = k; m.x0[0] = x0[0]; m.x0[1] = x0[1]; m.x0[2] = x0[2]; f = m.eval(s, g, D, w); }
        else if (type == 1) { StretchModel<2, double> m; m.mu = mu; m.la = la; m.k = k; m.x0[0] = x0[0]; m.x0[1] = x0[1]; m.x0[2] = x0[2]; f = m.eval(s, g, D, w); }
        else { StretchModel<3, double> m; m.mu = mu; m.la = la; m.k = k; m.x0[0] = x0[0]; m.x0[1] = x0[1]; m.x0[2] = x0[2]; f = m.eval(s, g, D, w); }
        H[0] = fma(la * w[0], w[0], D[0]); H[1] = la * w[0] * w[1]; H[2] = la * w[0] * w[2];
        H[3] = fma(la * w[1], w[1], D[1]); H[4] = la * w[1] * w[2]; H[5] = fma(la * w[2], w[2], D[2]);
        const double J = s[0] * s[1] * s[2], t = (1.0 - J) * (1.0 / 6.0);
        const double c0 = kappa * (1.0 / 12.0) * t * t * t, c1 = -kappa * (1.0 / 24.0) * t * t, c2 = kappa * (1.0 / 72.0) * t;
        const double dJ[3] = {s[1] * s[2], s[2] * s[0], s[0] * s[1]};
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = fma(c1, dJ[i], g[i]);
        H[0] = fma(c2 * dJ[0], dJ[0], H[0]); H[3] = fma(c2 * dJ[1], dJ[1], H[3]); H[5] = fma(c2 * dJ[2], dJ[2], H[5]);
        H[1] += fma(c2 * dJ[0], dJ[1], c1 * s[2]); H[2] += fma(c2 * dJ[0], dJ[2], c1 * s[1]); H[4] += fma(c2 * dJ[1], dJ[2], c1 * s[0]);
        return f + c0;
    }
};
// argmin_s Psi(s) + c(J) + k/2 |s - x0|^2: projected, safeguarded Newton with the dense Hessian (Cholesky of the free block,
// scaled steepest descent when it is not positive definite), Armijo backtracking; iterated until the step is below 1e-9.
template <class MODEL>
__device__ __forceinline__ int newton_stretch_dense(const MODEL &m, double *s, int max_it) {
    double g[3], H[6];
    double f = m.eval(s, g, H);
    const double fscale = 4.0 * (fabs(m.mu) + fabs(m.la) + fabs(m.k));
    int it = 0;
#pragma unroll 1
    for (; it < max_it; ++it) {
        bool fr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) fr[i] = !(m.type != 0 && s[i] <= m.lower() && g[i] > 0.0);   // components held at the bound
        // frozen components: unit row / column, zero right-hand side
        const double a00 = fr[0] ? H[0] : 1.0, a11 = fr[1] ? H[3] : 1.0, a22 = fr[2] ? H[5] : 1.0;
        const double a01 = (fr[0] && fr[1]) ? H[1] : 0.0, a02 = (fr[0] && fr[2]) ? H[2] : 0.0, a12 = (fr[1] && fr[2]) ? H[4] : 0.0;
        const double r0 = fr[0] ? -g[0] : 0.0, r1 = fr[1] ? -g[1] : 0.0, r2 = fr[2] ? -g[2] : 0.0;
        double d[3];
        bool newton = false;
        const double floorD = 1e-8 * (fabs(m.k) + fabs(m.mu)) + 1e-30;
        if (a00 > floorD) {   // LDL^T of the 3 x 3
            const double l10 = a01 / a00, l20 = a02 / a00;
            const double d1 = a11 - l10 * a01;
            if (d1 > floorD) {
                const double l21 = (a12 - l20 * a01) / d1;
                const double d2 = a22 - l20 * a02 - l21 * l21 * d1;
                if (d2 > floorD) {
                    const double y0 = r0, y1 = r1 - l10 * y0, y2 = r2 - l20 * y0 - l21 * y1;
                    d[2] = y2 / d2;
                    d[1] = y1 / d1 - l21 * d[2];
                    d[0] = y0 / a00 - l10 * d[1] - l20 * d[2];
                    newton = true;
                }
            }
        }
        double gd = 0.0;
        if (newton) { gd = g[0] * d[0] + g[1] * d[1] + g[2] * d[2]; newton = gd < 0.0; }
        if (!newton) {   // scaled steepest descent on the free components
            d[0] = r0 / fmax(fabs(a00), floorD); d[1] = r1 / fmax(fabs(a11), floorD); d[2] = r2 / fmax(fabs(a22), floorD);
            gd = g[0] * d[0] + g[1] * d[1] + g[2] * d[2];
            if (!(gd < 0.0)) break;   // zero (reduced) gradient
        }
        const double dmax = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2])));
        const double mag = fmax(1.0, fmax(fabs(s[0]), fmax(fabs(s[1]), fabs(s[2]))));
        if (dmax <= 1e-9 * mag) {   // final correction: apply and stop
            double sn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { sn[i] = s[i] + d[i]; if (m.type != 0) sn[i] = fmax(sn[i], m.lower()); }
            if (m.feasible(sn)) { s[0] = sn[0]; s[1] = sn[1]; s[2] = sn[2]; }
            ++it;
            break;
        }
        double t = 1.0, sn[3], gn[3], Hn[6], fn = f;
        bool ok = false;
#pragma unroll 1
        for (int ls = 0; ls < 50; ++ls) {
            double gs = 0.0;
            bool clipped = false;      // an INTERIOR component would land on the bound
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sn[i] = fma(t, d[i], s[i]);
                if (m.type != 0) { clipped = clipped || (sn[i] < m.lower() && s[i] > m.lower()); sn[i] = fmax(sn[i], m.lower()); }
                gs = fma(g[i], sn[i] - s[i], gs);
            }
            // A component parked on the bound with an outward gradient is frozen for good, so an overshooting step must not put it
            // there while a shorter one keeps it inside: from (1.78, 0.98, 0.10) with x0_3 = -0.10 (StVK, k = 0.1 mu) the full step
            // clipped s_3 to 0 and the iteration ended on the boundary point (1.16, 1.13, 0), objective 1.33e5, where the closed-form
            // kernel and the reference reach the interior minimiser (1.04, 1.00, 0.95), 3.31e4.  The first kInteriorTries halvings
            // therefore only accept interior points; a minimiser that IS on the bound is approached geometrically and taken once the
            // remaining distance is below 2^-kInteriorTries of the step.
#ifndef ADMM_INTERIOR_TRIES
#define ADMM_INTERIOR_TRIES 30      // (0 = the rule before this one; tests/test_local_step_edges.py builds both to count iterations)
#endif
            constexpr int kInteriorTries = ADMM_INTERIOR_TRIES;
            if (m.feasible(sn) && !(clipped && ls < kInteriorTries)) {
                fn = m.eval(sn, gn, Hn);
                if (fn <= f + 1e-4 * gs + 4e-16 * (fabs(f) + fscale)) { ok = true; break; }
            }
            t *= 0.5;
        }
        if (!ok) break;
        f = fn;
#pragma unroll
        for (int i = 0; i < 3; ++i) { s[i] = sn[i]; g[i] = gn[i]; }
#pragma unroll
        for (int i = 0; i < 6; ++i) H[i] = Hn[i];
    }
    return it;
}
// ---- USER-DEFINED xu::Spline (src/XuSpline.hpp:34-46: any object with f, g, h, df, dg, dh; src/TetEnergyTerm.hpp:197-204) ----
// The host samples the six functions once (admm_host_tabulate_spline) and the device evaluates the TABLES.  One table per
// function F in {f, g, h}: kSplineNodes nodes, uniform in t = ln x over [x_lo, x_hi] (stretches are positive and the relative
// resolution is what matters: f lives on stretches, g on products of two, h on J), per node (F, dF/dt, d2F/dt2) with dF/dt =
// x F'(x) from the spline's own derivative and the second derivative from central differences of it.  Between nodes: the
// QUINTIC Hermite interpolant -- C2, so value, gradient and Hessian of the interpolated energy are derivatives of ONE function
// and the safeguarded Newton iteration above converges on it exactly as on a closed form.  Interpolation error of the gradient:
// O(dt^5) ~ 1e-10 relative at 1024 nodes.  Outside the table the end node's Taylor quadratic in x continues the function (finite
// down to x = 0: the polynomial splines are reproduced there to O(x_lo^3); a spline that is singular at 0 is not, and does not
// need to be -- its minimiser stays away from 0).
constexpr int kSplineNodes = 1024;
constexpr int kSplineFnDoubles = 4 + 3 * kSplineNodes;          // {t0, dt, 1 / dt, n} + nodes
constexpr int kSplineTableDoubles = 3 * kSplineFnDoubles;       // f, g, h
// F(x), F'(x), F''(x) from one function's table
__device__ __forceinline__ void spline_table_eval(const double *tab, double x, double &F, double &F1, double &F2) {
    const double t0 = tab[0], dt = tab[1], idt = tab[2];
    const int n = (int)tab[3];
    const double t = t_log(fmax(x, 1e-300));
    double r = (t - t0) * idt;
    int i = (int)floor(r);
    i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
    double u = r - (double)i;
    const double *a = tab + 4 + 3 * i;
    double p, pt, ptt;
    if (u < 0.0 || u > 1.0) {      // outside the table: the Taylor quadratic IN x of the nearest end node (finite down to x = 0)
        const double *e = u < 0.0 ? a : a + 3;
        const double xe = exp(u < 0.0 ? t0 : fma(dt, (double)(n - 1), t0)), ixe = 1.0 / xe;
        const double d1 = e[1] * ixe, d2 = (e[2] - e[1]) * ixe * ixe, dx = x - xe;
        F = fma(dx, fma(0.5 * dx, d2, d1), e[0]); F1 = fma(dx, d2, d1); F2 = d2;
        return;
    } else {
        const double F0 = a[0], G0 = a[1] * dt, H0 = a[2] * dt * dt, F1n = a[3], G1 = a[4] * dt, H1 = a[5] * dt * dt;
        // quintic Hermite: p(u) = c0 + c1 u + c2 u^2 + c3 u^3 + c4 u^4 + c5 u^5
        const double c0 = F0, c1 = G0, c2 = 0.5 * H0;
        const double dF = F1n - F0;
        const double c3 = 10.0 * dF - 6.0 * G0 - 4.0 * G1 - 1.5 * H0 + 0.5 * H1;
        const double c4 = -15.0 * dF + 8.0 * G0 + 7.0 * G1 + 1.5 * H0 - H1;
        const double c5 = 6.0 * dF - 3.0 * (G0 + G1) - 0.5 * H0 + 0.5 * H1;
        p = fma(u, fma(u, fma(u, fma(u, fma(u, c5, c4), c3), c2), c1), c0);
        pt = fma(u, fma(u, fma(u, fma(u, 5.0 * c5, 4.0 * c4), 3.0 * c3), 2.0 * c2), c1) * idt;
        ptt = fma(u, fma(u, fma(u, 20.0 * c5, 12.0 * c4), 6.0 * c3), 2.0 * c2) * idt * idt;
    }
    const double ix = fast_rcp(fmax(x, 1e-300));
    F = p; F1 = pt * ix; F2 = (ptt - pt) * ix * ix;
}
struct SplineTableModel {
    int type;                 // 1: stretches are kept at or above the table's lower end (projected steps)
    const double *tab;        // [3][kSplineFnDoubles]
    double mu, la, k, x0[3], lo;
    __device__ __forceinline__ double lower() const { return lo; }
    __device__ __forceinline__ bool feasible(const double *s) const { return s[0] >= lo && s[1] >= lo && s[2] >= lo; }
    // Psi = sum f(s_i) + sum_{i<j} g(s_i s_j) + h(s_0 s_1 s_2) + k/2 |s - x0|^2 (src/TetEnergyTerm.cpp:243-265), dense Hessian
    __device__ __forceinline__ double eval(const double *s, double *g, double *H) const {
        double val = 0.0;
        const double *tf = tab, *tg = tab + kSplineFnDoubles, *th = tab + 2 * kSplineFnDoubles;
        double f0, f1, f2;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            spline_table_eval(tf, s[i], f0, f1, f2);
            const double dx = s[i] - x0[i];
            val += f0 + 0.5 * k * dx * dx;
            g[i] = fma(k, dx, f1);
            H[i == 0 ? 0 : i == 1 ? 3 : 5] = f2 + k;
        }
        H[1] = 0.0; H[2] = 0.0; H[4] = 0.0;
        // pairs (0,1), (0,2), (1,2)
        const int pi[3] = {0, 0, 1}, pj[3] = {1, 2, 2}, ph[3] = {1, 2, 4};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int i = pi[q], j = pj[q];
            spline_table_eval(tg, s[i] * s[j], f0, f1, f2);
            val += f0;
            g[i] = fma(f1, s[j], g[i]); g[j] = fma(f1, s[i], g[j]);
            H[i == 0 ? 0 : 3] = fma(f2 * s[j], s[j], H[i == 0 ? 0 : 3]);
            H[j == 1 ? 3 : 5] = fma(f2 * s[i], s[i], H[j == 1 ? 3 : 5]);
            H[ph[q]] = fma(f2 * s[i], s[j], H[ph[q]]) + f1;
        }
        const double J = s[0] * s[1] * s[2];
        spline_table_eval(th, J, f0, f1, f2);
        val += f0;
        const double dJ[3] = {s[1] * s[2], s[2] * s[0], s[0] * s[1]};
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = fma(f1, dJ[i], g[i]);
        H[0] = fma(f2 * dJ[0], dJ[0], H[0]); H[3] = fma(f2 * dJ[1], dJ[1], H[3]); H[5] = fma(f2 * dJ[2], dJ[2], H[5]);
        H[1] += fma(f2 * dJ[0], dJ[1], f1 * s[2]); H[2] += fma(f2 * dJ[0], dJ[2], f1 * s[1]); H[4] += fma(f2 * dJ[1], dJ[2], f1 * s[0]);
        return val;
    }
};
// HyperElasticTet::prox on the stretches (src/TetEnergyTerm.cpp:124-135) for a tabulated (user-defined) spline.  k_scale = a
// stiffness of the order of the spline's own (the tet's k) for the solver's round-off thresholds.
__device__ __forceinline__ void prox_stretches_table(const double *tab, double k, double *S) {
    SplineTableModel m;
    m.type = 1; m.tab = tab; m.k = k; m.mu = k; m.la = k;
    m.lo = 0.0;                                           // stretches stay >= 0 (the reference's objective is infinite below, src/TetEnergyTerm.cpp:211-214)
    m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];       // :124 set_x0 (before the fix-ups)
    const double eps = 1e-6;
    if (fabs(S[0]) < eps && fabs(S[1]) < eps && fabs(S[2]) < eps) { S[0] = eps; S[1] = eps; S[2] = eps; } // :128-131
    S[0] = fabs(S[0]); S[1] = fabs(S[1]); S[2] = fabs(S[2]);   // :133
    newton_stretch_dense(m, S, 200);
}
// HyperElasticTet::prox on the stretches (src/TetEnergyTerm.cpp:124-135) for a spline with kappa != 0
__device__ __forceinline__ int prox_stretches_kappa(int type, double mu, double la, double k, double kappa, double *S) {      // returns the Newton iterations
    SplineKappaModel m;
    const double ik = fast_rcp(k);
    m.type = type; m.mu = mu * ik; m.la = la * ik; m.k = 1.0; m.kappa = kappa * ik;
    m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];       // :124 set_x0 (before the fix-ups)
    const double eps = 1e-6;
    if (fabs(S[0]) < eps && fabs(S[1]) < eps && fabs(S[2]) < eps) { S[0] = eps; S[1] = eps; S[2] = eps; } // :128-131
    S[0] = fabs(S[0]); S[1] = fabs(S[1]); S[2] = fabs(S[2]);   // :133
    if (type == 0) { S[0] = fmax(S[0], 1e-12); S[1] = fmax(S[1], 1e-12); S[2] = fmax(S[2], 1e-12); }
    return newton_stretch_dense(m, S, 200);
}

// ---- STABLE NEO-HOOKEAN (the reference's README lists it as a TODO, README.md:23-28; no reference code: "parity unpinned") -------------
// Smith, de Goes, Kim, "Stable Neo-Hookean Flesh Simulation", ACM TOG 37(2), 2018, Eq. 14 with the re-parametrisation of their section
// 3.4 so that the model meets linear elasticity at the rest state with the TET's Lame constants:
//     Psi(F) = mu_s / 2 (I_C - 3) + la_s / 2 (J - alpha)^2 - mu_s / 2 log(I_C + 1),
//     mu_s = 4/3 mu,  la_s = lambda + 5/6 mu,  alpha = 1 + mu_s / la_s - mu_s / (4 la_s) = 1 + 3 mu_s / (4 la_s),
// I_C = |F|_F^2 = sum s_i^2, J = det F = s0 s1 s2: rotation invariant, so the prox of HyperElasticTet::prox (src/TetEnergyTerm.cpp:114-136)
// is a minimisation over the signed stretches like for the other models -- finite and smooth for inverted and degenerate elements (no
// log J barrier), which is the point of the model.  Gradient and Hessian in the stretches (dJ_i = prod_{j != i} s_j, q = 1 / (I_C + 1)):
//     g_i  = mu_s s_i (1 - q) + la_s (J - alpha) dJ_i + k (s_i - x0_i)
//     H_ii = mu_s (1 - q) + 2 mu_s q^2 s_i^2 + la_s dJ_i^2 + k
//     H_ij = 2 mu_s q^2 s_i s_j + la_s (dJ_i dJ_j + (J - alpha) s_k)
// minimised by the dense-Hessian safeguarded Newton above (no bound on the stretches: type 0, always feasible).
struct StableNHModel {
    int type;                 // 0: no projected steps (newton_stretch_dense)
    double mu, la, k, alpha, x0[3];      // mu, la = mu_s, la_s (already divided by k when the caller scales the problem)
    __device__ __forceinline__ double lower() const { return -1.7976931348623157e308; }
    __device__ __forceinline__ bool feasible(const double *) const { return true; }
    __device__ __forceinline__ double eval(const double *s, double *g, double *H) const {
        const double IC = fma(s[0], s[0], fma(s[1], s[1], s[2] * s[2])), J = s[0] * s[1] * s[2], q = 1.0 / (IC + 1.0);
        const double dJ[3] = {s[1] * s[2], s[2] * s[0], s[0] * s[1]};
        const double Ja = J - alpha, a1 = mu * (1.0 - q), a2 = 2.0 * mu * q * q;
        double f = 0.5 * mu * (IC - 3.0) + 0.5 * la * Ja * Ja - 0.5 * mu * log(IC + 1.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double dx = s[i] - x0[i];
            f = fma(0.5 * k * dx, dx, f);
            g[i] = fma(a1, s[i], fma(la * Ja, dJ[i], k * dx));
        }
        H[0] = a1 + a2 * s[0] * s[0] + la * dJ[0] * dJ[0] + k;
        H[3] = a1 + a2 * s[1] * s[1] + la * dJ[1] * dJ[1] + k;
        H[5] = a1 + a2 * s[2] * s[2] + la * dJ[2] * dJ[2] + k;
        H[1] = a2 * s[0] * s[1] + la * (dJ[0] * dJ[1] + Ja * s[2]);
        H[2] = a2 * s[0] * s[2] + la * (dJ[0] * dJ[2] + Ja * s[1]);
        H[4] = a2 * s[1] * s[2] + la * (dJ[1] * dJ[2] + Ja * s[0]);
        return f;
    }
};
// mu_s, la_s, alpha of the model from the tet's Lame constants (the formulas above)
__device__ __forceinline__ void stable_nh_params(double mu, double la, double &mus, double &las, double &alpha) {
    mus = (4.0 / 3.0) * mu; las = la + (5.0 / 6.0) * mu; alpha = 1.0 + 0.75 * mus / las;
}
// HyperElasticTet::prox on the stretches (src/TetEnergyTerm.cpp:124-135) for the stable Neo-Hookean model; mu, la = the tet's Lame constants
__device__ __forceinline__ void prox_stretches_stable_nh(double mu, double la, double k, double *S) {
    StableNHModel m;
    // (stable_nh_params restated: a call moves alpha in front of the two products below, and the local step's instances, which sit on
    // spilled registers, came out with another schedule)
    const double ik = fast_rcp(k), mus = (4.0 / 3.0) * mu, las = la + (5.0 / 6.0) * mu;
    m.type = 0; m.mu = mus * ik; m.la = las * ik; m.k = 1.0; m.alpha = 1.0 + 0.75 * mus / las;
    m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];       // :124 set_x0 (before the fix-ups)
    const double eps = 1e-6;
    if (fabs(S[0]) < eps && fabs(S[1]) < eps && fabs(S[2]) < eps) { S[0] = eps; S[1] = eps; S[2] = eps; } // :128-131
    S[0] = fabs(S[0]); S[1] = fabs(S[1]); S[2] = fabs(S[2]);   // :133 (the start only: the minimiser itself may cross zero)
    newton_stretch_dense(m, S, 200);
}

template <int KIND>
__device__ __forceinline__ void prox_stretches(double mu, double la, double k, double *S) {
    if (KIND == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) S[i] = 0.5 * (1.0 + S[i]);
        return;
    }
    double x0[3] = {S[0], S[1], S[2]};                      // :124 set_x0 (before the fix-ups)
    const double eps = 1e-6;
    if (fabs(S[0]) < eps && fabs(S[1]) < eps && fabs(S[2]) < eps) { S[0] = eps; S[1] = eps; S[2] = eps; } // :128-131
    S[0] = fabs(S[0]); S[1] = fabs(S[1]); S[2] = fabs(S[2]);   // :133 (flips the signed smallest stretch, wherever signed_svd3 left it)
    if (KIND == 1) { // keep the start strictly inside the log barrier
        S[0] = fmax(S[0], 1e-12); S[1] = fmax(S[1], 1e-12); S[2] = fmax(S[2], 1e-12);
    }
    minimize_stretch<(KIND == 0 ? 1 : KIND)>(mu, la, k, x0, S);
}

// src/TriEnergyTerm.cpp:73-101.  q = 3x2 column-major (6 doubles) -> z
__device__ __forceinline__ void prox_tri(const double *q, double lmin, double lmax, double *z) {
    // C = F^T F (2x2); one exact Jacobi rotation diagonalises it
    double c00 = dot3(q, q), c01 = dot3(q, q + 3), c11 = dot3(q + 3, q + 3);
    double cs = 1.0, sn = 0.0;
    if (fabs(c01) > 1e-17 * (c00 + c11)) {
        const double a = c11 - c00, b = 2.0 * c01;
        const double h2 = fma(a, a, b * b);
        const double t = copysign(1.0, a) * b * fast_rcp(fabs(a) + h2 * fast_rsqrt(h2));
        cs = fast_rsqrt(fma(t, t, 1.0));
        sn = t * cs;
    }
    // v0 = (cs, -sn), v1 = (sn, cs);  b_j = F v_j
    double b0[3], b1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        b0[r] = cs * q[r] - sn * q[3 + r];
        b1[r] = sn * q[r] + cs * q[3 + r];
    }
    double n0 = dot3(b0, b0), n1 = dot3(b1, b1);
    double u0[3], u1[3];
    // order so that (b0,n0) is the larger one
    bool swapped = false;
    if (n0 < n1) {
        swapped = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) { double t = b0[r]; b0[r] = b1[r]; b1[r] = t; }
        double t = n0; n0 = n1; n1 = t;
    }
    if (n0 > 1e-300) {
        const double inv = fast_rsqrt(n0);
#pragma unroll
        for (int r = 0; r < 3; ++r) u0[r] = b0[r] * inv;
    } else { u0[0] = 1.0; u0[1] = 0.0; u0[2] = 0.0; }
    const double pr = dot3(u0, b1);
    double w[3] = {fma(-pr, u0[0], b1[0]), fma(-pr, u0[1], b1[1]), fma(-pr, u0[2], b1[2])};
    double wn = dot3(w, w);
    if (!(wn > 1e-30 * n0) || !(wn > 1e-300)) {
        double e[3] = {0.0, 0.0, 0.0};
        const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
        if (a0 <= a1 && a0 <= a2) e[0] = 1.0; else if (a1 <= a2) e[1] = 1.0; else e[2] = 1.0;
        cross3(u0, e, w);
        wn = dot3(w, w);
    }
    {
        const double inv = fast_rsqrt(wn);
#pragma unroll
        for (int r = 0; r < 3; ++r) u1[r] = w[r] * inv;
    }
    // P = u0 v0^T + u1 v1^T  (v's in the possibly swapped order)
    double va[2], vb[2];
    if (!swapped) { va[0] = cs; va[1] = -sn; vb[0] = sn; vb[1] = cs; }
    else          { va[0] = sn; va[1] = cs;  vb[0] = cs; vb[1] = -sn; }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double p = fma(u0[r], va[c], u1[r] * vb[c]);
            z[c * 3 + r] = 0.5 * (p + q[c * 3 + r]);
        }
    if (lmin > 0.0 || lmax < 99.0) { // :91-99
        const double l0 = sqrt(dot3(z, z)), l1 = sqrt(dot3(z + 3, z + 3));
        double f0 = 1.0, f1 = 1.0;
        if (l0 < lmin) f0 = lmin / l0;
        if (l1 < lmin) f1 = lmin / l1;
        if (l0 > lmax) f0 = lmax / l0;
        if (l1 > lmax) f1 = lmax / l1;
#pragma unroll
        for (int r = 0; r < 3; ++r) { z[r] *= f0; z[3 + r] *= f1; }
    }
}

// ---- TANGENT STIFFNESS of one element: dP = (d2 psi / dF2) : dF  (tangent.hpp: k_tangent; tests/hostmath/tangent_host.cpp) -------------
// No reference code (the reference's gradient() throws, a Hessian does not exist there).  For a tet with F = U diag(sigma) V^T (the signed
// SVD) and psi an isotropic density, with A = U^T dF V:  dP = U B V^T,
//     B_ii = sum_j Hs_ij A_jj,                                   Hs = d2 psi / dsigma2
//     B_ij = al_ij (A_ij + A_ji) / 2 + be_ij (A_ij - A_ji) / 2,  al_ij = (p_i - p_j) / (sigma_i - sigma_j)   (twist)
//                                                                be_ij = (p_i + p_j) / (sigma_i + sigma_j)   (flip)
// p = dpsi/dsigma.  The quotients are never formed as written: every density here has a closed-form divided difference.  With e the
// stretches as the density takes them (e = |sigma|, or e = sigma for StVK and stable Neo-Hookean), g = dpsi/de, (i, j, l) a permutation:
//     linear        g_i = k (e_i - 1)                          al' = k                               be' = k ((e_i - 1) + (e_j - 1)) / (e_i + e_j)
//     Neo-Hookean   g_i = mu (e_i - 1/e_i) + la lnJ / e_i      al' = mu + (mu - la lnJ) / (e_i e_j)  be' = mu - (mu - la lnJ) / (e_i e_j)
//     StVK          g_i = e_i (mu (e_i^2 - 1) + la trE)        al' = mu (e_i^2 + e_i e_j + e_j^2 - 1) + la trE,  be': with - e_i e_j
//     co-rotated    g_i = 2 mu (e_i - 1) + la tr               al' = 2 mu                            be' = (g_i + g_j) / (e_i + e_j)
//     + c(J)        g_i += c' e_j e_l                          al' -= c' e_l                         be' += c' e_l
//     stable NH     g_i = a1 e_i + la_s (J - alpha) e_j e_l    al' = a1 - la_s (J - alpha) e_l       be' = a1 + la_s (J - alpha) e_l
//     tabulated     g_i = f'(e_i) + g'(e_i e_j) e_j + g'(e_i e_l) e_l + h'(J) e_j e_l
//                   al' = [f'](e_i, e_j) - g'(e_i e_j) + e_l^2 [g'](e_i e_l, e_j e_l) - h'(J) e_l,   be' = (g_i + g_j) / (e_i + e_j)
// [F'](x, y) = (F'(x) - F'(y)) / (x - y) = the mean of F'' between y and x: the quotient where x and y are 5 % apart (it loses 20 ulp
// there), the 3-point Gauss mean of the table's F'' where they are closer (exact for the interpolant's quintic pieces; across a node
// the interpolant's F''' jumps by the table's own representation error).  For the kinds taken at e = |sigma| the frame U diag(s) is an
// SVD of F with the unsigned stretches, in which the formulas hold as they stand with e_i + e_j > 0: carried back to the signed frame
// that is Hs_ij = s_i s_j H_ij and (al, be)_ij = (al', be')_ij, swapped where s_i s_j < 0 -- the energy is smooth at sigma_i = -sigma_j.
// StVK and stable Neo-Hookean take the signed stretches: their be' is a polynomial, finite at sigma_i = -sigma_j as well.
// Limits, as for the forces (forces.hpp): at a stretch sigma_i = 0 the |sigma| kinds have a kink (sign(0) counts as +, be' divides by
// e_i + e_j) and the Neo-Hookean kinds a log barrier at J -> 0; the outputs there are what the arithmetic gives, nothing is clamped.
// Nor is the tangent projected to a positive semi-definite one.
__device__ __forceinline__ double spline_table_dd1(const double *tab, double x, double y, double f1x, double f1y) {
    const double d = x - y;
    if (fabs(d) > 0.05 * fmax(fabs(x), fabs(y))) return (f1x - f1y) / d;
    const double m = 0.5 * (x + y), r = 0.5 * d * 0.7745966692414834;      // sqrt(3 / 5)
    double f0, f1, c, lo, hi;
    spline_table_eval(tab, m, f0, f1, c);
    spline_table_eval(tab, m - r, f0, f1, lo);
    spline_table_eval(tab, m + r, f0, f1, hi);
    return fma(4.0 / 9.0, c, (5.0 / 18.0) * (lo + hi));
}
// the tabulated spline's Hs, al', be' at the unsigned stretches A (out of line: 25 table evaluations that only this model pays for)
__device__ __attribute__((noinline)) inline void tet_tangent_table(const double *tab, const double *A, double *Hs, double *al, double *be) {
    const int pi[3] = {0, 0, 1}, pj[3] = {1, 2, 2}, pl[3] = {2, 1, 0};
    double g[3];
    SplineTableModel m; m.type = 1; m.tab = tab; m.mu = 0.0; m.la = 0.0; m.k = 0.0; m.lo = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
    (void)m.eval(A, g, Hs);
    const double *tf = tab, *tg = tab + kSplineFnDoubles, *th = tab + 2 * kSplineFnDoubles;
    double f0, f2, f1[3], g1[3], h1;      // f'(e_i); g' at the products e_0 e_1, e_0 e_2, e_1 e_2; h'(J)
    const double pr[3] = {A[0] * A[1], A[0] * A[2], A[1] * A[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) { spline_table_eval(tf, A[i], f0, f1[i], f2); spline_table_eval(tg, pr[i], f0, g1[i], f2); }
    spline_table_eval(th, A[0] * A[1] * A[2], f0, h1, f2);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = pi[q], j = pj[q], l = pl[q];
        // the products e_i e_l and e_j e_l: pairs (0,1) -> pr[1], pr[2]; (0,2) -> pr[0], pr[2]; (1,2) -> pr[0], pr[1]
        const int qi = q == 0 ? 1 : 0, qj = q == 2 ? 1 : 2;
        al[q] = spline_table_dd1(tf, A[i], A[j], f1[i], f1[j]) - g1[q]
              + A[l] * A[l] * spline_table_dd1(tg, pr[qi], pr[qj], g1[qi], g1[qj]) - h1 * A[l];
        be[q] = (g[i] + g[j]) / (A[i] + A[j]);
    }
}
// EnergyTerm::energy of a tet, as a density: psi at the signed stretches S of its model (the return value; the energy is psi vol) and
// sg[i] = s_i dpsi/da_i, the diagonal of P = dpsi/dF in the frame of the signed SVD.  THE dispatch from (grp, type) to a model, for value
// and gradient at once -- both come out of the same eval, a caller that needs one discards the other.  The densities are the stretch
// models' own eval with the prox's quadratic switched off (k = 0); the signs follow the reference: the linear tet takes a = |sigma|
// (src/TetEnergyTerm.cpp:94-100), Neo-Hookean and every SplineTet flip a negative smallest stretch (:138-149) -- there s_i = sign(sigma_i),
// and at sigma_i = 0 the gradient is one-sided (sign(0) counts as +); StVK is even in the stretches and stable Neo-Hookean keeps the sign
// (its point): a = sigma, s_i = 1.  grp, type, k, kappa: kernels.hpp: Mat; tab: the tabulated spline's table (read by grp 4, type 3 only).
__device__ __forceinline__ double tet_energy_grad(int grp, int type, double mu, double la, double k, double kappa, const double *tab,
                                                  const double *S, double *sg) {
    const double A[3] = {fabs(S[0]), fabs(S[1]), fabs(S[2])};
    double g[3], D[3], w[3], H[6], psi;
    bool use_abs = true;
    if (grp == 0) {
        psi = 0.5 * k * ((A[0] - 1.0) * (A[0] - 1.0) + (A[1] - 1.0) * (A[1] - 1.0) + (A[2] - 1.0) * (A[2] - 1.0));
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = k * (A[i] - 1.0);
    } else if (grp == 1) {
        StretchModel<1, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        psi = m.eval(A, g, D, w);
    } else if (grp == 2) {
        StretchModel<2, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
        psi = m.eval(S, g, D, w);
        use_abs = false;
    } else if (grp == 3) {
        StretchModel<3, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        psi = m.eval(A, g, D, w);
    } else if (type == 3) {
        SplineTableModel m; m.type = 1; m.tab = tab; m.mu = 0.0; m.la = 0.0; m.k = 0.0; m.lo = 0.0;
        m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        psi = m.eval(A, g, H);
    } else if (type == 4) {
        StableNHModel m; m.type = 0; m.k = 0.0;
        stable_nh_params(mu, la, m.mu, m.la, m.alpha);
        m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
        psi = m.eval(S, g, H);
        use_abs = false;
    } else {
        SplineKappaModel m; m.type = type; m.mu = mu; m.la = la; m.k = 0.0; m.kappa = kappa; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        psi = m.eval(A, g, H);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sg[i] = (use_abs && S[i] < 0.0) ? -g[i] : g[i];
    return psi;
}
// The derivative of tet_energy_grad's sg with respect to the constants a tet's Mat stores (adjoint.hpp: k_param_sens;
// tests/hostmath/param_sens_host.cpp): sg as tet_energy_grad returns it, and dsg[3 p + i] = d sg_i / d theta_p, theta = (mu, la, kappa).
// Every density above has a stretch gradient LINEAR in its stored (mu, la, kappa) -- stable Neo-Hookean too: la_s (J - alpha) =
// la_s (J - 1) - 3/4 mu_s -- so the derivative is the kind's own eval at the unit parameter vectors; no density is restated.  kappa
// reaches the three xu:: splines only (grp 4, type 0..2); a kind is never evaluated at parameters its own formula divides by (stable
// Neo-Hookean at mu = la = 0).  The linear tet (its k is the factor on the energy) and the tabulated spline have no (mu, la, kappa) on
// the device: their columns are exactly 0.  TABLE = false: for callers that hold no tabulated spline, as tet_tangent_coef.
template <bool TABLE = true>
__device__ __forceinline__ void tet_param_grad(int grp, int type, double mu, double la, double k, double kappa, const double *tab,
                                               const double *S, double *sg, double *dsg) {
    if (!TABLE && grp == 4 && type == 3) type = 0;      // (cannot occur: compiles the table path out)
    (void)tet_energy_grad(grp, type, mu, la, k, kappa, tab, S, sg);
#pragma unroll
    for (int q = 0; q < 9; ++q) dsg[q] = 0.0;
    if (grp == 0 || (grp == 4 && type == 3)) return;
    (void)tet_energy_grad(grp, type, 1.0, 0.0, k, 0.0, tab, S, dsg);
    (void)tet_energy_grad(grp, type, 0.0, 1.0, k, 0.0, tab, S, dsg + 3);
    if (grp == 4 && type < 3) (void)tet_energy_grad(grp, type, 0.0, 0.0, k, 1.0, tab, S, dsg + 6);
}
// Hs = {h00, h01, h02, h11, h12, h22}, al and be for the pairs (0,1), (0,2), (1,2), all in the frame of the signed SVD.
// grp: the tet's model group (0 linear, 1 Neo-Hookean, 2 StVK, 3 co-rotated, 4 the dense-Hessian models by `type`, kernels.hpp: Mat)
// TABLE = false: for callers that hold no tabulated spline (type 3 cannot occur) -- the table path and its registers are compiled out
template <bool TABLE = true>
__device__ __forceinline__ void tet_tangent_coef(int grp, int type, double mu, double la, double k, double kappa, const double *tab,
                                                 const double *S, double *Hs, double *al, double *be) {
    const double A[3] = {fabs(S[0]), fabs(S[1]), fabs(S[2])};
    const int pi[3] = {0, 0, 1}, pj[3] = {1, 2, 2}, pl[3] = {2, 1, 0}, ph[3] = {1, 2, 4};
    double g[3], D[3], w[3];
    bool use_abs = true;
    if (grp == 0) {
        Hs[0] = k; Hs[3] = k; Hs[5] = k; Hs[1] = 0.0; Hs[2] = 0.0; Hs[4] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int i = pi[q], j = pj[q];
            al[q] = k;
            be[q] = k * ((A[i] - 1.0) + (A[j] - 1.0)) / (A[i] + A[j]);
        }
    } else if (TABLE && grp == 4 && type == 3) {
        tet_tangent_table(tab, A, Hs, al, be);
    } else if (grp == 2 || (grp == 4 && type == 4)) {
        use_abs = false;
        if (grp == 2) {
            StretchModel<2, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
            (void)m.eval(S, g, D, w);
            Hs[0] = fma(la * w[0], w[0], D[0]); Hs[1] = la * w[0] * w[1]; Hs[2] = la * w[0] * w[2];
            Hs[3] = fma(la * w[1], w[1], D[1]); Hs[4] = la * w[1] * w[2]; Hs[5] = fma(la * w[2], w[2], D[2]);
            const double c = fma(la, 0.5 * (fma(S[0], S[0], fma(S[1], S[1], S[2] * S[2])) - 3.0), -mu);      // la trE - mu
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = pi[q], j = pj[q];
                const double ss = fma(S[i], S[i], S[j] * S[j]), sij = S[i] * S[j];
                al[q] = fma(mu, ss + sij, c);
                be[q] = fma(mu, ss - sij, c);
            }
        } else {
            StableNHModel m; m.type = 0; m.k = 0.0;
            stable_nh_params(mu, la, m.mu, m.la, m.alpha);
            m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
            (void)m.eval(S, g, Hs);
            const double IC = fma(S[0], S[0], fma(S[1], S[1], S[2] * S[2])), a1 = m.mu * (1.0 - 1.0 / (IC + 1.0));
            const double lj = m.la * (S[0] * S[1] * S[2] - m.alpha);
#pragma unroll
            for (int q = 0; q < 3; ++q) { al[q] = fma(-lj, S[pl[q]], a1); be[q] = fma(lj, S[pl[q]], a1); }
        }
    } else {
        // Neo-Hookean / StVK at |sigma| / co-rotated, plain (grp 1, 3) or with the compression term c(J) (grp 4, type 0..2)
        const int base = grp == 1 ? 0 : grp == 3 ? 2 : type;
        if (base == 0) {
            StretchModel<1, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
            (void)m.eval(A, g, D, w);
            const double c = fma(-la, t_log(A[0] * A[1] * A[2]), mu);      // mu - la ln J
#pragma unroll
            for (int q = 0; q < 3; ++q) { const double ww = w[pi[q]] * w[pj[q]]; al[q] = fma(c, ww, mu); be[q] = fma(-c, ww, mu); }
        } else if (base == 1) {
            StretchModel<2, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
            (void)m.eval(A, g, D, w);
            const double c = fma(la, 0.5 * (fma(A[0], A[0], fma(A[1], A[1], A[2] * A[2])) - 3.0), -mu);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = pi[q], j = pj[q];
                const double ss = fma(A[i], A[i], A[j] * A[j]), sij = A[i] * A[j];
                al[q] = fma(mu, ss + sij, c);
                be[q] = fma(mu, ss - sij, c);
            }
        } else {
            StretchModel<3, double> m; m.mu = mu; m.la = la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
            (void)m.eval(A, g, D, w);
            const double tr = (A[0] - 1.0) + (A[1] - 1.0) + (A[2] - 1.0);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = pi[q], j = pj[q];
                al[q] = 2.0 * mu;
                be[q] = 2.0 * fma(mu, (A[i] - 1.0) + (A[j] - 1.0), la * tr) / (A[i] + A[j]);
            }
        }
        Hs[0] = fma(la * w[0], w[0], D[0]); Hs[1] = la * w[0] * w[1]; Hs[2] = la * w[0] * w[2];
        Hs[3] = fma(la * w[1], w[1], D[1]); Hs[4] = la * w[1] * w[2]; Hs[5] = fma(la * w[2], w[2], D[2]);
        if (grp == 4) {      // c(J) = kappa / 12 ((1 - J) / 6)^3, as SplineKappaModel::eval
            const double J = A[0] * A[1] * A[2], t = (1.0 - J) * (1.0 / 6.0);
            const double c1 = -kappa * (1.0 / 24.0) * t * t, c2 = kappa * (1.0 / 72.0) * t;
            const double dJ[3] = {A[1] * A[2], A[2] * A[0], A[0] * A[1]};
            Hs[0] = fma(c2 * dJ[0], dJ[0], Hs[0]); Hs[3] = fma(c2 * dJ[1], dJ[1], Hs[3]); Hs[5] = fma(c2 * dJ[2], dJ[2], Hs[5]);
            Hs[1] += fma(c2 * dJ[0], dJ[1], c1 * A[2]); Hs[2] += fma(c2 * dJ[0], dJ[2], c1 * A[1]); Hs[4] += fma(c2 * dJ[1], dJ[2], c1 * A[0]);
#pragma unroll
            for (int q = 0; q < 3; ++q) { al[q] = fma(-c1, A[pl[q]], al[q]); be[q] = fma(c1, A[pl[q]], be[q]); }
        }
    }
    if (use_abs) {      // back to the frame of the signed SVD
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if ((S[pi[q]] < 0.0) != (S[pj[q]] < 0.0)) { Hs[ph[q]] = -Hs[ph[q]]; const double t = al[q]; al[q] = be[q]; be[q] = t; }
    }
}
// One Jacobi rotation of the symmetric 3x3 A in the plane (p, q), r the third index, accumulated into the eigenvector columns vp, vq
__device__ __forceinline__ void sym3_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *vp, double *vq) {
    if (apq == 0.0) return;
    const double th = (aqq - app) / (2.0 * apq);
    const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(fma(th, th, 1.0)));      // th = +-inf: t = 0
    const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
    app = fma(-t, apq, app); aqq = fma(t, apq, aqq); apq = 0.0;
    const double rp = arp, rq = arq;
    arp = fma(c, rp, -s * rq); arq = fma(s, rp, c * rq);
#pragma unroll
    for (int i = 0; i < 3; ++i) { const double a = vp[i], b = vq[i]; vp[i] = fma(c, a, -s * b); vq[i] = fma(s, a, c * b); }
}
// The Frobenius-nearest positive semi-definite tangent of a tet, on the coefficients of tet_tangent_coef: in the frame of the signed SVD
// dP/dF is block-diagonal -- three twist eigenvalues al, three flip eigenvalues be, the 3x3 block Hs -- so al <- max(al, 0),
// be <- max(be, 0), Hs <- its positive part (cyclic Jacobi in FP64, 6 sweeps; Hs - sum_{lambda_k < 0} lambda_k v_k v_k^T).  An Hs
// without a negative eigenvalue is left UNTOUCHED: an element that is positive semi-definite already keeps its bits.
// NEGATIVE means below -kPsdNoise h, h the largest coefficient of the element.  A stress-free element has exact zero eigenvalues (be = 0:
// an infinitesimal rotation costs nothing), which the arithmetic returns as +-(a few ulp of h); clamping on their sign would change the
// bits of elements at rest for nothing.  What is left below zero is <= 5.7e-14 h, the rounding of the coefficients themselves.
constexpr double kPsdNoise = 0x1p-44;
__device__ __forceinline__ void tet_tangent_psd(double *Hs, double *al, double *be) {
    double h = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) h = fmax(h, fabs(Hs[q]));
#pragma unroll
    for (int q = 0; q < 3; ++q) h = fmax(h, fmax(fabs(al[q]), fabs(be[q])));
    const double neg = -kPsdNoise * h;
#pragma unroll
    for (int q = 0; q < 3; ++q) { al[q] = al[q] < neg ? 0.0 : al[q]; be[q] = be[q] < neg ? 0.0 : be[q]; }
    double a00 = Hs[0], a01 = Hs[1], a02 = Hs[2], a11 = Hs[3], a12 = Hs[4], a22 = Hs[5];
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 6; ++sweep) {
        sym3_rotate(a00, a11, a01, a02, a12, v0, v1);
        sym3_rotate(a00, a22, a02, a01, a12, v0, v2);
        sym3_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    const double n0 = a00 < neg ? a00 : 0.0, n1 = a11 < neg ? a11 : 0.0, n2 = a22 < neg ? a22 : 0.0;
    if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) return;
    const int hi[6] = {0, 0, 0, 1, 1, 2}, hj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int i = hi[q], j = hj[q];
        Hs[q] -= fma(n0 * v0[i], v0[j], fma(n1 * v1[i], v1[j], n2 * v2[i] * v2[j]));
    }
}

// dP = U B V^T, B from A = U^T dF V: B_ii = sum_j Hs_ij A_jj, B_ij = a_ij A_ij + b_ij A_ji with a = (al + be) / 2, b = (al - be) / 2
// (pairs (0,1), (0,2), (1,2)).  dF, dP column-major.
__device__ __forceinline__ void tet_tangent_apply(const double *U, const double *V, const double *Hs, const double *a, const double *b,
                                                  const double *dF, double *dP) {
    double T[9], A[9], B[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(T, r, c) = fma(ADMM_M3(dF, r, 0), ADMM_M3(V, 0, c), fma(ADMM_M3(dF, r, 1), ADMM_M3(V, 1, c), ADMM_M3(dF, r, 2) * ADMM_M3(V, 2, c)));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(A, r, c) = fma(ADMM_M3(U, 0, r), ADMM_M3(T, 0, c), fma(ADMM_M3(U, 1, r), ADMM_M3(T, 1, c), ADMM_M3(U, 2, r) * ADMM_M3(T, 2, c)));
    const double a0 = ADMM_M3(A, 0, 0), a1 = ADMM_M3(A, 1, 1), a2 = ADMM_M3(A, 2, 2);
    ADMM_M3(B, 0, 0) = fma(Hs[0], a0, fma(Hs[1], a1, Hs[2] * a2));
    ADMM_M3(B, 1, 1) = fma(Hs[1], a0, fma(Hs[3], a1, Hs[4] * a2));
    ADMM_M3(B, 2, 2) = fma(Hs[2], a0, fma(Hs[4], a1, Hs[5] * a2));
    ADMM_M3(B, 0, 1) = fma(a[0], ADMM_M3(A, 0, 1), b[0] * ADMM_M3(A, 1, 0)); ADMM_M3(B, 1, 0) = fma(a[0], ADMM_M3(A, 1, 0), b[0] * ADMM_M3(A, 0, 1));
    ADMM_M3(B, 0, 2) = fma(a[1], ADMM_M3(A, 0, 2), b[1] * ADMM_M3(A, 2, 0)); ADMM_M3(B, 2, 0) = fma(a[1], ADMM_M3(A, 2, 0), b[1] * ADMM_M3(A, 0, 2));
    ADMM_M3(B, 1, 2) = fma(a[2], ADMM_M3(A, 1, 2), b[2] * ADMM_M3(A, 2, 1)); ADMM_M3(B, 2, 1) = fma(a[2], ADMM_M3(A, 2, 1), b[2] * ADMM_M3(A, 1, 2));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(T, r, c) = fma(ADMM_M3(U, r, 0), ADMM_M3(B, 0, c), fma(ADMM_M3(U, r, 1), ADMM_M3(B, 1, c), ADMM_M3(U, r, 2) * ADMM_M3(B, 2, c)));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(dP, r, c) = fma(ADMM_M3(T, r, 0), ADMM_M3(V, c, 0), fma(ADMM_M3(T, r, 1), ADMM_M3(V, c, 1), ADMM_M3(T, r, 2) * ADMM_M3(V, c, 2)));
}
// The derivative of a tet's s = a . f_e = -vol P : A in its REST edge matrix Dm (Binv = Dm^-1; adjoint.hpp: k_rest_sens;
// tests/hostmath/rest_sens_host.cpp), masses and material constants held fixed:  ds/dDm = Gs Binv^T with
//     Gs = -vol [ (P : A) I - F^T T - A^T P ],    A = Ds(a) Binv (dF here),  T = H[A] the element tangent on A,
// from dBinv = -Binv dDm Binv, dvol = vol tr(Binv dDm), dF = -F dDm Binv, dA = -A dDm Binv.  Formed in the frame of the signed SVD
// F = U diag(S) V^T, where P = U diag(sg) V^T (tet_energy_grad) and T = U T^ V^T (the B of tet_tangent_apply on A^ = U^T A V):
//     Gs = -vol V [ (sum_i sg_i A^_ii) I - diag(S) T^ - A^^T diag(sg) ] V^T
// -- neither F nor P in full.  Hs, a, b: the coefficients as tet_tangent_apply takes them.  Gs column-major; the caller's
// tet_corner_forces(Gs, Binv) gives rest corner m + 1 column m of Gs Binv^T and corner 0 minus their sum.
__device__ __forceinline__ void tet_rest_grad(const double *U, const double *V, const double *S, const double *sg, const double *Hs, const double *a,
                                              const double *b, const double *dF, double vol, double *Gs) {
    double T[9], A[9], B[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(T, r, c) = fma(ADMM_M3(dF, r, 0), ADMM_M3(V, 0, c), fma(ADMM_M3(dF, r, 1), ADMM_M3(V, 1, c), ADMM_M3(dF, r, 2) * ADMM_M3(V, 2, c)));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(A, r, c) = fma(ADMM_M3(U, 0, r), ADMM_M3(T, 0, c), fma(ADMM_M3(U, 1, r), ADMM_M3(T, 1, c), ADMM_M3(U, 2, r) * ADMM_M3(T, 2, c)));
    const double a0 = ADMM_M3(A, 0, 0), a1 = ADMM_M3(A, 1, 1), a2 = ADMM_M3(A, 2, 2);
    ADMM_M3(B, 0, 0) = fma(Hs[0], a0, fma(Hs[1], a1, Hs[2] * a2));
    ADMM_M3(B, 1, 1) = fma(Hs[1], a0, fma(Hs[3], a1, Hs[4] * a2));
    ADMM_M3(B, 2, 2) = fma(Hs[2], a0, fma(Hs[4], a1, Hs[5] * a2));
    ADMM_M3(B, 0, 1) = fma(a[0], ADMM_M3(A, 0, 1), b[0] * ADMM_M3(A, 1, 0)); ADMM_M3(B, 1, 0) = fma(a[0], ADMM_M3(A, 1, 0), b[0] * ADMM_M3(A, 0, 1));
    ADMM_M3(B, 0, 2) = fma(a[1], ADMM_M3(A, 0, 2), b[1] * ADMM_M3(A, 2, 0)); ADMM_M3(B, 2, 0) = fma(a[1], ADMM_M3(A, 2, 0), b[1] * ADMM_M3(A, 0, 2));
    ADMM_M3(B, 1, 2) = fma(a[2], ADMM_M3(A, 1, 2), b[2] * ADMM_M3(A, 2, 1)); ADMM_M3(B, 2, 1) = fma(a[2], ADMM_M3(A, 2, 1), b[2] * ADMM_M3(A, 1, 2));
    const double pa = fma(sg[0], a0, fma(sg[1], a1, sg[2] * a2));      // P : A
    // M = vol [ diag(S) T^ + A^^T diag(sg) - (P : A) I ]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double m = fma(S[r], ADMM_M3(B, r, c), ADMM_M3(A, c, r) * sg[c]);
            ADMM_M3(T, r, c) = vol * (r == c ? m - pa : m);
        }
    // Gs = V M V^T
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(B, r, c) = fma(ADMM_M3(V, r, 0), ADMM_M3(T, 0, c), fma(ADMM_M3(V, r, 1), ADMM_M3(T, 1, c), ADMM_M3(V, r, 2) * ADMM_M3(T, 2, c)));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ADMM_M3(Gs, r, c) = fma(ADMM_M3(B, r, 0), ADMM_M3(V, c, 0), fma(ADMM_M3(B, r, 1), ADMM_M3(V, c, 1), ADMM_M3(B, r, 2) * ADMM_M3(V, c, 2)));
}

// Triangle: E = w^2 / 2 sum (sigma_i - 1)^2 of the 3x2 F, P = w^2 (F - Q), Q = F C^(-1/2) the closest isometry (C = F^T F), so
// dP = w^2 (dF - dQ).  With F = Q S (S = C^(1/2)):  dQ = om Q J + (dF - Q Q^T dF) S^-1,  J = [[0, -1], [1, 0]],
// om = (q_1 . dF_0 - q_0 . dF_1) / (sigma_1 + sigma_2): the in-plane rotation, and the out-of-plane part.  The closed-form 2x2 inverse
// square root of forces.hpp.  tri_tangent_frame: Q (3x2 column-major), Si = {S^-1_00, S^-1_01, S^-1_11}, itr = 1 / (sigma_1 + sigma_2);
// at a collapsed triangle (sigma_1 sigma_2 -> 0) the outputs are what the arithmetic gives.
__device__ __forceinline__ void tri_tangent_frame(const double *F, double *Q, double *Si, double &itr) {
    const double c00 = dot3(F, F), c01 = dot3(F, F + 3), c11 = dot3(F + 3, F + 3);
    double cr[3];
    cross3(F, F + 3, cr);
    const double s = sqrt(dot3(cr, cr)), q = sqrt(c00 + c11 + 2.0 * s), iq = 1.0 / (q * s);
    Si[0] = (c11 + s) * iq; Si[1] = -c01 * iq; Si[2] = (c00 + s) * iq;
    itr = 1.0 / q;
#pragma unroll
    for (int j = 0; j < 3; ++j) { Q[j] = fma(F[j], Si[0], F[3 + j] * Si[1]); Q[3 + j] = fma(F[j], Si[1], F[3 + j] * Si[2]); }
}
// out = dF - dQ (3x2 column-major); the caller scales it by w^2
__device__ __forceinline__ void tri_tangent_apply(const double *Q, const double *Si, double itr, const double *dF, double *out) {
    const double m00 = dot3(Q, dF), m10 = dot3(Q + 3, dF), m01 = dot3(Q, dF + 3), m11 = dot3(Q + 3, dF + 3);
    const double om = (m10 - m01) * itr;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double n0 = dF[j] - fma(Q[j], m00, Q[3 + j] * m10), n1 = dF[3 + j] - fma(Q[j], m01, Q[3 + j] * m11);      // (I - Q Q^T) dF
        out[j] = dF[j] - fma(om, Q[3 + j], fma(n0, Si[0], n1 * Si[1]));
        out[3 + j] = dF[3 + j] - fma(-om, Q[j], fma(n0, Si[1], n1 * Si[2]));
    }
}
// The positive semi-definite part of a triangle's operator I - dQ/dF, on the frame of tri_tangent_frame.  Its eigenvalues: 1 (the
// in-plane symmetric modes), 1 - 2 / (sigma_1 + sigma_2) (the in-plane twist), 1 - 1 / sigma_i (the two out-of-plane modes, in the
// eigenbasis of S).  The twist factor is clamped at 0 (itr <- min(itr, 1/2)) and W = I - S^-1 replaced by its positive part (closed-form
// 2x2 symmetric eigen-decomposition; Si <- I - W+).  A frame without a negative eigenvalue keeps its bits; negative means below
// -kPsdNoise (the operator's scale is 1), as in tet_tangent_psd: a triangle at rest has these three eigenvalues at 0 +- rounding.
__device__ __forceinline__ void tri_tangent_psd(double *Si, double &itr) {
    if (1.0 - 2.0 * itr < -kPsdNoise) itr = 0.5;
    const double a = 1.0 - Si[0], b = -Si[1], d = 1.0 - Si[2];
    const double mean = 0.5 * (a + d), diff = 0.5 * (a - d), r = sqrt(fma(diff, diff, b * b));
    if (mean - r >= -kPsdNoise) return;
    if (mean + r <= 0.0) { Si[0] = 1.0; Si[1] = 0.0; Si[2] = 1.0; return; }
    const double lp = 0.5 * (mean + r), ir = 1.0 / r;      // W+ = lambda_+ / 2 (I + [[diff, b], [b, -diff]] / r)
    Si[0] = 1.0 - lp * fma(diff, ir, 1.0);
    Si[1] = -lp * (b * ir);
    Si[2] = 1.0 - lp * fma(-diff, ir, 1.0);
}
// out = the positive semi-definite part of (I - dQ/dF) applied to dF; the caller scales it by w^2
__device__ __forceinline__ void tri_tangent_apply_psd(const double *Q, const double *Si, double itr, const double *dF, double *out) {
    double Sp[3] = {Si[0], Si[1], Si[2]}, tw = itr;
    tri_tangent_psd(Sp, tw);
    tri_tangent_apply(Q, Sp, tw, dF, out);
}

// ---- Anderson acceleration (anderson.hpp): the small regularised solve ----
// theta = (H + kAaReg (tr H / n) I)^-1 b for the Gram matrix H [n][n] (n <= kAaMax; row-major with row stride kAaMax, the lower
// triangle is read) by Cholesky in FP64.  false -- the caller clears its history -- on a pivot that is not positive and finite or a
// theta that is not finite; theta is then zero.  work [kAaWork]: the factor and the intermediate vector (the device passes LDS: arrays
// indexed by a run-time n would otherwise live in scratch, a memory round trip per access of one serial thread).
constexpr int kAaMax = 8;
constexpr int kAaWork = kAaMax * kAaMax + kAaMax;
constexpr double kAaReg = 1e-10;
__device__ __forceinline__ bool aa_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)
__device__ __forceinline__ bool aa_small_solve(int n, const double *H, const double *b, double *theta, double *work) {
    double *L = work, *y = work + kAaMax * kAaMax;
    for (int i = 0; i < kAaMax; ++i) theta[i] = 0.0;
    if (n < 1 || n > kAaMax) return false;
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += H[i * kAaMax + i];
    const double reg = kAaReg * (tr / (double)n);
    bool ok = true;
    for (int j = 0; j < n && ok; ++j) {
        double d = H[j * kAaMax + j] + reg;
        for (int k = 0; k < j; ++k) d = fma(-L[j * kAaMax + k], L[j * kAaMax + k], d);
        if (!(d > 0.0) || !aa_finite(d)) { ok = false; break; }
        const double l = sqrt(d);
        L[j * kAaMax + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double s = H[i * kAaMax + j];
            for (int k = 0; k < j; ++k) s = fma(-L[i * kAaMax + k], L[j * kAaMax + k], s);
            L[i * kAaMax + j] = s / l;
        }
    }
    if (!ok) return false;
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = fma(-L[i * kAaMax + k], y[k], s);
        y[i] = s / L[i * kAaMax + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < n; ++k) s = fma(-L[k * kAaMax + i], theta[k], s);
        theta[i] = s / L[i * kAaMax + i];
    }
    for (int i = 0; i < n; ++i) ok = ok && aa_finite(theta[i]);
    if (!ok) for (int i = 0; i < kAaMax; ++i) theta[i] = 0.0;
    return ok;
}

// ---- the dense Rayleigh-Ritz of the block eigensolver (modal.hpp: k_modal_rr) ----
// G_A c = theta G_M c for symmetric G_A, G_M [n][n], n <= kModalMax, G_M positive definite: G_M is scaled to a unit diagonal and
// factorised by Cholesky (right-looking), L^-1 G_A L^-T is diagonalised by a parallel cyclic Jacobi (round-robin pairing: n / 2 disjoint
// rotations per stage, all row rotations of a stage, then all column rotations; sweeps until one rotates nothing, kModalSweeps at most),
// the eigenvalues are sorted ascending
// (ties by index) and C = D L^-T Q, so C^T G_M C = I and C^T G_A C = diag(ev).
//
// ONE text for the device and the host: the work is cut into PHASES of independent items; thread `tid` of `nt` takes the items tid,
// tid + nt, ... of every phase and `sync` separates the phases.  The device passes its 256 threads and __syncthreads, the host replay
// (tests/hostmath/modal_host.cpp) one thread and nothing: no item reads what another item of its phase writes, every entry sees the same
// operations in the same order, so the serial replay IS the device's arithmetic.  Every operation is a single rounding (explicit fma).
// Failure (false; ev and C zero): a diagonal of G_M or a Cholesky pivot that is not finite or below kModalPivot -- a multiple of eps
// times the scaled diagonal, which is 1 -- or a non-finite result.
constexpr int kModalMax = 48, kModalLd = 49;      // (an odd row stride: column accesses spread over the LDS banks)
constexpr int kModalSweeps = 12;                          // at most; a sweep without a rotation ends the Jacobi iteration
constexpr double kModalRotTol = 2.220446049250313e-16;      // |a_pq| <= eps sqrt(|a_pp a_qq|): no rotation
constexpr double kModalPivot = 64.0 * 2.220446049250313e-16;
struct ModalWork {            // the device keeps these in LDS
    double *A, *M, *Q;        // [kModalMax][kModalLd]: G_A -> H -> C; G_M -> L (strict lower triangle); the rotations
    double *ds, *dl, *ev, *cs;      // [kModalMax]: the scaling, L's diagonal, the eigenvalues; [kModalMax]: (c, s) of a stage's rotations
    int *perm, *ok;           // [kModalMax]; [2]: the verdict, "this sweep rotated"
};
__device__ __forceinline__ bool modal_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)
// the pair idx of stage `stage` of the round-robin over np (even) players; stage in [0, np - 1), idx in [0, np / 2)
__device__ __forceinline__ void modal_pair(int np, int stage, int idx, int &p, int &q) {
    const int r = np - 1;
    if (idx == 0) { p = stage; q = r; }
    else { p = stage + idx; p -= p >= r ? r : 0; q = stage - idx + r; q -= q >= r ? r : 0; }      // (both mod r)
    if (p > q) { const int t = p; p = q; q = t; }
}
// the rotation that annihilates a_pq: (c, s) with a'_pj = c a_pj - s a_qj, a'_qj = s a_pj + c a_qj
__device__ __forceinline__ bool modal_rotation(double app, double aqq, double apq, double &c, double &s) {
    c = 1.0; s = 0.0;
    if (fabs(apq) <= kModalRotTol * sqrt(fabs(app) * fabs(aqq))) return false;      // (a_pq = 0 included)
    const double th = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, th) / (fabs(th) + sqrt(fma(th, th, 1.0)));
    c = 1.0 / sqrt(fma(t, t, 1.0));
    s = t * c;
    return true;
}
template <class Sync>
__device__ __forceinline__ bool modal_geneig(int n, const ModalWork &w, int tid, int nt, Sync sync) {
    double *A = w.A, *M = w.M, *Q = w.Q;
    const int ld = kModalLd;
    // the scaling
    for (int i = tid; i < n; i += nt) { const double d = M[i * ld + i]; w.ds[i] = 1.0 / sqrt(d); }
    if (tid == 0) w.ok[0] = 1;
    sync();
    bool ok = true;
    for (int i = 0; i < n; ++i) { const double d = M[i * ld + i]; ok = ok && d > 0.0 && modal_finite(d) && modal_finite(w.ds[i]); }
    if (!ok) return false;
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        M[i * ld + j] = (M[i * ld + j] * w.ds[i]) * w.ds[j];
        A[i * ld + j] = (A[i * ld + j] * w.ds[i]) * w.ds[j];
        Q[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    sync();
    // Cholesky of M, right-looking: column j divided by its pivot, then the trailing lower triangle updated
    for (int j = 0; j < n; ++j) {
        const double d = M[j * ld + j];      // (every thread reads the same pivot: the verdict is uniform)
        if (!(d >= kModalPivot) || !modal_finite(d)) return false;
        const double l = sqrt(d);
        for (int i = j + tid; i < n; i += nt) {
            if (i == j) w.dl[j] = l;
            else M[i * ld + j] = M[i * ld + j] / l;
        }
        sync();
        const int r = n - 1 - j;
        for (int e = tid; e < r * r; e += nt) {
            const int i = j + 1 + e / r, k = j + 1 + e % r;
            if (k <= i) M[i * ld + k] = fma(-M[i * ld + j], M[k * ld + j], M[i * ld + k]);
        }
        sync();
    }
    // Y = L^-1 A (a column per item), H = Y L^-T (a row per item)
    for (int c = tid; c < n; c += nt)
        for (int i = 0; i < n; ++i) {
            double s = A[i * ld + c];
            for (int k = 0; k < i; ++k) s = fma(-M[i * ld + k], A[k * ld + c], s);
            A[i * ld + c] = s / w.dl[i];
        }
    sync();
    for (int r = tid; r < n; r += nt)
        for (int i = 0; i < n; ++i) {
            double s = A[r * ld + i];
            for (int k = 0; k < i; ++k) s = fma(-M[i * ld + k], A[r * ld + k], s);
            A[r * ld + i] = s / w.dl[i];
        }
    sync();
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        if (i < j) { const double h = 0.5 * (A[i * ld + j] + A[j * ld + i]); A[i * ld + j] = h; A[j * ld + i] = h; }
    }
    sync();
    // parallel cyclic Jacobi
    const int np = (n + 1) & ~1, hp = np / 2;
    for (int sweep = 0; sweep < kModalSweeps; ++sweep) {
        if (tid == 0) w.ok[1] = 0;
        sync();
        for (int stage = 0; stage < np - 1; ++stage) {
            for (int idx = tid; idx < hp; idx += nt) {
                int p, q;
                modal_pair(np, stage, idx, p, q);
                double c = 1.0, s = 0.0;
                if (q < n && modal_rotation(A[p * ld + p], A[q * ld + q], A[p * ld + q], c, s)) w.ok[1] = 1;      // (every writer stores 1)
                w.cs[2 * idx] = c; w.cs[2 * idx + 1] = s;
            }
            sync();
            for (int e = tid; e < hp * n; e += nt) {      // rows
                const int idx = e / n, j = e - idx * n;
                int p, q;
                modal_pair(np, stage, idx, p, q);
                if (q >= n) continue;
                const double c = w.cs[2 * idx], s = w.cs[2 * idx + 1], x = A[p * ld + j], y = A[q * ld + j];
                A[p * ld + j] = fma(c, x, -(s * y));
                A[q * ld + j] = fma(s, x, c * y);
            }
            sync();
            for (int e = tid; e < hp * n; e += nt) {      // columns, and the accumulated rotations
                const int idx = e / n, i = e - idx * n;
                int p, q;
                modal_pair(np, stage, idx, p, q);
                if (q >= n) continue;
                const double c = w.cs[2 * idx], s = w.cs[2 * idx + 1];
                double x = A[i * ld + p], y = A[i * ld + q];
                A[i * ld + p] = fma(c, x, -(s * y));
                A[i * ld + q] = fma(s, x, c * y);
                x = Q[i * ld + p]; y = Q[i * ld + q];
                Q[i * ld + p] = fma(c, x, -(s * y));
                Q[i * ld + q] = fma(s, x, c * y);
            }
            sync();
        }
        const int rotated = w.ok[1];      // (read behind the stage's last barrier: uniform; the barrier below: before the next sweep clears it)
        sync();
        if (!rotated) break;
    }
    // ascending order (ties by index)
    for (int i = tid; i < n; i += nt) w.ev[i] = A[i * ld + i];
    sync();
    for (int i = tid; i < n; i += nt) {
        const double d = w.ev[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double o = w.ev[j]; rank += (o < d || (o == d && j < i)) ? 1 : 0; }
        w.perm[rank] = i;
        if (!modal_finite(d)) w.ok[0] = 0;      // (a NaN ranks 0 in every item: the verdict below ends the call)
    }
    sync();
    if (!w.ok[0]) return false;
    // C = D L^-T Q[:, perm] into A (H is no longer needed; an item writes its own column and reads Q, L, ds, dl)
    for (int r = tid; r < n; r += nt) {
        const int src = w.perm[r];
        bool fin = true;
        for (int i = n - 1; i >= 0; --i) {
            double s = Q[i * ld + src];
            for (int k = i + 1; k < n; ++k) s = fma(-M[k * ld + i], A[k * ld + r], s);
            A[i * ld + r] = s / w.dl[i];
        }
        for (int i = 0; i < n; ++i) { A[i * ld + r] *= w.ds[i]; fin = fin && modal_finite(A[i * ld + r]); }
        if (!fin) w.ok[0] = 0;
    }
    sync();
    return w.ok[0] != 0;
}
// The Rayleigh-Ritz of an iteration with its restart rule.  GA, GM [3 nb][3 nb] row-major (the upper triangle is read) for S = [X W P];
// m = 3 nb with P, else 2 nb.  A failure on 3 nb columns is a RESTART: the leading 2 nb block ([X W], P dropped) is tried, *restarted = 1.
// Returns the number of columns used (0: failure on [X W] as well); th [nb] ascending, Cout [3 nb][nb] row-major (rows >= the columns
// used are zero), both zero on failure.
template <class Sync>
__device__ __forceinline__ int modal_rr(int nb, int m, const double *GA, const double *GM, const ModalWork &w, double *th, double *Cout,
                                        int *restarted, int tid, int nt, Sync sync) {
    const int m3 = 3 * nb, ld = kModalLd;
    int used = 0;
    if (tid == 0) *restarted = 0;
    for (int attempt = 0; attempt < 2 && !used; ++attempt) {
        const int n = attempt == 0 ? m : 2 * nb;
        if (attempt == 1 && (m <= 2 * nb)) break;
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, j = e - i * n, lo = i < j ? i : j, hi = i < j ? j : i;
            w.A[i * ld + j] = GA[lo * m3 + hi];
            w.M[i * ld + j] = GM[lo * m3 + hi];
        }
        sync();
        if (modal_geneig(n, w, tid, nt, sync)) used = n;
        else if (attempt == 0 && m > 2 * nb && tid == 0) *restarted = 1;
        sync();
    }
    for (int e = tid; e < m3 * nb; e += nt) {
        const int i = e / nb, j = e - i * nb;
        Cout[e] = i < used ? w.A[i * ld + j] : 0.0;
    }
    for (int j = tid; j < nb; j += nt) th[j] = used ? w.ev[w.perm[j]] : 0.0;
    sync();
    return used;
}
// the default start block of the eigensolver: a fixed integer hash of (column, vertex, axis) mapped to (-1, 1)
__device__ __forceinline__ double modal_start(unsigned col, unsigned vertex, unsigned axis) {
    unsigned h = col * 0x9E3779B1u + vertex * 0x85EBCA77u + axis * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return ((double)h + 0.5) * 4.656612873077393e-10 - 1.0;      // (h + 1/2) 2^-31 - 1: exact in FP64
}

// ---- the dense inverse of the two-level tangent preconditioner (tangent_precond.hpp: k_tc_invert) ----
// X = A^-1 for a symmetric A [n][n] (row-major; destroyed), by Cholesky of the diagonally scaled matrix (right-looking, as modal_geneig)
// and the two triangular solves against the identity; X is symmetrised at the end, so applying it is a symmetric operator to the bit.
// ONE text for the device and the host, cut into phases as modal_geneig is (tid, nt, sync).  The three sweeps are ROW-ORIENTED: step k
// finishes row k and then takes its share out of the other rows, (rows) x (columns) independent items between two barriers -- the
// threads form a grid of nt / 64 row groups by 64 columns, so a wave walks a row with unit stride and the loads of an item do not wait
// for the item before (a column per thread, the first form, was one dependent chain of n^2 loads per thread: 229 ms at n = 768).  Every
// entry sees the same operations in the same order whatever nt is.
//   DROPPED columns: |a_ii| <= kTcDrop max_k a_kk.  Row and column i of X are zero, the rest of X is the inverse of the rest of A.
//          Counted in *dropped.  (An aggregate whose vertices are all held; a flat cloth, where one affine function vanishes.)
//   VERDICT 0, X all zero: a diagonal that is not finite or below -kTcDrop max_k a_kk; a pivot of the scaled matrix (unit diagonal) that
//          is not finite or below 16 n eps -- the rounding of a pivot is up to n eps, a pivot of that size carries no digit: this is how
//          a singular A ends, P containing a null space of the operator or dependent columns --; a non-finite entry of X.
// Work: ds, dl, col [n], keep [n], flag [1].
constexpr double kTcDrop = 9.094947017729282e-13;      // 2^-40
template <class Sync>
__device__ __forceinline__ int tc_invert(int n, double *A, double *X, double *ds, double *dl, double *col, int *keep, int *flag, int *dropped,
                                         int tid, int nt, Sync sync) {
    const size_t ld = (size_t)n;
    const int W = nt >= 64 ? 64 : 1, tx = tid % W, ty = tid / W, ny = nt / W;      // (threads beyond ny W take no item of the sweeps)
    bool ok = true;
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) { const double d = A[i * ld + i]; ok = ok && modal_finite(d); dmax = d > dmax ? d : dmax; }      // (every thread: uniform)
    const double thr = kTcDrop * dmax;
    int nd = 0;
    for (int i = 0; i < n; ++i) { const double d = A[i * ld + i]; nd += d <= thr ? 1 : 0; ok = ok && d >= -thr; }
    if (tid == 0) { *dropped = nd; *flag = 1; }
    for (int i = tid; i < n; i += nt) { const double d = A[i * ld + i]; keep[i] = d > thr ? 1 : 0; ds[i] = d > thr ? 1.0 / sqrt(d) : 0.0; }
    sync();
    if (ok) {
        for (size_t e = (size_t)tid; e < ld * ld; e += (size_t)nt) {
            const int i = (int)(e / ld), j = (int)(e - i * ld);
            A[e] = keep[i] && keep[j] ? (A[e] * ds[i]) * ds[j] : (i == j ? 1.0 : 0.0);      // (a dropped column: the identity's, so the factorisation runs through)
            X[e] = i == j ? 1.0 : 0.0;
        }
        sync();
        const double pivot_min = 16.0 * n * 2.220446049250313e-16;
        for (int j = 0; j < n; ++j) {
            const double d = A[j * ld + j];      // (no item of this step writes a pivot: every thread reads the same one)
            if (!(d >= pivot_min) || !modal_finite(d)) { ok = false; break; }
            const double l = sqrt(d);
            for (int i = j + tid; i < n; i += nt) {
                if (i == j) dl[j] = l;
                else { const double v = A[i * ld + j] / l; A[i * ld + j] = v; col[i] = v; }      // (col: column j of L with unit stride)
            }
            sync();
            for (int i = j + 1 + ty; i < n && ty < ny; i += ny) {      // the trailing lower triangle
                const double lij = col[i];
                for (int k = j + 1 + tx; k <= i; k += W) A[i * ld + k] = fma(-lij, col[k], A[i * ld + k]);
            }
            sync();
        }
    }
    if (ok) {
        // L Y = I in place in X (Y is lower triangular: row k ends at column k)
        for (int k = 0; k < n; ++k) {
            for (int c = tid; c <= k; c += nt) X[k * ld + c] = X[k * ld + c] / dl[k];
            sync();
            for (int i = k + 1 + ty; i < n && ty < ny; i += ny) {
                const double lik = A[i * ld + k];
                for (int c = tx; c <= k; c += W) X[i * ld + c] = fma(-lik, X[k * ld + c], X[i * ld + c]);
            }
            sync();
        }
        // L^T X = Y in place
        for (int k = n - 1; k >= 0; --k) {
            for (int c = tid; c < n; c += nt) X[k * ld + c] = X[k * ld + c] / dl[k];
            sync();
            for (int i = ty; i < k && ty < ny; i += ny) {
                const double lki = A[k * ld + i];
                for (int c = tx; c < n; c += W) X[i * ld + c] = fma(-lki, X[k * ld + c], X[i * ld + c]);
            }
            sync();
        }
        for (size_t e = (size_t)tid; e < ld * ld; e += (size_t)nt) {
            const int i = (int)(e / ld), j = (int)(e - i * ld);
            if (i > j) continue;
            const double h = keep[i] && keep[j] ? (0.5 * (X[i * ld + j] + X[j * ld + i]) * ds[i]) * ds[j] : 0.0;
            if (!modal_finite(h)) *flag = 0;      // (every writer stores 0)
            X[i * ld + j] = h; X[j * ld + i] = h;
        }
        sync();
        ok = *flag != 0;
        sync();
    }
    if (!ok) {
        for (size_t e = (size_t)tid; e < ld * ld; e += (size_t)nt) X[e] = 0.0;
        if (tid == 0) *flag = 0;
        sync();
    }
    return ok ? 1 : 0;
}

} // namespace admm_dev
