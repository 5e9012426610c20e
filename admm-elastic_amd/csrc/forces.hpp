// forces.hpp -- internal forces f = -dE/dx of all energy terms, per-tet stress and the stationarity residual of a step, on the device
// (included once by admm_hip.hip).
//
// E is exactly what admm_hip_energy sums (monitor.hpp): the same sign rules for the tets, triangles without their strain limits, hinges,
// no energy for pins.  The reference leaves the gradient a TODO (TetEnergyTerm::gradient and TriEnergyTerm::gradient throw,
// HyperElasticTet::gradient exists in stretch space only), so like the energies of the f3 terms this has no reference code: it is pinned on
// the energies (tests/test_forces.py: the numpy forces are the gradient of the numpy energies, the device forces equal the numpy forces).
//
// k_forces walks the families in block ranges like k_monitor:
//   tets      one block per 256-tet CHUNK of the local step's plan (host_setup.hpp: TetChunks; chunks are numbered model by model and do
//             not straddle a model boundary), lane = tet.  F = D_i x = U diag(sigma) V^T (signed_svd3), g = dpsi/da from the kind's own
//             eval with the prox quadratic off (k = 0), a = |sigma| for the kinds whose energy is evaluated there (linear, Neo-Hookean,
//             every SplineTet) and a = sigma for StVK and stable Neo-Hookean; P = U diag(s_i g_i) V^T with s_i = sign(sigma_i) resp. 1;
//             corner forces H = -vol P Binv^T (corner m + 1: column m, corner 0: minus their sum), reduced per chunk into 32-byte records
//             exactly as tet_compute_store does.  No density is restated here.
//   triangles lane = triangle: E = w^2 / 2 sum (sigma_i - 1)^2 of the 3x2 F, P = w^2 (F - R), R = F (F^T F)^(-1/2) the closest isometry
//             (closed-form 2x2 inverse square root), corner forces through `rest` as k_local_tris forms them.
//   hinges    f_{v_k} = -stiffness c_k (D_i x).
// k_gather_forces (lane = vertex) sums records and corner forces through the incidence lists of k_gather_rhs, in list order.
//
// Limits.  At a stretch sigma_i = 0 the |sigma| kinds have a kink: the force there is a one-sided derivative (sign(0) counts as +).  The
// stress divides by J = sigma_1 sigma_2 sigma_3 and a triangle's R by sigma_1 sigma_2: at J -> 0 (a flat tet, a collapsed triangle) the
// outputs are what the arithmetic gives (inf / NaN), nothing is clamped.  The tangent of these forces (tangent.hpp) has the same limits:
// a kink at sigma_i = 0 of the |sigma| kinds, the log barrier of the Neo-Hookean kinds at J -> 0, a collapsed triangle.
//
// REPRODUCIBLE to the bit: fixed summation orders everywhere, ordinary vector stores, no floating-point atomics.
#pragma once
#include "monitor.hpp"

namespace admm_k {

constexpr int kStressQ = 13;      // per tet: P column-major (9), the signed stretches (3), von Mises of the Cauchy stress (1)

struct ForceArgs {
    const double *x;          // [nv][3]
    double dt2;               // sc = dt^2 w^2  ->  w^2 = sc / dt2
    // tets in device order (sorted by model group); kb = the groups' first tets, cb = their first chunks
    int nt, ldt; const int4 *t_idx; const double *t_Binv, *t_x0, *t_sc; const int *t_mat; const Mat *mats; const double *spl;
    int kb[6], cb[6];
    const unsigned short *ch_ent; const int *ch_group, *ch_rec; double *rec;      // the local step's chunk plan; records [n_rec + 1][4]
    double *stress;           // [kStressQ][ldt] in device order, or nullptr
    int ntri, ldr; const int4 *r_idx; const double *r_rest, *r_sc; double *r_cf;   // corner forces [9 of 12][ldr]
    int nbend, ldb; const int4 *h_idx; const double *h_coef, *h_k; double *h_cf;   // [12][ldb]
    int nb_t, nb_r;           // block ranges: [0, nb_t) tet chunks, [nb_t, nb_r) triangles, then hinges
    const int *stop;          // the stop word of the ADMM loop (kernels.hpp: kCntAdmmStop) or nullptr: set, the launch is a no-op
};

// psi's gradient g[i] = dpsi/da_i of tet t's model at the stretches S, a = |S| or S as its energy takes them (mon_tet_energy), and
// sg[i] = s_i g_i, the diagonal of P in the frame of the SVD
__device__ __forceinline__ void force_tet_grad(const Mat mt, int grp, const double *spl, const double *S, double *sg) {
    const double A[3] = {fabs(S[0]), fabs(S[1]), fabs(S[2])};
    double g[3], D[3], w[3], H[6];
    bool use_abs = true;
    if (grp == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = mt.k * (A[i] - 1.0);
    } else if (grp == 1) {
        StretchModel<1, double> m; m.mu = mt.mu; m.la = mt.la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        (void)m.eval(A, g, D, w);
    } else if (grp == 2) {
        StretchModel<2, double> m; m.mu = mt.mu; m.la = mt.la; m.k = 0.0; m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
        (void)m.eval(S, g, D, w);
        use_abs = false;
    } else if (grp == 3) {
        StretchModel<3, double> m; m.mu = mt.mu; m.la = mt.la; m.k = 0.0; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        (void)m.eval(A, g, D, w);
    } else if (mt.type == 3) {
        SplineTableModel m; m.type = 1; m.tab = spl + (size_t)mt.table * kSplineTableDoubles; m.mu = 0.0; m.la = 0.0; m.k = 0.0; m.lo = 0.0;
        m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        (void)m.eval(A, g, H);
    } else if (mt.type == 4) {
        StableNHModel m; m.type = 0; m.mu = (4.0 / 3.0) * mt.mu; m.la = mt.la + (5.0 / 6.0) * mt.mu; m.k = 0.0; m.alpha = 1.0 + 0.75 * m.mu / m.la;
        m.x0[0] = S[0]; m.x0[1] = S[1]; m.x0[2] = S[2];
        (void)m.eval(S, g, H);
        use_abs = false;
    } else {
        SplineKappaModel m; m.type = mt.type; m.mu = mt.mu; m.la = mt.la; m.k = 0.0; m.kappa = mt.kappa; m.x0[0] = A[0]; m.x0[1] = A[1]; m.x0[2] = A[2];
        (void)m.eval(A, g, H);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sg[i] = (use_abs && S[i] < 0.0) ? -g[i] : g[i];
}

// One chunk of tets.  The whole block takes part (signed_svd3 takes wave votes, the chunk's reduction synchronises the block): lanes
// past the end of the model's range redo its last tet and park values no list refers to.
__device__ __forceinline__ void force_tets(const ForceArgs &a, int chunk, LdsDk *sL) {
    const int tid = (int)threadIdx.x;
    const int grp = (chunk >= a.cb[1]) + (chunk >= a.cb[2]) + (chunk >= a.cb[3]) + (chunk >= a.cb[4]);
    const int c0 = grp == 0 ? a.cb[0] : grp == 1 ? a.cb[1] : grp == 2 ? a.cb[2] : grp == 3 ? a.cb[3] : a.cb[4];
    const int tb = grp == 0 ? a.kb[0] : grp == 1 ? a.kb[1] : grp == 2 ? a.kb[2] : grp == 3 ? a.kb[3] : a.kb[4];
    const int t_end = grp == 0 ? a.kb[1] : grp == 1 ? a.kb[2] : grp == 2 ? a.kb[3] : grp == 3 ? a.kb[4] : a.kb[5];
    const int t0 = tb + (chunk - c0) * 256 + tid;
    const bool valid = t0 < t_end;
    const int t = valid ? t0 : t_end - 1;
    LdsDk *sBi = sL + tid;                                   // row c of this thread: [c * kChunkLdK]
    if (tid < 3) sL[tid * kChunkLdK + 256] = 0.0;            // the padding column of the reduction lists
    // the reduction list of this thread's record (first pass) and the tet's scalars: in flight across the SVD
    const int g0 = __builtin_amdgcn_readfirstlane(a.ch_group[chunk]), g1 = __builtin_amdgcn_readfirstlane(a.ch_group[chunk + 1]);
    const int r0 = __builtin_amdgcn_readfirstlane(a.ch_rec[chunk]), nrec = __builtin_amdgcn_readfirstlane(a.ch_rec[chunk + 1]) - r0;
    const __amdgpu_buffer_rsrc_t re = soa_rsrc(a.ch_ent);
    union { bv4u v; unsigned short h[8]; } e;
    e.v = __builtin_amdgcn_raw_buffer_load_b128(re, (g0 * 256 + tid) * 16, 0, kStreamLdAux);
    const double w2 = a.t_sc[t] / a.dt2;
    const Mat mt = a.mats[a.t_mat[t]];
    double U[9], S[3], V[9], F[9];
    {
        const int4 id = a.t_idx[t];
        const int vid[4] = {id.x, id.y, id.z, id.w};
        double Bi[9];
        if (a.t_x0) {      // Binv from the rest positions, as the local step recomputes it (kernels.hpp: tet_rest_binv)
            double p[12];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int j = 0; j < 3; ++j) p[3 * v + j] = a.t_x0[3 * (size_t)vid[v] + j];
            double e0[3], e1[3], e2[3], q0[3], q1[3], q2[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { e0[j] = p[3 + j] - p[j]; e1[j] = p[6 + j] - p[j]; e2[j] = p[9 + j] - p[j]; }
            cross3(e1, e2, q0); cross3(e2, e0, q1); cross3(e0, e1, q2);
            const double idet = fast_rcp(fma(e0[0], q0[0], fma(e0[1], q0[1], e0[2] * q0[2])));
#pragma unroll
            for (int r = 0; r < 3; ++r) { Bi[r * 3 + 0] = q0[r] * idet; Bi[r * 3 + 1] = q1[r] * idet; Bi[r * 3 + 2] = q2[r] * idet; }
        } else {
#pragma unroll
            for (int c = 0; c < 9; ++c) Bi[c] = a.t_Binv[(size_t)c * a.ldt + t];
        }
        double x[12], Ds[9];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 3; ++j) x[3 * v + j] = a.x[3 * (size_t)vid[v] + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) { Ds[j] = x[3 + j] - x[j]; Ds[3 + j] = x[6 + j] - x[j]; Ds[6 + j] = x[9 + j] - x[j]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j) F[r * 3 + j] = fma(Ds[j], Bi[r * 3 + 0], fma(Ds[3 + j], Bi[r * 3 + 1], Ds[6 + j] * Bi[r * 3 + 2]));
        // Binv is needed again for the corner forces: parked in this thread's LDS column across the SVD, as the local step does
#pragma unroll
        for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];
    }
    signed_svd3(F, U, S, V);
    double sg[3];
    force_tet_grad(mt, grp, a.spl, S, sg);
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
    if (a.stress) {
        double P[9];
        usvt(U, sg, V, P);
        const double J = S[0] * S[1] * S[2];
        const double tau[3] = {sg[0] * S[0] / J, sg[1] * S[1] / J, sg[2] * S[2] / J};      // Cauchy = P F^T / J = U diag(tau) U^T
        const double d0 = tau[0] - tau[1], d1 = tau[1] - tau[2], d2 = tau[2] - tau[0];
        if (valid) {
#pragma unroll
            for (int c = 0; c < 9; ++c) a.stress[(size_t)c * a.ldt + t] = P[c];
#pragma unroll
            for (int i = 0; i < 3; ++i) a.stress[(size_t)(9 + i) * a.ldt + t] = S[i];
            a.stress[(size_t)12 * a.ldt + t] = sqrt(0.5 * (d0 * d0 + d1 * d1 + d2 * d2));
        }
    }
    double G[9];
    {
        const double dg[3] = {-vol * sg[0], -vol * sg[1], -vol * sg[2]};
        usvt(U, dg, V, G);
    }
    // corner forces: H(j,m) = sum_r G(j,r) Binv(m,r); corner m+1 gets H(:,m), corner 0 gets -sum_m H(:,m)  (as tet_compute_store)
    double f[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double b0 = sBi[(0 + m) * kChunkLdK], b1 = sBi[(3 + m) * kChunkLdK], b2 = sBi[(6 + m) * kChunkLdK];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double h = fma(G[j], b0, fma(G[3 + j], b1, G[6 + j] * b2));
            f[3 * (m + 1) + j] = h;
            f[j] -= h;
        }
    }
    // the chunk's reduction: thread j of pass p sums the <= 8 corner forces of record 256 p + j and stores it as one 32-byte sector
#pragma unroll
    for (int c = 0; c < 12; ++c) sBi[c * kChunkLdK] = f[c];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rr = soa_rsrc(a.rec);
    for (int g = g0; g < g1; ++g) {
        if (g > g0) e.v = __builtin_amdgcn_raw_buffer_load_b128(re, (g * 256 + tid) * 16, 0, kStreamLdAux);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < kChunkFanK; ++i) {
            const LdsDk *q = (const LdsDk *)((const __attribute__((address_space(3))) char *)sL + e.h[i]);
            s0 += q[0]; s1 += q[kChunkLdK]; s2 += q[2 * kChunkLdK];
        }
        const int j = (g - g0) * 256 + tid;
        if (j < nrec) {
            union { double d[2]; bv4u v; } p0; p0.d[0] = s0; p0.d[1] = s1;
            union { double d; bv2u v; } p1; p1.d = s2;
            __builtin_amdgcn_raw_buffer_store_b128(p0.v, rr, (r0 + j) * 32, 0, kStreamStAux);
            __builtin_amdgcn_raw_buffer_store_b64(p1.v, rr, (r0 + j) * 32 + 16, 0, kStreamStAux);
        }
    }
}

__global__ __launch_bounds__(256) void k_forces(ForceArgs a) {
    __shared__ double sLm[12 * kChunkLdK];      // rows 0..8: Binv across the SVD; rows 0..11: the chunk's corner forces
    if (a.stop && *a.stop) return;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        force_tets(a, blk, (LdsDk *)sLm);
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= a.ntri) return;
        const int4 id = a.r_idx[t];
        double R[4], F[6];
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = a.r_rest[(size_t)c * a.ldr + t];
        const double *p0 = a.x + 3 * (size_t)id.x, *p1 = a.x + 3 * (size_t)id.y, *p2 = a.x + 3 * (size_t)id.z;
#pragma unroll
        for (int j = 0; j < 3; ++j) {      // F (3x2) = [x1 - x0, x2 - x0] rest, as k_local_tris
            const double b = p0[j], e1 = p1[j] - b, e2 = p2[j] - b;
            F[j] = fma(e1, R[0], e2 * R[1]);
            F[3 + j] = fma(e1, R[2], e2 * R[3]);
        }
        const double w2 = a.r_sc[t] / a.dt2;
        // C = F^T F; sqrt(C) = (C + s I) / q with s = sqrt(det C) = sigma_1 sigma_2, q = sqrt(tr C + 2 s) = sigma_1 + sigma_2;
        // C^(-1/2) = adj(C + s I) / (q s); the closest isometry Q = F C^(-1/2)
        const double c00 = dot3(F, F), c01 = dot3(F, F + 3), c11 = dot3(F + 3, F + 3);
        double cr[3];
        cross3(F, F + 3, cr);
        const double s = sqrt(dot3(cr, cr)), q = sqrt(c00 + c11 + 2.0 * s), iq = 1.0 / (q * s);
        const double i00 = (c11 + s) * iq, i01 = -c01 * iq, i11 = (c00 + s) * iq;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double q0 = fma(F[j], i00, F[3 + j] * i01), q1 = fma(F[j], i01, F[3 + j] * i11);
            const double G0 = -w2 * (F[j] - q0), G1 = -w2 * (F[3 + j] - q1);      // G = -P
            const double h1 = fma(G0, R[0], G1 * R[2]);
            const double h2 = fma(G0, R[1], G1 * R[3]);
            a.r_cf[(size_t)(0 + j) * a.ldr + t] = -(h1 + h2);
            a.r_cf[(size_t)(3 + j) * a.ldr + t] = h1;
            a.r_cf[(size_t)(6 + j) * a.ldr + t] = h2;
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= a.nbend) return;
        const int4 id = a.h_idx[t];
        const int vid[4] = {id.x, id.y, id.z, id.w};
        double c[4], Dx[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {      // D_i x = sum_k c_k x_{v_k}, as k_local_bends
            c[k] = a.h_coef[(size_t)k * a.ldb + t];
            const double *p = a.x + 3 * (size_t)vid[k];
#pragma unroll
            for (int j = 0; j < 3; ++j) Dx[j] = fma(c[k], p[j], Dx[j]);
        }
        const double ks = -a.h_k[t];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) a.h_cf[(size_t)(3 * k + j) * a.ldb + t] = c[k] * (ks * Dx[j]);
    }
}

// f_v = sum of the records and corner forces incident to vertex v, through the incidence lists of k_gather_rhs in list order
struct ForceGatherArgs {
    int nv, n_slices;
    const int *t_ptr, *t_w, *t_inc; const double *t_rec;
    const int *r_ptr, *r_w, *r_inc; const double *r_cf; int r_ld;
    const int *h_ptr, *h_w, *h_inc; const double *h_cf; int h_ld;
    const int *order;
    double *f;                // [nv][3]
    const int *stop;
};
__global__ __launch_bounds__(256) void k_gather_forces(ForceGatherArgs a) {
    if (a.stop && *a.stop) return;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    if (s >= a.n_slices) return;
    const int r = s * 64 + lane;
    const int v = r < a.nv ? a.order[r] : a.nv;
    double acc[3] = {0.0, 0.0, 0.0};
    if (a.t_inc) gather_records(a.t_inc + a.t_ptr[s] + lane, a.t_w[s], a.t_rec, acc);
    if (a.r_inc) gather_corners<false>(a.r_inc + a.r_ptr[s] + lane, a.r_w[s], a.r_cf, a.r_ld, acc);
    if (a.h_inc) gather_corners<false>(a.h_inc + a.h_ptr[s] + lane, a.h_w[s], a.h_cf, a.h_ld, acc);
    if (v < a.nv) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.f[3 * (size_t)v + j] = acc[j];
    }
}

// STATIONARITY of implicit Euler: sum of r_i^2 over the degrees of freedom of every vertex without an active pin,
//   r = (m o x - M x_bar) / dt^2 - f      (the optimality condition M (x - x_bar) / dt^2 + grad E(x) = 0 of src/Solver.cpp:57-106)
// vert_pin / pin_active: the SpringPin and slide-pin TERMS (linsolver 0 / 2); pin_flag: the pins applied inside the GS sweeps (linsolver 1).
// Block partials by ordinary stores; k_stat_final sums them in index order and stores the sum (not its root).
__global__ __launch_bounds__(256) void k_stationarity(int nv, const double *__restrict__ x, const double *__restrict__ m, const double *__restrict__ Mxbar,
                                                      const double *__restrict__ f, double idt2, const int *__restrict__ vert_pin,
                                                      const int *__restrict__ pin_active, const int *__restrict__ pin_flag, double *__restrict__ part,
                                                      const int *stop) {
    __shared__ double lds[4];
    if (stop && *stop) return;
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[1] = {0.0};
    if (v < nv) {
        bool pinned = false;
        if (vert_pin) { const int pi = vert_pin[v]; pinned = pi >= 0 && pin_active[pi] != 0; }
        if (pin_flag) pinned = pinned || pin_flag[v] != 0;
        if (!pinned) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t i = 3 * (size_t)v + j;
                const double r = fma(m[i], x[i], -Mxbar[i]) * idt2 - f[i];
                q[0] = fma(r, r, q[0]);
            }
        }
    }
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) part[blk] = q[0];
}
__global__ __launch_bounds__(256) void k_stat_final(const double *__restrict__ part, int nb, double *__restrict__ out, const int *stop) {
    __shared__ double lds[4];
    if (stop && *stop) return;
    double q[1] = {0.0};
    for (int b = (int)threadIdx.x; b < nb; b += 256) q[0] += part[b];
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) out[0] = q[0];
}

} // namespace admm_k
