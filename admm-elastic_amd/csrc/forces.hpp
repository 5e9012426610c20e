// forces.hpp -- internal forces f = -dE/dx of all energy terms, per-tet stress and the stationarity residual of a step, on the device
// (included once by admm_hip.hip).
//
// E is exactly what admm_hip_energy sums (monitor.hpp): the same sign rules for the tets, triangles without their strain limits, hinges,
// no energy for pins.  The reference leaves the gradient a TODO (TetEnergyTerm::gradient and TriEnergyTerm::gradient throw,
// HyperElasticTet::gradient exists in stretch space only), so like the energies of the f3 terms this has no reference code: it is pinned on
// the energies (tests/test_forces.py: the numpy forces are the gradient of the numpy energies, the device forces equal the numpy forces).
//
// k_forces walks the families in block ranges like k_monitor and reads the elements through elements.hpp:
//   tets      one block per 256-tet CHUNK of the local step's plan (host_setup.hpp: TetChunks), lane = tet.  F = D_i x = U diag(sigma) V^T
//             (signed_svd3), P = U diag(s_i g_i) V^T with s_i g_i from the kind's own eval (device_math.hpp: tet_energy_grad -- the
//             dispatch the energy uses, so the two cannot differ); corner forces H = -vol P Binv^T.  No density is restated here.
//   triangles lane = triangle: E = w^2 / 2 sum (sigma_i - 1)^2 of the 3x2 F, P = w^2 (F - R), R = F (F^T F)^(-1/2) the closest isometry
//             (closed-form 2x2 inverse square root), corner forces through `rest`.
//   hinges    f_{v_k} = -stiffness c_k (D_i x).
// How the corner forces leave k_forces and reach a vertex in k_gather_forces (lane = vertex): the write side of elements.hpp, gather_vertex.
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
    ElemView v;               // the scene at x
    int cb[6];                // the model groups' first chunks (v.kb: their first tets)
    ChunkPlan plan; double *rec;      // the local step's chunk plan; records [n_rec + 1][4]
    double *stress;           // [kStressQ][ldt] in device order, or nullptr
    double *r_cf;             // corner forces of the triangles [9 of 12][ldr]
    double *h_cf;             // of the hinges [12][ldb]
    int nb_t, nb_r;           // block ranges: [0, nb_t) tet chunks, [nb_t, nb_r) triangles, then hinges
    const int *stop;          // the stop word of the ADMM loop (kernels.hpp: kCntAdmmStop) or nullptr: set, the launch is a no-op
};

// One chunk of tets; the whole block takes part (elements.hpp: chunk_locate).
__device__ __forceinline__ void force_tets(const ForceArgs &a, int chunk, LdsDk *sL) {
    const ElemView &v = a.v;
    const int tid = (int)threadIdx.x;
    const ChunkLane ln = chunk_locate(v.kb, a.cb, chunk, tid);
    const int t = ln.t;
    LdsDk *sBi = sL + tid;                                   // row c of this thread: [c * kChunkLdK]
    // the reduction list of this thread's record (first pass) and the tet's scalars: in flight across the SVD
    const ChunkOut co = chunk_out_begin(a.plan, chunk, sL);
    const double w2 = v.t_sc[t] / v.dt2;
    const Mat mt = v.mats[v.t_mat[t]];
    double U[9], S[3], V[9], F[9];
    {
        double Bi[9];
        tet_F_binv(v, v.t_idx[t], t, F, Bi);
        // Binv is needed again for the corner forces: parked in this thread's LDS column across the SVD
#pragma unroll
        for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];
    }
    signed_svd3(F, U, S, V);
    double sg[3];
    (void)tet_energy_grad(ln.grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, v.spl + (size_t)(ln.grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles, S, sg);
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
    if (a.stress) {
        double P[9];
        usvt(U, sg, V, P);
        const double J = S[0] * S[1] * S[2];
        const double tau[3] = {sg[0] * S[0] / J, sg[1] * S[1] / J, sg[2] * S[2] / J};      // Cauchy = P F^T / J = U diag(tau) U^T
        const double d0 = tau[0] - tau[1], d1 = tau[1] - tau[2], d2 = tau[2] - tau[0];
        if (ln.valid) {
#pragma unroll
            for (int c = 0; c < 9; ++c) a.stress[(size_t)c * v.ldt + t] = P[c];
#pragma unroll
            for (int i = 0; i < 3; ++i) a.stress[(size_t)(9 + i) * v.ldt + t] = S[i];
            a.stress[(size_t)12 * v.ldt + t] = sqrt(0.5 * (d0 * d0 + d1 * d1 + d2 * d2));
        }
    }
    double G[9], f[12];
    {
        const double dg[3] = {-vol * sg[0], -vol * sg[1], -vol * sg[2]};
        usvt(U, dg, V, G);
    }
    tet_corner_forces(G, sBi, f);
    chunk_out_store(co, sL, f, a.rec);
}

__global__ __launch_bounds__(256) void k_forces(ForceArgs a) {
    __shared__ double sLm[12 * kChunkLdK];      // rows 0..8: Binv across the SVD; rows 0..11: the chunk's corner forces
    if (a.stop && *a.stop) return;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        force_tets(a, blk, (LdsDk *)sLm);
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        double R[4], F[6];
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        tri_F(R, v.r_idx[t], v.x, F);
        const double w2 = v.r_sc[t] / v.dt2;
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
            tri_corner_store(-w2 * (F[j] - q0), -w2 * (F[3 + j] - q1), R, a.r_cf + (size_t)j * v.ldr, v.ldr, t);      // G = -P
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= v.nbend) return;
        int vid[4];
        double c[4], Dx[3], ks;
        hinge_load(v, t, c, vid, ks);
        hinge_Dx(c, vid, v.x, Dx);
        hinge_corner_store(c, -ks, Dx, a.h_cf, v.ldb, t);
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
// The head of every vertex gather: lane `lane` of slice s adds to acc [3] what is incident to its vertex in direction dir of a.t_rec,
// a.r_cf, a.h_cf (st: the doubles between two directions), in list order, and returns the vertex (a.nv past the end).
__device__ __forceinline__ int gather_vertex(const ForceGatherArgs &a, int s, int lane, double *acc, size_t dir = 0, const DirStrides &st = DirStrides{}) {
    const int r = s * 64 + lane;
    const int v = r < a.nv ? a.order[r] : a.nv;
    if (a.t_inc) gather_records(a.t_inc + a.t_ptr[s] + lane, a.t_w[s], a.t_rec + dir * st.rec, acc);
    if (a.r_inc) gather_corners<false>(a.r_inc + a.r_ptr[s] + lane, a.r_w[s], a.r_cf + dir * st.rcf, a.r_ld, acc);
    if (a.h_inc) gather_corners<false>(a.h_inc + a.h_ptr[s] + lane, a.h_w[s], a.h_cf + dir * st.hcf, a.h_ld, acc);
    return v;
}
__global__ __launch_bounds__(256) void k_gather_forces(ForceGatherArgs a) {
    if (a.stop && *a.stop) return;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    if (s >= a.n_slices) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int v = gather_vertex(a, s, lane, acc);
    if (v < a.nv) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.f[3 * (size_t)v + j] = acc[j];
    }
}

// STATIONARITY of implicit Euler: sum of r_i^2 over the degrees of freedom of every vertex without an active pin,
//   r = (m o x - M x_bar) / dt^2 - f      (the optimality condition M (x - x_bar) / dt^2 + grad E(x) = 0 of src/Solver.cpp:57-106)
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
        if (!vertex_held(v, vert_pin, pin_active, pin_flag)) {
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
