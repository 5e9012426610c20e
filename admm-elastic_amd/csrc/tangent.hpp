// tangent.hpp -- the tangent stiffness K(x) = d2E/dx2 = -df/dx of all energy terms applied to n_vec directions, on the device
// (included once by admm_hip.hip, after forces.hpp).
//
// E is the energy admm_hip_energy sums and admm_hip_forces differentiates: out_j = K(x) d_j + shift (m o d_j).  Like the forces this has
// no reference code; it is pinned on them (tests/test_stiffness.py: the numpy K d is the derivative of the numpy forces, an mpmath
// difference quotient of P(F) holds the per-element algebra, the device equals both).
//
// k_tangent walks the block ranges of k_forces and reads the elements through elements.hpp:
//   tets      one block per 256-tet chunk, lane = tet.  The signed SVD of F = D_i x runs ONCE, the tangent's 12 coefficients
//             (device_math.hpp: tet_tangent_coef -- Hs, al, be, collapsed to Hs, a = (al + be) / 2,
//             b = (al - be) / 2) are formed once; per direction only dF = Ds(d) Binv, dP = U B V^T (tet_tangent_apply), the corner
//             contributions vol dP Binv^T and the chunk's way out repeat.  U, V and the coefficients stay in registers, Binv in this
//             thread's LDS column (rows 12..20); rows 0..11 are reused between directions behind block barriers.
//   triangles lane = triangle: dP = w^2 (dF - dQ) (device_math.hpp: tri_tangent_frame once, tri_tangent_apply per direction); strain
//             limits ignored, as in energy() and forces().
//   hinges    K = stiffness c c^T (x) I3, constant.
// k_gather_tangent (lane = vertex, blockIdx.y = direction): gather_vertex on the direction's scratch, plus shift m o d.
//
// Limits: those of tet_tangent_coef and of the forces -- kinks at sigma_i = 0, the log barrier of the Neo-Hookean kinds at J -> 0, a
// collapsed triangle: the outputs are what the arithmetic gives.  K is not projected to a positive semi-definite matrix.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no floating-point atomics; a direction's result does not depend
// on the other directions of its call.
#pragma once
#include "forces.hpp"

namespace admm_k {

struct TangentArgs {
    ForceArgs f;              // the scene at x and the chunk plan (stress, stop unused); rec, r_cf, h_cf: direction 0
    const double *d;          // [n_vec][3 nv]
    int n_vec;
    DirStrides s;             // doubles between two directions
};

template <bool TABLE>
__device__ __forceinline__ void tangent_tets(const TangentArgs &ta, int chunk, LdsDk *sL) {
    const ForceArgs &a = ta.f;
    const ElemView &v = a.v;
    const int tid = (int)threadIdx.x;
    const ChunkLane ln = chunk_locate(v.kb, a.cb, chunk, tid);
    const int t = ln.t, grp = ln.grp;
    LdsDk *sBi = sL + 12 * kChunkLdK + tid;      // row c of this thread: [c * kChunkLdK]
    const ChunkOut co = chunk_out_begin(a.plan, chunk, sL);
    const double w2 = v.t_sc[t] / v.dt2;
    const Mat mt = v.mats[v.t_mat[t]];
    const int4 id = v.t_idx[t];
    const int vid[4] = {id.x, id.y, id.z, id.w};
    double U[9], S[3], V[9];
    {
        double Bi[9], F[9];
        tet_F_binv(v, id, t, F, Bi);
#pragma unroll
        for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];      // parked in this thread's LDS column for all the directions
        signed_svd3(F, U, S, V);
    }
    double Hs[6], ca[3], cb[3];
    {
        double al[3], be[3];
        tet_tangent_coef<TABLE>(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, v.spl + (size_t)(TABLE && grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles,
                         S, Hs, al, be);
#pragma unroll
        for (int q = 0; q < 3; ++q) { ca[q] = 0.5 * (al[q] + be[q]); cb[q] = 0.5 * (al[q] - be[q]); }
    }
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
    for (int dir = 0; dir < ta.n_vec; ++dir) {
        double G[9], f[12];
        {
            double Ds[9], dF[9];
            tet_edge_matrix(ta.d + (size_t)dir * ta.s.d, vid, Ds);
#pragma unroll
            for (int r = 0; r < 3; ++r) {      // dF = Ds(d) Binv, Binv from LDS
                const double b0 = sBi[(r * 3 + 0) * kChunkLdK], b1 = sBi[(r * 3 + 1) * kChunkLdK], b2 = sBi[(r * 3 + 2) * kChunkLdK];
#pragma unroll
                for (int j = 0; j < 3; ++j) dF[r * 3 + j] = fma(Ds[j], b0, fma(Ds[3 + j], b1, Ds[6 + j] * b2));
            }
            tet_tangent_apply(U, V, Hs, ca, cb, dF, G);
#pragma unroll
            for (int c = 0; c < 9; ++c) G[c] *= vol;
        }
        tet_corner_forces(G, sBi, f);
        if (dir > 0) __syncthreads();      // the previous direction's reduction has read rows 0..11
        chunk_out_store(co, sL, f, a.rec + (size_t)dir * ta.s.rec);
    }
}

// TABLE: the scene holds tabulated splines (a context without a table cannot hold a tet of that model, admm_hip_create refuses it); the
// instance without them does not carry the table path's registers
template <bool TABLE>
__global__ __launch_bounds__(256) void k_tangent(TangentArgs ta) {
    __shared__ double sLm[21 * kChunkLdK];      // rows 0..11: the chunk's corner contributions of one direction; rows 12..20: Binv
    const ForceArgs &a = ta.f;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        tangent_tets<TABLE>(ta, blk, (LdsDk *)sLm);
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        const int4 id = v.r_idx[t];
        double R[4], F[6], Q[6], Si[3], itr;
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        tri_F(R, id, v.x, F);
        tri_tangent_frame(F, Q, Si, itr);
        const double w2 = v.r_sc[t] / v.dt2;
        for (int dir = 0; dir < ta.n_vec; ++dir) {
            double dF[6], G[6];
            tri_F(R, id, ta.d + (size_t)dir * ta.s.d, dF);
            tri_tangent_apply(Q, Si, itr, dF, G);
            double *cf = a.r_cf + (size_t)dir * ta.s.rcf;
#pragma unroll
            for (int j = 0; j < 3; ++j) tri_corner_store(w2 * G[j], w2 * G[3 + j], R, cf + (size_t)j * v.ldr, v.ldr, t);
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= v.nbend) return;
        int vid[4];
        double c[4], ks;
        hinge_load(v, t, c, vid, ks);
        for (int dir = 0; dir < ta.n_vec; ++dir) {
            double Dx[3];
            hinge_Dx(c, vid, ta.d + (size_t)dir * ta.s.d, Dx);
            hinge_corner_store(c, ks, Dx, a.h_cf + (size_t)dir * ta.s.hcf, v.ldb, t);
        }
    }
}

// out_v = sum of the records and corner contributions incident to vertex v (the lists of k_gather_rhs, in list order) + shift m_v o d_v;
// blockIdx.y = direction
struct TangentGatherArgs {
    ForceGatherArgs g;        // t_rec, r_cf, h_cf, f: direction 0
    const double *d, *m;      // [n_vec][3 nv], [3 nv]
    double shift;
    DirStrides s;
};
__global__ __launch_bounds__(256) void k_gather_tangent(TangentGatherArgs ta) {
    const ForceGatherArgs &a = ta.g;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    if (s >= a.n_slices) return;
    const size_t dir = blockIdx.y;
    double acc[3] = {0.0, 0.0, 0.0};
    const int v = gather_vertex(a, s, lane, acc, dir, ta.s);
    if (v < a.nv) {
        const double *dv = ta.d + dir * ta.s.d;
        double *out = a.f + dir * ta.s.d;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = 3 * (size_t)v + j;
            out[i] = fma(ta.shift * ta.m[i], dv[i], acc[j]);
        }
    }
}

} // namespace admm_k
