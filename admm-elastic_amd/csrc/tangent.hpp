// tangent.hpp -- the tangent stiffness K(x) = d2E/dx2 = -df/dx of all energy terms applied to n_vec directions, on the device
// (included once by admm_hip.hip, after forces.hpp).
//
// E is the energy admm_hip_energy sums and admm_hip_forces differentiates: out_j = K(x) d_j + shift (m o d_j).  Like the forces this has
// no reference code; it is pinned on them (tests/test_stiffness.py: the numpy K d is the derivative of the numpy forces, an mpmath
// difference quotient of P(F) holds the per-element algebra, the device equals both).
//
// k_tangent walks the block ranges of k_forces:
//   tets      one block per 256-tet chunk, lane = tet.  x and x0 / Binv are gathered as force_tets does, the signed SVD runs ONCE, the
//             tangent's 12 coefficients (device_math.hpp: tet_tangent_coef -- Hs, al, be, collapsed to Hs, a = (al + be) / 2,
//             b = (al - be) / 2) are formed once; per direction only dF = Ds(d) Binv, dP = U B V^T (tet_tangent_apply), the corner
//             contributions vol dP Binv^T and the chunk's reduction into 32-byte records repeat.  U, V and the coefficients stay in
//             registers, Binv in this thread's LDS column (rows 12..20); rows 0..11 are the chunk's corner contributions, reused between
//             directions behind block barriers.
//   triangles lane = triangle: dP = w^2 (dF - dQ) (device_math.hpp: tri_tangent_frame once, tri_tangent_apply per direction); strain
//             limits ignored, as in energy() and forces().
//   hinges    K = stiffness c c^T (x) I3, constant.
// k_gather_tangent (lane = vertex, blockIdx.y = direction) sums records and corner contributions through the incidence lists of
// k_gather_rhs in list order and adds shift m o d.
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
    ForceArgs f;              // the scene at x, as k_forces takes it (stress, stop unused); rec, r_cf, h_cf: direction 0
    const double *d;          // [n_vec][3 nv]
    int n_vec;
    size_t d_stride, rec_stride, rcf_stride, hcf_stride;      // doubles between two directions
};

template <bool TABLE>
__device__ __forceinline__ void tangent_tets(const TangentArgs &ta, int chunk, LdsDk *sL) {
    const ForceArgs &a = ta.f;
    const int tid = (int)threadIdx.x;
    const int grp = (chunk >= a.cb[1]) + (chunk >= a.cb[2]) + (chunk >= a.cb[3]) + (chunk >= a.cb[4]);
    const int c0 = grp == 0 ? a.cb[0] : grp == 1 ? a.cb[1] : grp == 2 ? a.cb[2] : grp == 3 ? a.cb[3] : a.cb[4];
    const int tb = grp == 0 ? a.kb[0] : grp == 1 ? a.kb[1] : grp == 2 ? a.kb[2] : grp == 3 ? a.kb[3] : a.kb[4];
    const int t_end = grp == 0 ? a.kb[1] : grp == 1 ? a.kb[2] : grp == 2 ? a.kb[3] : grp == 3 ? a.kb[4] : a.kb[5];
    const int t0 = tb + (chunk - c0) * 256 + tid;
    const bool valid = t0 < t_end;
    const int t = valid ? t0 : t_end - 1;      // lanes past the model's range redo its last tet and park values no list refers to
    LdsDk *sCf = sL + tid, *sBi = sL + 12 * kChunkLdK + tid;      // row c of this thread: [c * kChunkLdK]
    if (tid < 3) sL[tid * kChunkLdK + 256] = 0.0;                 // the padding column of the reduction lists
    const int g0 = __builtin_amdgcn_readfirstlane(a.ch_group[chunk]), g1 = __builtin_amdgcn_readfirstlane(a.ch_group[chunk + 1]);
    const int r0 = __builtin_amdgcn_readfirstlane(a.ch_rec[chunk]), nrec = __builtin_amdgcn_readfirstlane(a.ch_rec[chunk + 1]) - r0;
    const __amdgpu_buffer_rsrc_t re = soa_rsrc(a.ch_ent);
    union { bv4u v; unsigned short h[8]; } e0;
    e0.v = __builtin_amdgcn_raw_buffer_load_b128(re, (g0 * 256 + tid) * 16, 0, kStreamLdAux);
    const double w2 = a.t_sc[t] / a.dt2;
    const Mat mt = a.mats[a.t_mat[t]];
    const int4 id = a.t_idx[t];
    const int vid[4] = {id.x, id.y, id.z, id.w};
    double U[9], S[3], V[9];
    {
        double Bi[9], F[9];
        if (a.t_x0) {      // Binv from the rest positions, as the local step recomputes it (kernels.hpp: tet_rest_binv)
            double p[12];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int j = 0; j < 3; ++j) p[3 * v + j] = a.t_x0[3 * (size_t)vid[v] + j];
            double e0v[3], e1[3], e2[3], q0[3], q1[3], q2[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { e0v[j] = p[3 + j] - p[j]; e1[j] = p[6 + j] - p[j]; e2[j] = p[9 + j] - p[j]; }
            cross3(e1, e2, q0); cross3(e2, e0v, q1); cross3(e0v, e1, q2);
            const double idet = fast_rcp(fma(e0v[0], q0[0], fma(e0v[1], q0[1], e0v[2] * q0[2])));
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
#pragma unroll
        for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];      // parked in this thread's LDS column for all the directions
        signed_svd3(F, U, S, V);
    }
    double Hs[6], ca[3], cb[3];
    {
        double al[3], be[3];
        tet_tangent_coef<TABLE>(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, a.spl + (size_t)(TABLE && grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles,
                         S, Hs, al, be);
#pragma unroll
        for (int q = 0; q < 3; ++q) { ca[q] = 0.5 * (al[q] + be[q]); cb[q] = 0.5 * (al[q] - be[q]); }
    }
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
    for (int dir = 0; dir < ta.n_vec; ++dir) {
        const double *dv = ta.d + (size_t)dir * ta.d_stride;
        double G[9];
        {
            double x[12], Ds[9], dF[9];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int j = 0; j < 3; ++j) x[3 * v + j] = dv[3 * (size_t)vid[v] + j];
#pragma unroll
            for (int j = 0; j < 3; ++j) { Ds[j] = x[3 + j] - x[j]; Ds[3 + j] = x[6 + j] - x[j]; Ds[6 + j] = x[9 + j] - x[j]; }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double b0 = sBi[(r * 3 + 0) * kChunkLdK], b1 = sBi[(r * 3 + 1) * kChunkLdK], b2 = sBi[(r * 3 + 2) * kChunkLdK];
#pragma unroll
                for (int j = 0; j < 3; ++j) dF[r * 3 + j] = fma(Ds[j], b0, fma(Ds[3 + j], b1, Ds[6 + j] * b2));
            }
            tet_tangent_apply(U, V, Hs, ca, cb, dF, G);
#pragma unroll
            for (int c = 0; c < 9; ++c) G[c] *= vol;
        }
        // corner contributions: H(j,m) = sum_r G(j,r) Binv(m,r); corner m+1 gets H(:,m), corner 0 gets -sum_m H(:,m)  (as force_tets)
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
        if (dir > 0) __syncthreads();      // the previous direction's reduction has read rows 0..11
#pragma unroll
        for (int c = 0; c < 12; ++c) sCf[c * kChunkLdK] = f[c];
        __syncthreads();
        const __amdgpu_buffer_rsrc_t rr = soa_rsrc(a.rec + (size_t)dir * ta.rec_stride);
        union { bv4u v; unsigned short h[8]; } e;
        e.v = e0.v;
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
}

// TABLE: the scene holds tabulated splines (a context without a table cannot hold a tet of that model, admm_hip_create refuses it); the
// instance without them does not carry the table path's registers
template <bool TABLE>
__global__ __launch_bounds__(256) void k_tangent(TangentArgs ta) {
    __shared__ double sLm[21 * kChunkLdK];      // rows 0..11: the chunk's corner contributions of one direction; rows 12..20: Binv
    const ForceArgs &a = ta.f;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        tangent_tets<TABLE>(ta, blk, (LdsDk *)sLm);
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= a.ntri) return;
        const int4 id = a.r_idx[t];
        double R[4], F[6], Q[6], Si[3], itr;
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = a.r_rest[(size_t)c * a.ldr + t];
        {
            const double *p0 = a.x + 3 * (size_t)id.x, *p1 = a.x + 3 * (size_t)id.y, *p2 = a.x + 3 * (size_t)id.z;
#pragma unroll
            for (int j = 0; j < 3; ++j) {      // F (3x2) = [x1 - x0, x2 - x0] rest, as k_forces
                const double b = p0[j], e1 = p1[j] - b, e2 = p2[j] - b;
                F[j] = fma(e1, R[0], e2 * R[1]);
                F[3 + j] = fma(e1, R[2], e2 * R[3]);
            }
        }
        tri_tangent_frame(F, Q, Si, itr);
        const double w2 = a.r_sc[t] / a.dt2;
        for (int dir = 0; dir < ta.n_vec; ++dir) {
            const double *dv = ta.d + (size_t)dir * ta.d_stride;
            const double *p0 = dv + 3 * (size_t)id.x, *p1 = dv + 3 * (size_t)id.y, *p2 = dv + 3 * (size_t)id.z;
            double dF[6], G[6];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double b = p0[j], e1 = p1[j] - b, e2 = p2[j] - b;
                dF[j] = fma(e1, R[0], e2 * R[1]);
                dF[3 + j] = fma(e1, R[2], e2 * R[3]);
            }
            tri_tangent_apply(Q, Si, itr, dF, G);
            double *cf = a.r_cf + (size_t)dir * ta.rcf_stride;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double G0 = w2 * G[j], G1 = w2 * G[3 + j];
                const double h1 = fma(G0, R[0], G1 * R[2]);
                const double h2 = fma(G0, R[1], G1 * R[3]);
                cf[(size_t)(0 + j) * a.ldr + t] = -(h1 + h2);
                cf[(size_t)(3 + j) * a.ldr + t] = h1;
                cf[(size_t)(6 + j) * a.ldr + t] = h2;
            }
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= a.nbend) return;
        const int4 id = a.h_idx[t];
        const int vid[4] = {id.x, id.y, id.z, id.w};
        double c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = a.h_coef[(size_t)k * a.ldb + t];
        const double ks = a.h_k[t];
        for (int dir = 0; dir < ta.n_vec; ++dir) {
            const double *dv = ta.d + (size_t)dir * ta.d_stride;
            double Dx[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {      // D_i d = sum_k c_k d_{v_k}
                const double *p = dv + 3 * (size_t)vid[k];
#pragma unroll
                for (int j = 0; j < 3; ++j) Dx[j] = fma(c[k], p[j], Dx[j]);
            }
            double *cf = a.h_cf + (size_t)dir * ta.hcf_stride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) cf[(size_t)(3 * k + j) * a.ldb + t] = c[k] * (ks * Dx[j]);
        }
    }
}

// out_v = sum of the records and corner contributions incident to vertex v (the lists of k_gather_rhs, in list order) + shift m_v o d_v;
// blockIdx.y = direction
struct TangentGatherArgs {
    ForceGatherArgs g;        // t_rec, r_cf, h_cf, f: direction 0
    const double *d, *m;      // [n_vec][3 nv], [3 nv]
    double shift;
    size_t d_stride, rec_stride, rcf_stride, hcf_stride;
};
__global__ __launch_bounds__(256) void k_gather_tangent(TangentGatherArgs ta) {
    const ForceGatherArgs &a = ta.g;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    if (s >= a.n_slices) return;
    const size_t dir = blockIdx.y;
    const int r = s * 64 + lane;
    const int v = r < a.nv ? a.order[r] : a.nv;
    double acc[3] = {0.0, 0.0, 0.0};
    if (a.t_inc) gather_records(a.t_inc + a.t_ptr[s] + lane, a.t_w[s], a.t_rec + dir * ta.rec_stride, acc);
    if (a.r_inc) gather_corners<false>(a.r_inc + a.r_ptr[s] + lane, a.r_w[s], a.r_cf + dir * ta.rcf_stride, a.r_ld, acc);
    if (a.h_inc) gather_corners<false>(a.h_inc + a.h_ptr[s] + lane, a.h_w[s], a.h_cf + dir * ta.hcf_stride, a.h_ld, acc);
    if (v < a.nv) {
        const double *dv = ta.d + dir * ta.d_stride;
        double *out = a.f + dir * ta.d_stride;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = 3 * (size_t)v + j;
            out[i] = fma(ta.shift * ta.m[i], dv[i], acc[j]);
        }
    }
}

} // namespace admm_k
