// elements.hpp -- both sides of an energy term.  READ: how a tet, a triangle and a bending hinge are read at positions x.  WRITE: how an
// element's corner contributions leave the kernel -- a chunk of tets through its reduction into 32-byte records (chunk_out_begin / _store),
// triangles and hinges through their corner rows -- for the incidence lists of k_gather_rhs to sum per vertex (forces.hpp: gather_vertex).
// ONE text under the device passes over all terms -- energy and residuals (monitor.hpp), forces and stress (forces.hpp), K(x) d (tangent.hpp),
// the frozen tangent (newton.hpp) -- so a change to how an element is read or written is made here once.  Included by monitor.hpp.
//
// The LOCAL STEP keeps its own text (kernels.hpp: tet_gather, tet_rest_binv, tet_compute_store): its 36 instances sit on spilled registers,
// and calling these helpers from it changed their register allocation and schedule.  What must agree with it to the bit is restated here
// operation for operation: Binv from the rest positions (the same cross products, fast_rcp of the determinant), F = Ds Binv in the same fma
// nesting, the corner forces and the chunk's reduction in the same summation order.
#pragma once
#include "kernels.hpp"

namespace admm_k {

// the scene at positions x, as every pass over the terms needs it
struct ElemView {
    const double *x;          // [nv][3] positions D is applied to
    double dt2;               // sc = dt^2 w^2  ->  w^2 = sc / dt2
    // tets (device order: sorted by model group, kb = the groups' starts, admm_hip_ctx::kind_begin)
    int nt, ldt; const int4 *t_idx; const double *t_Binv, *t_x0, *t_sc; const int *t_mat; const Mat *mats; const double *spl;
    int kb[6];
    // triangles
    int ntri, ldr; const int4 *r_idx; const double *r_rest, *r_sc;
    // bending hinges
    int nbend, ldb; const int4 *h_idx; const double *h_coef, *h_k;
};

// the edge matrix of a tet with the vertices vid at p (the positions or a direction): Ds[3 m + j] = (p_{m+1} - p_0)_j
__device__ __forceinline__ void tet_edge_matrix(const double *p, const int *vid, double *Ds) {
    double x[12];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int j = 0; j < 3; ++j) x[3 * v + j] = p[3 * (size_t)vid[v] + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) { Ds[j] = x[3 + j] - x[j]; Ds[3 + j] = x[6 + j] - x[j]; Ds[6 + j] = x[9 + j] - x[j]; }
}

// Binv (row-major: Bi[3 r + m] = Binv(m, r)) of tet t with the vertices id -- recomputed from the rest positions (t_x0 set) or streamed --
// and F = D_i x = Ds Binv (column-major, rows 3 r + j of the term)
__device__ __forceinline__ void tet_F_binv(const ElemView &a, const int4 id, int t, double *F, double *Bi) {
    const int vid[4] = {id.x, id.y, id.z, id.w};
    if (a.t_x0) {
        double p[12];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 3; ++j) p[3 * v + j] = a.t_x0[3 * (size_t)vid[v] + j];
        double e0[3], e1[3], e2[3], c0[3], c1[3], c2[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { e0[j] = p[3 + j] - p[j]; e1[j] = p[6 + j] - p[j]; e2[j] = p[9 + j] - p[j]; }
        cross3(e1, e2, c0); cross3(e2, e0, c1); cross3(e0, e1, c2);
        const double idet = fast_rcp(fma(e0[0], c0[0], fma(e0[1], c0[1], e0[2] * c0[2])));
#pragma unroll
        for (int r = 0; r < 3; ++r) { Bi[r * 3 + 0] = c0[r] * idet; Bi[r * 3 + 1] = c1[r] * idet; Bi[r * 3 + 2] = c2[r] * idet; }
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) Bi[c] = a.t_Binv[(size_t)c * a.ldt + t];
    }
    double x[12], Ds[9];      // (the text of tet_edge_matrix restated: with the call, k_monitor's instances came out with another schedule)
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
}

// Lane tid of chunk `chunk` of the local step's plan (host_setup.hpp: TetChunks; chunks are numbered model by model and do not straddle a
// model boundary; kb = the groups' first tets, cb = their first chunks): the model group and the tet.  Lanes past the end of the model's
// range are not valid and redo its last tet, because the whole block takes part in what follows (signed_svd3 takes wave votes, the chunk's
// reduction synchronises the block).
struct ChunkLane { int grp, t; bool valid; };
__device__ __forceinline__ ChunkLane chunk_locate(const int *kb, const int *cb, int chunk, int tid) {
    const int grp = (chunk >= cb[1]) + (chunk >= cb[2]) + (chunk >= cb[3]) + (chunk >= cb[4]);
    const int c0 = grp == 0 ? cb[0] : grp == 1 ? cb[1] : grp == 2 ? cb[2] : grp == 3 ? cb[3] : cb[4];
    const int tb = grp == 0 ? kb[0] : grp == 1 ? kb[1] : grp == 2 ? kb[2] : grp == 3 ? kb[3] : kb[4];
    const int t_end = grp == 0 ? kb[1] : grp == 1 ? kb[2] : grp == 2 ? kb[3] : grp == 3 ? kb[4] : kb[5];
    const int t0 = tb + (chunk - c0) * 256 + tid;
    const bool valid = t0 < t_end;
    return {grp, valid ? t0 : t_end - 1, valid};
}

// corner forces of a tet from G (3x3 column-major) and the Binv parked in this thread's LDS column sBi (row c: [c * kChunkLdK]):
// H(j,m) = sum_r G(j,r) Binv(m,r); corner m+1 gets H(:,m), corner 0 gets -sum_m H(:,m)
__device__ __forceinline__ void tet_corner_forces(const double *G, const LdsDk *sBi, double *f) {
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = 0.0;
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
}

// The chunk's reduction, after the block has parked its corner forces in rows 0..11 of sL and synchronised: thread j of pass p sums the
// <= 8 corner forces of record 256 p + j in list order and stores it as one 32-byte sector of rec.  re: the reduction lists (ch_ent),
// first: this thread's list of pass g0 (loaded early by the caller, in flight across the SVD); g0, g1: the chunk's passes; r0, nrec:
// its records.
__device__ __forceinline__ void chunk_reduce_store(const LdsDk *sL, const __amdgpu_buffer_rsrc_t re, bv4u first, int g0, int g1, int r0, int nrec,
                                                   double *rec) {
    const int tid = (int)threadIdx.x;
    const __amdgpu_buffer_rsrc_t rr = soa_rsrc(rec);
    union { bv4u v; unsigned short h[8]; } e;
    e.v = first;
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

// The way out of a chunk of tets, for every pass that writes records the incidence lists read.  chunk_out_begin, before the SVD or the
// frame load: zeroes the padding column of the reduction lists and issues the load of this thread's first list, in flight across what
// follows.  chunk_out_store: parks f [12] in this thread's column of rows 0..11 of sL, synchronises the block, reduces into rec.
struct ChunkPlan { const unsigned short *ch_ent; const int *ch_group, *ch_rec; };      // the local step's chunk plan (host_setup.hpp: TetChunks)
struct ChunkOut { __amdgpu_buffer_rsrc_t re; bv4u e0; int g0, g1, r0, nrec; };
__device__ __forceinline__ ChunkOut chunk_out_begin(const ChunkPlan &p, int chunk, LdsDk *sL) {
    const int tid = (int)threadIdx.x;
    if (tid < 3) sL[tid * kChunkLdK + 256] = 0.0;
    const int g0 = __builtin_amdgcn_readfirstlane(p.ch_group[chunk]), g1 = __builtin_amdgcn_readfirstlane(p.ch_group[chunk + 1]);
    const int r0 = __builtin_amdgcn_readfirstlane(p.ch_rec[chunk]), nrec = __builtin_amdgcn_readfirstlane(p.ch_rec[chunk + 1]) - r0;
    const __amdgpu_buffer_rsrc_t re = soa_rsrc(p.ch_ent);
    const bv4u e0 = __builtin_amdgcn_raw_buffer_load_b128(re, (g0 * 256 + tid) * 16, 0, kStreamLdAux);
    return ChunkOut{re, e0, g0, g1, r0, nrec};
}
__device__ __forceinline__ void chunk_out_store(const ChunkOut &co, LdsDk *sL, const double *f, double *rec) {
    LdsDk *sCf = sL + (int)threadIdx.x;
#pragma unroll
    for (int c = 0; c < 12; ++c) sCf[c * kChunkLdK] = f[c];
    __syncthreads();
    chunk_reduce_store(sL, co.re, co.e0, co.g0, co.g1, co.r0, co.nrec, rec);
}
struct DirStrides { size_t d, rec, rcf, hcf; };      // doubles between two directions: the vectors [3 nv], the records, the corner rows

// F (3x2 column-major) = [p1 - p0, p2 - p0] R of a triangle with the vertices id and the rest matrix R (2x2 column-major); p = the
// positions or a direction
__device__ __forceinline__ void tri_F(const double *R, const int4 id, const double *p, double *F) {
    const double *p0 = p + 3 * (size_t)id.x, *p1 = p + 3 * (size_t)id.y, *p2 = p + 3 * (size_t)id.z;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double b = p0[j], e1 = p1[j] - b, e2 = p2[j] - b;
        F[j] = fma(e1, R[0], e2 * R[1]);
        F[3 + j] = fma(e1, R[2], e2 * R[3]);
    }
}

// coordinate j of a triangle's corner forces from row j of G (3x2), G0 = G(j,0), G1 = G(j,1): H = G R^T, corner 1 gets H(:,0), corner 2
// H(:,1), corner 0 minus their sum.  cf: the corner-force rows [9][ld] offset to row j
__device__ __forceinline__ void tri_corner_store(double G0, double G1, const double *R, double *cf, int ld, int t) {
    const double h1 = fma(G0, R[0], G1 * R[2]);
    const double h2 = fma(G0, R[1], G1 * R[3]);
    cf[t] = -(h1 + h2);
    cf[(size_t)3 * ld + t] = h1;
    cf[(size_t)6 * ld + t] = h2;
}

// D_i p = sum_k c_k p_{v_k} of a hinge with the coefficients c and the vertices vid; p = the positions or a direction
__device__ __forceinline__ void hinge_Dx(const double *c, const int *vid, const double *p, double *Dx) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Dx[j] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double *pk = p + 3 * (size_t)vid[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) Dx[j] = fma(c[k], pk[j], Dx[j]);
    }
}

// hinge t: the vertices, the coefficients c and the stiffness
__device__ __forceinline__ void hinge_load(const ElemView &v, int t, double *c, int *vid, double &ks) {
    const int4 id = v.h_idx[t];
    vid[0] = id.x; vid[1] = id.y; vid[2] = id.z; vid[3] = id.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = v.h_coef[(size_t)k * v.ldb + t];
    ks = v.h_k[t];
}
// corner k of a hinge gets c_k s (D_i p): s = minus the stiffness for the forces, the stiffness for K d.  cf: the corner rows [12][ldb]
__device__ __forceinline__ void hinge_corner_store(const double *c, double s, const double *Dx, double *cf, int ldb, int t) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) cf[(size_t)(3 * k + j) * ldb + t] = c[k] * (s * Dx[j]);
}

// Is vertex v held?  vert_pin / pin_active: the SpringPin and slide-pin TERMS (linsolver 0 / 2); pin_flag: the pins applied inside the GS
// sweeps (linsolver 1).  The one rule of the stationarity residual and of the frozen tangent's pin mask.
__device__ __forceinline__ bool vertex_held(int v, const int *vert_pin, const int *pin_active, const int *pin_flag) {
    bool held = false;
    if (vert_pin) { const int pi = vert_pin[v]; held = pi >= 0 && pin_active[pi] != 0; }
    if (pin_flag) held = held || pin_flag[v] != 0;
    return held;
}

} // namespace admm_k
