// newton.hpp -- the second-order finish of a step on the device: a tangent FROZEN at x (optionally projected to its positive
// semi-definite part), applied many times; the Jacobi-PCG built on it (admm_hip_tangent_solve) and the vector kernels of the projected
// Newton polish (admm_hip_newton_polish).  Included once by admm_hip.hip, after tangent.hpp.
//
// k_tangent (tangent.hpp) runs the signed SVD and the coefficient evaluation on every call; a CG iteration must not.
//   k_tangent_setup<TABLE>  once per x.  The block ranges of k_tangent without the hinges, lane = tet / triangle, elements read through
//             elements.hpp.  Per tet: tet_F_binv, signed_svd3, tet_tangent_coef, with `psd` tet_tangent_psd; stores the frame, SoA
//             [kFrameTet][ldt] (one coalesced 512-byte wave access per component):  U (9), N = Binv V (9), vol {Hs (6), a (3), b (3)}.
//             Per triangle [kFrameTri][ldr]: Q (6), Si (3), itr (with `psd` through tri_tangent_psd), w^2.
//   k_tangent_frozen        per application.  A = U^T Ds(d) N, B from A and the coefficients (as tet_tangent_apply), corner contributions
//             U B N^T -- neither V nor Binv is needed again -- leaving as those of k_forces / k_tangent do (elements.hpp: the write
//             side).  Triangles: tri_tangent_apply on the stored frame; hinges as k_tangent.
//   k_tangent_diag          the diagonal of the frozen operator: per tet and corner the three entries e_k . K_el e_k from twelve frozen
//             applications to dF = e_k (x) grad N_a; they travel in the same records and corner buffers.
//   k_newton_gather<DIAG>   lane = vertex, gather_vertex.  DIAG = false: out = K d + shift m o d, rows
//             of held vertices zero, and the block's partial of d . out; DIAG = true: out = 1 / (diag K + shift m), 0 on held vertices.
// The PCG (y, r, p, Ap, D^-1; z = D^-1 r is not stored) per iteration: k_tangent_frozen on p, k_newton_gather, k_nw_cg_step (alpha; y, r;
// partials of r.z and r.r), k_nw_cg_dir (beta; p; the stop decision).  The update of p needs the complete r.z of the SAME iteration, so
// it is a launch of its own: no grid barrier, no persistent kernel.  Every block re-reduces the partials in the same order (as k_big_vec,
// k_stat_final), so all blocks hold the same alpha, beta and verdict.  WHO WRITES WHAT: the scalars of iteration it + 1 (NwCg st[(it + 1)
// & 1], the copy for the host st[2]) and the stop word are written by block 0 of k_nw_cg_dir(it) only and read by later launches only --
// k_nw_cg_dir itself looks at st[it & 1] -- its .done, and its iteration number, which tells a launch enqueued behind the end of the solve
// (two slots: the one behind the final one still says "running") -- not at the stop word (kernels.hpp: the rule of kCntAdmmStop).  The stop
// test reads the RECURSIVE residual; what the solve reports is the true one, rhs - A y formed once more after the last iteration.
//
// The BLOCK PCG (admm_hip_tangent_solve_block, admm_hip_step_adjoint_block; described where it stands, below k_nw_true_resid): up to
// kNwBlkCols of these recurrences on one frozen tangent, independent of each other, sharing the four launches of an iteration; column j
// has the bits of the single solve.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no floating-point atomics.
#pragma once
#include "tangent.hpp"

namespace admm_k {

constexpr int kFrameTet = 30, kFrameTri = 11;

struct FrozenArgs {
    ForceArgs f;              // the chunk plan and the element lists (f.v.x: the positions, read by the setup only); rec, r_cf, h_cf: the pass's output
    double *t_fr, *r_fr;      // the frames [kFrameTet][ldt], [kFrameTri][ldr]
    const double *d;          // the direction [3 nv] (k_tangent_frozen)
    int psd;                  // the setup projects the element tangents
    const int *stop;          // set: the launch is a no-op (or nullptr)
};

// corner contributions f [12] of a frozen tet (U, N column-major; Hs, a, b scaled by vol) for the edge matrix Ds (Ds[3 m + j] = (d_{m+1} - d_0)_j)
__device__ __forceinline__ void tet_frozen_apply(const double *U, const double *N, const double *Hs, const double *a, const double *b,
                                                 const double *Ds, double *f) {
    double T[9], A[9], B[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) ADMM_M3(T, j, c) = fma(Ds[j], ADMM_M3(N, 0, c), fma(Ds[3 + j], ADMM_M3(N, 1, c), Ds[6 + j] * ADMM_M3(N, 2, c)));
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
        for (int j = 0; j < 3; ++j) ADMM_M3(T, j, c) = fma(ADMM_M3(U, j, 0), ADMM_M3(B, 0, c), fma(ADMM_M3(U, j, 1), ADMM_M3(B, 1, c), ADMM_M3(U, j, 2) * ADMM_M3(B, 2, c)));
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double h = fma(ADMM_M3(T, j, 0), ADMM_M3(N, m, 0), fma(ADMM_M3(T, j, 1), ADMM_M3(N, m, 1), ADMM_M3(T, j, 2) * ADMM_M3(N, m, 2)));
            f[3 * (m + 1) + j] = h;
            f[j] -= h;
        }
}

template <bool TABLE>
__global__ __launch_bounds__(256) void k_tangent_setup(FrozenArgs fa) {
    if (fa.stop && *fa.stop) return;
    const ForceArgs &a = fa.f;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        const ChunkLane ln = chunk_locate(v.kb, a.cb, blk, tid);      // lanes past the model's range redo its last tet (signed_svd3 takes wave votes)
        const int t = ln.t, grp = ln.grp;
        const double w2 = v.t_sc[t] / v.dt2;
        const Mat mt = v.mats[v.t_mat[t]];
        double U[9], S[3], V[9], N[9];
        {
            double Bi[9], F[9];
            tet_F_binv(v, v.t_idx[t], t, F, Bi);
            signed_svd3(F, U, S, V);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int m = 0; m < 3; ++m) ADMM_M3(N, m, c) = fma(Bi[m], ADMM_M3(V, 0, c), fma(Bi[3 + m], ADMM_M3(V, 1, c), Bi[6 + m] * ADMM_M3(V, 2, c)));
        }
        double Hs[6], al[3], be[3];
        tet_tangent_coef<TABLE>(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, v.spl + (size_t)(TABLE && grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles,
                                S, Hs, al, be);
        if (fa.psd) tet_tangent_psd(Hs, al, be);
        const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
        if (!ln.valid) return;
        double *fr = fa.t_fr + t;
        const size_t ld = (size_t)v.ldt;
#pragma unroll
        for (int c = 0; c < 9; ++c) { fr[c * ld] = U[c]; fr[(9 + c) * ld] = N[c]; }
#pragma unroll
        for (int c = 0; c < 6; ++c) fr[(18 + c) * ld] = vol * Hs[c];
#pragma unroll
        for (int q = 0; q < 3; ++q) { fr[(24 + q) * ld] = vol * (0.5 * (al[q] + be[q])); fr[(27 + q) * ld] = vol * (0.5 * (al[q] - be[q])); }
    } else {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        double R[4], F[6], Q[6], Si[3], itr;
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        tri_F(R, v.r_idx[t], v.x, F);
        tri_tangent_frame(F, Q, Si, itr);
        if (fa.psd) tri_tangent_psd(Si, itr);
        double *fr = fa.r_fr + t;
        const size_t ld = (size_t)v.ldr;
#pragma unroll
        for (int c = 0; c < 6; ++c) fr[c * ld] = Q[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) fr[(6 + c) * ld] = Si[c];
        fr[9 * ld] = itr;
        fr[10 * ld] = v.r_sc[t] / v.dt2;
    }
}

// the frame of tet t into registers
__device__ __forceinline__ void tet_frame_load(const double *t_fr, size_t ld, int t, double *U, double *N, double *Hs, double *a, double *b) {
    const double *fr = t_fr + t;
#pragma unroll
    for (int c = 0; c < 9; ++c) { U[c] = fr[c * ld]; N[c] = fr[(9 + c) * ld]; }
#pragma unroll
    for (int c = 0; c < 6; ++c) Hs[c] = fr[(18 + c) * ld];
#pragma unroll
    for (int q = 0; q < 3; ++q) { a[q] = fr[(24 + q) * ld]; b[q] = fr[(27 + q) * ld]; }
}

// DIAG = false: the frozen operator applied to fa.d; DIAG = true: its diagonal (every corner's three entries in the place of its contribution)
template <bool DIAG>
__device__ __forceinline__ void tangent_frozen_body(const FrozenArgs &fa, double *sLm) {
    const ForceArgs &a = fa.f;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        LdsDk *sL = (LdsDk *)sLm;
        const ChunkLane ln = chunk_locate(v.kb, a.cb, blk, tid);
        const int t = ln.t;
        const ChunkOut co = chunk_out_begin(a.plan, blk, sL);
        double U[9], N[9], Hs[6], ca[3], cb[3], f[12];
        tet_frame_load(fa.t_fr, (size_t)v.ldt, t, U, N, Hs, ca, cb);
        if (!DIAG) {
            const int4 id = v.t_idx[t];
            const int vid[4] = {id.x, id.y, id.z, id.w};
            double Ds[9];
            tet_edge_matrix(fa.d, vid, Ds);
            tet_frozen_apply(U, N, Hs, ca, cb, Ds, f);
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) f[q] = 0.0;
#pragma unroll 1
            for (int q = 0; q < 12; ++q) {      // corner q / 3, coordinate q % 3: d = e_k at that corner
                const int c = q / 3, k = q - 3 * c;
                double Ds[9], g[12];
#pragma unroll
                for (int m = 0; m < 3; ++m)
#pragma unroll
                    for (int j = 0; j < 3; ++j) Ds[3 * m + j] = j != k ? 0.0 : c == 0 ? -1.0 : c == m + 1 ? 1.0 : 0.0;
                tet_frozen_apply(U, N, Hs, ca, cb, Ds, g);
#pragma unroll
                for (int p = 0; p < 12; ++p) f[p] = p == q ? g[p] : f[p];
            }
        }
        chunk_out_store(co, sL, f, a.rec);
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        const int4 id = v.r_idx[t];
        double R[4], Q[6], Si[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        const double *fr = fa.r_fr + t;
        const size_t ld = (size_t)v.ldr;
#pragma unroll
        for (int c = 0; c < 6; ++c) Q[c] = fr[c * ld];
#pragma unroll
        for (int c = 0; c < 3; ++c) Si[c] = fr[(6 + c) * ld];
        const double itr = fr[9 * ld], w2 = fr[10 * ld];
        if (!DIAG) {
            double dF[6], G[6];
            tri_F(R, id, fa.d, dF);
            tri_tangent_apply(Q, Si, itr, dF, G);
#pragma unroll
            for (int j = 0; j < 3; ++j) tri_corner_store(w2 * G[j], w2 * G[3 + j], R, a.r_cf + (size_t)j * v.ldr, v.ldr, t);
        } else {
#pragma unroll 1
            for (int q = 0; q < 9; ++q) {      // corner q / 3, coordinate q % 3
                const int c = q / 3, k = q - 3 * c;
                const double e1 = c == 1 ? 1.0 : c == 0 ? -1.0 : 0.0, e2 = c == 2 ? 1.0 : c == 0 ? -1.0 : 0.0;
                double dF[6], G[6];
#pragma unroll
                for (int j = 0; j < 3; ++j) { dF[j] = j == k ? fma(e1, R[0], e2 * R[1]) : 0.0; dF[3 + j] = j == k ? fma(e1, R[2], e2 * R[3]) : 0.0; }
                tri_tangent_apply(Q, Si, itr, dF, G);
                const double G0 = w2 * (k == 0 ? G[0] : k == 1 ? G[1] : G[2]), G1 = w2 * (k == 0 ? G[3] : k == 1 ? G[4] : G[5]);
                const double h1 = fma(G0, R[0], G1 * R[2]), h2 = fma(G0, R[1], G1 * R[3]);
                a.r_cf[(size_t)q * v.ldr + t] = c == 0 ? -(h1 + h2) : c == 1 ? h1 : h2;
            }
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= v.nbend) return;
        int vid[4];
        double c[4], ks;
        hinge_load(v, t, c, vid, ks);
        if (!DIAG) {
            double Dx[3];
            hinge_Dx(c, vid, fa.d, Dx);
            hinge_corner_store(c, ks, Dx, a.h_cf, v.ldb, t);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) a.h_cf[(size_t)(3 * k + j) * v.ldb + t] = c[k] * (ks * c[k]);
        }
    }
}
__global__ __launch_bounds__(256) void k_tangent_frozen(FrozenArgs fa) {
    __shared__ double sLm[12 * kChunkLdK];      // the chunk's corner contributions
    if (fa.stop && *fa.stop) return;
    tangent_frozen_body<false>(fa, sLm);
}
__global__ __launch_bounds__(256) void k_tangent_diag(FrozenArgs fa) {
    __shared__ double sLm[12 * kChunkLdK];
    tangent_frozen_body<true>(fa, sLm);
}

// lane = vertex: the sum of the records and corner contributions incident to it (the lists of k_gather_rhs, in list order)
struct NewtonGatherArgs {
    ForceGatherArgs g;        // t_rec, r_cf, h_cf: what the frozen pass left; f: the result [nv][3]
    const double *d, *m;      // the direction (DIAG: unused), the masses [3 nv]
    double shift;
    const int *pin;           // [nv] nonzero: a held vertex (row and column dropped), or nullptr
    double *part;             // [blocks] partials of d . out (DIAG: unused)
    const int *stop;
};
template <bool DIAG>
__global__ __launch_bounds__(256) void k_newton_gather(NewtonGatherArgs na) {
    __shared__ double lds[4];
    if (na.stop && *na.stop) return;
    const ForceGatherArgs &a = na.g;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    double q[1] = {0.0};
    if (s < a.n_slices) {
        double acc[3] = {0.0, 0.0, 0.0};
        const int v = gather_vertex(a, s, lane, acc);
        if (v < a.nv) {
            const bool held = na.pin && na.pin[v] != 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t i = 3 * (size_t)v + j;
                if (DIAG) {
                    const double dg = fma(na.shift, na.m[i], acc[j]);
                    a.f[i] = held ? 0.0 : dg > 0.0 ? 1.0 / dg : 1.0;      // (an indefinite unprojected operator: no scaling on that row)
                } else {
                    const double di = na.d[i], o = held ? 0.0 : fma(na.shift * na.m[i], di, acc[j]);
                    a.f[i] = o;
                    q[0] = fma(di, o, q[0]);
                }
            }
        }
    }
    if (!DIAG) {
        block_sum<1>(q, lds);
        if (threadIdx.x == 0) na.part[xcd_block()] = q[0];
    }
}

// ---- the frozen pass on a BLOCK of directions (admm_hip_stiffness_apply_ex with ADMM_HIP_TANGENT_BLOCK, modal.hpp) ----
// k_tangent_frozen_block: the block ranges of k_tangent_frozen; an element's frame (tets: 30 doubles, triangles: 11, hinges: their
// coefficients) is loaded ONCE and stays in registers across the loop over the directions, the way tangent_tets loops them: direction j
// reads fa.d + j s.d and leaves its records / corner rows j strides further (ElemScratch::ensure(c, n_vec)); rows 0..11 of the LDS are
// reused behind a block barrier.  Per direction the arithmetic and the summation orders are those of k_tangent_frozen, so column j has
// the bits of the single pass on the same direction (tests/test_modes.py).
struct FrozenBlockArgs {
    FrozenArgs fa;            // fa.d: [n_vec][s.d]; f.rec, f.r_cf, f.h_cf: direction 0
    int n_vec;
    DirStrides s;
    const int *cols;          // nullptr: the directions 0 .. n_vec; else cols[0] directions, cols[1 ..] (the block PCG's column list, below)
};
// the q-th direction of a block launch and their number
__device__ __forceinline__ int block_dirs(const int *cols, int n_vec) { return cols ? cols[0] : n_vec; }
__device__ __forceinline__ int block_dir(const int *cols, int q) { return cols ? cols[1 + q] : q; }
__global__ __launch_bounds__(256) void k_tangent_frozen_block(FrozenBlockArgs ba) {
    __shared__ double sLm[12 * kChunkLdK];
    const FrozenArgs &fa = ba.fa;
    if (fa.stop && *fa.stop) return;
    const ForceArgs &a = fa.f;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        LdsDk *sL = (LdsDk *)sLm;
        const ChunkLane ln = chunk_locate(v.kb, a.cb, blk, tid);
        const int t = ln.t;
        const ChunkOut co = chunk_out_begin(a.plan, blk, sL);
        double U[9], N[9], Hs[6], ca[3], cb[3];
        tet_frame_load(fa.t_fr, (size_t)v.ldt, t, U, N, Hs, ca, cb);
        const int4 id = v.t_idx[t];
        const int vid[4] = {id.x, id.y, id.z, id.w};
        const int nd = block_dirs(ba.cols, ba.n_vec);
#pragma unroll 1
        for (int q = 0; q < nd; ++q) {
            const int dir = block_dir(ba.cols, q);
            double Ds[9], f[12];
            tet_edge_matrix(fa.d + (size_t)dir * ba.s.d, vid, Ds);
            tet_frozen_apply(U, N, Hs, ca, cb, Ds, f);
            if (q > 0) __syncthreads();        // the previous direction's reduction has read rows 0..11
            chunk_out_store(co, sL, f, a.rec + (size_t)dir * ba.s.rec);
        }
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        const int4 id = v.r_idx[t];
        double R[4], Q[6], Si[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        const double *fr = fa.r_fr + t;
        const size_t ld = (size_t)v.ldr;
#pragma unroll
        for (int c = 0; c < 6; ++c) Q[c] = fr[c * ld];
#pragma unroll
        for (int c = 0; c < 3; ++c) Si[c] = fr[(6 + c) * ld];
        const double itr = fr[9 * ld], w2 = fr[10 * ld];
        const int nd = block_dirs(ba.cols, ba.n_vec);
#pragma unroll 1
        for (int q = 0; q < nd; ++q) {
            const int dir = block_dir(ba.cols, q);
            double dF[6], G[6];
            tri_F(R, id, fa.d + (size_t)dir * ba.s.d, dF);
            tri_tangent_apply(Q, Si, itr, dF, G);
            double *cf = a.r_cf + (size_t)dir * ba.s.rcf;
#pragma unroll
            for (int j = 0; j < 3; ++j) tri_corner_store(w2 * G[j], w2 * G[3 + j], R, cf + (size_t)j * v.ldr, v.ldr, t);
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= v.nbend) return;
        int vid[4];
        double c[4], ks;
        hinge_load(v, t, c, vid, ks);
        const int nd = block_dirs(ba.cols, ba.n_vec);
#pragma unroll 1
        for (int q = 0; q < nd; ++q) {
            const int dir = block_dir(ba.cols, q);
            double Dx[3];
            hinge_Dx(c, vid, fa.d + (size_t)dir * ba.s.d, Dx);
            hinge_corner_store(c, ks, Dx, a.h_cf + (size_t)dir * ba.s.hcf, v.ldb, t);
        }
    }
}
// k_newton_gather<false> on a block: blockIdx.y = direction; out_j = K d_j + shift m o d_j, rows of held vertices zero.  DOT = false: no
// d . Kd partials.  DOT = true (the block PCG): the partial of direction j at part[j spart + xcd_block()], in the block shape and the
// block_sum order of k_newton_gather<false> -- nw_reduce then returns the single solve's bits.  With `cols` blockIdx.y indexes that list
// and a block beyond it returns; block (0, 0) adds the list's length to passes[0] and 1 to passes[1].
struct NewtonGatherBlockArgs {
    NewtonGatherArgs n;       // g.t_rec, g.r_cf, g.h_cf, g.f, d: direction 0; part: direction 0 (DOT only)
    DirStrides s;
    const int *cols;          // as FrozenBlockArgs::cols, or nullptr
    size_t spart;             // doubles between the partials of two directions
    int *passes;              // [2]: columns, launches applied (needs cols), or nullptr
};
template <bool DOT>
__global__ __launch_bounds__(256) void k_newton_gather_block(NewtonGatherBlockArgs ba) {
    __shared__ double lds[4];
    const NewtonGatherArgs &na = ba.n;
    if (na.stop && *na.stop) return;
    if (ba.cols && (int)blockIdx.y >= ba.cols[0]) return;
    if (ba.passes && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { ba.passes[0] += ba.cols[0]; ba.passes[1] += 1; }
    const ForceGatherArgs &a = na.g;
    const int lane = threadIdx.x & 63;
    const int s = wave_slice();
    if (!DOT && s >= a.n_slices) return;
    const size_t dir = (size_t)block_dir(ba.cols, (int)blockIdx.y);
    double q[1] = {0.0};
    if (s < a.n_slices) {
        double acc[3] = {0.0, 0.0, 0.0};
        const int v = gather_vertex(a, s, lane, acc, dir, ba.s);
        if (v < a.nv) {
            const bool held = na.pin && na.pin[v] != 0;
            const double *dv = na.d + dir * ba.s.d;
            double *out = a.f + dir * ba.s.d;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t i = 3 * (size_t)v + j;
                if (DOT) {
                    const double di = dv[i], o = held ? 0.0 : fma(na.shift * na.m[i], di, acc[j]);
                    out[i] = o;
                    q[0] = fma(di, o, q[0]);
                } else out[i] = held ? 0.0 : fma(na.shift * na.m[i], dv[i], acc[j]);
            }
        }
    }
    if (DOT) {
        block_sum<1>(q, lds);
        if (threadIdx.x == 0) na.part[dir * ba.spart + xcd_block()] = q[0];
    }
}
// d_j = 0 on the held vertices, in place; blockIdx.y = direction (k_nw_mask on a block)
__global__ __launch_bounds__(256) void k_nw_mask_block(int nv, size_t stride, const int *__restrict__ pin, double *__restrict__ d) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv || !pin || pin[v] == 0) return;
    double *dj = d + (size_t)blockIdx.y * stride;
#pragma unroll
    for (int j = 0; j < 3; ++j) dj[3 * (size_t)v + j] = 0.0;
}

// ---- the vector kernels of the PCG: grid = blocks_for(nv), lane = vertex ----
struct NwCg { double rz, rr, bb; int it, done, conv, pad_; };      // r . z, r . r, |rhs|^2 over the free rows; iterations done; ended; met its tolerance

// q[i] = the sum of part[i nb + 0 .. nb) in a fixed order, in every thread
template <int NQ>
__device__ __forceinline__ void nw_reduce(const double *__restrict__ part, int nb, double *q, double *lds) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        q[i] = 0.0;
        for (int b = (int)threadIdx.x; b < nb; b += 256) q[i] += part[(size_t)i * nb + b];
    }
    block_sum<NQ>(q, lds);
}
__device__ __forceinline__ bool nw_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)

// pin[v] = 1 where k_stationarity skips a vertex (elements.hpp: vertex_held)
__global__ __launch_bounds__(256) void k_nw_pin_mask(int nv, const int *__restrict__ vert_pin, const int *__restrict__ pin_active,
                                                     const int *__restrict__ pin_flag, int *__restrict__ pin) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    pin[v] = vertex_held(v, vert_pin, pin_active, pin_flag) ? 1 : 0;
}
// out = in with the held vertices zeroed
__global__ __launch_bounds__(256) void k_nw_mask(int nv, const int *__restrict__ pin, const double *__restrict__ in, double *__restrict__ out) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    const bool held = pin && pin[v] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; out[i] = held ? 0.0 : in[i]; }
}

// ---- the stages of the PCG, one body each: the single (k_nw_cg_*), block (k_nw_cg_*_block) and two-level (k_tc_cg_*, tangent_precond.hpp)
// kernels call them on their own column, so the three paths cannot drift apart ----
// y = 0, r = rhs on the free rows, p = z = D^-1 r (P; the two-level start forms its p later); partials of r . D^-1 r and r . r
template <bool P>
__device__ __forceinline__ void nw_cg_init_col(int nv, int nb, const double *__restrict__ rhs, const int *__restrict__ pin, const double *__restrict__ dinv,
                                               double *__restrict__ y, double *__restrict__ r, double *__restrict__ p, double *__restrict__ part, double *lds) {
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[2] = {0.0, 0.0};
    if (v < nv) {
        const bool held = pin && pin[v] != 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = 3 * (size_t)v + j;
            const double ri = held ? 0.0 : rhs[i], zi = dinv[i] * ri;
            y[i] = 0.0; r[i] = ri;
            if (P) p[i] = zi;
            q[0] = fma(ri, zi, q[0]); q[1] = fma(ri, ri, q[1]);
        }
    }
    block_sum<2>(q, lds);
    if (threadIdx.x == 0) { part[nb + blk] = q[0]; part[2 * (size_t)nb + blk] = q[1]; }
}
// the scalars of iteration 0 from r . z and r . r (a zero or non-finite right-hand side ends the solve here), into ALL THREE slots: what
// an earlier solve left in slot 1 must not pass the test of k_nw_cg_dir(it odd) when this solve ends at once
__device__ __forceinline__ NwCg nw_cg_start(double rz, double rr, NwCg *st) {
    NwCg s;
    s.rz = rz; s.rr = rr; s.bb = rr; s.it = 0; s.pad_ = 0;
    s.done = !(rr > 0.0) || !nw_finite(rr) || !(rz > 0.0) || !nw_finite(rz);
    s.conv = rr == 0.0;
    st[0] = s; st[1] = s; st[2] = s;
    return s;
}
// alpha = s.rz / p.Ap (part[0 .. nb)); y += alpha p, r -= alpha Ap; partials of the new r . D^-1 r and r . r.  A breakdown (p.Ap <= 0 or a
// non-finite scalar) leaves y and r as they are; nw_cg_next reaches the same verdict from the same numbers and ends the solve.
__device__ __forceinline__ void nw_cg_step_col(const NwCg &s, int nv, int nb, const double *__restrict__ dinv, const double *__restrict__ p,
                                               const double *__restrict__ ap, double *__restrict__ y, double *__restrict__ r, double *__restrict__ part,
                                               double *lds) {
    double pap[1];
    nw_reduce<1>(part, nb, pap, lds);
    if (!(pap[0] > 0.0) || !nw_finite(pap[0])) return;
    const double alpha = s.rz / pap[0];
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[2] = {0.0, 0.0};
    if (v < nv) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = 3 * (size_t)v + j;
            y[i] = fma(alpha, p[i], y[i]);
            const double ri = fma(-alpha, ap[i], r[i]);
            r[i] = ri;
            q[0] = fma(ri * dinv[i], ri, q[0]); q[1] = fma(ri, ri, q[1]);
        }
    }
    block_sum<2>(q, lds);
    if (threadIdx.x == 0) { part[nb + blk] = q[0]; part[2 * (size_t)nb + blk] = q[1]; }
}
// the verdict of iteration s.it: the scalars of iteration s.it + 1 from p.Ap and the new r . z and r . r, or the end of the solve
// (k_nw_cg_dir_block, k_tc_cg_dir; k_nw_cg_dir writes the same lines out, see there)
__device__ __forceinline__ NwCg nw_cg_next(const NwCg &s, double pap, double rz_new, double rr_new, double tol2, int max_iters) {
    const bool broke = !(pap > 0.0) || !nw_finite(pap);
    NwCg n = s;
    if (broke) { n.done = 1; n.conv = 0; }
    else {
        n.rz = rz_new; n.rr = rr_new; n.it = s.it + 1;
        n.conv = rr_new <= tol2 * s.bb;
        n.done = n.conv || n.it >= max_iters || !nw_finite(rz_new) || !nw_finite(rr_new) || !(rz_new > 0.0);
    }
    return n;
}

// y = 0, r = rhs on the free rows, p = z = D^-1 r; partials of r . z and r . r
__global__ __launch_bounds__(256) void k_nw_cg_init(int nv, int nb, const double *__restrict__ rhs, const int *__restrict__ pin, const double *__restrict__ dinv,
                                                    double *__restrict__ y, double *__restrict__ r, double *__restrict__ p, double *__restrict__ part) {
    __shared__ double lds[8];
    nw_cg_init_col<true>(nv, nb, rhs, pin, dinv, y, r, p, part, lds);
}
// one block: the scalars of iteration 0 and the stop word
__global__ __launch_bounds__(256) void k_nw_cg_init2(int nb, const double *__restrict__ part, NwCg *__restrict__ st, int *__restrict__ stop) {
    __shared__ double lds[8];
    double q[2];
    nw_reduce<2>(part + nb, nb, q, lds);
    if (threadIdx.x == 0) *stop = nw_cg_start(q[0], q[1], st).done;
}
// nw_cg_step_col on the one column of the single solve
__global__ __launch_bounds__(256) void k_nw_cg_step(int it, int nv, int nb, const NwCg *__restrict__ st, const int *stop, const double *__restrict__ dinv,
                                                    const double *__restrict__ p, const double *__restrict__ ap, double *__restrict__ y,
                                                    double *__restrict__ r, double *__restrict__ part) {
    __shared__ double lds[8];
    if (*stop) return;
    const NwCg s = st[it & 1];
    nw_cg_step_col(s, nv, nb, dinv, p, ap, y, r, part, lds);
}
// beta = r.z new / r.z old; p = D^-1 r + beta p; block 0 writes the scalars of iteration it + 1, the verdict and the stop word
__global__ __launch_bounds__(256) void k_nw_cg_dir(int it, int nv, int nb, NwCg *st, int *stop, double tol2, int max_iters, const double *__restrict__ dinv,
                                                   const double *__restrict__ r, double *__restrict__ p, const double *__restrict__ part) {
    __shared__ double lds[12];
    const NwCg s = st[it & 1];
    if (s.done || s.it != it) return;      // ended, or a launch behind the end: st[it & 1] is then the slot of iteration it - 2
    double q[3];
    nw_reduce<3>(part, nb, q, lds);
    const bool broke = !(q[0] > 0.0) || !nw_finite(q[0]);      // nw_cg_next, written out: through the call the compiler schedules this kernel differently
    NwCg n = s;
    if (broke) { n.done = 1; n.conv = 0; }
    else {
        n.rz = q[1]; n.rr = q[2]; n.it = s.it + 1;
        n.conv = q[2] <= tol2 * s.bb;
        n.done = n.conv || n.it >= max_iters || !nw_finite(q[1]) || !nw_finite(q[2]) || !(q[1] > 0.0);
    }
    if (!n.done) {
        const double beta = q[1] / s.rz;
        const int v = xcd_block() * 256 + (int)threadIdx.x;
        if (v < nv) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; p[i] = fma(beta, p[i], dinv[i] * r[i]); }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[(it + 1) & 1] = n; st[2] = n;
        if (n.done) *stop = 1;
    }
}

// block partials of |rhs - ay|^2 over the free rows, ay = (K + shift M) y as k_newton_gather left it: the true residual of the iterate a
// solve returns
__global__ __launch_bounds__(256) void k_nw_true_resid(int nv, const double *__restrict__ rhs, const int *__restrict__ pin, const double *__restrict__ ay,
                                                       double *__restrict__ part) {
    __shared__ double lds[4];
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[1] = {0.0};
    if (v < nv && !(pin && pin[v] != 0)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; const double r = rhs[i] - ay[i]; q[0] = fma(r, r, q[0]); }
    }
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) part[blk] = q[0];
}

// ---- the block PCG (admm_hip_tangent_solve_block, admm_hip_step_adjoint_block): k <= kNwBlkCols INDEPENDENT recurrences on one frozen
// tangent that share every launch -- not a block-Krylov method.  Column j owns y_j, r_j, p_j, Ap_j [k][sv], its partials part[j][3][nb]
// and its scalars st[j][3], and runs the rules of k_nw_cg_step / k_nw_cg_dir on them with the arithmetic and the summation orders of
// the single solve: column j is the single solve of rhs_j, bit for bit.  grid = (blocks_for(nv), k); blockIdx.y selects the column.
// THE COLUMN LIST: list[it & 1] = {n, columns still running at iteration it}.  k_tangent_frozen_block loops over it, the gather and the
// vector kernels index it with blockIdx.y (a block beyond it returns), so a finished column costs nothing from the next iteration on.
// WHO WRITES WHAT, per column as in the single solve; the list of iteration it + 1 and the stop word (set when that list is empty) are
// written in k_nw_cg_dir_block(it) by the LAST of the running columns' blocks 0 to arrive at an integer ticket (every column's verdict is
// in memory by then; the list is filled in the order of the old one, so its content does not depend on who arrives last) and read by
// later launches only.  A launch enqueued behind the end sees the stop word, an empty list, or a column slot of another iteration.
constexpr int kNwBlkCols = 16;      // == kModalNb (modal.hpp)
struct NwBlockCtl { int list[2][kNwBlkCols + 1]; int arrive, passes[2]; };      // passes: columns, iterations applied in the iteration loop
struct NwBlockArgs {
    int nv, nb, k;            // vertices, their blocks, columns
    size_t sv;                // doubles between two columns of a block vector
    const double *rhs, *dinv;
    const int *pin;
    double *y, *r, *p, *ap;   // [k][sv] each
    double *part;             // [k][3][nb]
    double *rr;               // [k]: |rhs_j - A y_j|^2 over the free rows (k_nw_resid_final_block)
    NwCg *st;                 // [k][3]
    NwBlockCtl *ctl;
    int *stop;
    double tol2;
    int max_iters;
};
// k_nw_cg_init per column
__global__ __launch_bounds__(256) void k_nw_cg_init_block(NwBlockArgs a) {
    __shared__ double lds[8];
    const size_t col = blockIdx.y, o = col * a.sv;
    nw_cg_init_col<true>(a.nv, a.nb, a.rhs + o, a.pin, a.dinv, a.y + o, a.r + o, a.p + o, a.part + col * 3 * a.nb, lds);
}
// one block: k_nw_cg_init2 per column (all three slots), the list of iteration 0, the counters and the stop word
__global__ __launch_bounds__(256) void k_nw_cg_init2_block(NwBlockArgs a) {
    __shared__ double lds[8];
    int n = 0;
    for (int col = 0; col < a.k; ++col) {
        double q[2];
        nw_reduce<2>(a.part + (size_t)col * 3 * a.nb + a.nb, a.nb, q, lds);
        if (threadIdx.x == 0 && !nw_cg_start(q[0], q[1], a.st + 3 * col).done) a.ctl->list[0][1 + n++] = col;
    }
    if (threadIdx.x == 0) {
        a.ctl->list[0][0] = n; a.ctl->list[1][0] = 0; a.ctl->arrive = 0; a.ctl->passes[0] = 0; a.ctl->passes[1] = 0;
        *a.stop = n == 0;
    }
}
// k_nw_cg_step per running column
__global__ __launch_bounds__(256) void k_nw_cg_step_block(int it, NwBlockArgs a) {
    __shared__ double lds[8];
    if (*a.stop) return;
    const int *ls = a.ctl->list[it & 1];
    if ((int)blockIdx.y >= ls[0]) return;
    const size_t col = (size_t)ls[1 + blockIdx.y];
    const NwCg s = a.st[3 * col + (it & 1)];
    const size_t o = col * a.sv;
    nw_cg_step_col(s, a.nv, a.nb, a.dinv, a.p + o, a.ap + o, a.y + o, a.r + o, a.part + col * 3 * a.nb, lds);
}
// k_nw_cg_dir per running column; the list of iteration it + 1 and the stop word (above)
__global__ __launch_bounds__(256) void k_nw_cg_dir_block(int it, NwBlockArgs a) {
    __shared__ double lds[12];
    const int *ls = a.ctl->list[it & 1];
    const int nl = ls[0];
    if ((int)blockIdx.y >= nl) return;
    const size_t col = (size_t)ls[1 + blockIdx.y];
    NwCg *st = a.st + 3 * col;
    const NwCg s = st[it & 1];
    if (s.done || s.it != it) return;      // ended, or a launch behind the end (k_nw_cg_dir)
    double q[3];
    nw_reduce<3>(a.part + col * 3 * a.nb, a.nb, q, lds);
    const NwCg n = nw_cg_next(s, q[0], q[1], q[2], a.tol2, a.max_iters);
    if (!n.done) {
        const double beta = q[1] / s.rz;
        const double *r = a.r + col * a.sv;
        double *p = a.p + col * a.sv;
        const int v = xcd_block() * 256 + (int)threadIdx.x;
        if (v < a.nv) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; p[i] = fma(beta, p[i], a.dinv[i] * r[i]); }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[(it + 1) & 1] = n; st[2] = n;
        __threadfence();
        if (atomicAdd(&a.ctl->arrive, 1) == nl - 1) {      // the last column to arrive: every verdict of this iteration is in memory
            __threadfence();
            int *nx = a.ctl->list[(it + 1) & 1];
            int m = 0;
            for (int j = 0; j < nl; ++j) {
                const int cj = ls[1 + j];
                if (!__hip_atomic_load(&a.st[3 * cj + 2].done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) nx[1 + m++] = cj;
            }
            nx[0] = m;
            a.ctl->arrive = 0;
            if (m == 0) *a.stop = 1;
        }
    }
}
// k_nw_true_resid per column (ay_j in a.ap), and one block per column that sums its partials in the order of k_stat_final
__global__ __launch_bounds__(256) void k_nw_true_resid_block(NwBlockArgs a) {
    __shared__ double lds[4];
    const size_t col = blockIdx.y;
    const double *rhs = a.rhs + col * a.sv, *ay = a.ap + col * a.sv;
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[1] = {0.0};
    if (v < a.nv && !(a.pin && a.pin[v] != 0)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; const double r = rhs[i] - ay[i]; q[0] = fma(r, r, q[0]); }
    }
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) a.part[col * 3 * a.nb + blk] = q[0];
}
__global__ __launch_bounds__(256) void k_nw_resid_final_block(NwBlockArgs a) {
    __shared__ double lds[4];
    const double *part = a.part + (size_t)blockIdx.x * 3 * a.nb;
    double q[1] = {0.0};
    for (int b = (int)threadIdx.x; b < a.nb; b += 256) q[0] += part[b];
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) a.rr[blockIdx.x] = q[0];
}

// ---- the vector kernels of the Newton polish ----
// rhs = -g, g = (m o x - M x_bar) / dt^2 - f on the free rows (0 on held vertices); block partials of |g|^2 (k_stat_final sums them)
__global__ __launch_bounds__(256) void k_nw_grad(int nv, const double *__restrict__ x, const double *__restrict__ m, const double *__restrict__ Mxbar,
                                                 const double *__restrict__ f, double idt2, const int *__restrict__ pin, double *__restrict__ rhs,
                                                 double *__restrict__ part) {
    __shared__ double lds[4];
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[1] = {0.0};
    if (v < nv) {
        const bool held = pin[v] != 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = 3 * (size_t)v + j;
            const double g = held ? 0.0 : fma(m[i], x[i], -Mxbar[i]) * idt2 - f[i];
            rhs[i] = -g;
            q[0] = fma(g, g, q[0]);
        }
    }
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) part[blk] = q[0];
}
// block partials of g . delta (g = -rhs): the slope of the line search
__global__ __launch_bounds__(256) void k_nw_slope(int nv, const double *__restrict__ rhs, const double *__restrict__ delta, double *__restrict__ part) {
    __shared__ double lds[4];
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    double q[1] = {0.0};
    if (v < nv) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; q[0] = fma(-rhs[i], delta[i], q[0]); }
    }
    block_sum<1>(q, lds);
    if (threadIdx.x == 0) part[blk] = q[0];
}
// out = x + t delta; v_out = v + (t / dt) delta when v is given (the accepted step: x and out may be the same array)
__global__ __launch_bounds__(256) void k_nw_axpy(int n3, double t, double t_dt, const double *__restrict__ delta, const double *x, double *out, double *v) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n3) return;
    out[i] = fma(t, delta[i], x[i]);
    if (v) v[i] = fma(t_dt, delta[i], v[i]);
}

} // namespace admm_k
