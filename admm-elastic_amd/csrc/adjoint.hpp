// adjoint.hpp -- the adjoint of one implicit-Euler step on the device (included once by admm_hip.hip, after newton.hpp).
//
// A converged step satisfies, on every free degree of freedom (elements.hpp: vertex_held),
//     r(x; x_bar, m, theta) = m o (x - x_bar) / dt^2 - f(x; theta) = 0,   x_bar = x_prev + dt v_prev + dt^2 a_ext,   v = (x - x_prev) / dt.
// For a loss L(x, v) with Lx = dL/dx, Lv = dL/dv:
//     g_x = Lx + Lv / dt (held rows 0),    A lambda = g_x,  A = K(x) + M / dt^2 on the free rows (lambda = 0 on held rows)
//     dL/dx_bar = m o lambda / dt^2        dL/dx_prev = m o lambda / dt^2 - Lv / dt (held rows 0)        dL/dv_prev = m o lambda / dt
//     dL/dm = -lambda o (x - x_bar) / dt^2 (x_bar held fixed)                                            dL/dtheta = lambda^T df/dtheta
// A is the Jacobian newton_polish solves with (symmetric: its transpose is itself), so the solve is tangent_solve_device of newton.hpp.
// What is new here:
//   k_param_sens<TABLE>  a^T df/dtheta per ENERGY TERM for a stack of k <= kSensCols vectors a.  The block ranges of k_forces; a tet block
//             is a chunk of the local step's plan (the model is block-uniform), lane = tet, read through elements.hpp.  The signed SVD and
//             the kind's evaluations (device_math.hpp: tet_param_grad) run ONCE per tet; per column only A^_ii = (U^T Ds(a) Binv V)_ii:
//                 a . f_e          = -vol sum_i sg_i A^_ii                        (d_scale: the derivative in a factor on the tet's energy)
//                 a . df_e/dtheta  = -vol sum_i (d sg_i / d theta) A^_ii          theta = mu, la, kappa as the tet's Mat stores them
//             Out per tet and column (d_mu, d_la, d_kappa, d_scale), SoA [k][4][ldt] in device order.  Triangles and hinges have one
//             parameter, the factor on their energy (w^2; the hinge stiffness): sum_c a_c . f_{e,c} / that factor's unit, i.e. the value
//             is sum_c a_c . f_{e,c} itself -- [k][ldr], [k][ldb].  No cross-element sums, no atomics; lanes past a model's end redo its
//             last tet (signed_svd3 takes wave votes) and store nothing.  The tabulated spline is an instance of its own, as in
//             k_tangent_setup<TABLE>.  A column's arithmetic does not depend on k: column j of a stack has the bits of a alone.
//             REGISTERS: the evaluations are the peak.  With U and N = Binv V held across them the closed-form instance took 160 VGPRs
//             (3 waves / SIMD); a thread parks Binv across the SVD (as k_forces) and then U and N across the evaluations in its own LDS
//             column (18 rows, 37 KB a block: four blocks a CU fit the 160 KB), which brings it to 128 VGPRs, 4 waves / SIMD, no scratch.
//             (amdgpu_waves_per_eu(4, 4) instead spilled 18 VGPRs; running the evaluations as one looped text hoisted every model's
//             invariants out of the loop: 256 VGPRs.)  LDS is private to a thread here: no barrier.
//   k_adj_rhs, k_adj_out the vector kernels around the solve (lane = vertex).
//   k_rest_sens<TABLE>   a^T df/dX per REST vertex of the tets (the gradient in the rest shape), and
//   k_adj_held           dL/dx of the held vertices, g - K lam on their rows: both described where they stand, below k_param_sens.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no floating-point atomics.
#pragma once
#include "newton.hpp"

namespace admm_k {

constexpr int kSensCols = 16;      // the widest stack of one k_param_sens pass

struct SensArgs {
    ForceArgs f;              // the scene at x and the chunk plan (rec, r_cf, h_cf, stress unused)
    const double *a;          // [k][sa] the multiplier vectors
    size_t sa;                // doubles between two of them
    int k;
    double *o_t, *o_r, *o_h;  // [k][4][ldt], [k][ldr], [k][ldb]
};

template <bool TABLE>
__global__ __launch_bounds__(256) void k_param_sens(SensArgs sa) {
    __shared__ double sLm[18 * kChunkLdK];      // rows 0..8: Binv across the SVD; rows 0..17: U and N across the evaluations
    const ForceArgs &a = sa.f;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk < a.nb_t) {
        const ChunkLane ln = chunk_locate(v.kb, a.cb, blk, tid);
        const int t = ln.t, grp = ln.grp;
        const int4 id = v.t_idx[t];
        double U[9], N[9], S[3];
        {
            // Binv is needed again behind the SVD: parked in this thread's LDS column across it, as in k_forces
            LdsDk *sBi = (LdsDk *)sLm + tid;
            double F[9], V[9];
            {
                double Bi[9];
                tet_F_binv(v, id, t, F, Bi);
#pragma unroll
                for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];
            }
            signed_svd3(F, U, S, V);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    ADMM_M3(N, m, c) = fma(sBi[m * kChunkLdK], ADMM_M3(V, 0, c), fma(sBi[(3 + m) * kChunkLdK], ADMM_M3(V, 1, c), sBi[(6 + m) * kChunkLdK] * ADMM_M3(V, 2, c)));
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) { ((LdsDk *)sLm + tid)[c * kChunkLdK] = U[c]; ((LdsDk *)sLm + tid)[(9 + c) * kChunkLdK] = N[c]; }
        const double w2 = v.t_sc[t] / v.dt2;
        const Mat mt = v.mats[v.t_mat[t]];
        double cf[12];      // -vol {d sg / d mu, d sg / d la, d sg / d kappa, sg}
        {
            double sg[3], dsg[9];
            tet_param_grad<TABLE>(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, v.spl + (size_t)(TABLE && grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles,
                                  S, sg, dsg);
            const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
#pragma unroll
            for (int q = 0; q < 9; ++q) cf[q] = -vol * dsg[q];
#pragma unroll
            for (int i = 0; i < 3; ++i) cf[9 + i] = -vol * sg[i];
        }
        if (!ln.valid) return;      // (behind the last wave vote)
#pragma unroll
        for (int c = 0; c < 9; ++c) { U[c] = ((LdsDk *)sLm + tid)[c * kChunkLdK]; N[c] = ((LdsDk *)sLm + tid)[(9 + c) * kChunkLdK]; }
        const int vid[4] = {id.x, id.y, id.z, id.w};
        const size_t ld = (size_t)v.ldt;
#pragma unroll 1
        for (int j = 0; j < sa.k; ++j) {
            double Ds[9], d[3];
            tet_edge_matrix(sa.a + (size_t)j * sa.sa, vid, Ds);
#pragma unroll
            for (int i = 0; i < 3; ++i) {      // A^_ii = sum_r U(r, i) (sum_m Ds(r, m) N(m, i))
                double s = 0.0;
#pragma unroll
                for (int r = 2; r >= 0; --r) {
                    const double tr = fma(Ds[r], ADMM_M3(N, 0, i), fma(Ds[3 + r], ADMM_M3(N, 1, i), Ds[6 + r] * ADMM_M3(N, 2, i)));
                    s = r == 2 ? ADMM_M3(U, 2, i) * tr : fma(ADMM_M3(U, r, i), tr, s);
                }
                d[i] = s;
            }
            double *o = sa.o_t + (size_t)j * 4 * ld + t;
#pragma unroll
            for (int p = 0; p < 4; ++p) o[p * ld] = fma(cf[3 * p], d[0], fma(cf[3 * p + 1], d[1], cf[3 * p + 2] * d[2]));
        }
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t >= v.ntri) return;
        const int4 id = v.r_idx[t];
        double R[4], F[6], G[6];
#pragma unroll
        for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
        tri_F(R, id, v.x, F);
        const double w2 = v.r_sc[t] / v.dt2;
        // G = -P = -w^2 (F - Q), Q the closest isometry: the text of k_forces
        const double c00 = dot3(F, F), c01 = dot3(F, F + 3), c11 = dot3(F + 3, F + 3);
        double cr[3];
        cross3(F, F + 3, cr);
        const double s = sqrt(dot3(cr, cr)), q = sqrt(c00 + c11 + 2.0 * s), iq = 1.0 / (q * s);
        const double i00 = (c11 + s) * iq, i01 = -c01 * iq, i11 = (c00 + s) * iq;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double q0 = fma(F[j], i00, F[3 + j] * i01), q1 = fma(F[j], i01, F[3 + j] * i11);
            G[j] = -w2 * (F[j] - q0); G[3 + j] = -w2 * (F[3 + j] - q1);
        }
#pragma unroll 1
        for (int j = 0; j < sa.k; ++j) {      // sum_c a_c . f_c = G : (D_i a)
            double dF[6];
            tri_F(R, id, sa.a + (size_t)j * sa.sa, dF);
            double o = G[5] * dF[5];
#pragma unroll
            for (int c = 4; c >= 0; --c) o = fma(G[c], dF[c], o);
            sa.o_r[(size_t)j * v.ldr + t] = o;
        }
    } else {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t >= v.nbend) return;
        int vid[4];
        double c[4], Dx[3], ks;
        hinge_load(v, t, c, vid, ks);
        hinge_Dx(c, vid, v.x, Dx);
#pragma unroll 1
        for (int j = 0; j < sa.k; ++j) {      // sum_k a_k . (-ks c_k D_i x) = -ks (D_i x) . (D_i a)
            double Da[3];
            hinge_Dx(c, vid, sa.a + (size_t)j * sa.sa, Da);
            sa.o_h[(size_t)j * v.ldb + t] = -ks * fma(Dx[0], Da[0], fma(Dx[1], Da[1], Dx[2] * Da[2]));
        }
    }
}

// a^T df/dX per rest vertex, X the rest positions behind the tets, for a stack of k <= kSensCols vectors a (masses and material
// constants held fixed).  k_tangent's text with another 3x3 per column: the SVD, tet_energy_grad's sg and tet_tangent_coef run ONCE per
// tet; per column A = Ds(a) Binv, Gs (device_math.hpp: tet_rest_grad), the corner contributions Gs Binv^T (tet_corner_forces) and the
// chunk's way out into records, which k_gather_tangent (shift 0) sums per vertex in list order.  The whole block reaches every barrier:
// a lane past its model's end redoes the last tet and parks zeros; the trip count sa.k is block-uniform.  Tets only: a context with
// triangles or hinges is refused by the caller (their rest positions never reach the library).  No atomics; a column's arithmetic does
// not depend on k.
struct RestArgs {
    ForceArgs f;              // the scene at x and the chunk plan; rec: column 0
    const double *a;          // [k][sa] the multiplier vectors
    size_t sa, srec;          // doubles between two of them, between two columns' records
    int k;
};
template <bool TABLE>
__global__ __launch_bounds__(256) void k_rest_sens(RestArgs ra) {
    __shared__ double sLm[21 * kChunkLdK];      // rows 0..11: the chunk's corner contributions of one column; rows 12..20: Binv
    const ForceArgs &a = ra.f;
    const ElemView &v = a.v;
    const int chunk = xcd_block(), tid = (int)threadIdx.x;
    if (chunk >= a.nb_t) return;
    LdsDk *sL = (LdsDk *)sLm;
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
        for (int c = 0; c < 9; ++c) sBi[c * kChunkLdK] = Bi[c];      // parked in this thread's LDS column for all the columns
        signed_svd3(F, U, S, V);
    }
    const double *tab = v.spl + (size_t)(TABLE && grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles;
    double sg[3], Hs[6], ca[3], cb[3];
    (void)tet_energy_grad(grp, (!TABLE && grp == 4 && mt.type == 3) ? 0 : mt.type, mt.mu, mt.la, mt.k, mt.kappa, tab, S, sg);
    {
        double al[3], be[3];
        tet_tangent_coef<TABLE>(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, tab, S, Hs, al, be);
#pragma unroll
        for (int q = 0; q < 3; ++q) { ca[q] = 0.5 * (al[q] + be[q]); cb[q] = 0.5 * (al[q] - be[q]); }
    }
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
#pragma unroll 1
    for (int j = 0; j < ra.k; ++j) {
        double G[9], f[12];
        {
            double Ds[9], dF[9];
            tet_edge_matrix(ra.a + (size_t)j * ra.sa, vid, Ds);
#pragma unroll
            for (int r = 0; r < 3; ++r) {      // A = Ds(a) Binv, Binv from LDS
                const double b0 = sBi[(r * 3 + 0) * kChunkLdK], b1 = sBi[(r * 3 + 1) * kChunkLdK], b2 = sBi[(r * 3 + 2) * kChunkLdK];
#pragma unroll
                for (int i = 0; i < 3; ++i) dF[r * 3 + i] = fma(Ds[i], b0, fma(Ds[3 + i], b1, Ds[6 + i] * b2));
            }
            tet_rest_grad(U, V, S, sg, Hs, ca, cb, dF, vol, G);
        }
        tet_corner_forces(G, sBi, f);
        if (!ln.valid) {
#pragma unroll
            for (int c = 0; c < 12; ++c) f[c] = 0.0;
        }
        if (j > 0) __syncthreads();      // the previous column's reduction has read rows 0..11
        chunk_out_store(co, sL, f, a.rec + (size_t)j * ra.srec);
    }
}

// dL/dx of the held vertices: out = g - K lam on held rows with g = Lx + Lv / dt unmasked (Lv may be nullptr), 0 on free rows;
// Kl = K(x) lam, the exact tangent without the mass shift
__global__ __launch_bounds__(256) void k_adj_held(int nv, const double *__restrict__ Lx, const double *__restrict__ Lv, double idt, const int *__restrict__ pin,
                                                  const double *__restrict__ Kl, double *__restrict__ out) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    const bool held = pin[v] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t i = 3 * (size_t)v + j;
        const double g = Lv ? fma(idt, Lv[i], Lx[i]) : Lx[i];
        out[i] = held ? g - Kl[i] : 0.0;
    }
}

// g_x = Lx + Lv / dt, rows of held vertices zero (Lv may be nullptr)
__global__ __launch_bounds__(256) void k_adj_rhs(int nv, const double *__restrict__ Lx, const double *__restrict__ Lv, double idt, const int *__restrict__ pin,
                                                 double *__restrict__ g) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    const bool held = pin[v] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t i = 3 * (size_t)v + j;
        g[i] = held ? 0.0 : Lv ? fma(idt, Lv[i], Lx[i]) : Lx[i];
    }
}
// out [4][3 nv]: dL/dx_bar = m o lam / dt^2, dL/dx_prev = dL/dx_bar - Lv / dt (held rows 0), dL/dv_prev = m o lam / dt,
// dL/dm = -lam o (x - x_bar) / dt^2 with x_bar = Mxbar / m; lam is 0 on held rows
__global__ __launch_bounds__(256) void k_adj_out(int nv, size_t n3, const double *__restrict__ lam, const double *__restrict__ m, const double *__restrict__ Mxbar,
                                                 const double *__restrict__ x, const double *__restrict__ Lv, double idt, const int *__restrict__ pin,
                                                 double *__restrict__ out) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    const bool held = pin[v] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t i = 3 * (size_t)v + j;
        const double l = held ? 0.0 : lam[i], ml = m[i] * l, xb = ml * idt * idt;
        out[i] = xb;
        out[n3 + i] = held ? 0.0 : Lv ? fma(-idt, Lv[i], xb) : xb;
        out[2 * n3 + i] = ml * idt;
        out[3 * n3 + i] = held ? 0.0 : -l * (x[i] - Mxbar[i] / m[i]) * idt * idt;
    }
}

} // namespace admm_k
