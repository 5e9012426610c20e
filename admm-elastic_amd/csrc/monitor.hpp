// monitor.hpp -- energy and ADMM residuals of all energy terms, reduced on the device (included once by admm_hip.hip).
//
// What the library could not say before: how large the elastic energy is (EnergyTerm::energy, src/EnergyTerm.hpp:82,142-147;
// src/TetEnergyTerm.cpp:94-100,138-149; src/TriEnergyTerm.cpp:104-114) and how far an ADMM iteration is from its fixed point.  One
// kernel walks the families -- tets, triangles, bending hinges, pin terms, and (objective) the nodes -- in block ranges like
// k_local_tets_fused; a lane owns one element and reads it through elements.hpp (idx, Binv or the rest positions, sc = dt^2 w^2, mats,
// the spline tables) plus z and z_prev.  Per block and quantity one partial; k_mon_final sums the partials.
//
// Quantities (kMonQ = 8 per block partial and per record):
//   0  sum w_i^2 |D_i x - z_i|^2        2  sum w_i^2 |z_i|^2          4  energy of the tets       6  energy of the hinges
//   1  sum w_i^2 |z_i - zprev_i|^2      3  sum w_i^2 |D_i x|^2        5  energy of the triangles  7  sum_v m_v (x_v - xbar_v)^2
//
// REPRODUCIBLE to the bit from run to run: a lane adds its element's rows in a fixed order, the 64 lanes of a wave are summed by the
// xor butterfly (wave_sum), the four waves through LDS in wave order (block_sum), one thread stores the block's partials with ordinary
// vector stores, and the single block of k_mon_final has thread j add the partials j, j + 256, ... in index order before the same block
// sum.  No floating-point atomics anywhere: their arrival order would change the last bits between runs.
//
// z_prev is kept by WRITE-BACK: the residual pass stores z into z_prev after it has used both (INIT: stores D x, the reference's
// curr_z = D m_x of src/Solver.cpp:70).  The local step and its buffers stay as they are.
#pragma once
#include "elements.hpp"

namespace admm_k {

constexpr int kMonQ = 8;

// EARLY EXIT of the ADMM loop (admm_hip_set_admm_stop): does the record of an iteration meet tol?  rec = the record as admm_hip_get_monitor
// returns it: primal = |W(Dx - z)|, dz = |W(z - z_prev)|, wz = |W z|, wdx = |W D x| (the square roots of the sums 0..3 above).  The loop
// stops after an iteration when  primal <= tol max(wz, wdx)  and  dz <= tol wz.  In this product form with <=: no division, 0 <= 0 stops
// (a body at rest), a NaN anywhere never stops (every comparison with it is false), tol = 0 is "off" and never stops.  The ONE statement
// of the test: the decide kernel below and the host export admm_host_admm_stop_test both call it.
__host__ __device__ inline bool admm_stop_test(const double *rec, double tol) {
    if (!(tol > 0.0)) return false;
    const double primal = rec[0], dz = rec[1], wz = rec[2], wdx = rec[3];
    if (!(wz == wz && wdx == wdx)) return false;      // (max() below would drop a NaN on one side)
    const double big = wz > wdx ? wz : wdx;
    return primal <= tol * big && dz <= tol * wz;
}

struct MonArgs {
    ElemView v;               // the scene at x
    const double *t_z; double *t_zp;
    const double *r_z; double *r_zp;
    const double *h_sc, *h_z; double *h_zp;
    // pin terms: pin_dim rows per pin (3: the rows the device keeps; 6: the reference's row layout, rows 3..5 of D are empty)
    int npin, pin_dim; const int *pin_vert; const double *pin_z; double *pin_zp; double pin_w2;
    // nodes (inertia term of the objective); m == nullptr: none
    int n3; const double *m, *Mxbar;
    int nb_t, nb_r, nb_h, nb_p;      // block ranges: [0, nb_t) tets, [nb_t, nb_r) triangles, [nb_r, nb_h) hinges, [nb_h, nb_p) pins, then nodes
    double *part;             // [blocks][kMonQ]
    double *term;             // energy per element in device order [nt | ntri | nbend], or nullptr
    const int *stop;          // k_monitor<.., STOP = true> only: the stop word of the ADMM loop (kernels.hpp: kCntAdmmStop)
};

// one row of a term: adds to the four residual sums (without the weight, applied once per element)
__device__ __forceinline__ void mon_row(double dx, double z, double zp, double *r) {
    const double a = dx - z, b = z - zp;
    r[0] = fma(a, a, r[0]); r[1] = fma(b, b, r[1]); r[2] = fma(z, z, r[2]); r[3] = fma(dx, dx, r[3]);
}

// EnergyTerm::energy of tet t at F: its density (device_math.hpp: tet_energy_grad, the gradient discarded) times its volume
__device__ __forceinline__ double mon_tet_energy(const ElemView &a, int t, const double *F, double w2) {
    double U[9], S[3], V[9], sg[3];
    signed_svd3(F, U, S, V);
    const Mat mt = a.mats[a.t_mat[t]];
    const double vol = w2 / mt.k;      // w = sqrt(k vol), src/TetEnergyTerm.cpp:46-47
    const int grp = (t >= a.kb[1]) + (t >= a.kb[2]) + (t >= a.kb[3]) + (t >= a.kb[4]);
    const double psi = tet_energy_grad(grp, mt.type, mt.mu, mt.la, mt.k, mt.kappa, a.spl + (size_t)(grp == 4 && mt.type == 3 ? mt.table : 0) * kSplineTableDoubles, S, sg);
    return psi * vol;
}

// RES: the four residual sums, z_prev <- z.  ENERGY: the energies (+ the inertia sum when a.m is given).  INIT: z_prev <- D x only.
// STOP: an iteration of a step that skips on the device -- a set stop word makes the launch a no-op (nothing written: z_prev stays).
template <bool RES, bool ENERGY, bool INIT, bool STOP = false>
__global__ __launch_bounds__(256) void k_monitor(MonArgs a) {
    __shared__ double lds[4 * kMonQ];
    if (STOP && *a.stop) return;
    const ElemView &v = a.v;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    double q[kMonQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (blk < a.nb_t) {
        // every lane of the block computes (signed_svd3 takes wave-uniform decisions): lanes past the end redo the last tet and add nothing
        const int t0 = blk * 256 + tid;
        const bool valid = t0 < v.nt;
        const int t = valid ? t0 : v.nt - 1;
        double F[9], Bi[9];
        tet_F_binv(v, v.t_idx[t], t, F, Bi);
        const double w2 = v.t_sc[t] / v.dt2;
        if (INIT && valid) {
#pragma unroll
            for (int c = 0; c < 9; ++c) a.t_zp[(size_t)c * v.ldt + t] = F[c];
        }
        if (RES && valid) {
            double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double z = a.t_z[(size_t)c * v.ldt + t];
                mon_row(F[c], z, a.t_zp[(size_t)c * v.ldt + t], r);
                a.t_zp[(size_t)c * v.ldt + t] = z;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = w2 * r[i];
        }
        if (ENERGY) {
            const double e = mon_tet_energy(v, t, F, w2);
            if (valid) { q[4] = e; if (a.term) a.term[t] = e; }
        }
    } else if (blk < a.nb_r) {
        const int t = (blk - a.nb_t) * 256 + tid;
        if (t < v.ntri) {
            double R[4], F[6];
#pragma unroll
            for (int c = 0; c < 4; ++c) R[c] = v.r_rest[(size_t)c * v.ldr + t];
            tri_F(R, v.r_idx[t], v.x, F);
            const double w2 = v.r_sc[t] / v.dt2;
            if (INIT) {
#pragma unroll
                for (int c = 0; c < 6; ++c) a.r_zp[(size_t)c * v.ldr + t] = F[c];
            }
            if (RES) {
                double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double z = a.r_z[(size_t)c * v.ldr + t];
                    mon_row(F[c], z, a.r_zp[(size_t)c * v.ldr + t], r);
                    a.r_zp[(size_t)c * v.ldr + t] = z;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = w2 * r[i];
            }
            if (ENERGY) {
                // src/TriEnergyTerm.cpp:104-114: k / 2 area sum_{i<2} (sigma_i - 1)^2, strain limits ignored; k area = w^2.  The singular
                // values of the 3x2 F in closed form: sigma_1^2 = the larger eigenvalue of F^T F, sigma_1 sigma_2 = |f_0 x f_1|
                const double c00 = dot3(F, F), c01 = dot3(F, F + 3), c11 = dot3(F + 3, F + 3);
                double cr[3];
                cross3(F, F + 3, cr);
                const double d = c00 - c11, disc = sqrt(fma(d, d, 4.0 * c01 * c01));
                const double s1 = sqrt(0.5 * (c00 + c11 + disc));
                const double s2 = s1 > 0.0 ? sqrt(dot3(cr, cr)) / s1 : 0.0;
                const double e = 0.5 * w2 * ((s1 - 1.0) * (s1 - 1.0) + (s2 - 1.0) * (s2 - 1.0));
                q[5] = e;
                if (a.term) a.term[v.nt + t] = e;
            }
        }
    } else if (blk < a.nb_h) {
        const int t = (blk - a.nb_r) * 256 + tid;
        if (t < v.nbend) {
            const int4 id = v.h_idx[t];
            const int vid[4] = {id.x, id.y, id.z, id.w};
            double c[4], Dx[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = v.h_coef[(size_t)k * v.ldb + t];
            hinge_Dx(c, vid, v.x, Dx);
            if (INIT) {
#pragma unroll
                for (int j = 0; j < 3; ++j) a.h_zp[(size_t)j * v.ldb + t] = Dx[j];
            }
            if (RES) {
                const double w2 = a.h_sc[t] / v.dt2;
                double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double z = a.h_z[(size_t)j * v.ldb + t];
                    mon_row(Dx[j], z, a.h_zp[(size_t)j * v.ldb + t], r);
                    a.h_zp[(size_t)j * v.ldb + t] = z;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = w2 * r[i];
            }
            if (ENERGY) {
                const double e = 0.5 * v.h_k[t] * dot3(Dx, Dx);      // E = stiffness / 2 |D_i x|^2 (include/admm_hip.h: desc.bend_*)
                q[6] = e;
                if (a.term) a.term[v.nt + v.ntri + t] = e;
            }
        }
    } else if (blk < a.nb_p) {
        // SpringPin terms (src/SpringEnergyTerm.hpp:31-73): D-block I3 on the pinned vertex; no energy (the reference throws, :63-66)
        const int p = (blk - a.nb_h) * 256 + tid;
        if (p < a.npin && (RES || INIT)) {
            const double *xv = v.x + 3 * (size_t)a.pin_vert[p];
            double r[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < a.pin_dim; ++j) {
                const double dx = j < 3 ? xv[j] : 0.0;
                const size_t o = (size_t)p * a.pin_dim + j;
                if (INIT) a.pin_zp[o] = dx;
                if (RES) {
                    const double z = a.pin_z[o];
                    mon_row(dx, z, a.pin_zp[o], r);
                    a.pin_zp[o] = z;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = a.pin_w2 * r[i];
        }
    } else if (ENERGY && a.m) {
        // inertia term of the objective: sum m (x - x_bar)^2 with x_bar = M x_bar / m (src/Solver.cpp:65-66)
        const int i = (blk - a.nb_p) * 256 + tid;
        if (i < a.n3) {
            const double mi = a.m[i];
            if (mi > 0.0) {
                const double d = v.x[i] - a.Mxbar[i] / mi;
                q[7] = mi * d * d;
            }
        }
    }
    if (INIT) return;
    block_sum<kMonQ>(q, lds);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kMonQ; ++i) a.part[(size_t)blk * kMonQ + i] = q[i];
    }
}

// thread j adds the partials j, j + 256, ... in index order, then the block sum: q [kMonQ] holds the totals in thread 0
__device__ __forceinline__ void mon_sum_partials(const double *__restrict__ part, int nb, double *q, double *lds) {
#pragma unroll
    for (int i = 0; i < kMonQ; ++i) q[i] = 0.0;
    for (int b = (int)threadIdx.x; b < nb; b += 256) {
#pragma unroll
        for (int i = 0; i < kMonQ; ++i) q[i] += part[(size_t)b * kMonQ + i];
    }
    block_sum<kMonQ>(q, lds);
}

// the one block that sums the partials; out [kMonQ]
__global__ __launch_bounds__(256) void k_mon_final(const double *__restrict__ part, int nb, double *__restrict__ out) {
    __shared__ double lds[4 * kMonQ];
    double q[kMonQ];
    mon_sum_partials(part, nb, q, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMonQ; ++i) out[i] = q[i];
    }
}

// k_mon_final of a step with early exit (admm_hip_set_admm_stop): the same sum in the same order -- a record has the same bits with and
// without the feature -- then the decision on it.  s = the ADMM iteration.  A set stop word makes the launch a no-op like every other
// kernel of the loop.  Thread 0 writes, with ordinary vector stores: the executed count (cnt[kCntAdmmIters], sig[kSigAdmmIters]) and,
// when iteration s is the last, the stop word (cnt[kCntAdmmStop], sig[kSigAdmmStop]); sig is pinned host memory, for the host.
// veto (Anderson acceleration, anderson.hpp: AaCtl::mode of this iteration, written by the completed k_aa_solve; else nullptr): 2 = the
// evaluation was rejected -- its record is written, but it cannot end the step.
__global__ __launch_bounds__(256) void k_mon_decide(const double *__restrict__ part, int nb, double *__restrict__ out, double tol, int min_iters,
                                                    int s, int *__restrict__ cnt, int *__restrict__ sig, const int *__restrict__ veto) {
    __shared__ double lds[4 * kMonQ];
    if (cnt[kCntAdmmStop]) return;
    double q[kMonQ];
    mon_sum_partials(part, nb, q, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMonQ; ++i) out[i] = q[i];
        const double rec[4] = {sqrt(q[0]), sqrt(q[1]), sqrt(q[2]), sqrt(q[3])};      // (as admm_hip_get_monitor converts the sums)
        const bool stop = s + 1 >= min_iters && admm_stop_test(rec, tol) && !(veto && *veto == 2);
        cnt[kCntAdmmIters] = s + 1;
        __hip_atomic_store(sig + kSigAdmmIters, s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (stop) {
            cnt[kCntAdmmStop] = 1;
            __hip_atomic_store(sig + kSigAdmmStop, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

} // namespace admm_k
