// tangent_precond.hpp -- the TWO-LEVEL preconditioner of the tangent solves (admm_hip_set_tangent_precond): for the frozen tangent
// A = K(x) + shift M of newton.hpp
//     M^-1 = D^-1 + P (P^T A P)^-1 P^T,
// D = diag A (k_tangent_diag, unchanged) and P the affine DISPLACEMENTS of G compact aggregates of vertices (oc_plan.cpp: tangent_plan):
// 12 columns per aggregate g, phi_j(x_v) e_c with phi = {1, (x - mean_g) / h_g} at the CURRENT positions -- the x the tangent is frozen at,
// so the span holds the six rigid motions of the deformed aggregate -- and c in {x, y, z}; zero on held vertices and outside g.  Column
// 12 g + 3 j + c.  The matrix is the k_pcg2 / pcg_big.hpp preconditioner's; there the system matrix is constant and P^T A P is inverted
// once on the host, here it changes with x and is formed matrix-free, once per solve:
//   k_tc_basis            block = aggregate: mean and extent h (the largest side of the bounding box; 1 for a single point) of its current
//                         positions, then phi [nv][4] and the aggregate of every vertex
//   k_tc_fill             up to kModalNb columns of P into the direction block [n_vec][3 nv]; A P by the block pass of newton.hpp
//   k_tc_restrict_block   grid = aggregates x columns: the 12 entries (aggregate's rows, column) of P^T (A P), summed in agg_vert order
//   k_tc_sym              A_c <- (A_c + A_c^T) / 2
//   k_tc_invert           one block of 1024 threads, the matrix in global memory: device_math.hpp: tc_invert -- dropped columns, the verdict
//                         (or, with admm_hip_set_tangent_coarse(1), the k_tcb_ chain of tangent_coarse.hpp: the same contract in 64 x 64 tiles)
// and per CG iteration, behind the unchanged frozen pass on p and the unchanged k_nw_cg_step (alpha; y, r; partials of r . D^-1 r and r . r;
// z = D^-1 r + P y_c is not stored):
//   k_tc_restrict         block = aggregate: c = P^T r
//   k_tc_coarse           a wave per row: y_c = A_c^-1 c, and per block the partial of c . y_c
//   k_tc_cg_dir           r . z = r . D^-1 r + c . y_c (exact algebra: no second pass over r); beta; p = D^-1 r + P y_c + beta p; the
//                         verdict, the scalars and the stop word by the rules of k_nw_cg_dir (newton.hpp: WHO WRITES WHAT)
// A coarse matrix that is not positive definite (verdict 0: psd off at a compressed state; shift 0 on a body nothing holds) leaves
// A_c^-1 = 0: y_c = 0 and the iteration is Jacobi-PCG's, with no decision on the host.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no atomics, no grid barrier, nothing persistent.
#pragma once
#include "newton.hpp"

namespace admm_k {

constexpr int kTcMaxAgg = 64, kTcPer = 12;      // aggregates at most; columns per aggregate

// min and max over the block of three quantities (exact: the order does not matter); valid in all threads
__device__ __forceinline__ void tc_block_box(double *mn, double *mx, double *lds /* [24] */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[j] = fmin(mn[j], __shfl_xor(mn[j], o, 64)); mx[j] = fmax(mx[j], __shfl_xor(mx[j], o, 64)); }
        if (lane == 0) { lds[wv * 6 + j] = mn[j]; lds[wv * 6 + 3 + j] = mx[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        mn[j] = fmin(fmin(lds[j], lds[6 + j]), fmin(lds[12 + j], lds[18 + j]));
        mx[j] = fmax(fmax(lds[3 + j], lds[9 + j]), fmax(lds[15 + j], lds[21 + j]));
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_tc_basis(const int *__restrict__ agg_ptr, const int *__restrict__ agg_vert, const double *__restrict__ x,
                                                  const int *__restrict__ pin, double *__restrict__ phi, int *__restrict__ agg_of) {
    __shared__ double lds[24];
    const int g = blockIdx.x, lo = agg_ptr[g], hi = agg_ptr[g + 1];
    double q[3] = {0.0, 0.0, 0.0}, mn[3], mx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { mn[j] = 1.7976931348623157e308; mx[j] = -1.7976931348623157e308; }
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const size_t v = (size_t)agg_vert[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double xv = x[3 * v + j]; q[j] += xv; mn[j] = fmin(mn[j], xv); mx[j] = fmax(mx[j], xv); }
    }
    block_sum<3>(q, lds);
    tc_block_box(mn, mx, lds);
    double h = fmax(mx[0] - mn[0], fmax(mx[1] - mn[1], mx[2] - mn[2]));
    if (!(h > 0.0)) h = 1.0;
    const double cnt = (double)(hi - lo);
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const size_t v = (size_t)agg_vert[i];
        const bool held = pin && pin[v] != 0;
        phi[4 * v] = held ? 0.0 : 1.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) phi[4 * v + 1 + j] = held ? 0.0 : (x[3 * v + j] - q[j] / cnt) / h;
        agg_of[v] = g;
    }
}

// d_b = column col0 + b of P, b = blockIdx.y; d: [n_vec][3 nv]
__global__ __launch_bounds__(256) void k_tc_fill(int nv, int col0, size_t stride, const int *__restrict__ agg_of, const double *__restrict__ phi,
                                                 double *__restrict__ d) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= nv) return;
    const int col = col0 + (int)blockIdx.y, g = col / kTcPer, j = (col - g * kTcPer) / 3, cc = col - g * kTcPer - 3 * j;
    const double val = agg_of[v] == g ? phi[4 * (size_t)v + j] : 0.0;
    double *dv = d + (size_t)blockIdx.y * stride + 3 * (size_t)v;
#pragma unroll
    for (int k = 0; k < 3; ++k) dv[k] = k == cc ? val : 0.0;
}

// q[3 j + c] = sum over the aggregate's vertices, in agg_vert order, of phi_j(v) w[3 v + c]; valid in all threads
__device__ __forceinline__ void tc_restrict12(int lo, int hi, const int *__restrict__ agg_vert, const double *__restrict__ phi,
                                              const double *__restrict__ w, double *q, double *lds /* [48] */) {
#pragma unroll
    for (int i = 0; i < kTcPer; ++i) q[i] = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const size_t v = (size_t)agg_vert[i];
        double f[4], wv[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = phi[4 * v + j];
#pragma unroll
        for (int c = 0; c < 3; ++c) wv[c] = w[3 * v + c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) q[3 * j + c] = fma(f[j], wv[c], q[3 * j + c]);
    }
    block_sum<kTcPer>(q, lds);
}

// A_c[12 g + i][col0 + b] = (P^T (A P_b))_i for the aggregate g = blockIdx.x and the column b = blockIdx.y of the block pass
__global__ __launch_bounds__(256) void k_tc_restrict_block(int nc, int col0, size_t stride, const int *__restrict__ agg_ptr, const int *__restrict__ agg_vert,
                                                           const double *__restrict__ phi, const double *__restrict__ ap, double *__restrict__ Ac) {
    __shared__ double lds[4 * kTcPer];
    const int g = blockIdx.x;
    double q[kTcPer];
    tc_restrict12(agg_ptr[g], agg_ptr[g + 1], agg_vert, phi, ap + (size_t)blockIdx.y * stride, q, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kTcPer; ++i) Ac[(size_t)(kTcPer * g + i) * nc + col0 + (int)blockIdx.y] = q[i];
    }
}
__global__ __launch_bounds__(256) void k_tc_sym(int nc, const double *__restrict__ Ac, double *__restrict__ As) {
    const int e = blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= nc * nc) return;
    const int i = e / nc, j = e - i * nc;
    As[e] = 0.5 * (Ac[e] + Ac[(size_t)j * nc + i]);
}
// info: {coarse_ok, dropped columns}; As is destroyed
struct TcSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
__global__ __launch_bounds__(1024) void k_tc_invert(int nc, double *As, double *Ainv, double *ds, double *dl, double *col, int *keep, int *flag, int *info) {
    const int ok = admm_dev::tc_invert(nc, As, Ainv, ds, dl, col, keep, flag, info + 1, (int)threadIdx.x, 1024, TcSync());
    if (threadIdx.x == 0) info[0] = ok;
}

// y = 0, r = rhs on the free rows; partials of r . D^-1 r and r . r (k_nw_cg_init without p: it needs y_c)
__global__ __launch_bounds__(256) void k_tc_cg_init(int nv, int nb, const double *__restrict__ rhs, const int *__restrict__ pin, const double *__restrict__ dinv,
                                                    double *__restrict__ y, double *__restrict__ r, double *__restrict__ part) {
    __shared__ double lds[8];
    nw_cg_init_col<false>(nv, nb, rhs, pin, dinv, y, r, nullptr, part, lds);
}
// c = P^T r, block = aggregate
__global__ __launch_bounds__(256) void k_tc_restrict(const int *stop, const int *__restrict__ agg_ptr, const int *__restrict__ agg_vert,
                                                     const double *__restrict__ phi, const double *__restrict__ r, double *__restrict__ cvec) {
    __shared__ double lds[4 * kTcPer];
    if (*stop) return;
    const int g = blockIdx.x;
    double q[kTcPer];
    tc_restrict12(agg_ptr[g], agg_ptr[g + 1], agg_vert, phi, r, q, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kTcPer; ++i) cvec[kTcPer * g + i] = q[i];
    }
}
// y_c = A_c^-1 c: a wave per row, four rows per block (nc is a multiple of 12); cpart[block] = the block's share of c . y_c
__global__ __launch_bounds__(256) void k_tc_coarse(const int *stop, int nc, const double *__restrict__ Ainv, const double *__restrict__ cvec,
                                                   double *__restrict__ yc, double *__restrict__ cpart) {
    __shared__ double lds[4];
    if (*stop) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = blockIdx.x * 4 + wv;
    double s = 0.0;
    if (row < nc) {
        const double *a = Ainv + (size_t)row * nc;
        for (int k = lane; k < nc; k += 64) s = fma(a[k], cvec[k], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
        if (row < nc) yc[row] = s;
        lds[wv] = row < nc ? cvec[row] * s : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) cpart[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
// (P y_c) at vertex v, component c
__device__ __forceinline__ double tc_prolong(const double *__restrict__ phi, const double *__restrict__ yc, size_t v, int g, int c) {
    const double *f = phi + 4 * v, *y = yc + kTcPer * g + c;
    return fma(f[0], y[0], fma(f[1], y[3], fma(f[2], y[6], f[3] * y[9])));
}
// every block: r . z = r . D^-1 r + c . y_c and p = z = D^-1 r + P y_c; block 0: the scalars of iteration 0 and the stop word (k_nw_cg_init2)
__global__ __launch_bounds__(256) void k_tc_cg_init2(int nv, int nb, int ncb, const double *__restrict__ part, const double *__restrict__ cpart, NwCg *__restrict__ st,
                                                     int *__restrict__ stop, const double *__restrict__ dinv, const double *__restrict__ r,
                                                     const double *__restrict__ phi, const int *__restrict__ agg_of, const double *__restrict__ yc,
                                                     double *__restrict__ p) {
    __shared__ double lds[8];
    double q[2], cy[1];
    nw_reduce<2>(part + nb, nb, q, lds);
    nw_reduce<1>(cpart, ncb, cy, lds);
    const double rz = q[0] + cy[0];
    const int v = xcd_block() * 256 + (int)threadIdx.x;
    if (v < nv) {
        const int g = agg_of[v];
#pragma unroll
        for (int j = 0; j < 3; ++j) { const size_t i = 3 * (size_t)v + j; p[i] = fma(dinv[i], r[i], tc_prolong(phi, yc, (size_t)v, g, j)); }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *stop = nw_cg_start(rz, q[1], st).done;
}
// beta = r.z new / r.z old with r . z = r . D^-1 r + c . y_c; p = D^-1 r + P y_c + beta p; block 0 writes the scalars of iteration it + 1,
// the verdict and the stop word (k_nw_cg_dir).  After a breakdown in k_nw_cg_step, c and y_c are those of the unchanged r: not used.
__global__ __launch_bounds__(256) void k_tc_cg_dir(int it, int nv, int nb, int ncb, NwCg *st, int *stop, double tol2, int max_iters, const double *__restrict__ dinv,
                                                   const double *__restrict__ r, double *__restrict__ p, const double *__restrict__ part,
                                                   const double *__restrict__ cpart, const double *__restrict__ phi, const int *__restrict__ agg_of,
                                                   const double *__restrict__ yc) {
    __shared__ double lds[12];
    const NwCg s = st[it & 1];
    if (s.done || s.it != it) return;      // ended, or a launch behind the end: st[it & 1] is then the slot of iteration it - 2
    double q[3], cy[1];
    nw_reduce<3>(part, nb, q, lds);
    nw_reduce<1>(cpart, ncb, cy, lds);
    const double rz = q[1] + cy[0];
    const NwCg n = nw_cg_next(s, q[0], rz, q[2], tol2, max_iters);
    if (!n.done) {
        const double beta = rz / s.rz;
        const int v = xcd_block() * 256 + (int)threadIdx.x;
        if (v < nv) {
            const int g = agg_of[v];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t i = 3 * (size_t)v + j;
                p[i] = fma(beta, p[i], fma(dinv[i], r[i], tc_prolong(phi, yc, (size_t)v, g, j)));
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[(it + 1) & 1] = n; st[2] = n;
        if (n.done) *stop = 1;
    }
}

} // namespace admm_k
