// modal.hpp -- the lowest eigenpairs of the frozen tangent on the device (admm_hip_modes): K_s phi = theta M phi on the free rows,
// K_s = K_frozen(x) [projected] + shift M, M = diag(m), by LOBPCG with the Jacobi preconditioner of tangent_solve.  Included once by
// admm_hip.hip, after newton.hpp.
//
// The block S = [X W P] (nb columns each, [3 nb][3 nv]) and AS = K_s S.  Per iteration `it`:
//   k_modal_resid    lane = vertex.  R = AX - (M X) Theta, block partials of |r_i|^2 and |M x_i|^2 per column, W = D^-1 R (held rows: 0).
//   k_tangent_frozen_block + k_newton_gather_block (newton.hpp) on W: AW.  AX and AP are carried by k_modal_update, not re-applied.
//   k_modal_gram     the upper triangles of S^T AS and S^T M S as per-block partials: a block walks its row tiles (64 rows of S and AS
//                    staged in LDS), a thread owns the pairs tid, tid + 256, ... of the triangle.  Plain FP64 fma: the kernel is bound
//                    by reading 2 m 3 nv doubles.
//   k_modal_rr       ONE block.  Sums the partials in block order; the stop test on columns 0 .. k-1, |r_i| <= tol |theta_i| |M x_i|;
//                    the dense Rayleigh-Ritz with its restart rule (device_math.hpp: modal_rr); writes Theta, C, the state of iteration
//                    it + 1 and the stop word.
//   k_modal_update   lane = row.  X <- S C, P <- [W P] C_WP, the same on AS; in place (a thread holds its row of S in registers).
// WHO WRITES WHAT (the rules of k_nw_cg_dir): the state st[(it + 1) & 1], its copy st[2] and the stop word are written by k_modal_rr(it)
// only and read by later launches only; k_modal_rr looks at st[it & 1] -- its .done and its iteration number, which tells a launch
// enqueued behind the end -- and k_modal_update(it) runs only when st[2] says that iteration it + 1 has begun.  mode 0 is the
// Rayleigh-Ritz on X alone (before the first and after the last iteration: it M-orthonormalises X), without stop word and state.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no floating-point atomics.
#pragma once
#include "newton.hpp"

namespace admm_k {

constexpr int kModalNb = 16;                                        // columns of X at most
constexpr int kModalCols = 3 * kModalNb;                            // == admm_dev::kModalMax
constexpr int kModalPairs = kModalCols * (kModalCols + 1) / 2;      // 1176
constexpr int kModalOwn = (kModalPairs + 255) / 256;                // pairs a thread of k_modal_gram owns at most
constexpr int kModalTile = 64;                                      // rows per LDS tile of k_modal_gram

struct ModalSt { int it, done, ended, restarts, has_p, nconv, used, pad_; };      // ended: 0 tol, 1 max_iters, 2 breakdown
struct ModalArgs {
    int nv, n3, nb, k;
    int nbk, nbg, tpb;        // vertex blocks; blocks of k_modal_gram and the row tiles each of them walks
    double *S, *AS;           // [3 nb][n3]: X, W, P
    const double *m, *dinv;   // [n3]
    double *theta;            // [nb]
    double *rpart;            // [2 nb][nbk]: partials of |r_i|^2, |M x_i|^2
    double *gpart;            // [nbg][2][kModalPairs]
    double *GA, *GM;          // [3 nb][3 nb], upper triangles
    double *C;                // [3 nb][nb]
    ModalSt *st;              // [4]: two slots, the copy the host reads, the verdict of a mode-0 Rayleigh-Ritz
    int *stop;
    double tol;
    int max_iters;
};

// X = the default start block (init == 0) or what the caller uploaded, held vertices zeroed
__global__ __launch_bounds__(256) void k_modal_start(ModalArgs a, const int *__restrict__ pin, int init) {
    const int v = blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= a.nv) return;
    const bool held = pin && pin[v] != 0;
    for (int c = 0; c < a.nb; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t i = (size_t)c * a.n3 + 3 * (size_t)v + j;
            a.S[i] = held ? 0.0 : init ? a.S[i] : admm_dev::modal_start((unsigned)c, (unsigned)v, (unsigned)j);
        }
}

// mode 1: an iteration's residual pass (returns on the stop word); mode 2: the true residuals of the returned X (W is left alone)
__global__ __launch_bounds__(256) void k_modal_resid(ModalArgs a, int mode) {
    __shared__ double lds[8];
    if (mode == 1 && *a.stop) return;
    const int blk = xcd_block(), v = blk * 256 + (int)threadIdx.x;
    for (int c = 0; c < a.nb; ++c) {
        const double th = a.theta[c];
        double q[2] = {0.0, 0.0};
        if (v < a.nv) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t r = 3 * (size_t)v + j, i = (size_t)c * a.n3 + r;
                const double mx = a.m[r] * a.S[i], res = fma(-mx, th, a.AS[i]);
                q[0] = fma(res, res, q[0]); q[1] = fma(mx, mx, q[1]);
                if (mode == 1) a.S[(size_t)a.nb * a.n3 + i] = a.dinv[r] * res;
            }
        }
        block_sum<2>(q, lds);
        if (threadIdx.x == 0) { a.rpart[(size_t)(2 * c) * a.nbk + blk] = q[0]; a.rpart[(size_t)(2 * c + 1) * a.nbk + blk] = q[1]; }
    }
}

// pair p of the upper triangle of an n x n matrix, row by row -> (i, j), i <= j
__device__ __forceinline__ void modal_pair_ij(int n, int p, int &i, int &j) {
    int row = 0, off = 0;
    while (row < n - 1 && p >= off + (n - row)) { off += n - row; ++row; }
    i = row; j = row + (p - off);
}
__global__ __launch_bounds__(256) void k_modal_gram(ModalArgs a, int mode) {
    __shared__ double sS[kModalCols * (kModalTile + 1)], sA[kModalCols * (kModalTile + 1)], sM[kModalTile];
    if (mode == 1 && *a.stop) return;
    const int tid = (int)threadIdx.x, blk = (int)blockIdx.x;
    const int mc = mode == 0 ? a.nb : 3 * a.nb, np = mc * (mc + 1) / 2;
    constexpr int ldt = kModalTile + 1;
    int pi[kModalOwn], pj[kModalOwn];
    double ga[kModalOwn], gm[kModalOwn];
#pragma unroll
    for (int q = 0; q < kModalOwn; ++q) {
        const int p = tid + 256 * q;
        pi[q] = 0; pj[q] = 0; ga[q] = 0.0; gm[q] = 0.0;
        if (p < np) modal_pair_ij(mc, p, pi[q], pj[q]);
    }
    for (int t = 0; t < a.tpb; ++t) {
        const size_t r0 = ((size_t)blk * a.tpb + t) * kModalTile;
        if (r0 >= (size_t)a.n3) break;      // (uniform)
        for (int e = tid; e < mc * kModalTile; e += 256) {
            const int c = e / kModalTile, r = e - c * kModalTile;
            const size_t row = r0 + r;
            const bool in = row < (size_t)a.n3;
            sS[c * ldt + r] = in ? a.S[(size_t)c * a.n3 + row] : 0.0;
            sA[c * ldt + r] = in ? a.AS[(size_t)c * a.n3 + row] : 0.0;
        }
        if (tid < kModalTile) sM[tid] = r0 + tid < (size_t)a.n3 ? a.m[r0 + tid] : 0.0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kModalOwn; ++q) {
            if (tid + 256 * q >= np) continue;
            const double *si = sS + pi[q] * ldt, *sj = sS + pj[q] * ldt, *aj = sA + pj[q] * ldt;
            double x = ga[q], y = gm[q];
            for (int r = 0; r < kModalTile; ++r) {
                x = fma(si[r], aj[r], x);
                y = fma(si[r] * sM[r], sj[r], y);
            }
            ga[q] = x; gm[q] = y;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kModalOwn; ++q) {
        const int p = tid + 256 * q;
        if (p < np) {
            a.gpart[((size_t)blk * 2 + 0) * kModalPairs + p] = ga[q];
            a.gpart[((size_t)blk * 2 + 1) * kModalPairs + p] = gm[q];
        }
    }
}

struct ModalSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

// ONE block.  mode 1: iteration `it`; mode 0: the Rayleigh-Ritz on X alone (init = 1: a failure ends the run before it begins)
__global__ __launch_bounds__(256) void k_modal_rr(ModalArgs a, int it, int mode, int init) {
    using namespace admm_dev;
    __shared__ double sA[kModalMax * kModalLd], sM[kModalMax * kModalLd], sQ[kModalMax * kModalLd];
    __shared__ double sds[kModalMax], sdl[kModalMax], sev[kModalMax], scs[kModalMax], sth[kModalNb], srs[2 * kModalNb];
    __shared__ int sperm[kModalMax], sok[2], srst[1];
    const int tid = (int)threadIdx.x, nb = a.nb, m3 = 3 * nb;
    ModalSt s{};
    if (mode == 1) {
        s = a.st[it & 1];
        if (s.done || s.it != it) return;      // ended, or a launch behind the end
    }
    const int mc = mode == 0 ? nb : 3 * nb;
    // the Gram matrices: the blocks' partials in block order
    for (int e = tid; e < mc * mc; e += 256) {
        const int i = e / mc, j = e - i * mc;
        if (i > j) continue;
        const int p = i * mc - (i * (i - 1)) / 2 + (j - i);
        double x = 0.0, y = 0.0;
        for (int b = 0; b < a.nbg; ++b) { x += a.gpart[((size_t)b * 2 + 0) * kModalPairs + p]; y += a.gpart[((size_t)b * 2 + 1) * kModalPairs + p]; }
        a.GA[i * m3 + j] = x; a.GM[i * m3 + j] = y;
    }
    ModalSt n = s;
    if (mode == 1) {
        if (tid < 2 * nb) {
            double x = 0.0;
            for (int b = 0; b < a.nbk; ++b) x += a.rpart[(size_t)tid * a.nbk + b];
            srs[tid] = x;
        }
        __syncthreads();
        int nconv = 0; bool fin = true;
        for (int c = 0; c < a.k; ++c) {
            const double th = a.theta[c], r2 = srs[2 * c], mx2 = srs[2 * c + 1];
            fin = fin && modal_finite(r2) && modal_finite(mx2);
            nconv += r2 <= (a.tol * a.tol) * (th * th) * mx2 ? 1 : 0;
        }
        n.nconv = nconv;
        if (!fin || nconv == a.k) {
            n.done = 1; n.ended = fin ? 0 : 2;
            if (tid == 0) { a.st[(it + 1) & 1] = n; a.st[2] = n; *a.stop = 1; }
            return;
        }
    }
    __syncthreads();
    const ModalWork w{sA, sM, sQ, sds, sdl, sev, scs, sperm, sok};
    const int m = mode == 0 ? nb : s.has_p ? 3 * nb : 2 * nb;
    const int used = modal_rr(nb, m, a.GA, a.GM, w, sth, a.C, srst, tid, 256, ModalSync());
    if (used && tid < nb) a.theta[tid] = sth[tid];
    if (mode == 0) {
        if (tid == 0) {
            ModalSt r{}; r.used = used;
            a.st[3] = r;
            if (init && !used) { n.done = 1; n.ended = 2; a.st[0] = n; a.st[2] = n; *a.stop = 1; }
        }
        return;
    }
    n.used = used;
    if (!used) { n.done = 1; n.ended = 2; }
    else {
        n.it = it + 1; n.has_p = 1; n.restarts = s.restarts + srst[0];
        if (n.it >= a.max_iters) { n.done = 1; n.ended = 1; }
    }
    if (tid == 0) { a.st[(it + 1) & 1] = n; a.st[2] = n; if (n.done) *a.stop = 1; }
}

// lane = row: X <- S C and (mode 1) P <- [W P] C_WP, on S and on AS, in place
__global__ __launch_bounds__(256) void k_modal_update(ModalArgs a, int it, int mode) {
    __shared__ double sC[kModalCols * kModalNb];
    if (mode == 1 ? a.st[2].it != it + 1 : a.st[3].used == 0) return;
    const int tid = (int)threadIdx.x, nb = a.nb, mc = mode == 0 ? nb : 3 * nb;
    for (int e = tid; e < mc * nb; e += 256) sC[e] = a.C[e];
    __syncthreads();
    const size_t row = (size_t)blockIdx.x * 256 + tid;
    if (row >= (size_t)a.n3) return;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        double *arr = pass == 0 ? a.S : a.AS;
        double v[kModalCols];
#pragma unroll
        for (int c = 0; c < kModalCols; ++c) v[c] = c < mc ? arr[(size_t)c * a.n3 + row] : 0.0;
#pragma unroll 1
        for (int i = 0; i < nb; ++i) {
            double x = 0.0, p = 0.0;
#pragma unroll
            for (int c = 0; c < kModalCols; ++c) {
                if (c >= mc) continue;
                const double cc = sC[c * nb + i];
                x = fma(v[c], cc, x);
                if (c >= nb) p = fma(v[c], cc, p);
            }
            arr[(size_t)i * a.n3 + row] = x;
            if (mode == 1) arr[(size_t)(2 * nb + i) * a.n3 + row] = p;
        }
    }
}

} // namespace admm_k
