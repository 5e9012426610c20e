// tangent_coarse.hpp -- the BLOCKED dense inverse of the two-level tangent preconditioner (admm_hip_set_tangent_coarse, solver 1): the
// contract of device_math.hpp: tc_invert, rule for rule -- dropped columns, verdict 0 with X = 0, X symmetric to the bit -- spread over
// many workgroups in tiles of T x T = 64 x 64 doubles (32 KiB) held in LDS.  One launch per phase; the phases of n = 768 (nt = 12 tiles):
//   k_tcb_scan     1 block        the diagonal: dmax, the drop threshold, keep, ds = 1 / sqrt(a_ii), the dropped count, the VERDICT WORD
//   k_tcb_scale    grid           A <- ds A ds, a dropped row / column becomes the identity's
//   per tile step k (right-looking tiled Cholesky, in place in the lower triangle of A):
//     k_tcb_potrf  1 block        L_kk of the diagonal tile in LDS with the pivot test, and L_kk^-1 (a column per thread) -> Linv[k]
//     k_tcb_panel  nt - k - 1     L_ik = A_ik L_kk^-T, a tile product
//     k_tcb_update lower tiles    A_ij -= L_ik L_jk^T, k < j <= i
//   k_tcb_winv     nt x T / 16    W = L^-1 by independent strips of 16 columns: W_jj = L_jj^-1, W_ij = -L_ii^-1 sum_{j <= k < i} L_ik W_kj,
//                                 L's tiles streamed through LDS; a block reads only what it wrote itself
//   k_tcb_wtw      lower tiles    X_ij = sum_{k >= i} W_ki^T W_kj, mirrored into X_ji
//   k_tcb_unscale  grid           X <- ds (X + X^T) / 2 ds, zero in dropped rows / columns; a non-finite entry clears the verdict word
//   k_tcb_final    grid           verdict 0: X <- 0; block 0 reports the verdict
// 2 + 3 nt - 2 + 4 launches (40 at nt = 12).  X = W^T W in place of the two substitutions against the identity (LAPACK's potri): half
// the arithmetic, every tile independent, and the product is symmetric before it is symmetrised.
// EVERY kernel after the scan reads the verdict word and returns when it is 0; only k_tcb_final acts on it.  No block waits for another,
// no atomics, every loop bound is known at launch, every entry is summed in a fixed order: bit-reproducible.
// ONE text for the device and the host (tests/hostmath/tcb_invert_host.cpp), in the (tid, nt, sync) phase style of tc_invert: a routine
// below is ONE BLOCK of one launch; what an item carries from one phase to the next lives in memory (LDS or its own entries of the
// output), so one host thread can walk the items of every phase in order.  LDS tiles are K-MAJOR: tile[m * ld + r] with m the summed
// index, so the 4 x 4 entries of an item read two contiguous quadruples per m (the transposing loads pay for it with conflicting stores).
#pragma once
#include "device_math.hpp"

namespace admm_dev {

#ifndef ADMM_TCB_TILE
#define ADMM_TCB_TILE 64      // (the host build of the tests compiles a second tile size: the results agree to rounding)
#endif
constexpr int kTcbT = ADMM_TCB_TILE, kTcbStrip = 16, kTcbQ = kTcbT / 4;      // tile; columns of a strip of k_tcb_winv; 4 x 4 items along a tile side
constexpr int kTcbItems = kTcbQ * kTcbQ, kTcbStripItems = kTcbQ * kTcbStrip;      // items of a tile product (256 = the block); of a strip product (256)
static_assert(kTcbT % kTcbStrip == 0 && kTcbT >= 16, "a tile is whole strips of 4 x 4 items");
__host__ __device__ inline int tcb_tiles(int n) { return (n + kTcbT - 1) / kTcbT; }
__device__ __forceinline__ int tcb_rows(int n, int t) { const int r = n - t * kTcbT; return r < kTcbT ? r : kTcbT; }      // rows of tile row t

// dst[m * T + r] = src[r * ld + m] (r < nr, m < nm; 0 elsewhere): the TRANSPOSE of a row-major tile, k-major when m is its column
// (global reads coalesced along m; the LDS stores of a wave then have a stride of T doubles and fall on one bank -- 16 serialised stores
// per thread and tile, inside the measured times; the reads of tcb_mac are the conflict-free side)
__device__ __forceinline__ void tcb_load_t(double *dst, const double *src, size_t ld, int nr, int nm, int tid, int nt) {
    for (int e = tid; e < kTcbT * kTcbT; e += nt) {
        const int r = e / kTcbT, m = e - r * kTcbT;
        dst[m * kTcbT + r] = r < nr && m < nm ? src[r * ld + m] : 0.0;
    }
}
// dst[m * ldd + c] = src[m * ld + c] (m < nm, c < ncol; 0 elsewhere), m < T, c < ldd
__device__ __forceinline__ void tcb_load_d(double *dst, int ldd, const double *src, size_t ld, int nm, int ncol, int tid, int nt) {
    for (int e = tid; e < kTcbT * ldd; e += nt) {
        const int m = e / ldd, c = e - m * ldd;
        dst[e] = m < nm && c < ncol ? src[m * ld + c] : 0.0;
    }
}
// acc[a][b] += sum_{m < kk} At[m][ra + a] Bt[m][cb + b], m ascending
template <int RA, int RB>
__device__ __forceinline__ void tcb_mac(double (&acc)[RA][RB], const double *At, int lda, const double *Bt, int ldb, int kk, int ra, int cb) {
#pragma unroll 4
    for (int m = 0; m < kk; ++m) {      // (unrolled further, the loads of a whole tile are hoisted and the strip product spills)
        double a[RA], b[RB];
#pragma unroll
        for (int i = 0; i < RA; ++i) a[i] = At[m * lda + ra + i];
#pragma unroll
        for (int j = 0; j < RB; ++j) b[j] = Bt[m * ldb + cb + j];
#pragma unroll
        for (int i = 0; i < RA; ++i)
#pragma unroll
            for (int j = 0; j < RB; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
}

// the diagonal scan of tc_invert (one block): *flag = 1, or 0 for a diagonal that is not finite or below -kTcDrop dmax.  The threads
// share the diagonal and combine pairwise (nt a power of two): a maximum, a count and a conjunction do not depend on the order.
// rd, ri: LDS [nt] each.
template <class Sync>
__device__ __forceinline__ void tcb_scan(int n, const double *A, double *ds, int *keep, int *flag, int *dropped, double *rd, int *ri, int tid, int nt, Sync sync) {
    const size_t ld = (size_t)n;
    int ok = 1;
    double dmax = 0.0;
    for (int i = tid; i < n; i += nt) { const double d = A[i * ld + i]; ok = ok && modal_finite(d); dmax = d > dmax ? d : dmax; }
    rd[tid] = dmax; ri[tid] = ok;
    sync();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        if (tid < s) { rd[tid] = rd[tid + s] > rd[tid] ? rd[tid + s] : rd[tid]; ri[tid] = ri[tid] && ri[tid + s]; }
        sync();
    }
    dmax = rd[0]; ok = ri[0];
    sync();
    const double thr = kTcDrop * dmax;
    int nd = 0;
    for (int i = tid; i < n; i += nt) {
        const double d = A[i * ld + i];
        nd += d <= thr ? 1 : 0; ok = ok && d >= -thr;
        keep[i] = d > thr ? 1 : 0; ds[i] = d > thr ? 1.0 / sqrt(d) : 0.0;
    }
    rd[tid] = (double)nd; ri[tid] = ok;      // (a count below 2^53: exact)
    sync();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        if (tid < s) { rd[tid] += rd[tid + s]; ri[tid] = ri[tid] && ri[tid + s]; }
        sync();
    }
    if (tid == 0) { *dropped = (int)rd[0]; *flag = ri[0] ? 1 : 0; }
}
// A <- ds A ds in place (an entry depends on itself, ds and keep only); block blk of nblk
__device__ __forceinline__ void tcb_scale(int n, double *A, const double *ds, const int *keep, const int *flag, int blk, int nblk, int tid, int nt) {
    if (*flag == 0) return;
    const size_t ld = (size_t)n;
    for (size_t e = (size_t)blk * nt + tid; e < ld * ld; e += (size_t)nblk * nt) {
        const int i = (int)(e / ld), j = (int)(e - i * ld);
        A[e] = keep[i] && keep[j] ? (A[e] * ds[i]) * ds[j] : (i == j ? 1.0 : 0.0);
    }
}
// tile step k, one block: the diagonal tile A_kk -> L_kk (lower triangle, in place) and L_kk^-1 -> Linv[k] (T x T, zero above the
// diagonal and in the padding).  A pivot below 16 n eps or not finite clears the verdict word.  S, Y: LDS [T T] each; the column of
// the step and the pivots' roots live in Y until the inverse is formed there.
template <class Sync>
__device__ __forceinline__ void tcb_potrf(int n, int k, double *A, double *Linv, int *flag, double *S, double *Y, int tid, int nt, Sync sync) {
    if (*flag == 0) return;
    constexpr int T = kTcbT;
    const size_t ld = (size_t)n;
    const int r0 = k * T, tk = tcb_rows(n, k);
    const int W = nt >= 64 ? 64 : 1, tx = tid % W, ty = tid / W, ny = nt / W;
    double *At = A + (size_t)r0 * ld + r0, *col = Y, *dl = Y + T;
    for (int e = tid; e < T * T; e += nt) {
        const int i = e / T, j = e - i * T;
        S[e] = i < tk && j < tk ? At[i * ld + j] : 0.0;
    }
    sync();
    const double pivot_min = 16.0 * n * 2.220446049250313e-16;
    bool ok = true;
    for (int j = 0; j < tk; ++j) {
        const double d = S[j * T + j];      // (no item of this step writes a pivot: every thread reads the same one)
        if (!(d >= pivot_min) || !modal_finite(d)) { ok = false; break; }
        const double l = sqrt(d);
        for (int i = j + tid; i < tk; i += nt) {
            if (i == j) dl[j] = l;
            else { const double v = S[i * T + j] / l; S[i * T + j] = v; col[i] = v; }
        }
        sync();
        for (int i = j + 1 + ty; i < tk && ty < ny; i += ny) {
            const double lij = col[i];
            for (int c = j + 1 + tx; c <= i; c += W) S[i * T + c] = fma(-lij, col[c], S[i * T + c]);
        }
        sync();
    }
    if (!ok) {      // (uniform: every thread saw the same pivot)
        if (tid == 0) *flag = 0;
        return;
    }
    for (int i = tid; i < tk; i += nt) S[i * T + i] = dl[i];
    sync();
    for (int e = tid; e < T * T; e += nt) Y[e] = 0.0;
    sync();
    for (int c = tid; c < tk; c += nt) {      // column c of L_kk^-1 by forward substitution: no thread reads another's column.  (The
        for (int i = c; i < tk; ++i) {       // column-oriented form of the same sums, updates in place in Y, was slower: 189 us a tile against 115)
            double s = i == c ? 1.0 : 0.0;
            for (int m = c; m < i; ++m) s = fma(-S[i * T + m], Y[m * T + c], s);
            Y[i * T + c] = s / S[i * T + i];
        }
    }
    sync();
    for (int e = tid; e < T * T; e += nt) {
        const int i = e / T, j = e - i * T;
        if (i < tk && j <= i) At[i * ld + j] = S[e];
        Linv[(size_t)k * T * T + e] = Y[e];
    }
}
// tile step k, the block of tile row i > k: L_ik = A_ik L_kk^-T in place.  Ta, Tb: LDS [T T] each.
template <class Sync>
__device__ __forceinline__ void tcb_panel(int n, int k, int i, double *A, const double *Linv, const int *flag, double *Ta, double *Tb, int tid, int nt, Sync sync) {
    if (*flag == 0) return;
    constexpr int T = kTcbT;
    const size_t ld = (size_t)n;
    const int ri = tcb_rows(n, i);
    double *Aik = A + (size_t)i * T * ld + (size_t)k * T;
    tcb_load_t(Ta, Aik, ld, ri, T, tid, nt);                                   // Ta[m][r] = A_ik[r][m]
    tcb_load_t(Tb, Linv + (size_t)k * T * T, (size_t)T, T, T, tid, nt);      // Tb[m][c] = L_kk^-1[c][m]
    sync();
    for (int it = tid; it < kTcbItems; it += nt) {
        const int ra = 4 * (it / kTcbQ), cb = 4 * (it % kTcbQ);
        double acc[4][4] = {};
        tcb_mac<4, 4>(acc, Ta, T, Tb, T, T, ra, cb);
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                if (ra + a < ri) Aik[(ra + a) * ld + cb + b] = acc[a][b];
    }
}
// tile step k, the block of the tile (i, j), k < j <= i: A_ij -= L_ik L_jk^T in place
template <class Sync>
__device__ __forceinline__ void tcb_update(int n, int k, int i, int j, double *A, const int *flag, double *Ta, double *Tb, int tid, int nt, Sync sync) {
    if (*flag == 0) return;
    constexpr int T = kTcbT;
    const size_t ld = (size_t)n;
    const int ri = tcb_rows(n, i), rj = tcb_rows(n, j);
    tcb_load_t(Ta, A + (size_t)i * T * ld + (size_t)k * T, ld, ri, T, tid, nt);
    tcb_load_t(Tb, A + (size_t)j * T * ld + (size_t)k * T, ld, rj, T, tid, nt);
    sync();
    double *Aij = A + (size_t)i * T * ld + (size_t)j * T;
    for (int it = tid; it < kTcbItems; it += nt) {
        const int ra = 4 * (it / kTcbQ), cb = 4 * (it % kTcbQ);
        double acc[4][4] = {};
        tcb_mac<4, 4>(acc, Ta, T, Tb, T, T, ra, cb);
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                if (ra + a < ri && cb + b < rj) Aij[(ra + a) * ld + cb + b] -= acc[a][b];
    }
}
// the block of strip s of tile column j of W = L^-1 (columns j T + 16 s ..).  Ta: LDS [T T]; Ws, Sg: LDS [T 16] each (the strip of
// W_kj; the sum over k of tile row i, which the items carry from phase to phase).  Wm [n][n]: only the lower tiles are written.
template <class Sync>
__device__ __forceinline__ void tcb_winv(int n, int j, int s, const double *A, const double *Linv, double *Wm, const int *flag, double *Ta, double *Ws, double *Sg,
                                         int tid, int nt, Sync sync) {
    if (*flag == 0) return;
    constexpr int T = kTcbT, SW = kTcbStrip;
    const size_t ld = (size_t)n;
    const int ntile = tcb_tiles(n), c0 = j * T + s * SW;
    if (c0 >= n) return;
    const int cw = n - c0 < SW ? n - c0 : SW, rj = tcb_rows(n, j);
    for (int e = tid; e < T * SW; e += nt) {
        const int r = e / SW, c = e - r * SW;
        if (r < rj && c < cw) Wm[(size_t)(j * T + r) * ld + c0 + c] = Linv[(size_t)j * T * T + r * T + s * SW + c];
    }
    sync();
    for (int i = j + 1; i < ntile; ++i) {
        const int ri = tcb_rows(n, i);
        for (int k = j; k < i; ++k) {
            tcb_load_t(Ta, A + (size_t)i * T * ld + (size_t)k * T, ld, ri, T, tid, nt);       // Ta[m][r] = L_ik[r][m]
            tcb_load_d(Ws, SW, Wm + (size_t)k * T * ld + c0, ld, T, cw, tid, nt);              // Ws[m][c] = W_kj[m][c] of the strip
            sync();
            for (int it = tid; it < kTcbStripItems; it += nt) {
                const int ra = 4 * (it / SW), cb = it % SW;
                double acc[4][1];
                for (int a = 0; a < 4; ++a) acc[a][0] = k == j ? 0.0 : Sg[(ra + a) * SW + cb];
                tcb_mac<4, 1>(acc, Ta, T, Ws, SW, T, ra, cb);
                for (int a = 0; a < 4; ++a) Sg[(ra + a) * SW + cb] = acc[a][0];
            }
            sync();
        }
        tcb_load_t(Ta, Linv + (size_t)i * T * T, (size_t)T, T, T, tid, nt);      // Ta[m][r] = L_ii^-1[r][m]
        sync();
        for (int it = tid; it < kTcbStripItems; it += nt) {
            const int ra = 4 * (it / SW), cb = it % SW;
            double acc[4][1] = {};
            tcb_mac<4, 1>(acc, Ta, T, Sg, SW, T, ra, cb);
            for (int a = 0; a < 4; ++a)
                if (ra + a < ri && cb < cw) Wm[(size_t)(i * T + ra + a) * ld + c0 + cb] = -acc[a][0];
        }
        sync();
    }
}
// the block of the tile (i, j), j <= i, of X = W^T W: X_ij = sum_{k >= i} W_ki^T W_kj (an item carries its sum in its own entries of
// X), mirrored into X_ji after the last k
template <class Sync>
__device__ __forceinline__ void tcb_wtw(int n, int i, int j, const double *Wm, double *X, const int *flag, double *Ta, double *Tb, int tid, int nt, Sync sync) {
    if (*flag == 0) return;
    constexpr int T = kTcbT;
    const size_t ld = (size_t)n;
    const int ntile = tcb_tiles(n), ri = tcb_rows(n, i), rj = tcb_rows(n, j);
    for (int k = i; k < ntile; ++k) {
        const int rk = tcb_rows(n, k);
        tcb_load_d(Ta, T, Wm + (size_t)k * T * ld + (size_t)i * T, ld, rk, ri, tid, nt);      // Ta[m][r] = W_ki[m][r]
        tcb_load_d(Tb, T, Wm + (size_t)k * T * ld + (size_t)j * T, ld, rk, rj, tid, nt);
        sync();
        for (int it = tid; it < kTcbItems; it += nt) {
            const int ra = 4 * (it / kTcbQ), cb = 4 * (it % kTcbQ);
            double acc[4][4];
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = k > i && ra + a < ri && cb + b < rj ? X[(size_t)(i * T + ra + a) * ld + j * T + cb + b] : 0.0;
            tcb_mac<4, 4>(acc, Ta, T, Tb, T, rk, ra, cb);
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b)
                    if (ra + a < ri && cb + b < rj) {
                        X[(size_t)(i * T + ra + a) * ld + j * T + cb + b] = acc[a][b];
                        if (k == ntile - 1 && i != j) X[(size_t)(j * T + cb + b) * ld + i * T + ra + a] = acc[a][b];
                    }
        }
        sync();
    }
}
// X <- ds (X + X^T) / 2 ds, zero in the dropped rows and columns (tc_invert's last sweep); a non-finite entry clears the verdict word
__device__ __forceinline__ void tcb_unscale(int n, double *X, const double *ds, const int *keep, int *flag, int blk, int nblk, int tid, int nt) {
    if (*flag == 0) return;
    const size_t ld = (size_t)n;
    bool fin = true;
    for (size_t e = (size_t)blk * nt + tid; e < ld * ld; e += (size_t)nblk * nt) {
        const int i = (int)(e / ld), j = (int)(e - i * ld);
        if (i > j) continue;
        const double h = keep[i] && keep[j] ? (0.5 * (X[i * ld + j] + X[j * ld + i]) * ds[i]) * ds[j] : 0.0;
        fin = fin && modal_finite(h);
        X[i * ld + j] = h; X[j * ld + i] = h;
    }
    if (!fin) *flag = 0;      // (every writer stores 0.  A block of this launch that starts later may read the 0 on entry and return
                              // early, leaving its part of X unscaled: harmless, k_tcb_final zeroes all of X on a verdict of 0)
}
// verdict 0: X <- 0.  Block 0 reports the verdict in *ok.
__device__ __forceinline__ void tcb_final(int n, double *X, const int *flag, int *ok, int blk, int nblk, int tid, int nt) {
    const int v = *flag != 0 ? 1 : 0;
    if (blk == 0 && tid == 0) *ok = v;
    if (v) return;
    const size_t ld = (size_t)n;
    for (size_t e = (size_t)blk * nt + tid; e < ld * ld; e += (size_t)nblk * nt) X[e] = 0.0;
}
// the tile (i, j) of the t-th block over the lower triangle of m tile rows, row by row: t = i (i + 1) / 2 + j, j <= i < m
__device__ __forceinline__ void tcb_lower_tile(int t, int *i, int *j) {
    int r = 0;
    while (t > r) { t -= r + 1; ++r; }      // (r < m <= 12)
    *i = r; *j = t;
}

} // namespace admm_dev

#ifdef __HIPCC__
namespace admm_k {

struct TcbSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
// info: {coarse_ok, dropped columns}, as k_tc_invert's
__global__ __launch_bounds__(256) void k_tcb_scan(int n, const double *A, double *ds, int *keep, int *flag, int *info) {
    __shared__ double rd[256];
    __shared__ int ri[256];
    admm_dev::tcb_scan(n, A, ds, keep, flag, info + 1, rd, ri, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_scale(int n, double *A, const double *ds, const int *keep, const int *flag) {
    admm_dev::tcb_scale(n, A, ds, keep, flag, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, 256);
}
__global__ __launch_bounds__(256) void k_tcb_potrf(int n, int k, double *A, double *Linv, int *flag) {
    __shared__ double S[admm_dev::kTcbT * admm_dev::kTcbT], Y[admm_dev::kTcbT * admm_dev::kTcbT];
    admm_dev::tcb_potrf(n, k, A, Linv, flag, S, Y, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_panel(int n, int k, double *A, const double *Linv, const int *flag) {
    __shared__ double Ta[admm_dev::kTcbT * admm_dev::kTcbT], Tb[admm_dev::kTcbT * admm_dev::kTcbT];
    admm_dev::tcb_panel(n, k, k + 1 + (int)blockIdx.x, A, Linv, flag, Ta, Tb, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_update(int n, int k, double *A, const int *flag) {
    __shared__ double Ta[admm_dev::kTcbT * admm_dev::kTcbT], Tb[admm_dev::kTcbT * admm_dev::kTcbT];
    int i, j;
    admm_dev::tcb_lower_tile((int)blockIdx.x, &i, &j);
    admm_dev::tcb_update(n, k, k + 1 + i, k + 1 + j, A, flag, Ta, Tb, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_winv(int n, const double *A, const double *Linv, double *Wm, const int *flag) {
    __shared__ double Ta[admm_dev::kTcbT * admm_dev::kTcbT], Ws[admm_dev::kTcbT * admm_dev::kTcbStrip], Sg[admm_dev::kTcbT * admm_dev::kTcbStrip];
    admm_dev::tcb_winv(n, (int)blockIdx.x, (int)blockIdx.y, A, Linv, Wm, flag, Ta, Ws, Sg, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_wtw(int n, const double *Wm, double *X, const int *flag) {
    __shared__ double Ta[admm_dev::kTcbT * admm_dev::kTcbT], Tb[admm_dev::kTcbT * admm_dev::kTcbT];
    int i, j;
    admm_dev::tcb_lower_tile((int)blockIdx.x, &i, &j);
    admm_dev::tcb_wtw(n, i, j, Wm, X, flag, Ta, Tb, (int)threadIdx.x, 256, TcbSync());
}
__global__ __launch_bounds__(256) void k_tcb_unscale(int n, double *X, const double *ds, const int *keep, int *flag) {
    admm_dev::tcb_unscale(n, X, ds, keep, flag, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, 256);
}
__global__ __launch_bounds__(256) void k_tcb_final(int n, double *X, const int *flag, int *info) {
    admm_dev::tcb_final(n, X, flag, info, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, 256);
}

} // namespace admm_k
#endif
