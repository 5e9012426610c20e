// anderson.hpp -- Anderson acceleration of the fixed-point map of the ADMM iteration (Zhang, Peng, Ouyang, Deng 2019: "Accelerating ADMM
// for efficient simulation and optimization"), on the device.  Included once by admm_hip.hip, after newton.hpp.
//
// The state of the map is s = (x, u): curr [3 nv] and the multipliers t_u [9][ldt], r_u [6][ldr], h_u [3][ldb], pin_u [npin][3]; an
// iteration (local step, right-hand side, global solve) takes s_k to g_k = G(s_k), F_k = g_k - s_k.  The inner product is
// <a, b> = sum_v (m_v / dt^2) a_x b_x + sum_rows w^2 a_u b_u (sc = dt^2 w^2 of the row's term; the pin weight for pins); padding lanes
// of the SoA buffers enter no sum and are never written.  A history vector is the concatenation of the five buffers in their own layouts
// [N]; the ring holds S = window + 1 pairs (g_j, F_j) in FP64, slot by slot.
//
// Three launches per iteration, the same ones every iteration -- the host never waits:
//   k_aa_record  one pass over the state: F_k = g_k - s_k (g_k: the live buffers; s_k: the newest ring entry after a plain state, the copy
//                k_aa_apply left after an extrapolated one), g_k and F_k into the ring slot behind the head, and the block partials of
//                <F_k, F_k>, <dF_j, F_k> and <dF_new, dF_j> (dF_j = F_{j+1} - F_j over the entries that stay, dF_new = F_k - F_newest).
//   k_aa_solve   one block: the sums in a fixed order, the safeguard, the push, the new row of H (the older entries are kept, indexed
//                by ring slot), the regularised Cholesky solve (device_math.hpp: aa_small_solve), the record for the host.
//   k_aa_apply   one pass: s_{k+1} = g_k - sum_j theta_j (g_{j+1} - g_j) into the live buffers and the copy (mode 1), the newest accepted
//                g back into the live buffers after a rejection (mode 2), nothing after a plain evaluation (mode 0).
// WHO WRITES WHAT: AaCtl is written by k_aa_init (the step's start) and by thread 0 of k_aa_solve only, and read by later launches only
// (kernels.hpp: the rule of kCntAdmmStop); k_mon_decide reads AaCtl::mode so that a rejected evaluation cannot end the step.
//
// REPRODUCIBLE to the bit: fixed summation orders, ordinary vector stores, no floating-point atomics.
#pragma once
#include "newton.hpp"

namespace admm_k {

constexpr int kAaSlots = kAaMax + 1;         // ring slots at the largest window
constexpr int kAaQ = 1 + 2 * kAaMax;         // block partials: <F, F>; <dF_j, F> [kAaMax]; <dF_new, dF_j> [kAaMax]
constexpr int kAaRec = 4 + kAaMax;           // a record for the host: accepted, accelerated, entries, |F|^2, theta [kAaMax]

struct AaCtl {
    double r_acc;                            // |F|^2 of the last accepted evaluation (+inf at the start of a step)
    double H[kAaSlots * kAaSlots];           // <dF_a, dF_b>, a difference named by the ring slot of its newer entry
    double theta[kAaMax];
    int head, cnt;                           // the newest entry's slot, entries in the ring (oldest first: head - cnt + 1 .. head, mod S)
    int s_src;                               // where the next record phase finds s_k: a ring slot's g, or -1: the copy
    int accel;                               // s_k is an extrapolated state
    int mode;                                // this iteration's verdict for k_aa_apply: 0 plain, 1 extrapolate, 2 rejected
    int pad_[3];
};

// one family of the state: entry (e, c) lives at live[c stride_c + e stride_e], weight sc[e] wk (sc == nullptr: wk)
struct AaSeg { double *live; const double *sc; double wk; long long off; int n, nc, stride_c, stride_e, blk0, pad_; };
struct AaArgs {
    AaSeg seg[5];
    int nseg, nb, S, last;                   // families present, blocks, ring slots, k_aa_apply: the step's last iteration
    long long N;                             // doubles of a history vector
    double *hg, *hf, *scopy;                 // [S][N], [S][N], [N]
    AaCtl *ctl;
    double *part;                            // [kAaQ][nb]
    double *rec;                             // k_aa_solve: this iteration's record [kAaRec]
    const int *stop;                         // the stop word of the ADMM loop, or nullptr
};

__device__ __forceinline__ AaSeg aa_locate(const AaArgs &a, int blk) {
    int si = 0;
    for (int i = 1; i < a.nseg; ++i) if (blk >= a.seg[i].blk0) si = i;
    return a.seg[si];
}

// the step's start: the copy <- the live state (x_bar and u = 0), the ring empty
__global__ __launch_bounds__(256) void k_aa_init(AaArgs a) {
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    if (blk == 0 && tid == 0) {
        AaCtl *c = a.ctl;
        c->r_acc = __builtin_huge_val();
        c->head = 0; c->cnt = 0; c->s_src = -1; c->accel = 0; c->mode = 0;
    }
    const AaSeg sg = aa_locate(a, blk);
    const int e = (blk - sg.blk0) * 256 + tid;
    if (e >= sg.n) return;
    for (int c = 0; c < sg.nc; ++c) {
        const size_t li = (size_t)c * sg.stride_c + (size_t)e * sg.stride_e;
        a.scopy[sg.off + li] = sg.live[li];
    }
}

__global__ __launch_bounds__(256) void k_aa_record(AaArgs a) {
    __shared__ double lds[4 * kAaQ];
    if (a.stop && *a.stop) return;
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    const int S = a.S, head = a.ctl->head, cnt = a.ctl->cnt, ssrc = a.ctl->s_src;
    const int nold = cnt < S - 1 ? cnt : S - 1, slot = (head + 1) % S;      // entries that stay; where this evaluation goes
    const size_t N = (size_t)a.N;
    const AaSeg sg = aa_locate(a, blk);
    const int e = (blk - sg.blk0) * 256 + tid;
    double acc[kAaQ];
#pragma unroll
    for (int i = 0; i < kAaQ; ++i) acc[i] = 0.0;
    if (e < sg.n) {
        const double w = sg.sc ? sg.sc[e] * sg.wk : sg.wk;
        const double *sp = ssrc < 0 ? a.scopy : a.hg + (size_t)ssrc * N;
        const double *fo[kAaMax];
#pragma unroll
        for (int j = 0; j < kAaMax; ++j) fo[j] = a.hf + (size_t)((head - nold + 1 + j + 2 * S) % S) * N;
        double *gq = a.hg + (size_t)slot * N, *fq = a.hf + (size_t)slot * N;
#pragma unroll 1
        for (int c = 0; c < sg.nc; ++c) {
            const size_t li = (size_t)c * sg.stride_c + (size_t)e * sg.stride_e, idx = (size_t)sg.off + li;
            const double g = sg.live[li], F = g - sp[idx];
            double Fo[kAaMax], dF[kAaMax], dFn = 0.0;
#pragma unroll
            for (int j = 0; j < kAaMax; ++j) Fo[j] = j < nold ? fo[j][idx] : 0.0;
            gq[idx] = g; fq[idx] = F;
            acc[0] = fma(w * F, F, acc[0]);
#pragma unroll
            for (int j = 0; j < kAaMax; ++j) {
                const double nxt = (j + 1 < kAaMax && j + 1 < nold) ? Fo[j + 1 < kAaMax ? j + 1 : j] : F;
                dF[j] = j < nold ? nxt - Fo[j] : 0.0;
                if (j == nold - 1) dFn = dF[j];
            }
#pragma unroll
            for (int j = 0; j < kAaMax; ++j) {
                acc[1 + j] = fma(w * dF[j], F, acc[1 + j]);
                acc[1 + kAaMax + j] = fma(w * dFn, dF[j], acc[1 + kAaMax + j]);
            }
        }
    }
    block_sum<kAaQ>(acc, lds);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kAaQ; ++i) a.part[(size_t)i * a.nb + blk] = acc[i];
    }
}

// AaCtl travels through LDS: every thread fetches a part, thread 0 decides and solves on the LDS copy (its run-time-indexed arrays --
// H by slot, the small system, the factor -- would otherwise be serial round trips to memory), every thread stores a part back
constexpr int kAaCtlDoubles = (int)(sizeof(AaCtl) / sizeof(double));
static_assert(sizeof(AaCtl) % sizeof(double) == 0, "AaCtl is copied as doubles");
__global__ __launch_bounds__(256) void k_aa_solve(AaArgs a) {
    __shared__ double lds[4 * kAaQ];
    __shared__ double sctl[kAaCtlDoubles];
    __shared__ double sw[kAaMax * kAaMax + 2 * kAaMax + kAaWork];      // the small system, its right-hand side, theta, aa_small_solve's work
    if (a.stop && *a.stop) return;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kAaCtlDoubles; i += 256) sctl[i] = ((const double *)a.ctl)[i];
    // the partials in index order per quantity (thread j adds blocks j, j + 256, ...; then the block sum), the quantities of one block
    // fetched together: 17 independent loads per trip instead of 17 chains of dependent ones.  Quantities beyond the entries that stay
    // are zero and not read.
    const int nold0 = a.ctl->cnt < a.S - 1 ? a.ctl->cnt : a.S - 1;
    double q[kAaQ];
#pragma unroll
    for (int i = 0; i < kAaQ; ++i) q[i] = 0.0;
#pragma unroll 4
    for (int b = tid; b < a.nb; b += 256) {
#pragma unroll
        for (int i = 0; i < kAaQ; ++i)
            if (i == 0 || (i - 1) % kAaMax < nold0) q[i] += a.part[(size_t)i * a.nb + b];
    }
    block_sum<kAaQ>(q, lds);      // (its barriers also publish sctl)
    if (tid == 0) {
        AaCtl *c = (AaCtl *)sctl;
        const int S = a.S, head = c->head, cnt = c->cnt, accel = c->accel;
        const double FF = q[0];
        double rec[kAaRec];
#pragma unroll
        for (int i = 0; i < kAaRec; ++i) rec[i] = 0.0;
        rec[1] = accel; rec[3] = FF;
        if (accel && FF > c->r_acc) {      // the safeguard: back to the newest accepted g (still at the head), the ring empty, r_acc stays
            c->mode = 2; c->cnt = 0; c->s_src = head; c->accel = 0;
        } else {
            const int nold = cnt < S - 1 ? cnt : S - 1, slot = (head + 1) % S;
            // the differences, oldest first, named by the slot of their newer entry
            auto diff = [&](int j) { return j + 1 < nold ? (head - nold + 2 + j + 2 * S) % S : slot; };
            double *Hm = sw, *bq = sw + kAaMax * kAaMax, *th = bq + kAaMax, *work = th + kAaMax;
#pragma unroll
            for (int j = 0; j < kAaMax; ++j) {
                bq[j] = q[1 + j];
                if (j < nold) { const int dj = diff(j); c->H[slot * kAaSlots + dj] = q[1 + kAaMax + j]; c->H[dj * kAaSlots + slot] = q[1 + kAaMax + j]; }
            }
            c->r_acc = FF; c->head = slot; c->cnt = nold + 1; c->s_src = slot; c->accel = 0; c->mode = 0;
            rec[0] = 1.0; rec[2] = nold + 1;
            if (nold >= 1) {
                for (int i = 0; i < nold; ++i)
                    for (int j = 0; j < nold; ++j) Hm[i * kAaMax + j] = c->H[diff(i) * kAaSlots + diff(j)];
                if (aa_small_solve(nold, Hm, bq, th, work)) {
                    c->mode = 1; c->accel = 1; c->s_src = -1;
#pragma unroll
                    for (int j = 0; j < kAaMax; ++j) { c->theta[j] = th[j]; rec[4 + j] = th[j]; }
                } else { c->cnt = 0; rec[2] = 0.0; }      // (the ring is cleared; g_k stays where the next record phase reads s)
            }
        }
#pragma unroll
        for (int i = 0; i < kAaRec; ++i) a.rec[i] = rec[i];
    }
    __syncthreads();
    for (int i = tid; i < kAaCtlDoubles; i += 256) ((double *)a.ctl)[i] = sctl[i];
}

__global__ __launch_bounds__(256) void k_aa_apply(AaArgs a) {
    if (a.stop && *a.stop) return;
    const int mode = a.ctl->mode;
    if (mode == 0 || (mode == 1 && a.last)) return;      // (no extrapolation behind the step's last iteration)
    const int blk = xcd_block(), tid = (int)threadIdx.x;
    const int S = a.S, head = a.ctl->head, cnt = a.ctl->cnt;
    const size_t N = (size_t)a.N;
    const AaSeg sg = aa_locate(a, blk);
    const int e = (blk - sg.blk0) * 256 + tid;
    if (e >= sg.n) return;
    if (mode == 2) {
        const double *gh = a.hg + (size_t)head * N;
        for (int c = 0; c < sg.nc; ++c) {
            const size_t li = (size_t)c * sg.stride_c + (size_t)e * sg.stride_e;
            sg.live[li] = gh[sg.off + li];
        }
        return;
    }
    double th[kAaMax];
    const double *gp[kAaSlots];
#pragma unroll
    for (int j = 0; j < kAaMax; ++j) th[j] = a.ctl->theta[j];
#pragma unroll
    for (int j = 0; j < kAaSlots; ++j) gp[j] = a.hg + (size_t)((head - cnt + 1 + j + 2 * S) % S) * N;
#pragma unroll 1
    for (int c = 0; c < sg.nc; ++c) {
        const size_t li = (size_t)c * sg.stride_c + (size_t)e * sg.stride_e, idx = (size_t)sg.off + li;
        double G[kAaSlots];
#pragma unroll
        for (int j = 0; j < kAaSlots; ++j) G[j] = j < cnt ? gp[j][idx] : 0.0;
        double val = 0.0;
#pragma unroll
        for (int j = 0; j < kAaSlots; ++j) if (j == cnt - 1) val = G[j];
#pragma unroll
        for (int j = 0; j < kAaMax; ++j) if (j + 1 < cnt) val = fma(-th[j], G[j + 1] - G[j], val);
        sg.live[li] = val;
        a.scopy[idx] = val;
    }
}

} // namespace admm_k
