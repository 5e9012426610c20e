// admm_hip.hip -- context, launch sequencing and the C ABI (include/admm_hip.h) of the MI355X-native
// ADMM elastic hot path.  gfx950 only.  Reference call stack being replaced: Solver::initialize
// (src/Solver.cpp:167-261) -> admm_hip_create, Solver::step (src/Solver.cpp:35-110) -> admm_hip_step.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>
#include <chrono>

#include "../../include/admm_hip.h"
#include "host_setup.hpp"
#include "kernels.hpp"
#include "monitor.hpp"
#include "forces.hpp"
#include "tangent.hpp"
#include "newton.hpp"
#include "adjoint.hpp"
#include "modal.hpp"
#include "tangent_precond.hpp"
#include "tangent_coarse.hpp"
#include "anderson.hpp"
#include "pcg_onchip2.hpp"
#include "pcg_big.hpp"
#include "gs_persist.hpp"
#include "uz_persist.hpp"

using namespace admm_k;
using admm_host::env_flag;
using admm_host::env_int;

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(ADMM_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

// live DevBuf allocations of the process (admm_hip_device_buffers)
std::atomic<int64_t> g_dev_buffers{0}, g_dev_bytes{0};

// One device allocation, owned: freed by the destructor, by release(), and by alloc() before it allocates again.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {      // (a failed allocation leaves the buffer empty)
        release();
        if (count == 0) return hipSuccess;
        T *q = nullptr;
        const hipError_t e = hipMalloc((void **)&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p = q; n = count;
        g_dev_buffers += 1; g_dev_bytes += (int64_t)(count * sizeof(T));
        return hipSuccess;
    }
    hipError_t upload(const std::vector<T> &h) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    // hipMemset runs on the NULL stream and may return before it has run; the contexts' streams are non-blocking and do not wait for
    // it, so the memset is waited for here (set-up paths only: nothing in a step calls this)
    hipError_t zero() {
        if (!n) return hipSuccess;
        const hipError_t e = hipMemset(p, 0, n * sizeof(T));
        return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
    }
    // Allocated (again) and zeroed ON THE STREAM THAT USES THE BUFFER (z_prev, the padding record / element the incidence lists point at).
    // Not zero(): its hipMemset on the NULL stream could land AFTER the work enqueued next on the non-blocking stream -- a z_prev <- D x
    // overwritten with zeros made dz of iteration 0 |W z|, off by 3e5 in test_monitor_matches_oracle_trace[cloth6], once in a few runs.
    hipError_t alloc_zeroed(size_t count, hipStream_t st) {
        const hipError_t e = alloc(count);
        return e != hipSuccess || !count ? e : hipMemsetAsync(p, 0, count * sizeof(T), st);
    }
    void release() {
        if (p) { (void)hipFree(p); g_dev_buffers -= 1; g_dev_bytes -= (int64_t)(n * sizeof(T)); }
        p = nullptr; n = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<int> >::value && !std::is_copy_assignable<DevBuf<int> >::value, "DevBuf owns its allocation");

struct SellDev {
    DevBuf<int> ptr, w, idx;
    DevBuf<double> val;
    int n_rows = 0, n_slices = 0;
    hipError_t upload(const admm_host::Sell &S) {
        n_rows = S.n_rows; n_slices = S.n_slices;
        hipError_t e;
        if ((e = ptr.upload(S.slice_ptr)) != hipSuccess) return e;
        if ((e = w.upload(S.slice_width)) != hipSuccess) return e;
        if ((e = idx.upload(S.idx)) != hipSuccess) return e;
        return val.upload(S.val);
    }
};

// RCCL is bound lazily (dlopen) so single-GPU use never loads it.
struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;          // (optional: admm_hip_comm_info)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    bool load() {
        if (h) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) return false;
        GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
        GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
        CommCount = (decltype(CommCount))dlsym(h, "ncclCommCount");
        CommUserRank = (decltype(CommUserRank))dlsym(h, "ncclCommUserRank");
        return GetUniqueId && CommInitRank && CommDestroy && AllReduce && GetErrorString;
    }
};
RcclApi g_rccl;

// Where a pass over the energy terms leaves what the vertex gather sums (elements.hpp: the write side), for `dirs` directions: records
// [dirs][n_rec + 1][4], corner rows [dirs][12][ldr] and [dirs][12][ldb]; no buffer for a family the scene lacks.  Zeroed: the lists' padding.
struct ElemScratch {
    DevBuf<double> rec, rcf, hcf;
    int dirs = 0;
    hipError_t ensure(admm_hip_ctx *c, int dirs);      // room for `dirs` directions; a call that failed is made again
};

} // namespace

struct admm_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_step0 = nullptr, ev_step1 = nullptr;
    hipEvent_t ev_coll0 = nullptr, ev_coll1 = nullptr;   // around Collider::detect (UzawaCG path), when stats are requested
    bool timing = false; double coll_ms_step = 0.0;
    // kernel-level timing of the tet local-step launches (device wall clock, kernels.hpp: ts_enter / ts_exit)
    DevBuf<unsigned long long> lk_ts, lk_out; int lk_tsn = 0, lk_launch = 0, lk_cap = 0; double lk_tick_ms = 0.0;
    std::vector<hipEvent_t> ev_phase; // 3 per ADMM iteration (+1) when stats are requested
    bool lt_on = false; std::vector<hipEvent_t> lt_ev; size_t lt_used = 0;   // admm_hip_time_local_launches: event pairs of the lean steps
    bool lt_taken = false;   // mode 2: a kernel of this ADMM iteration took the pair (a scene without elements leaves it unrecorded: the pair is then not counted)
    int lt_mode = 1; hipEvent_t lt_k0 = nullptr, lt_k1 = nullptr;   // mode 2: the pair is attached to the dominant local-step kernel's dispatch (hipExtLaunchKernelGGL)

    int nv = 0, n3 = 0;
    double dt = 1.0 / 24.0;
    int linsolver = 0;
    double constraint_w = 1.0;
    int pcg_max_iters = 500; double pcg_tol = 1e-10;
    int gs_max_iters = 30; double gs_tol = 1e-10, gs_omega = 1.9;
    int uz_max_iters = 20; double uz_tol = 1e-10;
    bool state_set = false;
    int rank = 0, world = 1;

    // multi-GPU (element-block partition, replicated global solve, RCCL all-reduce of the partial RHS)
    ncclComm_t comm = nullptr;
    admm_allreduce_fn ar_fn = nullptr; void *ar_user = nullptr; double *ar_host = nullptr;   // admm_hip_set_rhs_allreduce: the caller's own transport
    // DISTRIBUTED global solve (ADMM_HIP_DIST_SOLVE=1 with world_size > 1): rank r owns the vertex rows [row_lo, row_hi) of the PCG
    bool dist_solve = false; int row_lo = 0, row_hi = 0x7fffffff;
    int nt_total = 0, ntri_total = 0; // element counts of the whole scene (row layout of z/u)
    int tri_begin = 0;                // first triangle owned by this rank

    // COMPONENT-AWARE partition (admm_hip_create with world_size > 1 on a scene of >= world_size connected components, SURVEY 8e
    // "element / vertex blocks" taken at the one place a mesh cuts for free): this context then holds ONLY the bodies assigned to
    // its rank, renumbered locally, and steps them like a single-GPU scene -- no exchange inside a step, the solve is the block
    // of the block-diagonal Ahat that belongs to these bodies.  The caller's arrays keep the GLOBAL numbering; admm_hip_get_state
    // merges the ranks' parts over RCCL when a communicator was given (cm_comm; never used inside a step).
    struct CompMode { bool on = false; int rank = 0, world = 1; int nv_global = 0, n_components = 0; std::vector<int32_t> l2g, g2l; } cm;
    ncclComm_t cm_comm = nullptr; DevBuf<double> cm_buf;
    // node vectors
    DevBuf<double> x, v, m, Mxbar, curr, b, dinv;
    // tets (sorted by constitutive model; perm[new] = caller's index)
    int nt = 0, ldt = 0;
    int n_rec = 0;
    int kind_begin[6] = {0, 0, 0, 0, 0, 0}; // [linear | NH (+ NH spline) | StVK (+ StVK spline) | co-rotated spline | splines with kappa != 0 | end]
    std::vector<int> tet_perm;
    std::vector<int> tri_perm;        // device slot -> caller's triangle index (sorted like the tets: lowest vertex first)
    DevBuf<int4> t_idx;
    DevBuf<double> t_x0;      // rest positions [nv][3] when the tets' Binv is recomputed from them (tet_rest_mode != 0; t_Binv is then empty)
    int tet_rest_mode = 0;    // 0 streamed Binv, 1 rest positions = desc.vert_xyz, 2 rest positions propagated through the tets
    DevBuf<double> t_Binv, t_u, t_z, t_sc, t_rec;     // t_rec: per-chunk partial sums of the corner forces, [n_rec + 1][4]
    DevBuf<unsigned short> ch_ent; DevBuf<int> ch_group, ch_rec; int chunk_base[6] = {0, 0, 0, 0, 0, 0};   // host_setup.hpp: TetChunks
    DevBuf<int> t_mat;
    DevBuf<Mat> mats; DevBuf<double> spl_tab;   // tabulated user splines (ADMM_TET_SPLINE_TABLE)
    SellDev t_inc; DevBuf<int> g_order;   // incidence lists, and the vertex every row of them gathers for
    DevBuf<double> big_agree;     // distributed solve: the ranks' agreement on the solver (launch_pcg)
    bool defl_armed = false;      // launch_pcg2 armed the fused end projection for the solve just launched
    // tris
    int ntri = 0, ldr = 0;
    DevBuf<int4> r_idx;
    DevBuf<double> r_rest, r_u, r_z, r_sc, r_cf, r_lmin, r_lmax;
    SellDev r_inc;
    // bending hinges (desc.bend_*): SoA like the triangles, corner forces [12][ld], vertex incidence
    int nbend = 0, ldb = 0, nbend_total = 0, bend_begin = 0;
    std::vector<int> bend_perm;
    DevBuf<int4> h_idx; DevBuf<double> h_coef, h_u, h_z, h_sc, h_gam, h_cf; SellDev h_inc;
    // pins
    int npin_terms = 0;      // SpringPin energy terms (linsolver 0/2)
    std::vector<int> pin_vert_h; // creation-time pin vertices (terms), in term order
    DevBuf<int> vert_pin, pin_active;
    DevBuf<double> pin_xyz, pin_u, pin_z;
    double pin_weight = 0.0;
    // slide pins (desc.pin_normal): unit normals per pin term (linsolver 0 / 2) or per vertex (linsolver 1); zero = ordinary pin
    DevBuf<double> pin_nrm, gs_pin_nrm; std::vector<double> pin_nrm_h; bool has_slide = false;
    // in-sweep pins (linsolver 1)
    DevBuf<int> gs_pin_flag;
    DevBuf<double> gs_pin_xyz;
    bool gs_has_pins = false;
    // system matrix
    admm_host::Csr Ahat;
    SellDev A;
    int A_wmax = 4;
    DevBuf<int> csr_rowptr, csr_col;
    DevBuf<double> csr_val;
    // PCG work
    int NB = 1, NBV = 1;
    DevBuf<double> cg_r, cg_u, cg_w, cg_p, cg_s, part, part_b;
    DevBuf<CgScal> cg_scal;
    DevBuf<int> counters;         // kCntWords words (layout: kernels.hpp, kCnt*)
    // PCG launch control.  Iterations are launched in chunks of kChunk, one chunk speculatively ahead
    // of the GPU; the vec kernel signals convergence (kSigConverged) and progress
    // (kSigChunks) through pinned, device-mapped host memory, so the host stops
    // launching as soon as a solve has converged -- without ever synchronising the stream.
    int *h_sig = nullptr;         // pinned + mapped: kSigWords signal words (layout: kernels.hpp, kSig*)
    int *d_sig = nullptr;         // device alias of h_sig
    // on-chip PCG (pcg_onchip2.hpp): one persistent launch per solve when the system fits the chip
    bool oc_enabled = false;
    int oc_G = 0, oc_spb = 0, oc_T = 0; size_t oc_lds = 0;
    DevBuf<double> oc_ubuf, oc_part, oc_rc_part;
    DevBuf<unsigned> oc_bar;
    DevBuf<int> oc_nbr; DevBuf<unsigned long long> oc_flags;   // neighbour hand-off of the pipelined iteration
    DevBuf<unsigned long long> oc_prof;   // diagnosis (ADMM_HIP_OC_PROF=1)
    bool oc_debug = false, oc_always_verify = false; int oc_prof_block = 0;
    // k_pcg2 has a generic and a hot instance (pcg_onchip2.hpp); launch_pcg2 chooses per launch (pcg2_hot_ok)
    bool oc_force_generic = false;      // diagnosis (ADMM_HIP_OC_GENERIC=1): every launch takes the generic instance
    int oc_last_instance = 0;           // of the last main-stream launch: 0 none yet, 1 generic, 2 hot
    int64_t oc_instance_launches[4] = {0, 0, 0, 0};   // hot, generic, of these on column lanes: hot (never), generic
    // general-mesh plan of the on-chip PCG (oc_plan.cpp): internal row order, its SELL, slab shares, two-level data
    double oc_sm_ab = 0.0, oc_sm_b = 0.0, oc_lam_bb = 0.0;   // block-local smoother of k_pcg2 (pcg_onchip2.hpp: smooth)
    bool oc_plan = false, oc_coarse = false; int oc_rows = 0, oc_bcols = 0, oc_nc = 0, oc_ncp = 0, oc_veclen = 0;
    SellDev oc_A; DevBuf<int> oc_orig, oc_ldsoff, oc_wls, oc_haloptr, oc_halosrc, oc_halovert; DevBuf<unsigned short> oc_col16;
    DevBuf<double> oc_mdiag, oc_ainv, oc_cbuf; DevBuf<float> oc_cwt; bool oc_affine = false;
    const double *create_xyz = nullptr;   // desc.vert_xyz, valid during admm_hip_create only (coarse space of the plan)
    int64_t oc_stat[6] = {0, 0, 0, 0, 0, 0};   // nnz, stored, on chip, block-local, max neighbour blocks, coarse unknowns
    int oc_nbr_max = 0;   // most neighbour blocks of a block of the plan, -1: a block has more than 64 (no hand-off lists; admm_hip_pcg_plan_info)
    // Recovery from a grid barrier that cannot complete (the persistent PCG kernel needs all its blocks resident at once:
    // another persistent kernel, a second context or CU masking can break that).  The state at the last point known to be
    // good is kept, with the steps issued since; a timed-out barrier (detected at the next synchronisation) switches the
    // context to the launch-per-iteration PCG for good, restores that state and replays the steps.
    DevBuf<double> bk_x, bk_v, bk_y; int bk_prev_hits = -1, bk_prev_iters = 0; std::vector<std::pair<int, double> > pending; bool oc_gave_up = false;   // bk_y, bk_prev_*: UzawaCG's multipliers and the row count they belong to (kept across solves, UzawaCG.hpp:74)
    // WindForce on the device (admm_hip_set_wind): triangles, their vertex incidence, per-triangle forces
    int wind_n = 0; double wind_dir[3] = {0.0, 0.0, 0.0}; DevBuf<int> wind_tris; SellDev wind_inc; DevBuf<double> wind_force;
    DevBuf<unsigned long long> gs_proj; long long uz_rows_total = 0;   // admm_hip_contact_totals: rows projected inside the GS sweeps (device), rows of C over all UzawaCG solves (host)
    // launch-path two-level PCG (pcg_big.hpp): systems beyond the chip's LDS, and the fall-back of the on-chip kernel
    bool big_enabled = false, big_tried = false, big_allowed = true; int defl_start = 2; bool defl_start_hold = false; std::vector<double> xyz_h;
    int big_G = 0, big_ra = 0, big_rows = 0, big_nc = 0, big_ncp = 0, big_NBt = 0;
    SellDev big_A; DevBuf<int> big_orig; DevBuf<float> big_ainv;
    DevBuf<double> big_mass, big_dinv, big_cwt, big_xi, big_r, big_u, big_w, big_p, big_s, big_part, big_cvec, big_rho, big_dots; DevBuf<int> big_tick;
    long long big_solves = 0;
    int oc_dbg_sm_off = -1;        // ADMM_HIP_OC_DEBUG: last seen state of kCntSmootherOff (block smoother switched off for the context)
    bool defl_use_resid = true;    // launch_deflation after a launch-path solve: the solve's own final residual (ADMM_HIP_DEFL_RESID=0 at create: b - A x again)
    bool big_rfin_valid = false;   // c->cg_u holds D^-1 (final residual) of the launch-path solve that has just returned (launch_deflation)
    int big_its_hist[32] = {};    // iterations the launch-path solve at position s of the previous frame needed (first chunk of the next one)
    int big_row_lo = 0, big_row_hi = 0x7fffffff, big_nif = 0; DevBuf<int> big_if_rows; DevBuf<double> big_ifbuf;      // distributed solve: owned internal rows, interface rows
    // end projection of every PCG solve on soft modes (admm_hip_set_soft_modes; kernels.hpp: k_defl_*)
    int defl_k = 0; bool defl_fused = false; DevBuf<double> defl_Z, defl_Ginv, defl_part, defl_y, defl_rec; DevBuf<float> defl_Zint;
    std::vector<int32_t> oc_orig_h;      // internal row -> vertex of the on-chip plan (host copy: the soft modes are stored in that order for k_pcg2)
    long long oc_launches = 0, gsp_launches = 0;   // persistent launches since create (admm_hip_persistent_launches)
    bool kernel_clock = false;      // ADMM_HIP_KERNEL_CLOCK=1: wall-clock stamps of the local-step launches (step_impl)
    bool uz_lanes_debug = false;    // ADMM_HIP_UZ_LANES_DEBUG=1: the column lanes report on stderr
    int test_abort_seq = 0;   // tests only (ADMM_HIP_TEST_ABORT_SOLVE=k): the k-th on-chip solve of the context finds its barrier aborted
    int test_abort_uzp = 0;   // tests only (ADMM_HIP_TEST_ABORT_SCHUR=k): the k-th persistent Schur launch finds its hand-off given up
    int n_cus = 256;   // multiProcessorCount of the device (persistent kernels need all their blocks resident at once)
    int n3i = 0;   // length of the solver-internal scratch vectors (recycled pairs): max(n3, 3 * oc_rows)
    int solve_seq = 0;
    int marks_expected = 0;       // chunks closed so far (host count)
    int last_launched_iters = 0;
    // recycled warm start (k_rc_*): ring of kRc (correction, initial residual) pairs
    // The projection basis of solve s is the last kRc pairs of the frame, so the pairs live in a ring of kRc + 1 slots
    // (the slot being written is never one of the kRc being read): 2 (kRc + 1) node vectors, allocated only when the
    // recycled start is enabled.
    static constexpr int kRcSlots = kRc + 1;
    DevBuf<double> rc_buf, rc_r0, rc_xs, rc_part, rc_coef;
    int rc_iter = 0, rc_frame = 0, rc_prev_valid = 0, NBR = 1; // pairs of the previous frame valid for s < rc_prev_valid
    int rc_pairs = kRc; bool rc_decided = false; long long rc_snap[2] = {0, 0};   // pairs per projection: see step_impl
    bool rc_enabled = true;
    // Slots: the pairs of the FIRST kRc solves of a frame have slots of their own (0 .. kRc - 1), later solves share a ring of
    // kRcSlots behind them.  Slot j < kRc therefore keeps "the most recent pair of solve index j" across the frame boundary: when
    // solve s < kRc of the next frame starts, slots 0 .. s - 1 hold this frame's pairs and slots s .. kRc - 1 still the PREVIOUS
    // frame's -- which it projects on as well (launch_pcg_recycled).
    static constexpr int kRcAllSlots = kRc + kRcSlots;
    static int rc_slot(int s) { return s < kRc ? s : kRc + (s - kRc) % kRcSlots; }
    double *rc_E(int s) { return rc_buf.p + ((size_t)rc_slot(s) * 2 + 0) * (size_t)n3i; }
    double *rc_R(int s) { return rc_buf.p + ((size_t)rc_slot(s) * 2 + 1) * (size_t)n3i; }
    // FRAME HISTORY of the first kRcHist solves (round 4): their pairs are kept for three frames (slot by frame mod 3), so that solve s
    // of frame f projects on the pairs of the same (and the next) solve index of frames f - 1 AND f - 2 as well.  At the bench
    // tolerance the first five solves of a frame were 60 % of its PCG iterations (body: 31 56 25 43 25 of ~300); two frames of
    // history bring solves 2-4 to 10-12 (frame total ~225, -25 %; 2 123 -> 2 404 ADMM it/s same-box).  For later solves the frame's own
    // most recent pairs are worth more than any history (cube, history for all 20 solves: 556 -> 735 iterations per frame).
    // Round 6 measured history for MORE solves (8, 12, 20 solves) with three and four pairs: on the bench body 8.68 -> 7.32 iterations
    // per solve in the driver's window, 2 500 -> 2 660 ADMM it/s -- and the 200-frame drift goes from 3.2e-6 to 8.3e-6 (8 solves), 2.4e-5 (12),
    // 3.4e-5 (20): OVER the bar.  The history pairs are nearly the same from frame to frame, so what the projection leaves behind is the SAME
    // error every frame -- a bias that enters the velocity and accumulates, where the error of plain PCG iterations is spread over the spectrum.
    // At equal drift (tolerance tightened to 2-3e-10) the longer history is no faster (profiles/r06_history_sweep.txt).  Five stays.
    static constexpr int kRcHist = 5;
    static constexpr int kRcDepth = 3;      // frames the history keeps (this one included)
    int rc_hist = 0, rc_prev2_valid = 0;    // rc_hist: set by the plan (on-chip kernel with its plan), 0 after an aborted solve
    int rc_loc(int s, int frame) const { return (rc_hist && s < kRcHist) ? kRcAllSlots + ((frame % kRcDepth + kRcDepth) % kRcDepth) * kRcHist + s : rc_slot(s); }
    double *rc_Ef(int s, int frame) { return rc_buf.p + ((size_t)rc_loc(s, frame) * 2 + 0) * (size_t)n3i; }
    double *rc_Rf(int s, int frame) { return rc_buf.p + ((size_t)rc_loc(s, frame) * 2 + 1) * (size_t)n3i; }
    // UzawaCG (per-vertex constraint rows)
    DevBuf<double> uz_cn, uz_cc, uz_y, uz_r, uz_d, uz_q3, uz_q1, uz_q2, uz_part, uz_dmax; DevBuf<long long> uz_dacc;   // uz_dacc / uz_dmax: dyn_collide.hpp, k_uz_ct_dyn
    DevBuf<UzScal> uz_scal;
    int uz_prev_hits = -1, uz_last_hits = 0, NBU = 1, uz_iters_step = 0, uz_prev_iters = 0; bool uz_hits_cleared = false;
    // cached columns of K^-1 for the Schur iterations (kernels.hpp: k_uz_cols_apply).  uzc_slot_h[v] = column slot of vertex v or -1.
    bool uzc_on = false, uzc_usable = false;
    size_t uzc_cap = 0; int uzc_n = 0, uzc_n_act = 0;
    DevBuf<double> uzc_cols; DevBuf<int> uzc_slot, uzc_act, uzc_miss, uzc_info, uzc_counts; DevBuf<unsigned char> uzc_flag;
    int uzc_one_block_max = 4;      // active list by ONE block up to this many passes of 4096 vertices (ADMM_HIP_UZ_LIST_BLOCKS: tests)
    // the Schur CG on the active rows as one persistent launch (uz_persist.hpp)
    DevBuf<int> uzp_rowlist; int uzp_rowinfo[2] = {0, 0}; DevBuf<double> uzp_S;   // coupled (dynamic) rows: the row vertices and their Schur matrix
    DevBuf<uint4> uzp_dbox, uzp_sbox; DevBuf<unsigned> uzp_abort; bool uzp_enabled = true; unsigned uzp_seq = 0; long long uzp_launches = 0; int uzp_rows = 0;   // uzp_rows: 8 | 16 forced (ADMM_HIP_UZ_PERSIST_ROWS, tests)
    DevBuf<double> uzc_G, uzc_part, uzc_gq, uz_y0; DevBuf<int> uzc_pos;   // Schur iterations on the active vertices (kernels.hpp: k_uzc_*)
    int uzc_test_iters = 0;   // tests (ADMM_HIP_TEST_UZ_COL_ITERS=n): the column solves get n iterations, so they do not converge
    bool uzc_compact = true; int uzc_one_max = 1024, uzc_compact_max = 8192;   // (the limits are lowered by tests to reach the general paths on small scenes)
    std::vector<int> uzc_slot_h;
    // Column solves on side streams (uz_ensure_columns): on a small body k_pcg2 occupies a fraction of the chip (77 blocks at 20 k
    // vertices) and its iteration is bound by the grid barrier's latency, so several independent solves run side by side.  A lane owns
    // every buffer the kernel WRITES (published vector, partial sums, barrier words, hand-off flags, coarse sums, counters, b, x, u).
    struct OcLane {
        hipStream_t st = nullptr; hipEvent_t done = nullptr; int seq = 0;
        DevBuf<char> slab;      // one allocation per lane (hipMalloc costs ~0.3 ms: a lane is set up inside a frame)
        double *ubuf = nullptr, *part = nullptr, *cbuf = nullptr, *b = nullptr, *x = nullptr, *u = nullptr;
        unsigned *bar = nullptr; unsigned long long *flags = nullptr; CgScal *scal = nullptr; int *counters = nullptr;
        ~OcLane() {
            if (st) (void)hipStreamSynchronize(st);      // (look-ahead solves may still be in flight)
            if (done) (void)hipEventDestroy(done);
            if (st) (void)hipStreamDestroy(st);
        }
    };
    std::vector<std::unique_ptr<OcLane> > uz_lanes; hipEvent_t uz_fork = nullptr; int uz_lanes_cfg = -1;   // uz_lanes_cfg: ADMM_HIP_UZ_LANES (1 = the main stream only; default: what fits, <= 8)
    long long uzc_lane_batches = 0;
    // columns solved AHEAD of the contact (uz_ahead_launch): in flight on the lanes while the ADMM loop goes on, committed when they are done
    bool pf_on = false, in_step = false; double pf_frames = 0.0; int uz_fit = -1;
    DevBuf<int> pf_list; std::vector<int> pf_v, pf_slot; int pf_launched = 0, pf_lanes = 0;
    long long pf_batches = 0, pf_columns = 0, pf_waits = 0;
    long long uzc_col_solves = 0, uzc_applies = 0, uzc_pcg_solves = 0, uzc_evictions = 0, uzc_unconverged = 0;
    bool uz_freeze = false, uz_detected = false;   // tests (ADMM_HIP_UZ_FREEZE=1): Collider::detect only in the first ADMM iteration of a step
    // GS: the whole solve (colours x sweeps + residual tests, ~500 tiny launches) is captured once into a
    // hipGraph and replayed -- the per-colour kernels are far below the host launch rate
    hipGraphExec_t gs_exec = nullptr;
    const double *gs_graph_b = nullptr; double *gs_graph_x = nullptr;
    std::vector<int> color_h; int n_colors = 0;
    std::vector<int> color_ptr_h;
    DevBuf<int> color_nodes;
    SellDev gs_sell; DevBuf<int> gs_slot_node; DevBuf<double> gs_diag; std::vector<int> gs_color_slice;
    DevBuf<double> gs_xb, gs_part2;   // two-colour scheme (k_gs_color2): roll-back copy, partial sums
    DevBuf<unsigned char> gs_low; bool gs_fusedN = false;   // >= 3 colours: residual test fused into the colour kernels (k_gs_colorN)
    // persistent multi-colour GS (gs_persist.hpp): one launch per solve on the plan of oc_plan.cpp: build_gs_plan
    bool gsp_enabled = false; int gsp_G = 0, gsp_C = 0; size_t gsp_lds = 0; int64_t gsp_stat[6] = {0, 0, 0, 0, 0, 0};
    DevBuf<int> gsp_hdr, gsp_orig, gsp_out, gsp_hbox, gsp_horig; DevBuf<double> gsp_diag, gsp_vals; DevBuf<unsigned short> gsp_cols;
    DevBuf<uint4> gsp_box, gsp_part, gsp_meet; DevBuf<unsigned> gsp_abort; DevBuf<unsigned long long> gsp_prof; int gsp_prof_block = 0;
    Obstacles obst{}; DevBuf<Obstacles> obst_dev; DevBuf<double> obst_gmeta, obst_gdata;   // (sampled obstacles: ADMM_OBJ_GRID)
    // dynamic (self-)collision (dyn_collide.hpp): one entry per TetMeshCollision, payload arrays per vertex
    struct DynDev {
        DynMesh m{};
        DevBuf<int4> tet; DevBuf<int> tet_id, face, face_id; DevBuf<double> t_box, f_box, rest;
    };
    std::vector<std::unique_ptr<DynDev> > dyn;
    DevBuf<int> dyn_face, surf_list; DevBuf<double> dyn_bary, dyn_n, dyn_dx; DevBuf<unsigned char> surf_mask;
    int n_surf = 0;   // Solver::surface_inds (0 = every vertex is a collision candidate)
    // dynamic hits inside the multi-colour GS (per solve: hit list, touched rows, mask, residual partials)
    DevBuf<DynHit> gsd_hits; DevBuf<unsigned char> gsd_skip; DevBuf<double> gsd_part;
    DevBuf<int> gsd_int; DevBuf<double> gsd_dbl; DevBuf<int4> gsd_hnode;
    int gsd_last_hits = 0;
    // energy / ADMM monitor (monitor.hpp; admm_hip_energy, admm_hip_residuals, admm_hip_set_monitor).  h_kst, pin_vert_d: rest data only the
    // monitor reads (the hinges' stiffness, pin term -> vertex), uploaded at create; everything else is allocated by the first call that needs it
    int mon_mode = 0, mon_n = 0;      // mode in effect from the next step; records the last step wrote
    // early exit of the ADMM loop (admm_hip_set_admm_stop; monitor.hpp: admm_stop_test, k_mon_decide; kernels.hpp: kCntAdmmStop)
    double stop_tol = 0.0; int stop_min = 1;      // in effect from the next step; tol = 0: off
    int stop_last = 0, stop_on_dev = 0;           // the last step: iterations executed; 1 = the remaining ones were skipped on the device
    bool stop_host = false;                       // ADMM_HIP_STOP_HOST=1 (read at create): every path decides on the host
    const int *stop_dev = nullptr;                // while step_impl enqueues a step that skips on the device: the stop word -- the launch helpers
                                                  // then take the STOP instantiations (k_pcg2: the generic instance with Oc2Args::skip)
    hipEvent_t ev_stop = nullptr;                 // behind k_mon_decide, on the paths that decide on the host
    DevBuf<double> h_kst; DevBuf<int> pin_vert_d;
    DevBuf<double> mon_tzp, mon_rzp, mon_hzp, mon_pzp, mon_pz6;   // z_prev per family (pins: room for the reference's 6 rows), pin z in the reference's row layout
    DevBuf<double> mon_part, mon_rec, mon_out, mon_term;          // block partials, records [admm_iters][8], one result [8], per-term energies
    // internal forces / stress / stationarity (forces.hpp; admm_hip_forces, admm_hip_stress, monitor mode 3): buffers of their own, allocated
    // by the first call that needs them -- the step's t_rec, r_cf, h_cf are not borrowed
    ElemScratch f_el; DevBuf<double> f_out, f_stress, f_part, f_stat;      // f [3 nv], stress [13][ldt], block partials, sums [admm_iters]
    int mon_stat_n = 0;      // stationarity sums the last step wrote (mode 3), else 0
    // tangent stiffness (tangent.hpp; admm_hip_stiffness_apply): buffers of their own for k_el.dirs directions, allocated by the first call
    // and again by a call with more directions
    ElemScratch k_el; DevBuf<double> k_d, k_out;      // the directions and the result [k_el.dirs][3 nv]
    // frozen tangent, tangent_solve and newton_polish (newton.hpp): buffers of their own, allocated by the first call
    DevBuf<double> nw_tfr, nw_rfr; ElemScratch nw_el;      // the frames [30][ldt], [11][ldr]; the scratch of one direction
    DevBuf<double> nw_dinv, nw_y, nw_r, nw_p, nw_ap, nw_rhs, nw_part;      // [3 nv] each; block partials [3][blocks]
    DevBuf<NwCg> nw_st; DevBuf<int> nw_stop, nw_pin;      // the PCG's scalars [3], its stop word, the held vertices [nv]
    int *nw_hstop = nullptr;      // pinned: the stop word as the host reads it between chunks
    hipEvent_t nw_ev[2] = {nullptr, nullptr};
    bool nw_ready = false;
    // the frozen pass on a block of directions (newton.hpp: k_tangent_frozen_block; admm_hip_stiffness_apply_ex with ADMM_HIP_TANGENT_BLOCK,
    // admm_hip_modes): the scratch of up to kModalNb directions and the columns of a blocked stiffness_apply_ex, allocated by the first call
    ElemScratch bk_el; DevBuf<double> bk_d, bk_out;      // [n_vec][3 nv] each
    // block PCG (newton.hpp; admm_hip_tangent_solve_block, admm_hip_step_adjoint_block): buffers of their own for bp_cols <= kNwBlkCols
    // columns, allocated by the first call and again by a call with a wider slab -- never per call
    int bp_cols = 0;
    DevBuf<double> bp_rhs, bp_y, bp_r, bp_p, bp_ap, bp_part, bp_rr;      // [bp_cols][3 nv] five times; partials [bp_cols][3][blocks]; true residuals [kNwBlkCols]
    DevBuf<NwCg> bp_st; DevBuf<NwBlockCtl> bp_ctl;                       // the scalars [kNwBlkCols][3]; the column lists and counters
    DevBuf<double> adj_bl, adj_bout;                                     // the adjoint's stacks: Lx, Lv [2][bp_cols][3 nv]; the gradients [bp_cols][4][3 nv]
    // block eigensolver (modal.hpp; admm_hip_modes): buffers of their own, allocated by the first call
    DevBuf<double> md_S, md_AS, md_theta, md_rpart, md_gpart, md_GA, md_GM, md_C;
    DevBuf<ModalSt> md_st; int md_nbg = 0, md_tpb = 0;
    bool md_ready = false;
    // two-level preconditioner of the tangent solves (tangent_precond.hpp; admm_hip_set_tangent_precond): buffers of their own, allocated
    // by the first solve that runs with it (and again when the number of aggregates changes)
    int tc_kind = 0, tc_aggregates = 0;      // in effect from the next solve: 0 Jacobi, 1 two-level; aggregates wanted (0: n_verts / 256 in 1 .. 64)
    int tc_G = 0, tc_nc = 0, tc_ncb = 0;     // of the buffers: aggregates planned, 12 G, blocks of k_tc_coarse
    int tc_last_nc = 0, tc_last_passes = 0;  // the last solve: coarse dimension (0: Jacobi), block passes of its setup
    // the dense inverse behind it (admm_hip_set_tangent_coarse): 0 one block (k_tc_invert), 1 blocked over the chip (tangent_coarse.hpp), in
    // effect from the next solve; the launches of the last inverse; the blocked chain's scratch, allocated only when it is selected
    int tc_coarse_solver = 0, tc_last_launches = 0;
    DevBuf<double> tcb_W, tcb_Linv;          // [nc][nc]: L^-1; [ceil(nc / 64)][64][64]: the inverted diagonal tiles
    std::vector<double> tc_xyz_h;            // desc.vert_xyz (the aggregates are cut in the rest positions)
    DevBuf<int> tc_agg_ptr, tc_agg_vert, tc_agg_of, tc_keep, tc_info;      // [G + 1], [nv], [nv]; tc_invert's columns kept [nc]; {flag, coarse_ok, dropped}
    DevBuf<double> tc_phi, tc_d, tc_ad, tc_Ac, tc_As, tc_Ainv, tc_ds, tc_dl, tc_col, tc_c, tc_yc, tc_cpart;      // [nv][4]; [16][3 nv] twice; [nc][nc] three times; [nc] five times; [ncb]
    // adjoint of a step (adjoint.hpp; admm_hip_param_sensitivity, admm_hip_step_adjoint): buffers of their own, allocated by the first call
    DevBuf<double> adj_a, adj_ps, adj_l, adj_out;      // the stack [kSensCols][3 nv]; its sensitivities; Lx, Lv [2][3 nv]; the gradients [4][3 nv]
    bool adj_ready = false;
    // gradients in the rest shape and in the held vertices (adjoint.hpp: k_rest_sens, k_adj_held; admm_hip_rest_sensitivity,
    // admm_hip_adjoint_held): the records of up to kSensCols columns and their sums [rs_el.dirs][3 nv]; dL/dx of the held vertices [3 nv]
    ElemScratch rs_el; DevBuf<double> rs_out, adj_h;
    // Anderson acceleration of the ADMM loop (anderson.hpp; admm_hip_set_anderson): buffers of their own, allocated by the first step that
    // runs with a window, and again by a step with a larger one
    int aa_window = 0, aa_slots = 0, aa_n = 0;      // window in effect from the next step; ring slots allocated; records the last step wrote
    bool aa_on = false;                             // while step_impl enqueues an accelerated step
    DevBuf<double> aa_hg, aa_hf, aa_scopy, aa_part, aa_rec;      // the ring [slots][N] twice, the copy [N], block partials [kAaQ][blocks], records [admm_iters][kAaRec]
    DevBuf<AaCtl> aa_ctl;
    bool tri_limited = false;     // a triangle carries a strain limit that can act (min > 0 or max < 100)
    bool xbar_of_state = false;   // Mxbar is the last step's and x its result (no set_state since)

    ~admm_hip_ctx() {      // (every DevBuf member, lane and dynamic collider frees its own memory after this body)
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);      // nothing is freed under a kernel still in flight
        for (const std::unique_ptr<OcLane> &ln : uz_lanes) if (ln->st) (void)hipStreamSynchronize(ln->st);
        if (comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm);
        if (cm_comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(cm_comm);
        if (uz_fork) (void)hipEventDestroy(uz_fork);
        if (nw_hstop) (void)hipHostFree(nw_hstop);
        for (hipEvent_t e : nw_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_phase) (void)hipEventDestroy(e);
        for (hipEvent_t e : lt_ev) (void)hipEventDestroy(e);
        if (gs_exec) (void)hipGraphExecDestroy(gs_exec);
        if (h_sig) (void)hipHostFree(h_sig);
        if (ar_host) (void)hipHostFree(ar_host);
        if (ev_coll0) (void)hipEventDestroy(ev_coll0);
        if (ev_coll1) (void)hipEventDestroy(ev_coll1);
        if (ev_stop) (void)hipEventDestroy(ev_stop);
        if (ev_step0) (void)hipEventDestroy(ev_step0);
        if (ev_step1) (void)hipEventDestroy(ev_step1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

static int step_impl(admm_hip_ctx *c, int32_t admm_iters, double gravity, admm_hip_stats *stats);
static int recover_from_abort(admm_hip_ctx *c, admm_hip_stats *stats_of_last);
static int settle(admm_hip_ctx *c);

namespace {

inline int blocks_for(int n) { return (n + 255) / 256; }

SellA sell_arg(const SellDev &S) { return SellA{S.n_rows, S.n_slices, S.ptr.p, S.w.p, S.idx.p, S.val.p}; }

// ---- launch helpers (all on ctx->stream) -------------------------------------------------------------
template <bool WRITE_Z, bool REST, bool STOP = false>
void launch_local_impl(admm_hip_ctx *c) {
    hipStream_t st = c->stream;
    if (c->nt > 0) {
        const int b0 = c->kind_begin[0], b1 = c->kind_begin[1], b2 = c->kind_begin[2], b3 = c->kind_begin[3];
        TetArgs a{c->ldt, c->t_idx.p, c->t_Binv.p, c->t_u.p, c->t_z.p, c->t_sc.p, c->t_mat.p, c->mats.p, c->curr.p, c->t_x0.p,
                  c->ch_ent.p, c->ch_group.p, c->ch_rec.p, c->t_rec.p, 0, c->spl_tab.p, nullptr, 0, c->stop_dev};
        auto stamp = [&]() {   // the next launch gets its own pair of stamp arrays
            if (c->timing && c->lk_launch < c->lk_cap) { a.ts = c->lk_ts.p + (size_t)c->lk_launch * 2 * c->lk_tsn; a.ts_n = c->lk_tsn; c->lk_launch += 1; }
            else a.ts = nullptr;
        };
        const int b4 = c->kind_begin[4], b5 = c->kind_begin[5];
        const int kinds = (b1 > b0) + (b2 > b1) + (b3 > b2);
        // (measurement, admm_hip_time_local_launches(2): the event pair rides on ONE kernel's own dispatch -- the dominant one: the
        // launch over the linear / NH / StVK groups when the scene has any, else the co-rotated splines', else the dense-Hessian group's)
        const int dom = b3 > b0 ? 0 : b4 > b3 ? 3 : 4;
        if (b5 > b4) {    // SplineTet splines with a compression term, tabulated splines, stable Neo-Hookean: their own launch
            stamp(); a.chunk0 = c->chunk_base[4];
            if (dom == 4 && c->lt_k0) { hipExtLaunchKernelGGL((k_local_tets<4, WRITE_Z, REST, STOP>), dim3(blocks_for(b5 - b4)), dim3(256), 0, st, c->lt_k0, c->lt_k1, 0, b4, b5, a); c->lt_taken = true; }
            else hipLaunchKernelGGL((k_local_tets<4, WRITE_Z, REST, STOP>), dim3(blocks_for(b5 - b4)), dim3(256), 0, st, b4, b5, a);
        }
        if (b4 > b3) {    // co-rotated spline tets: their own launch (no BASELINE config mixes them in)
            stamp(); a.chunk0 = c->chunk_base[3];
            if (dom == 3 && c->lt_k0) { hipExtLaunchKernelGGL((k_local_tets<3, WRITE_Z, REST, STOP>), dim3(blocks_for(b4 - b3)), dim3(256), 0, st, c->lt_k0, c->lt_k1, 0, b3, b4, a); c->lt_taken = true; }
            else hipLaunchKernelGGL((k_local_tets<3, WRITE_Z, REST, STOP>), dim3(blocks_for(b4 - b3)), dim3(256), 0, st, b3, b4, a);
        }
        if (b3 > b0) stamp();
        a.chunk0 = b1 > b0 ? 0 : b2 > b1 ? c->chunk_base[1] : c->chunk_base[2];   // (fused: chunks 0 .. of the models it covers)
        // (its begin and end time stamps: what rocprofv3 reports as the kernel's duration -- instead of bracketing the launches)
        hipEvent_t k0 = c->lt_k0, k1 = c->lt_k1;
        if (k0 && b3 > b0) c->lt_taken = true;
        if (kinds >= 2) { // mixed scene: one launch over all models
            const int n0 = blocks_for(b1 - b0), n1 = blocks_for(b2 - b1), n2 = blocks_for(b3 - b2);
            if (k0) hipExtLaunchKernelGGL((k_local_tets_fused<WRITE_Z, REST, STOP>), dim3(n0 + n1 + n2), dim3(256), 0, st, k0, k1, 0, b0, b1, b2, b3, n0, n0 + n1, a);
            else hipLaunchKernelGGL((k_local_tets_fused<WRITE_Z, REST, STOP>), dim3(n0 + n1 + n2), dim3(256), 0, st, b0, b1, b2, b3, n0, n0 + n1, a);
        } else if (b1 > b0) {
            if (k0) hipExtLaunchKernelGGL((k_local_tets<0, WRITE_Z, REST, STOP>), dim3(blocks_for(b1 - b0)), dim3(256), 0, st, k0, k1, 0, b0, b1, a);
            else hipLaunchKernelGGL((k_local_tets<0, WRITE_Z, REST, STOP>), dim3(blocks_for(b1 - b0)), dim3(256), 0, st, b0, b1, a);
        } else if (b2 > b1) {
            if (k0) hipExtLaunchKernelGGL((k_local_tets<1, WRITE_Z, REST, STOP>), dim3(blocks_for(b2 - b1)), dim3(256), 0, st, k0, k1, 0, b1, b2, a);
            else hipLaunchKernelGGL((k_local_tets<1, WRITE_Z, REST, STOP>), dim3(blocks_for(b2 - b1)), dim3(256), 0, st, b1, b2, a);
        } else if (b3 > b2) {
            if (k0) hipExtLaunchKernelGGL((k_local_tets<2, WRITE_Z, REST, STOP>), dim3(blocks_for(b3 - b2)), dim3(256), 0, st, k0, k1, 0, b2, b3, a);
            else hipLaunchKernelGGL((k_local_tets<2, WRITE_Z, REST, STOP>), dim3(blocks_for(b3 - b2)), dim3(256), 0, st, b2, b3, a);
        }
    }
    if (c->ntri > 0) {
        if (c->nt == 0 && c->lt_k0 && (c->lt_taken = true))      // (a scene of triangles only: their kernel is the dominant one)
            hipExtLaunchKernelGGL((k_local_tris<WRITE_Z, STOP>), dim3(blocks_for(c->ntri)), dim3(256), 0, st, c->lt_k0, c->lt_k1, 0, c->ntri, c->ldr, c->r_idx.p,
                                  c->r_rest.p, c->r_u.p, c->r_z.p, c->r_sc.p, c->r_lmin.p, c->r_lmax.p, c->curr.p, c->r_cf.p, c->stop_dev);
        else
            hipLaunchKernelGGL((k_local_tris<WRITE_Z, STOP>), dim3(blocks_for(c->ntri)), dim3(256), 0, st, c->ntri, c->ldr, c->r_idx.p,
                               c->r_rest.p, c->r_u.p, c->r_z.p, c->r_sc.p, c->r_lmin.p, c->r_lmax.p, c->curr.p, c->r_cf.p, c->stop_dev);
    }
    if (c->nbend > 0)
        hipLaunchKernelGGL((k_local_bends<WRITE_Z, STOP>), dim3(blocks_for(c->nbend)), dim3(256), 0, st, c->nbend, c->ldb, c->h_idx.p, c->h_coef.p, c->h_u.p, c->h_z.p,
                           c->h_sc.p, c->h_gam.p, c->curr.p, c->h_cf.p, c->stop_dev);
}
template <bool WRITE_Z>
void launch_local(admm_hip_ctx *c) {      // Binv recomputed from the rest positions / streamed: decided once, in admm_hip_create
    if constexpr (WRITE_Z) {      // (a step with early exit runs with the monitor: the WRITE_Z instantiations)
        if (c->stop_dev) { if (c->tet_rest_mode) launch_local_impl<true, true, true>(c); else launch_local_impl<true, false, true>(c); return; }
    }
    if (c->tet_rest_mode) launch_local_impl<WRITE_Z, true>(c);
    else launch_local_impl<WRITE_Z, false>(c);
}

// ---- energy / ADMM monitor (monitor.hpp) ----
// single-GPU contexts only: a rank of a multi-GPU job holds a part of the terms (element blocks) or of the bodies (components)
bool monitor_allowed(const admm_hip_ctx *c) { return c->world == 1 && !c->comm && !c->ar_fn && !c->cm.on; }
// Early exit of the ADMM loop: may this step SKIP ON THE DEVICE?  Only where every launch of an iteration is one the stop word reaches and
// the host takes no decision of its own inside the loop: the on-chip PCG (k_pcg2) and the persistent GS sweep (k_gs_persist) without
// colliders that need the host.  Everything else -- bodies beyond the chip on the launch path, UzawaCG with obstacle or dynamic rows (its
// host logic reads a row count per iteration, its column lanes run on other streams), the GS colour-kernel fall-backs, dynamic
// colliders, contexts that have given up their persistent kernels, ADMM_HIP_STOP_HOST=1 -- takes the same decision on the host.
bool stop_device_ok(const admm_hip_ctx *c) {
    if (c->stop_host || !c->dyn.empty() || c->dist_solve) return false;
    if (c->linsolver == 1) return c->gsp_enabled && (int64_t)c->gs_max_iters * c->gsp_C < 2000;      // (launch_gs: the persistent kernel)
    if (c->linsolver == 2 && c->obst.n > 0) return false;
    return c->oc_enabled && c->oc_plan;
}
int mon_blocks(const admm_hip_ctx *c, bool nodes) {
    return blocks_for(c->nt) + blocks_for(c->ntri) + blocks_for(c->nbend) + blocks_for(c->npin_terms) + (nodes ? blocks_for(c->n3) : 0);
}
// buffers of the monitor, allocated by the first call that needs them: block partials and the result always, z_prev / the per-term
// energies on demand
hipError_t mon_ensure(admm_hip_ctx *c, bool zprev, bool term) {
    hipError_t e;
    const size_t np = (size_t)kMonQ * std::max(1, mon_blocks(c, true));
    if (c->mon_part.n < np && (e = c->mon_part.alloc(np)) != hipSuccess) return e;
    if (!c->mon_out.p && (e = c->mon_out.alloc(kMonQ)) != hipSuccess) return e;
    if (zprev) {
        if (c->nt && !c->mon_tzp.p && (e = c->mon_tzp.alloc_zeroed((size_t)9 * c->ldt, c->stream)) != hipSuccess) return e;
        if (c->ntri && !c->mon_rzp.p && (e = c->mon_rzp.alloc_zeroed((size_t)6 * c->ldr, c->stream)) != hipSuccess) return e;
        if (c->nbend && !c->mon_hzp.p && (e = c->mon_hzp.alloc_zeroed((size_t)3 * c->ldb, c->stream)) != hipSuccess) return e;
        if (c->npin_terms && !c->mon_pzp.p && (e = c->mon_pzp.alloc_zeroed((size_t)6 * c->npin_terms, c->stream)) != hipSuccess) return e;
    }
    const size_t nterm = (size_t)c->nt + c->ntri + c->nbend;
    if (term && nterm && !c->mon_term.p && (e = c->mon_term.alloc(nterm)) != hipSuccess) return e;
    return hipSuccess;
}
// the scene at positions x as every pass over the terms reads it (elements.hpp)
ElemView elem_view(const admm_hip_ctx *c, const double *x) {
    ElemView v{};
    v.x = x; v.dt2 = c->dt * c->dt;
    v.nt = c->nt; v.ldt = c->ldt; v.t_idx = c->t_idx.p; v.t_Binv = c->t_Binv.p; v.t_x0 = c->tet_rest_mode ? c->t_x0.p : nullptr; v.t_sc = c->t_sc.p;
    v.t_mat = c->t_mat.p; v.mats = c->mats.p; v.spl = c->spl_tab.p;
    for (int i = 0; i < 6; ++i) v.kb[i] = c->kind_begin[i];
    v.ntri = c->ntri; v.ldr = c->ldr; v.r_idx = c->r_idx.p; v.r_rest = c->r_rest.p; v.r_sc = c->r_sc.p;
    v.nbend = c->nbend; v.ldb = c->ldb; v.h_idx = c->h_idx.p; v.h_coef = c->h_coef.p; v.h_k = c->h_kst.p;
    return v;
}
// the monitor's view of the context at positions x; the pin rows as the step keeps them (3 per pin)
MonArgs mon_args(const admm_hip_ctx *c, const double *x, bool nodes) {
    MonArgs a{};
    a.v = elem_view(c, x);
    a.t_z = c->t_z.p; a.t_zp = c->mon_tzp.p;
    a.r_z = c->r_z.p; a.r_zp = c->mon_rzp.p;
    a.h_sc = c->h_sc.p; a.h_z = c->h_z.p; a.h_zp = c->mon_hzp.p;
    a.npin = c->npin_terms; a.pin_dim = 3; a.pin_vert = c->pin_vert_d.p; a.pin_z = c->pin_z.p; a.pin_zp = c->mon_pzp.p; a.pin_w2 = c->pin_weight * c->pin_weight;
    a.n3 = c->n3; a.m = nodes ? c->m.p : nullptr; a.Mxbar = c->Mxbar.p;
    a.nb_t = blocks_for(c->nt); a.nb_r = a.nb_t + blocks_for(c->ntri); a.nb_h = a.nb_r + blocks_for(c->nbend); a.nb_p = a.nb_h + blocks_for(c->npin_terms);
    a.part = c->mon_part.p; a.term = nullptr; a.stop = c->stop_dev;
    return a;
}
// one pass over the terms + the sum of its partials into out [kMonQ] (device).  s >= 0: record s of a step with early exit -- k_mon_decide
// in the place of k_mon_final, the same record, then the decision on it (STOP: the pass itself reads the stop word)
template <bool RES, bool ENERGY, bool STOP = false>
void launch_monitor(admm_hip_ctx *c, const MonArgs &a, double *out, int s = -1) {
    const int nb = std::max(1, a.nb_p + (a.m ? blocks_for(a.n3) : 0));
    hipLaunchKernelGGL((k_monitor<RES, ENERGY, false, STOP>), dim3(nb), dim3(256), 0, c->stream, a);
    if (s < 0) hipLaunchKernelGGL(k_mon_final, dim3(1), dim3(256), 0, c->stream, a.part, nb, out);
    else hipLaunchKernelGGL(k_mon_decide, dim3(1), dim3(256), 0, c->stream, a.part, nb, out, c->stop_tol, c->stop_min, s, c->counters.p, c->d_sig,
                            c->aa_on ? (const int *)&c->aa_ctl.p->mode : nullptr);
}
// z_prev <- D x: the reference's curr_z = D m_x at step entry (src/Solver.cpp:70)
void launch_monitor_init(admm_hip_ctx *c, const double *x) {
    const MonArgs a = mon_args(c, x, false);
    if (a.nb_p > 0) hipLaunchKernelGGL((k_monitor<false, false, true>), dim3(a.nb_p), dim3(256), 0, c->stream, a);
}
// record s of the running step: after the global solve of ADMM iteration s, x = curr
// decide = true: a step with early exit; with c->stop_dev the pass itself is the STOP instantiation
void launch_monitor_step(admm_hip_ctx *c, int s, bool decide = false) {
    const MonArgs a = mon_args(c, c->curr.p, c->mon_mode >= 2);
    double *out = c->mon_rec.p + (size_t)kMonQ * s;
    const int sd = decide ? s : -1;
    if (decide && c->stop_dev) {
        if (c->mon_mode >= 2) launch_monitor<true, true, true>(c, a, out, sd);
        else launch_monitor<true, false, true>(c, a, out, sd);
    } else {
        if (c->mon_mode >= 2) launch_monitor<true, true>(c, a, out, sd);
        else launch_monitor<true, false>(c, a, out, sd);
    }
}

// ---- Anderson acceleration of the ADMM loop (anderson.hpp) ----
// the state (curr, t_u, r_u, h_u, pin_u) as the three phases walk it: families present, their blocks, their place in a history vector
AaArgs aa_args(const admm_hip_ctx *c) {
    AaArgs a{};
    const double idt2 = 1.0 / (c->dt * c->dt);
    int nb = 0; long long off = 0;
    auto add = [&](double *live, const double *sc, double wk, int n, int nc, int stride_c, int stride_e, long long len) {
        if (n <= 0) return;
        AaSeg &g = a.seg[a.nseg++];
        g.live = live; g.sc = sc; g.wk = wk; g.off = off; g.n = n; g.nc = nc; g.stride_c = stride_c; g.stride_e = stride_e; g.blk0 = nb;
        nb += blocks_for(n); off += len;
    };
    add(c->curr.p, c->m.p, idt2, c->n3, 1, 0, 1, c->n3);
    add(c->t_u.p, c->t_sc.p, idt2, c->nt, 9, c->ldt, 1, 9LL * c->ldt);
    add(c->r_u.p, c->r_sc.p, idt2, c->ntri, 6, c->ldr, 1, 6LL * c->ldr);
    add(c->h_u.p, c->h_sc.p, idt2, c->nbend, 3, c->ldb, 1, 3LL * c->ldb);
    add(c->pin_u.p, nullptr, c->pin_weight * c->pin_weight, c->npin_terms, 3, 1, 3, 3LL * c->npin_terms);
    a.nb = std::max(1, nb); a.N = std::max(1LL, off); a.S = c->aa_window + 1;
    a.hg = c->aa_hg.p; a.hf = c->aa_hf.p; a.scopy = c->aa_scopy.p; a.ctl = c->aa_ctl.p; a.part = c->aa_part.p; a.stop = c->stop_dev;
    return a;
}
// buffers, allocated by the first step that needs them (and again for a larger window or more iterations)
hipError_t aa_ensure(admm_hip_ctx *c, int iters) {
    hipError_t e;
    const AaArgs a = aa_args(c);
    if (c->aa_slots < a.S) {
        if ((e = c->aa_hg.alloc((size_t)a.S * a.N)) != hipSuccess) return e;
        if ((e = c->aa_hf.alloc((size_t)a.S * a.N)) != hipSuccess) return e;
        c->aa_slots = a.S;
    }
    if (!c->aa_scopy.p && (e = c->aa_scopy.alloc((size_t)a.N)) != hipSuccess) return e;
    if (!c->aa_part.p && (e = c->aa_part.alloc((size_t)kAaQ * a.nb)) != hipSuccess) return e;
    if (!c->aa_ctl.p) {
        if ((e = c->aa_ctl.alloc(1)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c->aa_ctl.p, 0, sizeof(AaCtl), c->stream)) != hipSuccess) return e;
    }
    if (c->aa_rec.n < (size_t)kAaRec * std::max(1, iters) && (e = c->aa_rec.alloc((size_t)kAaRec * std::max(1, iters))) != hipSuccess) return e;
    return hipSuccess;
}
void launch_aa_init(admm_hip_ctx *c) {
    const AaArgs a = aa_args(c);
    hipLaunchKernelGGL(k_aa_init, dim3(a.nb), dim3(256), 0, c->stream, a);
}
// after the global solve of ADMM iteration s: the record pass and the decision
void launch_aa_record(admm_hip_ctx *c, int s) {
    AaArgs a = aa_args(c);
    a.rec = c->aa_rec.p + (size_t)kAaRec * s;
    hipLaunchKernelGGL(k_aa_record, dim3(a.nb), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_aa_solve, dim3(1), dim3(256), 0, c->stream, a);
}
void launch_aa_apply(admm_hip_ctx *c, bool last) {
    AaArgs a = aa_args(c);
    a.last = last ? 1 : 0;
    hipLaunchKernelGGL(k_aa_apply, dim3(a.nb), dim3(256), 0, c->stream, a);
}

hipError_t ElemScratch::ensure(admm_hip_ctx *c, int want) {
    if (want <= dirs) return hipSuccess;
    hipError_t e;
    dirs = 0;
    const size_t k = (size_t)want;
    if (c->nt && (e = rec.alloc_zeroed(k * 4 * (c->n_rec + 1), c->stream)) != hipSuccess) return e;
    if (c->ntri && (e = rcf.alloc_zeroed(k * 12 * c->ldr, c->stream)) != hipSuccess) return e;
    if (c->nbend && (e = hcf.alloc_zeroed(k * 12 * c->ldb, c->stream)) != hipSuccess) return e;
    dirs = want;
    return hipSuccess;
}

// ---- internal forces, stress, stationarity (forces.hpp) ----
// buffers, allocated by the first call that needs them
hipError_t force_ensure(admm_hip_ctx *c, bool stress, int stat_records) {
    hipError_t e;
    if ((e = c->f_el.ensure(c, 1)) != hipSuccess) return e;
    if (!c->f_out.p && (e = c->f_out.alloc_zeroed((size_t)std::max(1, c->n3), c->stream)) != hipSuccess) return e;
    if (stress && c->nt && !c->f_stress.p && (e = c->f_stress.alloc_zeroed((size_t)kStressQ * c->ldt, c->stream)) != hipSuccess) return e;
    if (stat_records > 0) {
        if (!c->f_part.p && (e = c->f_part.alloc_zeroed((size_t)std::max(1, blocks_for(c->nv)), c->stream)) != hipSuccess) return e;
        if (c->f_stat.n < (size_t)stat_records && (e = c->f_stat.alloc((size_t)stat_records)) != hipSuccess) return e;
    }
    return hipSuccess;
}
// the scene and the chunk plan at positions x; el: where the pass leaves the records and corner forces
ForceArgs force_args(const admm_hip_ctx *c, const double *x, const ElemScratch &el) {
    ForceArgs a{};
    a.v = elem_view(c, x);
    for (int i = 0; i < 6; ++i) a.cb[i] = c->chunk_base[i];
    a.plan = ChunkPlan{c->ch_ent.p, c->ch_group.p, c->ch_rec.p}; a.rec = el.rec.p; a.r_cf = el.rcf.p; a.h_cf = el.hcf.p;
    a.nb_t = c->nt > 0 ? c->chunk_base[5] : 0; a.nb_r = a.nb_t + blocks_for(c->ntri);
    return a;
}
// the incidence lists of the three families (those of k_gather_rhs) over the records and corner forces a force_args pass left; out [nv][3]
ForceGatherArgs force_gather_args(const admm_hip_ctx *c, const ForceArgs &a, double *out) {
    ForceGatherArgs g{};
    g.nv = c->nv; g.n_slices = (c->nv + 63) / 64;
    if (c->nt > 0) { g.t_ptr = c->t_inc.ptr.p; g.t_w = c->t_inc.w.p; g.t_inc = c->t_inc.idx.p; g.t_rec = a.rec; }
    if (c->ntri > 0) { g.r_ptr = c->r_inc.ptr.p; g.r_w = c->r_inc.w.p; g.r_inc = c->r_inc.idx.p; g.r_cf = a.r_cf; g.r_ld = c->ldr; }
    if (c->nbend > 0) { g.h_ptr = c->h_inc.ptr.p; g.h_w = c->h_inc.w.p; g.h_inc = c->h_inc.idx.p; g.h_cf = a.h_cf; g.h_ld = c->ldb; }
    g.order = c->g_order.p; g.f = out;
    return g;
}
// f_out = -dE/dx at positions x (device); stress: also the per-tet stress into f_stress; stop: the stop word or nullptr
void launch_forces(admm_hip_ctx *c, const double *x, bool stress, const int *stop) {
    ForceArgs a = force_args(c, x, c->f_el);
    a.stress = stress ? c->f_stress.p : nullptr;
    a.stop = stop;
    const int nb = a.nb_r + blocks_for(c->nbend);
    if (nb > 0) hipLaunchKernelGGL(k_forces, dim3(nb), dim3(256), 0, c->stream, a);
    ForceGatherArgs g = force_gather_args(c, a, c->f_out.p);
    g.stop = stop;
    hipLaunchKernelGGL(k_gather_forces, dim3(std::max(1, (g.n_slices + 3) / 4)), dim3(256), 0, c->stream, g);
}
// ---- tangent stiffness (tangent.hpp) ----
// buffers for n_vec directions (a failed allocation leaves its buffer empty: the call is made again)
hipError_t tangent_ensure(admm_hip_ctx *c, int n_vec) {
    hipError_t e;
    const size_t n = (size_t)n_vec * std::max(1, c->n3);
    if ((e = c->k_el.ensure(c, n_vec)) != hipSuccess) return e;
    if (c->k_d.n < n && (e = c->k_d.alloc_zeroed(n, c->stream)) != hipSuccess) return e;
    if (c->k_out.n < n && (e = c->k_out.alloc_zeroed(n, c->stream)) != hipSuccess) return e;
    return hipSuccess;
}
// k_out[j] = K(x) k_d[j] + shift m o k_d[j], j < n_vec, at positions x (device)
void launch_tangent(admm_hip_ctx *c, const double *x, int n_vec, double shift) {
    TangentArgs t{};
    t.f = force_args(c, x, c->k_el);
    t.d = c->k_d.p; t.n_vec = n_vec;
    t.s = DirStrides{(size_t)c->n3, (size_t)4 * (c->n_rec + 1), (size_t)12 * c->ldr, (size_t)12 * c->ldb};      // (the sizes of ElemScratch::ensure)
    const int nb = t.f.nb_r + blocks_for(c->nbend);
    if (nb > 0) {
        if (c->spl_tab.p) hipLaunchKernelGGL(k_tangent<true>, dim3(nb), dim3(256), 0, c->stream, t);
        else hipLaunchKernelGGL(k_tangent<false>, dim3(nb), dim3(256), 0, c->stream, t);
    }
    TangentGatherArgs q{};
    q.g = force_gather_args(c, t.f, c->k_out.p);
    q.d = c->k_d.p; q.m = c->m.p; q.shift = shift; q.s = t.s;
    hipLaunchKernelGGL(k_gather_tangent, dim3(std::max(1, (q.g.n_slices + 3) / 4), n_vec), dim3(256), 0, c->stream, q);
}

// monitor mode 3, record s of the running step: the stationarity sum at x = curr into f_stat[s].  Launched BEFORE the record's decision
// (k_mon_decide), so the last executed iteration of a step with early exit has its figure.
void launch_stationarity(admm_hip_ctx *c, int s) {
    launch_forces(c, c->curr.p, false, c->stop_dev);
    const int nb = std::max(1, blocks_for(c->nv));
    const bool gs = c->linsolver == 1;
    hipLaunchKernelGGL(k_stationarity, dim3(nb), dim3(256), 0, c->stream, c->nv, c->curr.p, c->m.p, c->Mxbar.p, c->f_out.p, 1.0 / (c->dt * c->dt),
                       (!gs && c->npin_terms > 0) ? c->vert_pin.p : nullptr, c->pin_active.p, gs ? c->gs_pin_flag.p : nullptr, c->f_part.p, c->stop_dev);
    hipLaunchKernelGGL(k_stat_final, dim3(1), dim3(256), 0, c->stream, c->f_part.p, nb, c->f_stat.p + s, c->stop_dev);
}

// ---- frozen tangent (newton.hpp) ----
hipError_t newton_ensure(admm_hip_ctx *c) {
    if (c->nw_ready) return hipSuccess;
    hipError_t e;
    hipStream_t st = c->stream;
    if (c->nt && (e = c->nw_tfr.alloc_zeroed((size_t)kFrameTet * c->ldt, st)) != hipSuccess) return e;
    if (c->ntri && (e = c->nw_rfr.alloc_zeroed((size_t)kFrameTri * c->ldr, st)) != hipSuccess) return e;
    if ((e = c->nw_el.ensure(c, 1)) != hipSuccess) return e;
    const size_t n = (size_t)std::max(1, c->n3);
    for (DevBuf<double> *b : {&c->nw_dinv, &c->nw_y, &c->nw_r, &c->nw_p, &c->nw_ap, &c->nw_rhs})
        if ((e = b->alloc_zeroed(n, st)) != hipSuccess) return e;
    if ((e = c->nw_part.alloc_zeroed((size_t)3 * std::max(1, blocks_for(c->nv)) + 8, st)) != hipSuccess) return e;      // (+ 8: the polish's sums)
    if ((e = c->nw_st.alloc(3)) != hipSuccess) return e;
    if ((e = c->nw_stop.alloc(1)) != hipSuccess) return e;
    if ((e = c->nw_pin.alloc((size_t)std::max(1, c->nv))) != hipSuccess) return e;
    if (!c->nw_hstop && (e = hipHostMalloc((void **)&c->nw_hstop, 2 * sizeof(int), hipHostMallocDefault)) != hipSuccess) return e;      // (a call that failed further down is made again)
    for (hipEvent_t &ev : c->nw_ev)
        if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    c->nw_ready = true;
    return hipSuccess;
}
int nw_blocks(const admm_hip_ctx *c) { return std::max(1, blocks_for(c->nv)); }
FrozenArgs frozen_args(const admm_hip_ctx *c, const double *x, const double *d, int psd, const int *stop) {
    FrozenArgs a{};
    a.f = force_args(c, x, c->nw_el);
    a.t_fr = c->nw_tfr.p; a.r_fr = c->nw_rfr.p; a.d = d; a.psd = psd; a.stop = stop;
    return a;
}
// the frames of the tangent at x (device) into nw_tfr / nw_rfr
void launch_tangent_setup(admm_hip_ctx *c, const double *x, int psd) {
    const FrozenArgs a = frozen_args(c, x, nullptr, psd, nullptr);
    if (a.f.nb_r <= 0) return;
    if (c->spl_tab.p) hipLaunchKernelGGL(k_tangent_setup<true>, dim3(a.f.nb_r), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(k_tangent_setup<false>, dim3(a.f.nb_r), dim3(256), 0, c->stream, a);
}
NewtonGatherArgs newton_gather_args(const admm_hip_ctx *c, const FrozenArgs &a, const double *d, double *out, double shift, const int *pin, const int *stop) {
    NewtonGatherArgs q{};
    q.g = force_gather_args(c, a.f, out);
    q.d = d; q.m = c->m.p; q.shift = shift; q.pin = pin; q.part = c->nw_part.p; q.stop = stop;
    return q;
}
// out = K_frozen d + shift m o d (rows of held vertices zero); nw_part[0 .. blocks) = the partials of d . out
void launch_frozen(admm_hip_ctx *c, const double *d, double *out, double shift, const int *pin, const int *stop) {
    const FrozenArgs a = frozen_args(c, nullptr, d, 0, stop);
    const int nb = a.f.nb_r + blocks_for(c->nbend);
    if (nb > 0) hipLaunchKernelGGL(k_tangent_frozen, dim3(nb), dim3(256), 0, c->stream, a);
    const NewtonGatherArgs q = newton_gather_args(c, a, d, out, shift, pin, stop);
    hipLaunchKernelGGL(k_newton_gather<false>, dim3(nw_blocks(c)), dim3(256), 0, c->stream, q);
}
// nw_dinv = 1 / (diag K_frozen + shift m), 0 on held vertices
void launch_frozen_diag(admm_hip_ctx *c, double shift, const int *pin) {
    const FrozenArgs a = frozen_args(c, nullptr, nullptr, 0, nullptr);
    const int nb = a.f.nb_r + blocks_for(c->nbend);
    if (nb > 0) hipLaunchKernelGGL(k_tangent_diag, dim3(nb), dim3(256), 0, c->stream, a);
    const NewtonGatherArgs q = newton_gather_args(c, a, nullptr, c->nw_dinv.p, shift, pin, nullptr);
    hipLaunchKernelGGL(k_newton_gather<true>, dim3(nw_blocks(c)), dim3(256), 0, c->stream, q);
}
// nw_pin = the vertices k_stationarity skips
void launch_pin_mask(admm_hip_ctx *c) {
    const bool gs = c->linsolver == 1;
    hipLaunchKernelGGL(k_nw_pin_mask, dim3(nw_blocks(c)), dim3(256), 0, c->stream, c->nv, (!gs && c->npin_terms > 0) ? c->vert_pin.p : nullptr,
                       c->pin_active.p, gs ? c->gs_pin_flag.p : nullptr, c->nw_pin.p);
}
// THE CHUNK PROTOCOL of every iterative solve on the frozen tangent (tangent_solve_device, tangent_solve_block_device, modes_device):
// iterations are enqueued in chunks of 8, one chunk ahead of the device; behind each chunk the stop word goes to one of two pinned words,
// followed by an event.  The host waits for the chunk BEFORE the one just enqueued and stops enqueueing when that chunk left the stop word
// set; the launches of a chunk enqueued behind the stop are no-ops.  enqueue_iteration(it) launches iteration it.
template <class F>
int run_chunked(admm_hip_ctx *c, int max_iters, F enqueue_iteration) {
    constexpr int chunk = 8;
    hipStream_t st = c->stream;
    int launched = 0, chunks = 0;
    while (launched < max_iters) {
        const int n = std::min(chunk, max_iters - launched);
        for (int it = launched; it < launched + n; ++it) enqueue_iteration(it);
        launched += n;
        HIP_TRY(hipMemcpyAsync(c->nw_hstop + (chunks & 1), c->nw_stop.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(c->nw_ev[chunks & 1], st));
        if (chunks >= 1) {
            HIP_TRY(hipEventSynchronize(c->nw_ev[(chunks - 1) & 1]));
            if (c->nw_hstop[(chunks - 1) & 1]) break;
        }
        ++chunks;
    }
    return ADMM_HIP_OK;
}
// PCG for (K(x) [psd] + shift M) y = nw_rhs on the free vertices, x on the device, with the preconditioner selected (Jacobi, or the
// two-level one of tangent_precond.hpp); leaves y in nw_y and the verdict in nw_st[2].  The caller synchronises.  (Defined behind the
// two-level launches it needs.)
int tangent_solve_device(admm_hip_ctx *c, const double *xd, double shift, int flags, double tol, int max_iters);
// ---- the frozen pass on a block of directions (newton.hpp), the block eigensolver (modal.hpp) ----
DirStrides block_strides(const admm_hip_ctx *c) {      // (the sizes of ElemScratch::ensure)
    return DirStrides{(size_t)c->n3, (size_t)4 * (c->n_rec + 1), (size_t)12 * c->ldr, (size_t)12 * c->ldb};
}
// out_j = K_frozen d_j + shift m o d_j (rows of held vertices zero), j < n_vec <= kModalNb; d, out: [n_vec][3 nv].  Column j has the bits
// of launch_frozen on d_j.
// With `cols` (device: {n, columns}) only the listed columns are applied; with `part` the gather leaves the partials of d_j . out_j at
// part[j][0][blocks] of [n_vec][3][blocks] and adds the list's length to *passes (the block PCG, below).
void launch_frozen_block(admm_hip_ctx *c, const double *d, double *out, int n_vec, double shift, const int *pin, const int *stop,
                         const int *cols = nullptr, double *part = nullptr, int *passes = nullptr) {
    FrozenBlockArgs b{};
    b.fa = frozen_args(c, nullptr, d, 0, stop);
    b.fa.f.rec = c->bk_el.rec.p; b.fa.f.r_cf = c->bk_el.rcf.p; b.fa.f.h_cf = c->bk_el.hcf.p;
    b.n_vec = n_vec; b.s = block_strides(c); b.cols = cols;
    const int nb = b.fa.f.nb_r + blocks_for(c->nbend);
    if (nb > 0) hipLaunchKernelGGL(k_tangent_frozen_block, dim3(nb), dim3(256), 0, c->stream, b);
    NewtonGatherBlockArgs q{};
    q.n = newton_gather_args(c, b.fa, d, out, shift, pin, stop);
    q.s = b.s; q.cols = cols; q.spart = (size_t)3 * nw_blocks(c); q.passes = passes;
    if (part) {
        q.n.part = part;
        hipLaunchKernelGGL(k_newton_gather_block<true>, dim3(nw_blocks(c), n_vec), dim3(256), 0, c->stream, q);
    } else hipLaunchKernelGGL(k_newton_gather_block<false>, dim3(nw_blocks(c), n_vec), dim3(256), 0, c->stream, q);
}
static_assert(kNwBlkCols == kModalNb, "newton.hpp and modal.hpp disagree on the widest block");
static_assert(kNwBlkCols <= kSensCols, "one k_param_sens pass takes a slab of the block adjoint");
// room for a slab of `cols` <= kNwBlkCols columns of the block PCG
hipError_t block_pcg_ensure(admm_hip_ctx *c, int cols) {
    hipError_t e;
    hipStream_t st = c->stream;
    if ((e = c->bk_el.ensure(c, cols)) != hipSuccess) return e;
    if (!c->bp_st.p && (e = c->bp_st.alloc_zeroed((size_t)3 * kNwBlkCols, st)) != hipSuccess) return e;
    if (!c->bp_ctl.p && (e = c->bp_ctl.alloc_zeroed(1, st)) != hipSuccess) return e;
    if (!c->bp_rr.p && (e = c->bp_rr.alloc_zeroed(kNwBlkCols, st)) != hipSuccess) return e;
    if (cols <= c->bp_cols) return hipSuccess;
    c->bp_cols = 0;
    const size_t n = (size_t)cols * std::max(1, c->n3);
    for (DevBuf<double> *b : {&c->bp_rhs, &c->bp_y, &c->bp_r, &c->bp_p, &c->bp_ap})
        if ((e = b->alloc_zeroed(n, st)) != hipSuccess) return e;
    if ((e = c->bp_part.alloc_zeroed((size_t)cols * 3 * nw_blocks(c), st)) != hipSuccess) return e;
    c->bp_cols = cols;
    return hipSuccess;
}
NwBlockArgs block_pcg_args(admm_hip_ctx *c, int k, const int *pin, double tol, int max_iters) {
    NwBlockArgs a{};
    a.nv = c->nv; a.nb = nw_blocks(c); a.k = k; a.sv = (size_t)c->n3;
    a.rhs = c->bp_rhs.p; a.dinv = c->nw_dinv.p; a.pin = pin;
    a.y = c->bp_y.p; a.r = c->bp_r.p; a.p = c->bp_p.p; a.ap = c->bp_ap.p; a.part = c->bp_part.p; a.rr = c->bp_rr.p;
    a.st = c->bp_st.p; a.ctl = c->bp_ctl.p; a.stop = c->nw_stop.p; a.tol2 = tol * tol; a.max_iters = max_iters;
    return a;
}
// The block Jacobi-PCG on the k <= kNwBlkCols columns of bp_rhs (newton.hpp): the frames and nw_dinv are in place (the caller ran the
// head of tangent_solve_device once for all slabs).  Four launches per iteration under run_chunked.  Leaves y in bp_y, the verdicts in
// bp_st[j][2], the true residuals in bp_rr, the column passes in bp_ctl; the caller synchronises.
int tangent_solve_block_device(admm_hip_ctx *c, int k, double shift, const int *pin, double tol, int max_iters) {
    hipStream_t st = c->stream;
    const int nb = nw_blocks(c);
    const NwBlockArgs a = block_pcg_args(c, k, pin, tol, max_iters);
    HIP_TRY(hipMemsetAsync(c->nw_stop.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_nw_cg_init_block, dim3(nb, k), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_nw_cg_init2_block, dim3(1), dim3(256), 0, st, a);
    if (int rc = run_chunked(c, max_iters, [&](int it) {
            launch_frozen_block(c, a.p, a.ap, k, shift, pin, c->nw_stop.p, a.ctl->list[it & 1], a.part, a.ctl->passes);
            hipLaunchKernelGGL(k_nw_cg_step_block, dim3(nb, k), dim3(256), 0, st, it, a);
            hipLaunchKernelGGL(k_nw_cg_dir_block, dim3(nb, k), dim3(256), 0, st, it, a);
        })) return rc;
    launch_frozen_block(c, a.y, a.ap, k, shift, pin, nullptr);      // the TRUE residuals of the returned iterates (tangent_solve_device), every column
    hipLaunchKernelGGL(k_nw_true_resid_block, dim3(nb, k), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_nw_resid_final_block, dim3(k), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return ADMM_HIP_OK;
}
struct BlockVerdict { NwCg st[kNwBlkCols]; double rr[kNwBlkCols]; int passes = 0, iters = 0; };
// One slab: the k <= kNwBlkCols columns of bp_rhs -> bp_y, bp_st[j][2], bp_rr.  blocked: the block PCG behind tangent_solve_head; else
// column after column through tangent_solve_device (the two-level preconditioner has no block form): the launches and the bits of
// single calls.  Enqueues only.
int block_solve_slab(admm_hip_ctx *c, const double *xd, int k, double shift, int flags, const int *pin, double tol, int max_iters, bool blocked) {
    if (blocked) return tangent_solve_block_device(c, k, shift, pin, tol, max_iters);
    hipStream_t st = c->stream;
    const size_t n3 = (size_t)c->n3;
    for (int j = 0; j < k; ++j) {
        if (n3) HIP_TRY(hipMemcpyAsync(c->nw_rhs.p, c->bp_rhs.p + j * n3, n3 * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (int rc = tangent_solve_device(c, xd, shift, flags, tol, max_iters)) return rc;
        if (n3) HIP_TRY(hipMemcpyAsync(c->bp_y.p + j * n3, c->nw_y.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->bp_st.p + 3 * j + 2, c->nw_st.p + 2, sizeof(NwCg), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->bp_rr.p + j, c->nw_part.p + (size_t)3 * nw_blocks(c) + 2, sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return ADMM_HIP_OK;
}
// the verdicts of a slab to the host, on the stream; the caller synchronises, then block_verdict_finish
hipError_t block_verdict_download(admm_hip_ctx *c, int k, bool blocked, std::vector<NwCg> &st3, BlockVerdict *v, NwBlockCtl *ctl) {
    st3.resize((size_t)3 * k);
    if (hipError_t e = hipMemcpyAsync(st3.data(), c->bp_st.p, st3.size() * sizeof(NwCg), hipMemcpyDeviceToHost, c->stream)) return e;
    if (hipError_t e = hipMemcpyAsync(v->rr, c->bp_rr.p, k * sizeof(double), hipMemcpyDeviceToHost, c->stream)) return e;
    if (blocked)
        if (hipError_t e = hipMemcpyAsync(ctl, c->bp_ctl.p, sizeof(NwBlockCtl), hipMemcpyDeviceToHost, c->stream)) return e;
    return hipSuccess;
}
void block_verdict_finish(int k, bool blocked, const std::vector<NwCg> &st3, const NwBlockCtl &ctl, BlockVerdict *v) {
    v->passes = 0; v->iters = 0;
    for (int j = 0; j < k; ++j) {
        v->st[j] = st3[(size_t)3 * j + 2];
        if (!blocked) { v->passes += v->st[j].it; v->iters = std::max(v->iters, v->st[j].it); }
    }
    if (blocked) { v->passes = ctl.passes[0]; v->iters = ctl.passes[1]; }
}
hipError_t modal_ensure(admm_hip_ctx *c) {
    if (c->md_ready) return hipSuccess;
    hipError_t e;
    hipStream_t st = c->stream;
    if ((e = c->bk_el.ensure(c, kModalNb)) != hipSuccess) return e;
    const size_t n = (size_t)std::max(1, c->n3), nbk = (size_t)nw_blocks(c);
    const int tiles = (int)((n + kModalTile - 1) / kModalTile);
    c->md_tpb = std::max(1, (tiles + 255) / 256);      // (at most 256 blocks of partials for k_modal_rr to sum)
    c->md_nbg = (tiles + c->md_tpb - 1) / c->md_tpb;
    if ((e = c->md_S.alloc_zeroed((size_t)kModalCols * n, st)) != hipSuccess) return e;
    if ((e = c->md_AS.alloc_zeroed((size_t)kModalCols * n, st)) != hipSuccess) return e;
    if ((e = c->md_theta.alloc_zeroed(kModalNb, st)) != hipSuccess) return e;
    if ((e = c->md_rpart.alloc_zeroed((size_t)2 * kModalNb * nbk, st)) != hipSuccess) return e;
    if ((e = c->md_gpart.alloc_zeroed((size_t)c->md_nbg * 2 * kModalPairs, st)) != hipSuccess) return e;
    if ((e = c->md_GA.alloc_zeroed((size_t)kModalCols * kModalCols, st)) != hipSuccess) return e;
    if ((e = c->md_GM.alloc_zeroed((size_t)kModalCols * kModalCols, st)) != hipSuccess) return e;
    if ((e = c->md_C.alloc_zeroed((size_t)kModalCols * kModalNb, st)) != hipSuccess) return e;
    if ((e = c->md_st.alloc(4)) != hipSuccess) return e;
    c->md_ready = true;
    return hipSuccess;
}
static_assert(kModalCols == admm_dev::kModalMax, "modal.hpp and device_math.hpp disagree on the widest block");
ModalArgs modal_args(admm_hip_ctx *c, int k, int nb, double tol, int max_iters) {
    ModalArgs a{};
    a.nv = c->nv; a.n3 = c->n3; a.nb = nb; a.k = k;
    a.nbk = nw_blocks(c); a.nbg = c->md_nbg; a.tpb = c->md_tpb;
    a.S = c->md_S.p; a.AS = c->md_AS.p; a.m = c->m.p; a.dinv = c->nw_dinv.p;
    a.theta = c->md_theta.p; a.rpart = c->md_rpart.p; a.gpart = c->md_gpart.p; a.GA = c->md_GA.p; a.GM = c->md_GM.p; a.C = c->md_C.p;
    a.st = c->md_st.p; a.stop = c->nw_stop.p; a.tol = tol; a.max_iters = max_iters;
    return a;
}
// the Rayleigh-Ritz on X alone: X becomes M-orthonormal, AX follows, Theta = the Ritz values
void launch_modal_rr0(admm_hip_ctx *c, const ModalArgs &a, int init) {
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_modal_gram, dim3(a.nbg), dim3(256), 0, st, a, 0);
    hipLaunchKernelGGL(k_modal_rr, dim3(1), dim3(256), 0, st, a, 0, 0, init);
    hipLaunchKernelGGL(k_modal_update, dim3(std::max(1, blocks_for(a.n3))), dim3(256), 0, st, a, 0, 0);
}
// LOBPCG on the device; X (md_S) holds the start block on entry.  The iterations run under run_chunked.  Leaves X, Theta, the true
// residual partials (md_rpart) and the state st[2]; the caller synchronises.
int modes_device(admm_hip_ctx *c, const double *xd, int k, int nb, double shift, int flags, double tol, int max_iters, const int *pin) {
    hipStream_t st = c->stream;
    const ModalArgs a = modal_args(c, k, nb, tol, max_iters);
    const size_t n3 = (size_t)c->n3;
    HIP_TRY(hipMemsetAsync(c->nw_stop.p, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->md_st.p, 0, 4 * sizeof(ModalSt), st));
    launch_tangent_setup(c, xd, flags & 1);
    launch_frozen_diag(c, shift, pin);
    launch_frozen_block(c, a.S, a.AS, nb, shift, pin, nullptr);
    launch_modal_rr0(c, a, 1);
    const int nrow = std::max(1, blocks_for(a.n3));
    if (int rc = run_chunked(c, max_iters, [&](int it) {
            hipLaunchKernelGGL(k_modal_resid, dim3(a.nbk), dim3(256), 0, st, a, 1);
            launch_frozen_block(c, a.S + (size_t)nb * n3, a.AS + (size_t)nb * n3, nb, shift, pin, c->nw_stop.p);
            hipLaunchKernelGGL(k_modal_gram, dim3(a.nbg), dim3(256), 0, st, a, 1);
            hipLaunchKernelGGL(k_modal_rr, dim3(1), dim3(256), 0, st, a, it, 1, 0);
            hipLaunchKernelGGL(k_modal_update, dim3(nrow), dim3(256), 0, st, a, it, 1);
        })) return rc;
    // the returned X once more through the Rayleigh-Ritz (M-orthonormal to rounding) and the block pass: the TRUE residuals
    launch_modal_rr0(c, a, 0);
    launch_frozen_block(c, a.S, a.AS, nb, shift, pin, nullptr);
    hipLaunchKernelGGL(k_modal_resid, dim3(a.nbk), dim3(256), 0, st, a, 2);
    HIP_TRY(hipGetLastError());
    return ADMM_HIP_OK;
}
// ---- the two-level preconditioner of the tangent solves (tangent_precond.hpp) ----
// the aggregates (planned in the rest positions, uploaded once per number of aggregates) and every tc_ buffer
int tc_ensure(admm_hip_ctx *c) {
    const int nv = c->nv;
    const int G = c->tc_aggregates > 0 ? c->tc_aggregates : std::min(kTcMaxAgg, std::max(1, nv / 256));
    if (c->tc_G == G && (c->tc_coarse_solver == 0 || c->tcb_W.p)) return ADMM_HIP_OK;
    if (c->tc_G == G) {      // the blocked inverse was selected after the buffers were made: its scratch alone
        const size_t nc = (size_t)c->tc_nc, ntile = (size_t)admm_dev::tcb_tiles(c->tc_nc);
        HIP_TRY(c->tcb_W.alloc_zeroed(nc * nc, c->stream));
        HIP_TRY(c->tcb_Linv.alloc_zeroed(ntile * admm_dev::kTcbT * admm_dev::kTcbT, c->stream));
        return ADMM_HIP_OK;
    }
    if (c->tc_xyz_h.size() != (size_t)c->n3) return fail(ADMM_HIP_ERR_ARG, "tangent_precond: the two-level preconditioner needs desc.vert_xyz (the aggregates are cut in the rest positions)");
    std::vector<int32_t> ptr, vert;
    if (!admm_host::tangent_plan(nv, c->tc_xyz_h.data(), G, ptr, vert)) return fail(ADMM_HIP_ERR_ARG, "tangent_precond: more aggregates than vertices");
    hipStream_t st = c->stream;
    c->tc_G = 0;
    HIP_TRY(c->bk_el.ensure(c, kModalNb));
    const size_t nc = (size_t)kTcPer * G, n = (size_t)std::max(1, c->n3), nvv = (size_t)std::max(1, nv), ncb = (nc + 3) / 4;
    if (vert.empty()) vert.push_back(0);
    HIP_TRY(c->tc_agg_ptr.alloc(ptr.size())); HIP_TRY(c->tc_agg_vert.alloc(vert.size()));
    HIP_TRY(hipMemcpyAsync(c->tc_agg_ptr.p, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->tc_agg_vert.p, vert.data(), vert.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c->tc_agg_of.alloc_zeroed(nvv, st)); HIP_TRY(c->tc_keep.alloc_zeroed(nc, st)); HIP_TRY(c->tc_info.alloc_zeroed(3, st));
    HIP_TRY(c->tc_phi.alloc_zeroed(4 * nvv, st));
    HIP_TRY(c->tc_d.alloc_zeroed((size_t)kModalNb * n, st)); HIP_TRY(c->tc_ad.alloc_zeroed((size_t)kModalNb * n, st));
    for (DevBuf<double> *b : {&c->tc_Ac, &c->tc_As, &c->tc_Ainv}) HIP_TRY(b->alloc_zeroed(nc * nc, st));
    for (DevBuf<double> *b : {&c->tc_ds, &c->tc_dl, &c->tc_col, &c->tc_c, &c->tc_yc}) HIP_TRY(b->alloc_zeroed(nc, st));
    HIP_TRY(c->tc_cpart.alloc_zeroed(ncb, st));
    c->tcb_W.release(); c->tcb_Linv.release();
    if (c->tc_coarse_solver == 1) {
        HIP_TRY(c->tcb_W.alloc_zeroed(nc * nc, st));
        HIP_TRY(c->tcb_Linv.alloc_zeroed((size_t)admm_dev::tcb_tiles((int)nc) * admm_dev::kTcbT * admm_dev::kTcbT, st));
    }
    HIP_TRY(hipStreamSynchronize(st));      // (ptr and vert leave scope)
    c->tc_G = G; c->tc_nc = (int)nc; c->tc_ncb = (int)ncb;
    return ADMM_HIP_OK;
}
// The blocked inverse (tangent_coarse.hpp): X = A^-1 by the chain of k_tcb_ launches; A [n][n] is destroyed.  info = {flag, ok, dropped} as
// k_tc_invert's.  Returns the launches.
int launch_tcb_invert(hipStream_t st, int n, double *A, double *X, double *ds, int *keep, int *info, double *Linv, double *Wm) {
    const int ntile = admm_dev::tcb_tiles(n), grid = std::min(1024, blocks_for(n * n));
    int *flag = info;
    int launches = 0;
    hipLaunchKernelGGL(k_tcb_scan, dim3(1), dim3(256), 0, st, n, A, ds, keep, flag, info + 1); ++launches;
    hipLaunchKernelGGL(k_tcb_scale, dim3(grid), dim3(256), 0, st, n, A, ds, keep, flag); ++launches;
    for (int k = 0; k < ntile; ++k) {
        const int m = ntile - k - 1;      // tile rows below the diagonal tile
        hipLaunchKernelGGL(k_tcb_potrf, dim3(1), dim3(256), 0, st, n, k, A, Linv, flag); ++launches;
        if (!m) break;
        hipLaunchKernelGGL(k_tcb_panel, dim3(m), dim3(256), 0, st, n, k, A, Linv, flag); ++launches;
        hipLaunchKernelGGL(k_tcb_update, dim3(m * (m + 1) / 2), dim3(256), 0, st, n, k, A, flag); ++launches;
    }
    hipLaunchKernelGGL(k_tcb_winv, dim3(ntile, admm_dev::kTcbT / admm_dev::kTcbStrip), dim3(256), 0, st, n, A, Linv, Wm, flag); ++launches;
    hipLaunchKernelGGL(k_tcb_wtw, dim3(ntile * (ntile + 1) / 2), dim3(256), 0, st, n, Wm, X, flag); ++launches;
    hipLaunchKernelGGL(k_tcb_unscale, dim3(grid), dim3(256), 0, st, n, X, ds, keep, flag); ++launches;
    hipLaunchKernelGGL(k_tcb_final, dim3(grid), dim3(256), 0, st, n, X, flag, info + 1); ++launches;
    return launches;
}
// A_c^-1 of the tangent frozen at xd (frames and nw_dinv are in place): the basis, A P in block passes of kModalNb columns, P^T (A P), the inverse
void launch_tc_setup(admm_hip_ctx *c, const double *xd, double shift, const int *pin) {
    hipStream_t st = c->stream;
    const int nv = c->nv, nb = nw_blocks(c), G = c->tc_G, nc = c->tc_nc;
    const size_t n3 = (size_t)c->n3;
    hipLaunchKernelGGL(k_tc_basis, dim3(G), dim3(256), 0, st, c->tc_agg_ptr.p, c->tc_agg_vert.p, xd, pin, c->tc_phi.p, c->tc_agg_of.p);
    c->tc_last_passes = 0;
    for (int col0 = 0; col0 < nc; col0 += kModalNb, ++c->tc_last_passes) {
        const int n = std::min<int>(kModalNb, nc - col0);
        hipLaunchKernelGGL(k_tc_fill, dim3(nb, n), dim3(256), 0, st, nv, col0, n3, c->tc_agg_of.p, c->tc_phi.p, c->tc_d.p);
        launch_frozen_block(c, c->tc_d.p, c->tc_ad.p, n, shift, pin, nullptr);
        hipLaunchKernelGGL(k_tc_restrict_block, dim3(G, n), dim3(256), 0, st, nc, col0, n3, c->tc_agg_ptr.p, c->tc_agg_vert.p, c->tc_phi.p, c->tc_ad.p, c->tc_Ac.p);
    }
    hipLaunchKernelGGL(k_tc_sym, dim3(blocks_for(nc * nc)), dim3(256), 0, st, nc, c->tc_Ac.p, c->tc_As.p);
    if (c->tc_coarse_solver == 1) c->tc_last_launches = launch_tcb_invert(st, nc, c->tc_As.p, c->tc_Ainv.p, c->tc_ds.p, c->tc_keep.p, c->tc_info.p, c->tcb_Linv.p, c->tcb_W.p);
    else {
        hipLaunchKernelGGL(k_tc_invert, dim3(1), dim3(1024), 0, st, nc, c->tc_As.p, c->tc_Ainv.p, c->tc_ds.p, c->tc_dl.p, c->tc_col.p, c->tc_keep.p, c->tc_info.p, c->tc_info.p + 1);
        c->tc_last_launches = 1;
    }
    c->tc_last_nc = nc;
}
// r = nw_rhs on the free rows, y = 0, p = z = M^-1 r and the scalars of iteration 0 (the stop word is 0 on entry)
void launch_tc_start(admm_hip_ctx *c, const int *pin) {
    hipStream_t st = c->stream;
    const int nv = c->nv, nb = nw_blocks(c);
    hipLaunchKernelGGL(k_tc_cg_init, dim3(nb), dim3(256), 0, st, nv, nb, c->nw_rhs.p, pin, c->nw_dinv.p, c->nw_y.p, c->nw_r.p, c->nw_part.p);
    hipLaunchKernelGGL(k_tc_restrict, dim3(c->tc_G), dim3(256), 0, st, c->nw_stop.p, c->tc_agg_ptr.p, c->tc_agg_vert.p, c->tc_phi.p, c->nw_r.p, c->tc_c.p);
    hipLaunchKernelGGL(k_tc_coarse, dim3(c->tc_ncb), dim3(256), 0, st, c->nw_stop.p, c->tc_nc, c->tc_Ainv.p, c->tc_c.p, c->tc_yc.p, c->tc_cpart.p);
    hipLaunchKernelGGL(k_tc_cg_init2, dim3(nb), dim3(256), 0, st, nv, nb, c->tc_ncb, c->nw_part.p, c->tc_cpart.p, c->nw_st.p, c->nw_stop.p, c->nw_dinv.p, c->nw_r.p,
                       c->tc_phi.p, c->tc_agg_of.p, c->tc_yc.p, c->nw_p.p);
}
// The head every solve on the frozen tangent shares: the pin mask in effect (flags bit 1) -> *pin, the stop word cleared, the frames of the
// tangent at xd (flags bit 0: projected), nw_dinv and, two_level, A_c^-1
int tangent_solve_head(admm_hip_ctx *c, const double *xd, double shift, int flags, bool two_level, const int **pin) {
    if (two_level) { if (int rc = tc_ensure(c)) return rc; }
    else { c->tc_last_nc = 0; c->tc_last_passes = 0; }
    *pin = nullptr;
    if (flags & 2) { launch_pin_mask(c); *pin = c->nw_pin.p; }
    HIP_TRY(hipMemsetAsync(c->nw_stop.p, 0, sizeof(int), c->stream));
    launch_tangent_setup(c, xd, flags & 1);
    launch_frozen_diag(c, shift, *pin);
    if (two_level) launch_tc_setup(c, xd, shift, *pin);
    return ADMM_HIP_OK;
}
// (declared above)  Four launches per iteration with Jacobi, six with the two-level preconditioner: the frozen pass on p (two launches) and
// k_nw_cg_step are common, the direction kernel differs.
int tangent_solve_device(admm_hip_ctx *c, const double *xd, double shift, int flags, double tol, int max_iters) {
    hipStream_t st = c->stream;
    const int nv = c->nv, nb = nw_blocks(c);
    const bool two_level = c->tc_kind == 1;
    const int *pin;
    if (int rc = tangent_solve_head(c, xd, shift, flags, two_level, &pin)) return rc;
    if (two_level) launch_tc_start(c, pin);
    else {
        hipLaunchKernelGGL(k_nw_cg_init, dim3(nb), dim3(256), 0, st, nv, nb, c->nw_rhs.p, pin, c->nw_dinv.p, c->nw_y.p, c->nw_r.p, c->nw_p.p, c->nw_part.p);
        hipLaunchKernelGGL(k_nw_cg_init2, dim3(1), dim3(256), 0, st, nb, c->nw_part.p, c->nw_st.p, c->nw_stop.p);
    }
    if (int rc = run_chunked(c, max_iters, [&](int it) {
            launch_frozen(c, c->nw_p.p, c->nw_ap.p, shift, pin, c->nw_stop.p);
            hipLaunchKernelGGL(k_nw_cg_step, dim3(nb), dim3(256), 0, st, it, nv, nb, c->nw_st.p, c->nw_stop.p, c->nw_dinv.p, c->nw_p.p, c->nw_ap.p,
                               c->nw_y.p, c->nw_r.p, c->nw_part.p);
            if (!two_level) {
                hipLaunchKernelGGL(k_nw_cg_dir, dim3(nb), dim3(256), 0, st, it, nv, nb, c->nw_st.p, c->nw_stop.p, tol * tol, max_iters, c->nw_dinv.p,
                                   c->nw_r.p, c->nw_p.p, c->nw_part.p);
                return;
            }      // two-level: r . z needs c = P^T r and y_c = A_c^-1 c first
            hipLaunchKernelGGL(k_tc_restrict, dim3(c->tc_G), dim3(256), 0, st, c->nw_stop.p, c->tc_agg_ptr.p, c->tc_agg_vert.p, c->tc_phi.p, c->nw_r.p, c->tc_c.p);
            hipLaunchKernelGGL(k_tc_coarse, dim3(c->tc_ncb), dim3(256), 0, st, c->nw_stop.p, c->tc_nc, c->tc_Ainv.p, c->tc_c.p, c->tc_yc.p, c->tc_cpart.p);
            hipLaunchKernelGGL(k_tc_cg_dir, dim3(nb), dim3(256), 0, st, it, nv, nb, c->tc_ncb, c->nw_st.p, c->nw_stop.p, tol * tol, max_iters, c->nw_dinv.p,
                               c->nw_r.p, c->nw_p.p, c->nw_part.p, c->tc_cpart.p, c->tc_phi.p, c->tc_agg_of.p, c->tc_yc.p);
        })) return rc;
    // the TRUE residual rhs - (K + shift M) y of the iterate the solve returns, over the free rows: what info4 reports.  The recursive residual
    // the stop test reads drifts from it by about eps cond(A) |rhs| -- 7e-4 of a residual of 1e-12 |rhs|.  (This pass carries no stop word.)
    launch_frozen(c, c->nw_y.p, c->nw_ap.p, shift, pin, nullptr);
    hipLaunchKernelGGL(k_nw_true_resid, dim3(nb), dim3(256), 0, st, nv, c->nw_rhs.p, pin, c->nw_ap.p, c->nw_part.p);
    hipLaunchKernelGGL(k_stat_final, dim3(1), dim3(256), 0, st, c->nw_part.p, nb, c->nw_part.p + (size_t)3 * nb + 2, nullptr);
    HIP_TRY(hipGetLastError());
    return ADMM_HIP_OK;
}
int newton_args_ok(const char *who, double shift, int32_t flags, int32_t flag_max = 3) {
    if (!std::isfinite(shift)) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": shift must be finite");
    if (flag_max == 7 && (flags < 0 || flags > 7)) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": flags must be a combination of 1 (positive semi-definite projection), 2 (hold pinned vertices) and 4 (block pass)");
    if (flags < 0 || flags > flag_max) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": flags must be a combination of 1 (positive semi-definite projection) and 2 (hold pinned vertices)");
    return ADMM_HIP_OK;
}
int solve_args_ok(const char *who, double tol, int32_t max_iters) {
    if (!(tol >= 0.0) || !std::isfinite(tol) || max_iters < 1) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": tol must be finite and >= 0, max_iters >= 1");
    return ADMM_HIP_OK;
}
// out4 = iterations, converged, |rhs - A y| / |rhs| from the true residual rr_true, |rhs|
void fill_solve_info(const NwCg &h, double rr_true, double *out4) {
    out4[0] = h.it; out4[1] = h.conv; out4[2] = h.bb > 0.0 ? std::sqrt(rr_true / h.bb) : 0.0; out4[3] = std::sqrt(h.bb);
}
// nw_part[3 blocks] = |g_free|^2 of the step's objective at the device-resident state, dst = -g (k_nw_grad): the polish's figure; needs nw_pin
void launch_state_residual(admm_hip_ctx *c, double idt2, double *dst) {
    const int nb = nw_blocks(c);
    launch_forces(c, c->x.p, false, nullptr);
    hipLaunchKernelGGL(k_nw_grad, dim3(nb), dim3(256), 0, c->stream, c->nv, c->x.p, c->m.p, c->Mxbar.p, c->f_out.p, idt2, c->nw_pin.p, dst, c->nw_part.p);
    hipLaunchKernelGGL(k_stat_final, dim3(1), dim3(256), 0, c->stream, c->nw_part.p, nb, c->nw_part.p + (size_t)3 * nb, nullptr);
}

// ---- adjoint of a step (adjoint.hpp) ----
hipError_t adjoint_ensure(admm_hip_ctx *c) {
    if (c->adj_ready) return hipSuccess;
    hipError_t e;
    hipStream_t st = c->stream;
    const size_t n = (size_t)std::max(1, c->n3);
    if ((e = c->adj_a.alloc_zeroed((size_t)kSensCols * n, st)) != hipSuccess) return e;
    if ((e = c->adj_ps.alloc_zeroed((size_t)kSensCols * ((size_t)4 * c->ldt + c->ldr + c->ldb) + 1, st)) != hipSuccess) return e;
    if ((e = c->adj_l.alloc_zeroed(2 * n, st)) != hipSuccess) return e;
    if ((e = c->adj_out.alloc_zeroed(4 * n, st)) != hipSuccess) return e;
    c->adj_ready = true;
    return hipSuccess;
}
// adj_ps = a_j^T df/dtheta per term at x (device) for the k <= kSensCols vectors a [k][stride] (device)
void launch_param_sens(admm_hip_ctx *c, const double *x, const double *a, size_t stride, int k) {
    SensArgs s{};
    s.f = force_args(c, x, c->f_el);      // (the scene and the chunk plan only: the pass writes no records)
    s.f.rec = nullptr; s.f.r_cf = nullptr; s.f.h_cf = nullptr;
    s.a = a; s.sa = stride; s.k = k;
    s.o_t = c->adj_ps.p; s.o_r = s.o_t + (size_t)kSensCols * 4 * c->ldt; s.o_h = s.o_r + (size_t)kSensCols * c->ldr;
    const int nb = s.f.nb_r + blocks_for(c->nbend);
    if (nb <= 0) return;
    if (c->spl_tab.p) hipLaunchKernelGGL(k_param_sens<true>, dim3(nb), dim3(256), 0, c->stream, s);
    else hipLaunchKernelGGL(k_param_sens<false>, dim3(nb), dim3(256), 0, c->stream, s);
}
// rs_out[j] = a_j^T df/dX per rest vertex at x (device) for the k <= kSensCols vectors a [k][3 nv] (device): tets only
hipError_t rest_sens_ensure(admm_hip_ctx *c, int k) {
    hipError_t e;
    if ((e = c->rs_el.ensure(c, k)) != hipSuccess) return e;
    const size_t n = (size_t)k * std::max(1, c->n3);
    if (c->rs_out.n < n && (e = c->rs_out.alloc_zeroed(n, c->stream)) != hipSuccess) return e;
    return hipSuccess;
}
void launch_rest_sens(admm_hip_ctx *c, const double *x, const double *a, int k) {
    RestArgs r{};
    r.f = force_args(c, x, c->rs_el);
    r.a = a; r.sa = (size_t)c->n3; r.srec = (size_t)4 * (c->n_rec + 1); r.k = k;      // (the sizes of ElemScratch::ensure)
    if (r.f.nb_t > 0) {
        if (c->spl_tab.p) hipLaunchKernelGGL(k_rest_sens<true>, dim3(r.f.nb_t), dim3(256), 0, c->stream, r);
        else hipLaunchKernelGGL(k_rest_sens<false>, dim3(r.f.nb_t), dim3(256), 0, c->stream, r);
    }
    TangentGatherArgs q{};
    q.g = force_gather_args(c, r.f, c->rs_out.p);
    q.d = a; q.m = c->m.p; q.shift = 0.0; q.s = DirStrides{r.sa, r.srec, 0, 0};
    hipLaunchKernelGGL(k_gather_tangent, dim3(std::max(1, (q.g.n_slices + 3) / 4), k), dim3(256), 0, c->stream, q);
}
int rest_refuse(const admm_hip_ctx *c, const char *who) {
    if (c->ntri_total > 0 || c->nbend_total > 0)
        return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": the context has triangles or hinges; their rest positions do not reach the library, and a gradient of the tets alone would be partial");
    return ADMM_HIP_OK;
}
// the first k columns of adj_ps into h (the layout of the device buffer), on the stream; the caller synchronises
hipError_t param_sens_download(const admm_hip_ctx *c, std::vector<double> &h, int k) {
    const size_t ot = 0, orr = (size_t)kSensCols * 4 * c->ldt, oh = orr + (size_t)kSensCols * c->ldr;
    const size_t n[3] = {(size_t)k * 4 * c->ldt, (size_t)k * c->ldr, (size_t)k * c->ldb}, o[3] = {ot, orr, oh};
    for (int q = 0; q < 3; ++q)
        if (n[q])
            if (hipError_t e = hipMemcpyAsync(h.data() + o[q], c->adj_ps.p + o[q], n[q] * sizeof(double), hipMemcpyDeviceToHost, c->stream)) return e;
    return hipSuccess;
}
// the k columns of adj_ps (downloaded into h) into the columns j0 .. j0 + k of the outputs, in the caller's term order; any output may be NULL
void param_sens_unpermute(const admm_hip_ctx *c, const std::vector<double> &h, int j0, int k, double *out_tets, double *out_tris, double *out_bends) {
    const double *ht = h.data(), *hr = ht + (size_t)kSensCols * 4 * c->ldt, *hh = hr + (size_t)kSensCols * c->ldr;
    for (int j = 0; j < k; ++j) {
        if (out_tets)
            for (int n = 0; n < c->nt; ++n)
                for (int q = 0; q < 4; ++q) out_tets[((size_t)(j0 + j) * c->nt_total + c->tet_perm[n]) * 4 + q] = ht[((size_t)j * 4 + q) * c->ldt + n];
        if (out_tris)
            for (int t = 0; t < c->ntri; ++t) out_tris[(size_t)(j0 + j) * c->ntri_total + c->tri_perm[t]] = hr[(size_t)j * c->ldr + t];
        if (out_bends)
            for (int t = 0; t < c->nbend; ++t) out_bends[(size_t)(j0 + j) * c->nbend_total + c->bend_perm[t]] = hh[(size_t)j * c->ldb + t];
    }
}
template <bool REF = false>
void launch_gather(admm_hip_ctx *c) {
    GatherArgs a{};
    a.nv = c->nv; a.n_slices = (c->nv + 63) / 64;
    if (c->nt > 0) { a.t_ptr = c->t_inc.ptr.p; a.t_w = c->t_inc.w.p; a.t_inc = c->t_inc.idx.p; a.t_rec = c->t_rec.p; }
    if (c->ntri > 0) { a.r_ptr = c->r_inc.ptr.p; a.r_w = c->r_inc.w.p; a.r_inc = c->r_inc.idx.p; a.r_cf = c->r_cf.p; a.r_ld = c->ldr; }
    if (c->nbend > 0) { a.h_ptr = c->h_inc.ptr.p; a.h_w = c->h_inc.w.p; a.h_inc = c->h_inc.idx.p; a.h_cf = c->h_cf.p; a.h_ld = c->ldb; }
    if (c->npin_terms > 0) {
        a.pin_nrm = c->has_slide ? c->pin_nrm.p : nullptr;
        a.vert_pin = c->vert_pin.p; a.pin_xyz = c->pin_xyz.p; a.pin_active = c->pin_active.p;
        a.pin_u = c->pin_u.p; a.pin_z = c->pin_z.p; a.pin_sc = c->dt * c->dt * c->pin_weight * c->pin_weight;
    }
    a.x = c->curr.p; a.Mxbar = c->Mxbar.p; a.b = c->b.p; a.add_mxbar = (c->rank == 0) ? 1 : 0;
    a.order = c->g_order.p; a.stop = c->stop_dev;
    const int grid = std::max(1, (a.n_slices + 3) / 4);
    if (c->stop_dev) hipLaunchKernelGGL((k_gather_rhs<true, REF>), dim3(grid), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL((k_gather_rhs<false, REF>), dim3(grid), dim3(256), 0, c->stream, a);
}

// in-place sum all-reduce of n doubles on the context's stream: RCCL, or the caller's transport staged through pinned host memory
int comm_allreduce(admm_hip_ctx *c, double *p, size_t n) {
    if (c->comm) return g_rccl.AllReduce(p, p, n, ncclDouble, ncclSum, c->comm, c->stream) == ncclSuccess ? 0 : -3;
    if (!c->ar_fn) return c->world > 1 ? -2 : 0;
    if (n > (size_t)c->n3) return -3;
    if (hipMemcpyAsync(c->ar_host, p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -3;
    if (c->ar_fn(c->ar_user, c->ar_host, (int64_t)n) != 0) return -3;
    return hipMemcpyAsync(p, c->ar_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess ? 0 : -3;
}

// b = M x_bar + dt^2 D^T W^2 (z - u): per-rank gather over the owned elements, then (multi-GPU) one
// in-place RCCL sum all-reduce over xGMI; rank 0 contributed M x_bar and the pin terms.
int launch_rhs(admm_hip_ctx *c) {
    launch_gather(c);
    if (c->world > 1 || c->comm) return comm_allreduce(c, c->b.p, (size_t)c->n3);
    return 0;
}

// PCG solve of A x = b, x = curr (warm start).  See the launch-control comment in admm_hip_ctx.
constexpr int kChunk = 32;

// Diagnosis only (ADMM_HIP_OC_DEBUG=1 / ADMM_HIP_OC_PROF=1): synchronises after every solve and prints its verdict /
// the per-phase times seen by block ADMM_HIP_OC_PROF_BLOCK (s_memrealtime ticks, 100 MHz).
int oc_diagnostics(admm_hip_ctx *c, int seq) {
    hipStream_t st = c->stream;
    if (c->oc_debug) {
        CgScal h;
        if (hipMemcpyAsync(&h, c->cg_scal.p, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
        int sm_off[2] = {0, 0};
        if (hipMemcpyAsync(sm_off, c->counters.p + kCntSmootherOff, sizeof(sm_off), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
        if (sm_off[0] != c->oc_dbg_sm_off) { c->oc_dbg_sm_off = sm_off[0]; fprintf(stderr, "[oc] seq %d: block smoother switched %s for the context (kCntSmootherOff), sm_b %.3g, trust revoked %d\n", h.seq, sm_off[0] ? "OFF" : "on", c->oc_sm_b, sm_off[1]); }
        fprintf(stderr, "[oc] seq %d iters %d (pipelined %d) verifications %d (last: true gamma / (tol^2 gamma_b) = %.2f) phases %d conv %d gamma %.3e %.3e %.3e gb %.3e %.3e %.3e\n", h.seq, h.iters, h.pad_,
                (int)h.alpha[0], h.alpha[2], (int)h.alpha[1], h.converged, h.gamma[0], h.gamma[1], h.gamma[2], h.gamma_b[0], h.gamma_b[1], h.gamma_b[2]);
    }
    if (!c->oc_prof.p) return 0;
    std::vector<unsigned long long> h(64 * 8);
    if (hipMemcpyAsync(h.data(), c->oc_prof.p, h.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
    auto us = [&](int a, int b) { return (double)(h[a] - h[b]) / 100.0; };
    if (c->oc_plan) {   // k_pcg2: eight stamps per pipelined iteration
        fprintf(stderr, "[oc_prof] seq %d: LDS fill %.2f  start phase %.2f  loop + end game %.2f  epilogue %.2f us\n", seq, us(63 * 8 + 1, 63 * 8), us(63 * 8 + 2, 63 * 8 + 1),
                us(63 * 8 + 3, 63 * 8 + 2), us(63 * 8 + 4, 63 * 8 + 3));
        if (h[63 * 8 + 7] > h[63 * 8 + 3])
            fprintf(stderr, "[oc_prof] end projection on the soft modes: pair stores + dots %.2f  grid barrier %.2f  reduce %.2f  G^-1 d + update + stores %.2f us\n",
                    us(63 * 8 + 5, 63 * 8 + 3), us(63 * 8 + 6, 63 * 8 + 5), us(63 * 8 + 7, 63 * 8 + 6), us(63 * 8 + 4, 63 * 8 + 7));
        if (h[62 * 8 + 6] > h[62 * 8])
            fprintf(stderr, "[oc_prof] start: entry residual %.2f  recycled sums %.2f  barrier %.2f  reduce + Cholesky %.2f  coarse(r) %.2f  u exchange + rows %.2f  record %.2f  barrier + reduce + coarse(w) %.2f us\n",
                    us(62 * 8, 63 * 8 + 1), us(62 * 8 + 1, 62 * 8), us(62 * 8 + 2, 62 * 8 + 1), us(62 * 8 + 3, 62 * 8 + 2), us(62 * 8 + 4, 62 * 8 + 3),
                    us(62 * 8 + 5, 62 * 8 + 4), us(62 * 8 + 6, 62 * 8 + 5), us(63 * 8 + 2, 62 * 8 + 6));
        double d[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int n = 0;
        for (int it = 0; it + 1 < 62 && h[(it + 1) * 8] > h[it * 8 + 7] && h[it * 8 + 7] > h[it * 8]; ++it, ++n) {
            for (int k = 0; k < 7; ++k) d[k] += us(it * 8 + k + 1, it * 8 + k);
            d[7] += us((it + 1) * 8, it * 8);
        }
        if (n) fprintf(stderr, "[oc_prof] n=%d  m+publish %.2f  neighbour wait %.2f  halo+rows %.2f  record %.2f  barrier %.2f  reduce+coarse %.2f  decide+update %.2f | iteration %.2f us\n",
                       n, d[0] / n, d[1] / n, d[2] / n, d[3] / n, d[4] / n, d[5] / n, d[6] / n, d[7] / n);
        if (hipMemsetAsync(c->oc_prof.p, 0, h.size() * 8, st) != hipSuccess) return -1;
        return 0;
    }
    fprintf(stderr, "[oc_prof] seq %d: LDS fill %.2f  start phase %.2f  loop %.2f  epilogue %.2f us\n", seq, us(63 * 8 + 1, 63 * 8), us(63 * 8 + 2, 63 * 8 + 1),
            us(63 * 8 + 3, 63 * 8 + 2), us(63 * 8 + 4, 63 * 8 + 3));
    if (h[62 * 8 + 5])
        fprintf(stderr, "[oc_prof] recycled start: x gather %.2f  pair loads + sums %.2f  barrier %.2f  read sums %.2f  cholesky %.2f (us)\n",
                us(62 * 8 + 1, 62 * 8), us(62 * 8 + 2, 62 * 8 + 1), us(62 * 8 + 3, 62 * 8 + 2), us(62 * 8 + 4, 62 * 8 + 3), us(62 * 8 + 5, 62 * 8 + 4));
    double d[5] = {0, 0, 0, 0, 0}, drain = 0; int n = 0;
    for (int it = 1; it + 1 < 62 && h[(it + 1) * 8] > h[it * 8 + 4] && h[it * 8 + 4] > h[it * 8]; ++it, ++n) {
        for (int k = 0; k < 4; ++k) d[k] += us(it * 8 + k + 1, it * 8 + k);
        drain += us(it * 8 + 5, it * 8 + 1);
        d[4] += us((it + 1) * 8, it * 8);
    }
    if (n) fprintf(stderr, "[oc_prof] n=%d  dots+publish %.2f  barrier %.2f  gather+reduce %.2f  update %.2f  | iteration %.2f us; of the barrier, store drain %.2f\n",
                   n, d[0] / n, d[1] / n, d[2] / n, d[3] / n, d[4] / n, drain / n);
    if (hipMemsetAsync(c->oc_prof.p, 0, h.size() * 8, st) != hipSuccess) return -1;
    return 0;
}

struct OcRc { bool on = false; RcBasis B{}; double *Eslot = nullptr, *Rslot = nullptr; const int *skip = nullptr;
              bool loop = false; };      // loop: a solve of the ADMM loop (launch_global's `loop`), not a stand-alone admm_hip_global_solve

// The instances of k_pcg2 (pcg_onchip2.hpp) by block size and configuration
static const void *pcg2_instance(int T, bool hot) {
    if (T <= 768) return hot ? (const void *)k_pcg2<768, true> : (const void *)k_pcg2<768, false>;
    return hot ? (const void *)k_pcg2<1024, true> : (const void *)k_pcg2<1024, false>;
}
// May this launch take the hot instance?  Only when everything that instance fixed at compile time holds: a solve of the ADMM loop on the
// main stream with the recycled warm start and no skip word, the two-level preconditioner, the neighbour hand-off lists, no profiling or
// debugging, at most two record units per thread.  Everything else is the generic instance's.  (The halo may be of any length: fixing it
// at two entries per thread was tried and changed nothing in the instance's registers or its iteration.)
static bool pcg2_hot_ok(const admm_hip_ctx *c, const OcRc &rc, const admm_hip_ctx::OcLane *ln) {
    if (c->oc_force_generic || !rc.loop || ln || !rc.on || rc.skip || c->stop_dev) return false;      // (a step with early exit: the generic instance reads the skip word)
    if (!c->oc_coarse || !c->oc_ainv.p || c->oc_nc > 2 * c->oc_T) return false;
    if (!c->oc_nbr.p || !c->oc_flags.p) return false;
    if (c->oc_prof.p || c->oc_debug) return false;
    return 4 * c->oc_G <= 2 * c->oc_T;
}

// General-mesh plan: k_pcg2 (pcg_onchip2.hpp)
int launch_pcg2(admm_hip_ctx *c, const double *b, double *x, int max_iters, const OcRc &rc, admm_hip_ctx::OcLane *ln = nullptr) {
    hipStream_t st = ln ? ln->st : c->stream;
    Oc2Args a{};
    a.n_rows = c->oc_rows; a.n_slices = c->oc_A.n_slices;
    a.ptr = c->oc_A.ptr.p; a.w = c->oc_A.w.p; a.val = c->oc_A.val.p; a.col16 = c->oc_col16.p;
    a.lds_off = c->oc_ldsoff.p; a.wl_s = c->oc_wls.p; a.bcols = c->oc_bcols;
    a.orig = c->oc_orig.p; a.halo_ptr = c->oc_haloptr.p; a.halo_src = c->oc_halosrc.p; a.halo_vert = c->oc_halovert.p; a.vec_len = c->oc_veclen;
    a.mdiag = c->oc_mdiag.p; a.dinv = c->dinv.p; a.b = b; a.x = x; a.u_out = c->cg_u.p;
    a.ubuf = c->oc_ubuf.p; a.part = c->oc_part.p; a.bar = c->oc_bar.p;
    a.nbr = c->oc_nbr.p; a.flags = c->oc_flags.p;
    a.counters = c->counters.p; a.scal = c->cg_scal.p; a.sig = c->d_sig;
    a.prof = c->oc_prof.p; a.prof_block = c->oc_prof_block;
    a.spb = c->oc_spb; a.G = c->oc_G; a.max_iters = max_iters; a.seq = ln ? ++ln->seq : ++c->solve_seq;
    if (!ln && c->test_abort_seq > 0 && a.seq == c->test_abort_seq)   // test hook: raise the abort word of this solve's barrier set
        if (hipMemsetAsync(c->oc_bar.p + 32 * 16 * (a.seq & 1) + 16 * 17, 1, sizeof(unsigned), st) != hipSuccess) return -1;
    a.tol2 = c->pcg_tol * c->pcg_tol;
    a.rc_on = rc.on ? 1 : 0; a.rc = rc.B; a.rc_xs = c->rc_xs.p; a.rc_r0 = c->rc_r0.p; a.rc_Eslot = rc.Eslot; a.rc_Rslot = rc.Rslot;
    a.rc_part = c->oc_rc_part.p;
    if (c->oc_coarse) { a.ainv = c->oc_ainv.p; a.cbuf = c->oc_cbuf.p; a.nc = c->oc_nc; a.ncp = c->oc_ncp; }
    a.cwt = c->oc_cwt.p;
    a.skip = rc.skip ? rc.skip : (ln ? nullptr : c->stop_dev);      // (a step with early exit: the solves behind the stop are no-ops)
    // (every 16th solve and a context's first 40 verify whatever the rule says: the sample that can revoke the trust, pcg_onchip2.hpp)
    a.trust_short = (c->oc_always_verify || c->oc_launches < 40 || (c->oc_launches & 15) == 0) ? 0 : 1;
    if (rc.on && c->defl_fused && c->defl_k > 0) { c->defl_armed = true; a.defl_k = c->defl_k; a.defl_Z = c->defl_Zint.p; a.defl_Ginv = c->defl_Ginv.p; a.defl_rec = c->defl_rec.p; }      // (the ADMM loop's solves only: not the K^-1 columns of UzawaCG)
    a.sm_ab = c->oc_sm_ab; a.sm_b = c->oc_sm_b;
    c->oc_launches += 1;
    if (ln) {      // a side-stream solve (UzawaCG's columns): the lane's own copies of everything the kernel writes, no diagnosis
        a.u_out = ln->u; a.ubuf = ln->ubuf; a.part = ln->part; a.bar = ln->bar; a.flags = c->oc_flags.p ? ln->flags : nullptr;
        a.counters = ln->counters; a.scal = ln->scal; a.prof = nullptr;
        if (c->oc_coarse) a.cbuf = ln->cbuf;
        a.trust_short = 0;
    }
    const bool hot = pcg2_hot_ok(c, rc, ln);
    if (c->oc_T <= 768) {
        if (hot) hipLaunchKernelGGL((k_pcg2<768, true>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a);
        else hipLaunchKernelGGL((k_pcg2<768, false>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a);
    } else {
        if (hot) hipLaunchKernelGGL((k_pcg2<1024, true>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a);
        else hipLaunchKernelGGL((k_pcg2<1024, false>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a);
    }
    c->oc_instance_launches[hot ? 0 : 1] += 1;
    if (ln) { c->oc_instance_launches[hot ? 2 : 3] += 1; return 0; }
    c->oc_last_instance = hot ? 2 : 1;
    c->last_launched_iters = 0;
    if (c->oc_debug || c->oc_prof.p) return oc_diagnostics(c, a.seq);
    return 0;
}

int launch_pcg_onchip(admm_hip_ctx *c, const double *b, double *x, int max_iters, const OcRc &rc = OcRc()) {
    return launch_pcg2(c, b, x, max_iters, rc);      // (oc_enabled implies the plan)
}

// Decide whether the system fits the chip: one SELL slice per wave, <= 16 waves per block, one block per CU.
hipError_t plan_pcg_onchip(admm_hip_ctx *c) {
    c->oc_enabled = false;
    if (env_flag("ADMM_HIP_PCG_LAUNCHES", false)) return hipSuccess;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, c->device);
    if (e != hipSuccess) return e;
    const int cus = prop.multiProcessorCount, ns = c->A.n_slices;
    if (ns <= 0 || cus <= 0) return hipSuccess;
    int G = std::min(cus, ns);
    int spb = (ns + G - 1) / G;
    if (spb > 16) return hipSuccess;
    if (!env_flag("ADMM_HIP_OC_PLAN", true)) return hipSuccess;      // no on-chip solve (A/B against the launch-per-iteration path, like ADMM_HIP_PCG_LAUNCHES=1)
    // the two-level preconditioner lets every thread handle two coarse unknowns (4 G <= 2 x 64 spb); small systems therefore
    // use fewer, larger blocks (which also makes their grid barrier cheaper)
    while (spb < 16 && (ns + spb - 1) / spb > 32 * spb) ++spb;
    {   // ADMM_HIP_OC_SPB=n: slices (waves) per block forced (experiments: barrier cost against block-local work on small systems)
        const int se = env_int("ADMM_HIP_OC_SPB", 0);
        if (se >= 1 && se <= 16 && (ns + se - 1) / se <= cus) spb = se;
    }
    G = (ns + spb - 1) / spb;
    const int T = 64 * spb;
    size_t lds_max = std::min<size_t>(prop.sharedMemPerBlock, 160 * 1024);
    {   // ADMM_HIP_OC_LDS_KB=n (>= 32): plan for less LDS (experiments, tests of the slab's streamed tail: more of the matrix comes from L2)
        const int kb = env_int("ADMM_HIP_OC_LDS_KB", 0);
        if (kb >= 32) lds_max = std::min<size_t>(lds_max, (size_t)kb * 1024);
    }
    size_t lds = 0;
    // The plan: compact blocks by graph bisection, rows sorted by length, local vector + halo list + slab in LDS,
    // two-level preconditioner (ADMM_HIP_OC_COARSE=0: Jacobi on the same layout) -- oc_plan.cpp, pcg_onchip2.hpp.
    admm_host::OcPlan plan;
    {
        const bool coarse = env_flag("ADMM_HIP_OC_COARSE", true);
        {
            std::vector<double> mass(c->n3);
            if ((e = hipMemcpy(mass.data(), c->m.p, mass.size() * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return e;
            plan = admm_host::build_oc_plan(c->Ahat, mass.data(), G, spb, (int)lds_max - kOc2Scratch, coarse, c->create_xyz);
            if (plan.ok && plan.bcols >= 4) {
                c->oc_plan = true;
                c->oc_rows = plan.n_rows; c->oc_bcols = plan.bcols; c->oc_veclen = plan.vec_len;
                lds = (size_t)kOc2Scratch + (size_t)3 * 8 * plan.vec_len + (size_t)plan.bcols * 64 * 10;
                if ((e = c->oc_A.ptr.upload(plan.A.slice_ptr)) != hipSuccess) return e;
                if ((e = c->oc_A.w.upload(plan.A.slice_width)) != hipSuccess) return e;
                if ((e = c->oc_A.val.upload(plan.A.val)) != hipSuccess) return e;
                c->oc_A.n_rows = plan.A.n_rows; c->oc_A.n_slices = plan.A.n_slices;
                if ((e = c->oc_col16.upload(plan.col16)) != hipSuccess) return e;
                c->oc_orig_h.assign(plan.orig.begin(), plan.orig.end());
                std::vector<int> oa(plan.orig);
                for (size_t r = 0; r < oa.size(); ++r) if (oa[r] >= 0) oa[r] |= (int)plan.row_agg[r] << 28;
                if ((e = c->oc_orig.upload(oa)) != hipSuccess) return e;
                if ((e = c->oc_ldsoff.upload(plan.lds_off)) != hipSuccess) return e;
                if ((e = c->oc_wls.upload(plan.wl_s)) != hipSuccess) return e;
                if ((e = c->oc_haloptr.upload(plan.halo_ptr)) != hipSuccess) return e;
                {   // never empty: the kernel reads two entries per thread unconditionally guarded by nh
                    std::vector<int> hs(plan.halo_src); if (hs.empty()) hs.push_back(0);
                    if ((e = c->oc_halosrc.upload(hs)) != hipSuccess) return e;
                    std::vector<int> hv(plan.halo_vert); hv.push_back(0);      // (the vertex of every entry: the entry residual's halo of x; one entry of
                                                                               // padding: the kernel's two loads per thread are unconditional, at a clamped index)
                    if ((e = c->oc_halovert.upload(hv)) != hipSuccess) return e;
                }
                if ((e = c->oc_mdiag.upload(plan.mdiag)) != hipSuccess) return e;
                c->oc_coarse = plan.coarse_ok && plan.nc <= 2 * T;
                c->oc_affine = plan.affine;
                if ((e = c->oc_cwt.upload(plan.cwt)) != hipSuccess) return e;
                if (c->oc_coarse) {
                    c->oc_nc = plan.nc; c->oc_ncp = plan.ncp;
                    if ((e = c->oc_ainv.upload(plan.ainv)) != hipSuccess) return e;
                    if ((e = c->oc_cbuf.alloc((size_t)2 * 3 * plan.ncp)) != hipSuccess) return e;
                    if ((e = c->oc_cbuf.zero()) != hipSuccess) return e;
                }
                {   // block-local smoother: degree-2 Chebyshev polynomial of D^-1 A_bb on [hi / ratio, hi], hi = the plan's estimate
                    // of lambda_max + 10 % (the polynomial stays positive up to 1.125 hi); ADMM_HIP_OC_CHEB=0: plain Jacobi
                    c->oc_sm_ab = 0.0; c->oc_sm_b = 0.0; c->oc_lam_bb = plan.lam_bb;
                    if (env_flag("ADMM_HIP_OC_CHEB", true) && plan.lam_bb > 0.0) {
                        const double ratio = 400.0;      // (16 until round 6's last session: with the wider interval 1-2.5 % fewer iterations on the 1 M-tet bodies, 200-frame drift unchanged -- profiles/r06_block_smoother_fix.txt)
                        // upper end of the interval: the plan's estimate of lambda_max(D^-1 A_bb) (power iterations from three
                        // starts, run until they stagnate) + 10 %, never above the plan's rigorous Gershgorin bound; the polynomial
                        // stays positive up to 1.125 x this value
                        const double hi = std::min(1.1 * plan.lam_bb, std::max(plan.lam_bb_gersh, 1.0)), lo = hi / ratio, th = 0.5 * (hi + lo), de = 0.5 * (hi - lo);
                        const double sg = th / de, r0 = 1.0 / sg, r1 = 1.0 / (2.0 * sg - r0);
                        const double al = (1.0 + r1 * r0) / th + 2.0 * r1 / de, be = 2.0 * r1 / (de * th);
                        c->oc_sm_ab = al - be; c->oc_sm_b = be;
                    }
                }
                if (getenv("ADMM_HIP_OC_DIAG"))
                    fprintf(stderr, "[oc_plan] lanes on the busiest LDS bank pair per half-wave column: %.2f by index, %.2f as placed; lambda_max(D^-1 A_bb) ~ %.3f\n",
                            plan.stat_bank_sorted, plan.stat_bank_placed, plan.lam_bb);
                c->oc_stat[0] = plan.stat_nnz; c->oc_stat[1] = plan.stat_stored; c->oc_stat[2] = plan.stat_onchip; c->oc_stat[3] = plan.stat_local;
                c->oc_stat[4] = plan.nbr_max; c->oc_stat[5] = c->oc_coarse ? plan.nc : 0;
            }
        }
    }
    if (!c->oc_plan) return hipSuccess;      // no plan (halo too large for 16-bit columns, per-dof masses, ...): the launch path serves the system
    for (int hot = 0; hot < 2; ++hot)      // (both instances of this block size: launch_pcg2 chooses per launch)
        if ((e = hipFuncSetAttribute(pcg2_instance(T, hot != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    if (T <= 768 && (e = hipFuncSetAttribute((const void *)k_sync_probe<768>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    if (T > 768 && (e = hipFuncSetAttribute((const void *)k_sync_probe<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    int per_cu = 0;     // (the kernels that will actually be launched with this LDS size: the tighter of the two instances)
    for (int hot = 0; hot < 2; ++hot) {
        int n = 0;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pcg2_instance(T, hot != 0), T, lds)) != hipSuccess) return e;
        per_cu = hot ? std::min(per_cu, n) : n;
    }
    if (per_cu < 1 || G > cus) return hipSuccess; // one block per CU keeps every block resident whatever the LDS split
    c->oc_G = G; c->oc_spb = spb; c->oc_T = T; c->oc_lds = lds;
    if ((e = c->oc_ubuf.alloc((size_t)2 * G * spb * 64 * 4)) != hipSuccess) return e;
    if ((e = c->oc_part.alloc((size_t)2 * 8 * G)) != hipSuccess) return e;
    if ((e = c->oc_rc_part.alloc((size_t)72 * G)) != hipSuccess) return e;
    if ((e = c->oc_bar.alloc(2 * 32 * 16)) != hipSuccess) return e;
    if ((e = c->oc_bar.zero()) != hipSuccess) return e;
    if ((e = hipMemset(c->oc_ubuf.p, 0, c->oc_ubuf.n * sizeof(double))) != hipSuccess) return e;
    // diagnosis switches
    c->oc_debug = env_flag("ADMM_HIP_OC_DEBUG", false);
    c->oc_always_verify = env_flag("ADMM_HIP_OC_VERIFY", false);      // A/B, tests: verify every pass (pcg_onchip2.hpp: kOc2TrustIters)
    c->oc_prof_block = env_int("ADMM_HIP_OC_PROF_BLOCK", 0);
    c->oc_force_generic = env_flag("ADMM_HIP_OC_GENERIC", false);     // A/B, tests: the generic instance of k_pcg2 for every launch
    if (env_flag("ADMM_HIP_OC_PROF", false)) { if ((e = c->oc_prof.alloc(64 * 8)) != hipSuccess) return e; if ((e = c->oc_prof.zero()) != hipSuccess) return e; }
    c->oc_nbr_max = plan.nbr_ok ? plan.nbr_max : -1;
    // tests (ADMM_HIP_OC_HANDOFF=0): no hand-off lists although the plan has them -- k_pcg2 orders its vector exchanges with grid barriers,
    // as it does for a plan with more than 64 neighbour blocks of a block (same arithmetic, same bits; generic instance only)
    if (plan.nbr_ok && env_flag("ADMM_HIP_OC_HANDOFF", true)) {      // which blocks does every block gather from?
        if ((e = c->oc_nbr.upload(plan.nbr)) != hipSuccess) return e;
        if ((e = c->oc_flags.alloc((size_t)8 * G)) != hipSuccess) return e;
        if ((e = c->oc_flags.zero()) != hipSuccess) return e;
    }
    c->oc_enabled = true;
    c->test_abort_seq = env_int("ADMM_HIP_TEST_ABORT_SOLVE", 0);
    return hipSuccess;
}

// DISTRIBUTED PCG of one body (SURVEY 8e option B; BASELINE configs[3]: "all-reduce per CG iteration"): the launch-per-iteration
// solver with the rows split into contiguous vertex blocks.  A rank computes the matrix-vector product, the dot-product partials
// and the vector updates of ITS rows only; per iteration two sum all-reduces assemble what the others need -- the partial sums
// (6 x NB doubles: every rank then derives the same alpha / beta in the same order) and the preconditioned residual u, the input of
// the next product (3 nv doubles; rows of other ranks are zero in every contribution).  x is assembled once, after the loop.  The
// convergence decision is the device's as on one GPU; the host reads it after every iteration (one stream synchronisation) so that
// all ranks leave the loop at the same iteration and issue the same collectives.  Compute shards 1 / N; the exchange does not:
// this pays for bodies that do not fit one chip's LDS, not at 1 M tets.
int launch_pcg_dist(admm_hip_ctx *c, const double *b, double *x, int max_iters) {
    hipStream_t st = c->stream;
    const SellA A = sell_arg(c->A);
    const int NB = c->NB, lo = c->row_lo, hi = c->row_hi;
    const double tol2 = c->pcg_tol * c->pcg_tol;
    const int seq = ++c->solve_seq;
    hipLaunchKernelGGL(k_cg_resid, dim3(NB), dim3(256), 0, st, A, c->m.p, c->dinv.p, b, x, c->cg_u.p, c->part_b.p, NB, c->cg_scal.p, seq, lo, hi);
    if (int r = comm_allreduce(c, c->cg_u.p, (size_t)c->n3)) return r;
    if (int r = comm_allreduce(c, c->part_b.p, (size_t)3 * NB)) return r;
    int launched = 0, converged = 0;
    for (int it = 0; it < max_iters; ++it) {
        const CgScal *prev = c->cg_scal.p + (it & 1);
        CgScal *next = c->cg_scal.p + ((it + 1) & 1);
        hipLaunchKernelGGL(k_cg_spmv, dim3(NB), dim3(256), 0, st, A, c->m.p, c->cg_u.p, c->dinv.p, c->cg_w.p, c->part.p, NB, prev, lo, hi);
        if (int r = comm_allreduce(c, c->part.p, (size_t)6 * NB)) return r;
        hipLaunchKernelGGL(k_cg_vec, dim3(c->NBV), dim3(256), 0, st, it, c->nv, NB, c->part.p, c->part_b.p, prev, next, tol2,
                           c->counters.p, c->dinv.p, c->cg_p.p, c->cg_s.p, x, c->cg_u.p, c->cg_w.p, c->d_sig, 0, lo, hi);
        launched = it + 1;
        if (hipMemcpyAsync(&converged, &next->converged, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
        if (converged) break;       // (u is still the assembled one of the previous iteration: the converged k_cg_vec wrote nothing)
        if (int r = comm_allreduce(c, c->cg_u.p, (size_t)c->n3)) return r;
    }
    hipLaunchKernelGGL(k_keep_own_rows, dim3(blocks_for(c->nv)), dim3(256), 0, st, c->nv, lo, hi, x);
    if (int r = comm_allreduce(c, x, (size_t)c->n3)) return r;
    c->last_launched_iters = launched;
    return 0;
}

// Plan of the launch-path two-level PCG, made the first time a solve needs it (a body beyond the chip, or after the on-chip kernel was given up)
bool ensure_big_plan(admm_hip_ctx *c) {
    if (c->big_tried) return c->big_enabled;
    c->big_tried = true;
    if (!c->big_allowed) return false;      // ADMM_HIP_BIG=0 at create: the Jacobi PCG of rounds 1-4 (A/B, tests)
    std::vector<double> mass(c->n3);
    if (hipMemcpy(mass.data(), c->m.p, mass.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return false;
    const admm_host::BigPlan P = admm_host::build_big_plan(c->Ahat, mass.data(), c->xyz_h.size() == (size_t)c->n3 ? c->xyz_h.data() : nullptr, env_int("ADMM_HIP_BIG_AGGREGATES", 1024, 1));
    if (!P.ok) return false;
    auto ok = [](hipError_t e) { return e == hipSuccess; };
    const size_t n3r = 3 * (size_t)P.n_rows;
    if (!ok(c->big_A.upload(P.A)) || !ok(c->big_orig.upload(std::vector<int>(P.orig.begin(), P.orig.end()))) || !ok(c->big_ainv.upload(P.ainv)) ||
        !ok(c->big_mass.upload(P.mass)) || !ok(c->big_dinv.upload(P.dinv)) || !ok(c->big_cwt.upload(P.cwt)) ||
        !ok(c->big_xi.alloc(n3r)) || !ok(c->big_r.alloc(n3r)) || !ok(c->big_u.alloc(n3r)) || !ok(c->big_w.alloc(n3r)) || !ok(c->big_p.alloc(n3r)) || !ok(c->big_s.alloc(n3r)) ||
        !ok(c->big_u.zero()) || !ok(c->big_w.zero()) || !ok(c->big_r.zero()) ||
        !ok(c->big_part.alloc((size_t)6 * (P.n_rows / 256))) || !ok(c->big_dots.alloc(8)) || !ok(c->big_dots.zero()) || !ok(c->big_tick.alloc(2)) || !ok(c->big_tick.zero()) || !ok(c->big_cvec.alloc((size_t)3 * P.ncp + (size_t)3 * P.G)) || !ok(c->big_cvec.zero())) {      // (c and rho side by side: one all-reduce in the distributed solve)
        (void)hipGetLastError();
        return false;
    }
    c->big_G = P.G; c->big_ra = P.ra; c->big_rows = P.n_rows; c->big_nc = P.nc; c->big_ncp = P.ncp; c->big_NBt = P.n_rows / 256;
    if (c->dist_solve) {      // rank r owns a contiguous range of aggregates (compact subdomains of the recursive bisection); interface rows of ALL ranks
        const int glo = (int)((int64_t)P.G * c->rank / c->world), ghi = (int)((int64_t)P.G * (c->rank + 1) / c->world);
        c->big_row_lo = glo * P.ra; c->big_row_hi = ghi * P.ra;
        std::vector<int> agg_owner(P.G, 0);
        for (int r = 0; r < c->world; ++r) for (int g = (int)((int64_t)P.G * r / c->world); g < (int)((int64_t)P.G * (r + 1) / c->world); ++g) agg_owner[g] = r;
        auto owner = [&](int32_t row) { return agg_owner[row / P.ra]; };
        std::vector<char> is_if(P.n_rows, 0);
        for (int32_t sl = 0; sl < P.A.n_slices; ++sl)
            for (int l = 0; l < 64; ++l) {
                const int32_t row = 64 * sl + l;
                if (row >= P.n_rows || P.orig[row] < 0) continue;
                const int ro = owner(row);
                for (int32_t k = 0; k < P.A.slice_width[sl]; ++k) {
                    const size_t e = (size_t)P.A.slice_ptr[sl] + 64 * (size_t)k + l;
                    if (P.A.val[e] != 0.0 && owner(P.A.idx[e]) != ro) is_if[P.A.idx[e]] = 1;
                }
            }
        std::vector<int> ifr;
        for (int32_t r = 0; r < P.n_rows; ++r) if (is_if[r]) ifr.push_back(r);
        c->big_nif = (int)ifr.size();
        if (ifr.empty()) ifr.push_back(0);
        if (!ok(c->big_if_rows.upload(ifr)) || !ok(c->big_ifbuf.alloc((size_t)3 * ifr.size()))) { (void)hipGetLastError(); return false; }
    }
    c->big_enabled = true;
    if (getenv("ADMM_HIP_OC_DIAG")) fprintf(stderr, "[big_plan] %d aggregates of %d rows, %d coarse unknowns (dense inverse %.1f MB), SELL %d slices\n", P.G, P.ra, P.nc, 4e-6 * (double)P.nc * P.ncp, P.A.n_slices);
    return true;
}

// The launch-path two-level PCG (pcg_big.hpp): three launches per iteration, chunks of iterations one ahead of the GPU, the device
// signals convergence through pinned host memory (as launch_pcg below).
int launch_pcg_big(admm_hip_ctx *c, const double *b, double *x, int max_iters) {
    hipStream_t st = c->stream;
    BigArgs a{};
    a.A = sell_arg(c->big_A); a.mass = c->big_mass.p; a.dinv = c->big_dinv.p; a.cwt = c->big_cwt.p; a.ainv = c->big_ainv.p; a.orig = c->big_orig.p;
    a.n_rows = c->big_rows; a.NBt = c->big_NBt; a.G = c->big_G; a.ra = c->big_ra; a.nc = c->big_nc; a.ncp = c->big_ncp;
    a.b_api = b; a.x_api = x; a.u_api = c->cg_u.p; a.dinv_api = c->dinv.p;
    a.xi = c->big_xi.p; a.r = c->big_r.p; a.u = c->big_u.p; a.w = c->big_w.p; a.p = c->big_p.p; a.s = c->big_s.p;
    a.part = c->big_part.p; a.dots = c->big_dots.p; a.tick = c->big_tick.p; a.cvec = c->big_cvec.p; a.rho = c->big_cvec.p + (size_t)3 * c->big_ncp;
    a.scal = c->cg_scal.p; a.counters = c->counters.p; a.sig = c->d_sig;
    a.tol2 = c->pcg_tol * c->pcg_tol; a.seq = ++c->solve_seq;
    a.row_lo = c->big_row_lo; a.row_hi = c->big_row_hi;
    const int nbr = c->big_rows / 256;
    if (c->dist_solve) {
        // DISTRIBUTED: the same kernels on the rank's own aggregates; per iteration three small sum all-reduces -- the six dot products
        // (summed per rank by its last block), c = P^T r with rho (3 ncp + 3 G), the interface rows of u (3 n_if) -- instead of the whole vector (round 4).  Every
        // rank derives the same scalars from the same numbers, reaches the same verdict at the same iteration, and stops at the same chunk
        // boundary (the device reports the iteration it converged at), so the ranks issue the same collectives.
        const size_t ncr = (size_t)3 * c->big_ncp + (size_t)3 * c->big_G;
        const int nif = c->big_nif, gif = std::max(1, blocks_for(nif));
        auto xchg_u = [&]() -> int {
            if (nif == 0) return 0;
            hipLaunchKernelGGL(k_big_if_pack, dim3(gif), dim3(256), 0, st, a, c->big_if_rows.p, nif, c->big_ifbuf.p);
            if (int r = comm_allreduce(c, c->big_ifbuf.p, (size_t)3 * nif)) return r;
            hipLaunchKernelGGL(k_big_if_unpack, dim3(gif), dim3(256), 0, st, a, c->big_if_rows.p, nif, c->big_ifbuf.p);
            return 0;
        };
        hipLaunchKernelGGL(k_big_gather, dim3(nbr), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_big_resid, dim3(c->big_NBt), dim3(256), 0, st, a);
        if (int r = comm_allreduce(c, c->big_dots.p, 3)) return r;
        hipLaunchKernelGGL(k_big_vec, dim3(c->big_G), dim3(kBigVecT), 0, st, a, -1, 0);
        if (int r = comm_allreduce(c, c->big_cvec.p, ncr)) return r;
        hipLaunchKernelGGL(k_big_coarse, dim3(c->big_G), dim3(kBigVecT), 0, st, a, -1);
        if (int r = xchg_u()) return r;
        volatile int *sig = c->h_sig;
        int launched = 0, chunks = 0;
        const int chunk = 8;
        while (launched < max_iters) {
            const int n = std::min(chunk, max_iters - launched);
            for (int it = launched; it < launched + n; ++it) {
                hipLaunchKernelGGL(k_big_spmv, dim3(c->big_NBt), dim3(256), 0, st, a, it);
                if (int r = comm_allreduce(c, c->big_dots.p, 6)) return r;
                hipLaunchKernelGGL(k_big_vec, dim3(c->big_G), dim3(kBigVecT), 0, st, a, it, (it == launched + n - 1) ? 1 : 0);
                if (int r = comm_allreduce(c, c->big_cvec.p, ncr)) return r;
                hipLaunchKernelGGL(k_big_coarse, dim3(c->big_G), dim3(kBigVecT), 0, st, a, it);
                if (int r = xchg_u()) return r;
            }
            const int end_prev = launched;        // iterations [0, launched) belong to the chunks before this one
            launched += n;
            ++chunks;
            ++c->marks_expected;
            if (chunks >= 2 && launched < max_iters) {
                const int need = c->marks_expected - 1;
                long spins = 0;
                while (sig[kSigChunks] < need) { if (++spins > 2000000000L) return -1; }
                // Converged inside the chunks that have DRAINED: a fact every rank must read the same way.  The mark the host has just seen is
                // written by k_big_vec of the previous chunk's LAST iteration (end_prev - 1, 0-based); the verdict of that iteration is written
                // by the k_big_coarse BEHIND it and may or may not be visible yet -- one rank leaving on it while another launches one more
                // chunk of collectives is a deadlock (seen once in 40 runs of the suite: a 30-minute gloo time-out).  Verdicts of the iterations
                // before it (count <= end_prev - 1) precede the mark in stream order: visible to every rank that has seen the mark.
                if (sig[kSigConverged] == a.seq && sig[kSigConvIter] <= end_prev - 1) break;
            }
        }
        hipLaunchKernelGGL(k_big_scatter, dim3(nbr), dim3(256), 0, st, a, launched & 1);
        if (int r = comm_allreduce(c, x, (size_t)c->n3)) return r;
        if (int r = comm_allreduce(c, c->cg_u.p, (size_t)c->n3)) return r;
        c->last_launched_iters = launched;
        c->big_solves += 1;
        c->big_rfin_valid = true;      // (cg_u = D^-1 r_final, assembled over the ranks)
        return 0;
    }
    hipLaunchKernelGGL(k_big_gather, dim3(nbr), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_big_resid, dim3(c->big_NBt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_big_vec, dim3(c->big_G), dim3(kBigVecT), 0, st, a, -1, 0);
    hipLaunchKernelGGL(k_big_coarse, dim3(c->big_G), dim3(kBigVecT), 0, st, a, -1);
    volatile int *sig = c->h_sig;
    int launched = 0, chunks = 0;
    // Iterations launched behind a converged one are no-ops, but three launches each, and the host learns of convergence one chunk late.  Fixed
    // chunks of 8 cost a late solve of an ADMM frame (1-5 iterations) 11-15 idle iterations = 33-45 empty launches.  Since round 6 the FIRST chunk
    // is what the solve at the same position of the previous frame needed (+ 1: the iteration that reports convergence), the chunks behind it
    // are short (an iteration is >= 70 us of kernels at these sizes; the host needs ~ 20 us to see a mark and launch the next chunk).
    constexpr int tail_chunk = 2;
    const int pos = std::min(std::max(c->rc_iter, 0), (int)(sizeof(c->big_its_hist) / sizeof(c->big_its_hist[0])) - 1);
    const int first = c->big_its_hist[pos] > 0 ? c->big_its_hist[pos] + 1 : 8;
    bool seen = false;
    while (launched < max_iters) {
        const int n = std::min(chunks == 0 ? first : tail_chunk, max_iters - launched);
        for (int it = launched; it < launched + n; ++it) {
            hipLaunchKernelGGL(k_big_spmv, dim3(c->big_NBt), dim3(256), 0, st, a, it);
            hipLaunchKernelGGL(k_big_vec, dim3(c->big_G), dim3(kBigVecT), 0, st, a, it, (it == launched + n - 1) ? 1 : 0);
            hipLaunchKernelGGL(k_big_coarse, dim3(c->big_G), dim3(kBigVecT), 0, st, a, it);
        }
        launched += n;
        ++chunks;
        ++c->marks_expected;
        if (chunks >= 2 && launched < max_iters) {
            const int need = c->marks_expected - 1;
            long spins = 0;
            while (sig[kSigChunks] < need) { if (++spins > 2000000000L) return -1; }
            if (sig[kSigConverged] == a.seq) { seen = true; break; }
        }
    }
    if (seen) c->big_its_hist[pos] = std::max(1, (int)sig[kSigConvIter]);
    else if (launched >= max_iters) c->big_its_hist[pos] = 0;       // (ran to the cap: nothing learnt)
    hipLaunchKernelGGL(k_big_scatter, dim3(nbr), dim3(256), 0, st, a, launched & 1);
    c->last_launched_iters = launched;
    c->big_solves += 1;
    c->big_rfin_valid = true;          // (cg_u = D^-1 r_final: launch_deflation)
    return 0;
}

int launch_pcg(admm_hip_ctx *c, const double *b, double *x, int max_iters, const int *skip = nullptr) {
    if (c->dist_solve) {      // rows split over the ranks: the two-level PCG on the rank's aggregates (ADMM_HIP_BIG=0: the Jacobi PCG of round 4)
        if (!c->big_tried) {
            // Every rank must take the SAME branch (the two solvers issue different collectives: a rank whose plan failed -- an allocation, an
            // upload -- would hang the others until the communicator times out): the first solve agrees on it with one sum all-reduce.
            const bool mine = ensure_big_plan(c);
            double v = mine ? 1.0 : 0.0;
            if (!c->big_agree.p && c->big_agree.alloc(1) != hipSuccess) return -1;
            if (hipMemcpyAsync(c->big_agree.p, &v, sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) return -1;
            if (int r = comm_allreduce(c, c->big_agree.p, 1)) return r < 0 ? -1 : r;
            if (hipMemcpyAsync(&v, c->big_agree.p, sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
            c->big_enabled = mine && v > (double)c->world - 0.5;
        }
        const int r = ensure_big_plan(c) ? launch_pcg_big(c, b, x, max_iters) : launch_pcg_dist(c, b, x, max_iters);
        return r ? -1 : 0;
    }
    if (c->oc_enabled) { OcRc rc; rc.skip = skip; return launch_pcg_onchip(c, b, x, max_iters, rc); }
    if (ensure_big_plan(c)) return launch_pcg_big(c, b, x, max_iters);
    hipStream_t st = c->stream;
    const SellA A = sell_arg(c->A);
    const int NB = c->NB;
    const double tol2 = c->pcg_tol * c->pcg_tol;
    const int seq = ++c->solve_seq;
    hipLaunchKernelGGL(k_cg_resid, dim3(NB), dim3(256), 0, st, A, c->m.p, c->dinv.p, b, x, c->cg_u.p, c->part_b.p, NB,
                       c->cg_scal.p, seq);
    volatile int *sig = c->h_sig;
    int launched = 0, chunks = 0;
    while (launched < max_iters) {
        const int n = std::min(kChunk, max_iters - launched);
        for (int it = launched; it < launched + n; ++it) {
            const CgScal *prev = c->cg_scal.p + (it & 1);
            CgScal *next = c->cg_scal.p + ((it + 1) & 1);
            hipLaunchKernelGGL(k_cg_spmv, dim3(NB), dim3(256), 0, st, A, c->m.p, c->cg_u.p, c->dinv.p, c->cg_w.p, c->part.p, NB, prev);
            hipLaunchKernelGGL(k_cg_vec, dim3(c->NBV), dim3(256), 0, st, it, c->nv, NB, c->part.p, c->part_b.p, prev, next, tol2,
                               c->counters.p, c->dinv.p, c->cg_p.p, c->cg_s.p, x, c->cg_u.p, c->cg_w.p, c->d_sig,
                               (it == launched + n - 1) ? 1 : 0);
        }
        launched += n;
        ++chunks;
        ++c->marks_expected;
        if (chunks >= 2 && launched < max_iters) {
            // wait until the chunk BEFORE the one just launched has drained, then look at the flag
            const int need = c->marks_expected - 1;
            long spins = 0;
            while (sig[kSigChunks] < need) {
                if (++spins > 2000000000L) return -1; // the GPU stopped making progress
            }
            if (sig[kSigConverged] == seq) break;
        }
    }
    c->last_launched_iters = launched;
    return 0;
}

// End projection of a finished solve on the soft modes (kernels.hpp: k_defl_*)
// have_resid: x is the iterate a launch-path solve has just returned and c->cg_u still holds D^-1 times ITS final residual (k_big_scatter): the
// projection takes the residual from there instead of forming b - A x again (ADMM_HIP_DEFL_RESID=0: always the product -- A/B, tests).
template <bool STOP> void launch_deflation_impl(admm_hip_ctx *c, const double *b, double *x, bool have_resid);
void launch_deflation(admm_hip_ctx *c, const double *b, double *x, bool have_resid = false) {      // (c->stop_dev: the STOP instantiations)
    if (c->stop_dev) launch_deflation_impl<true>(c, b, x, have_resid);
    else launch_deflation_impl<false>(c, b, x, have_resid);
}
template <bool STOP>
void launch_deflation_impl(admm_hip_ctx *c, const double *b, double *x, bool have_resid) {
    hipStream_t st = c->stream;
    const int NB = c->NB, k = c->defl_k;
    if (have_resid && c->defl_use_resid) {
        const int NBd = (c->nv + 256 * kDeflRV - 1) / (256 * kDeflRV);
        hipLaunchKernelGGL(k_defl_dots_r<STOP>, dim3(NBd), dim3(256), 0, st, c->nv, c->cg_u.p, c->dinv.p, k, c->defl_Z.p, c->defl_part.p, NBd, c->stop_dev);
        hipLaunchKernelGGL(k_defl_solve<STOP>, dim3(1), dim3(1024), 0, st, k, c->defl_part.p, NBd, c->defl_Ginv.p, c->defl_y.p, c->stop_dev);
        hipLaunchKernelGGL(k_defl_apply<STOP>, dim3(blocks_for(c->nv)), dim3(256), 0, st, c->nv, k, c->defl_Z.p, c->defl_y.p, x, c->stop_dev);
        return;
    }
    hipLaunchKernelGGL(k_defl_dots<STOP>, dim3(NB), dim3(256), 0, st, sell_arg(c->A), c->m.p, b, x, k, c->defl_Z.p, c->nv, c->defl_part.p, NB, c->stop_dev);
    hipLaunchKernelGGL(k_defl_solve<STOP>, dim3(1), dim3(1024), 0, st, k, c->defl_part.p, NB, c->defl_Ginv.p, c->defl_y.p, c->stop_dev);
    hipLaunchKernelGGL(k_defl_apply<STOP>, dim3(blocks_for(c->nv)), dim3(256), 0, st, c->nv, k, c->defl_Z.p, c->defl_y.p, x, c->stop_dev);
}

int launch_pcg_recycled_impl(admm_hip_ctx *c, const double *b, double *x, bool loop);
// The ADMM global solve with the recycled (Galerkin) warm start around the PCG (+ the end projection on the soft modes, when set).
int launch_pcg_recycled(admm_hip_ctx *c, const double *b, double *x, bool loop = true) {      // loop: see OcRc
    // The Galerkin step on the soft modes ALSO IN FRONT of the solves of a frame whose bit is set in defl_start (ADMM_HIP_DEFL_START=mask at
    // create; default 2 = the SECOND solve of a frame).  That solve is ADMM's transient -- the first dual update of the frame moves the
    // right-hand side along the soft modes, by an amount the corrections of earlier frames do not predict -- and it alone took 65-69 of a
    // frame's ~190 PCG iterations on the bench body whatever the recycled basis held; with the step in front 18-22 (experiments/iters_log.py),
    // 8.2 -> 5.4 iterations per solve over 200 frames, drift 3.9e-6 -> 3.2e-6 (profiles/r05_drift_start_projection.txt).  In front of the first
    // solve (mask 3) or the third (mask 6) it costs more than it saves.  Three small launches (k_defl_*), ~0.1 ms per frame.
    if (c->defl_start && !c->defl_start_hold && c->defl_k > 0 && c->rc_iter < 31 && ((c->defl_start >> c->rc_iter) & 1)) launch_deflation(c, b, x);
    c->defl_armed = false;
    c->big_rfin_valid = false;
    const int rc = launch_pcg_recycled_impl(c, b, x, loop);
    // (fused into k_pcg2's epilogue when the on-chip kernel ran WITH it -- launch_pcg2 says so: a solve that went there without the recycled
    // basis, ADMM_HIP_NO_RECYCLE=1, or down the launch path gets the separate kernels)
    if (rc == 0 && c->defl_k > 0 && !c->defl_armed) launch_deflation(c, b, x, c->big_rfin_valid);
    return rc;
}
int launch_pcg_recycled_impl(admm_hip_ctx *c, const double *b, double *x, bool loop) {
    const int s = c->rc_iter;
    if (!c->rc_enabled) return launch_pcg(c, b, x, c->pcg_max_iters);
    hipStream_t st = c->stream;
    RcBasis B{};
    // basis: the (up to) kRc most recent pairs of THIS frame.  (Adding the previous frame's pair at the same
    // index was measured: it does not help the first solves of a frame.)
    const int rc_pairs = c->rc_pairs;
    const int fr = c->rc_frame;
    if (c->rc_hist && c->oc_enabled && c->oc_plan) {   // (the history slots hold pairs in the on-chip kernel's internal row order: only it may project on them)
        // own pairs and the history of the same solve index, interleaved by expected value: own(s-1), prev(s), prev2(s), own(s-2),
        // prev(s+1), own(s-3), prev2(s+1), own(s-4)
        auto add = [&](int q, int frame, bool valid) { if (valid && B.cnt < rc_pairs) { B.E[B.cnt] = c->rc_Ef(q, frame); B.R[B.cnt] = c->rc_Rf(q, frame); ++B.cnt; } };
        const int H = admm_hip_ctx::kRcHist;
        add(s - 1, fr, s - 1 >= 0);
        add(s, fr - 1, s < H && s < c->rc_prev_valid);
        add(s, fr - 2, s < H && s < c->rc_prev2_valid);
        add(s - 2, fr, s - 2 >= 0);
        add(s + 1, fr - 1, s + 1 < H && s + 1 < c->rc_prev_valid);
        add(s - 3, fr, s - 3 >= 0);
        add(s + 1, fr - 2, s + 1 < H && s + 1 < c->rc_prev2_valid);
        add(s - 4, fr, s - 4 >= 0);
        OcRc rc; rc.on = true; rc.loop = loop; rc.B = B; rc.Eslot = c->rc_Ef(s, fr); rc.Rslot = c->rc_Rf(s, fr);
        const int r = launch_pcg_onchip(c, b, x, c->pcg_max_iters, rc);
        c->rc_iter = s + 1;
        return r;
    }
    for (int j = 1; j <= rc_pairs && s - j >= 0; ++j) { B.E[B.cnt] = c->rc_E(s - j); B.R[B.cnt] = c->rc_R(s - j); ++B.cnt; }
    // The first solves of a frame have few pairs of their own (the very first none: 85 of the 194 PCG iterations of a blob1m_mix
    // frame were its).  The free places of the basis go to the PREVIOUS frame's pairs of the same and the following solve indices
    // (slots s .. kRc - 1, not yet overwritten): in steady motion the first corrections of consecutive frames are nearly
    // parallel.  (E, A E) pairs stay exact whatever the state does -- the matrix of a scene never changes -- so this can only
    // help or do nothing.  Round 1 measured "no gain" for this with the Jacobi preconditioner; with the two-level one the CPU
    // prototype (experiments/first_solve_proto.py) gives 53 -> 19..26 iterations for the first solve, 30 -> 11..17 for the second.
    for (int q = s; q < kRc && q < c->rc_prev_valid && B.cnt < rc_pairs; ++q) { B.E[B.cnt] = c->rc_E(q); B.R[B.cnt] = c->rc_R(q); ++B.cnt; }
    if (c->oc_enabled) {   // (the plan's pairs live in its internal row order: k_rc_* cannot read them)   // projection, solve and the new pair in ONE persistent launch
        OcRc rc; rc.on = true; rc.loop = loop; rc.B = B; rc.Eslot = c->rc_E(s); rc.Rslot = c->rc_R(s);
        const int r = launch_pcg_onchip(c, b, x, c->pcg_max_iters, rc);
        c->rc_iter = s + 1;
        return r;
    }
    hipLaunchKernelGGL(k_rc_resid, dim3(c->NB), dim3(256), 0, st, sell_arg(c->A), c->m.p, b, x, c->rc_r0.p, c->rc_xs.p);
    if (B.cnt > 0) {
        hipLaunchKernelGGL(k_rc_dots, dim3(c->NBR), dim3(256), 0, st, c->nv, B, c->rc_r0.p, b, c->dinv.p, c->rc_part.p, c->NBR);
        hipLaunchKernelGGL(k_rc_solve, dim3(1), dim3(1024), 0, st, B.cnt, c->rc_part.p, c->NBR, c->pcg_tol * c->pcg_tol, c->rc_coef.p);
        hipLaunchKernelGGL(k_rc_apply, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, B, c->rc_coef.p, x);
    }
    const int rc = launch_pcg(c, b, x, c->pcg_max_iters);
    hipLaunchKernelGGL(k_rc_record, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, x, c->rc_xs.p, c->rc_r0.p, c->cg_u.p, c->dinv.p,
                       c->rc_E(s), c->rc_R(s));
    c->rc_iter = s + 1;
    return rc;
}

// face-vertex part of C^T v for the dynamic rows (dyn_collide.hpp): largest magnitude, integer scatter, apply
static void launch_ct_dyn(admm_hip_ctx *c, int nq, const int *qlist, int mode, const double *v, const int *dface, const double *dbary, double *out) {
    hipStream_t st = c->stream;
    const int gq = blocks_for(nq);
    hipLaunchKernelGGL(k_uz_ct_dyn_max, dim3(gq), dim3(256), 0, st, nq, qlist, c->uz_cn.p, v, dface, dbary, c->uz_dmax.p);
    hipLaunchKernelGGL(k_uz_ct_dyn, dim3(gq), dim3(256), 0, st, nq, qlist, mode, c->uz_cn.p, v, dface, dbary, c->uz_dmax.p, c->uz_dacc.p);
    hipLaunchKernelGGL(k_uz_ct_dyn_apply, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, c->uz_dmax.p, c->uz_dacc.p, out);
}

// Collider::detect, dynamic objects (src/Collider.hpp:166-168,192-201): refit every tet tree at x, then query the
// candidates against the objects in add_dynamic_collider order.  Payloads land in dyn_face / dyn_bary / dyn_n / dyn_dx.
int enqueue_dyn_detect(admm_hip_ctx *c, const double *x) {
    hipStream_t st = c->stream;
    const int nq = c->n_surf > 0 ? c->n_surf : c->nv;
    const int *qlist = c->n_surf > 0 ? c->surf_list.p : nullptr;
    if (hipMemsetAsync(c->dyn_face.p, 0xff, 3 * (size_t)c->nv * sizeof(int), st) != hipSuccess) return -1;
    for (auto &d : c->dyn) {
        hipLaunchKernelGGL(k_dyn_refit0, dim3(blocks_for(d->m.tt.n[0])), dim3(256), 0, st, d->m, x);
        int l = 1;
        for (; l < d->m.tt.n_levels && d->m.tt.n[l] > 256; ++l)
            hipLaunchKernelGGL(k_dyn_refit_up, dim3(blocks_for(d->m.tt.n[l])), dim3(256), 0, st, d->m, l);
        if (l < d->m.tt.n_levels) hipLaunchKernelGGL(k_dyn_refit_top, dim3(1), dim3(256), 0, st, d->m, l);
        hipLaunchKernelGGL(k_dyn_query, dim3((nq + 31) / 32), dim3(256), 0, st, d->m, nq, qlist, x, c->dyn_face.p, c->dyn_bary.p,
                           c->dyn_n.p, c->dyn_dx.p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// How many column solves may run side by side: as many instances of k_pcg2 as the chip holds at once (every block of a persistent
// kernel must be resident: the occupancy query decides, never the switch), at most 8.  1 = the main stream only.  The lanes cycle
// through the stream priorities: the runtime multiplexes streams of ONE priority on four hardware queues, where two lanes on the same
// queue serialise (measured, 243 launches on the 20 k-vertex cube: 231 ms on the main stream; equal priorities 116 / 84-152 / 116 / 91 ms
// on 2 / 3 / 4 / 8 lanes depending on which lanes collide; cycled priorities 117 / 89 / 70 / 49 / 38 ms on 2 / 3 / 4 / 6 / 8 lanes --
// profiles/r05_uzawa_column_lanes.txt).  Final assignment of the priorities: uz_make_lanes.
int uz_lane_fit(admm_hip_ctx *c) {      // instances of k_pcg2 the chip holds at once
    if (c->uz_fit >= 0) return c->uz_fit;
    int per_cu = 0;      // (the lanes run the generic instance, the loop's own solves the hot one: the tighter of the two)
    for (int hot = 0; hot < 2; ++hot) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pcg2_instance(c->oc_T, hot != 0), c->oc_T, c->oc_lds) != hipSuccess) { (void)hipGetLastError(); n = 0; }
        per_cu = hot ? std::min(per_cu, n) : n;
    }
    if (per_cu <= 0) per_cu = 1;
    c->uz_fit = (int)std::min<long long>(64, (long long)per_cu * c->n_cus / std::max(1, c->oc_G));
    return c->uz_fit;
}
int uz_lane_count(admm_hip_ctx *c, int launches) {
    if (!c->oc_enabled || c->dist_solve || c->oc_debug || c->oc_prof.p || launches < 2) return 1;
    if (c->uz_lanes_cfg == 1) return 1;
    return std::max(1, std::min(std::min(c->uz_lanes_cfg > 0 ? c->uz_lanes_cfg : 8, uz_lane_fit(c)), launches));
}

// The lanes of uz_columns_on_lanes: stream, event and one slab of device memory each (set up at create for scenes with colliders, so
// that the first touchdown does not pay for it).  0 ok.
int uz_make_lanes(admm_hip_ctx *c, int L) {
    typedef admm_hip_ctx::OcLane Lane;
    if (!c->uz_fork && hipEventCreateWithFlags(&c->uz_fork, hipEventDisableTiming) != hipSuccess) return -1;
    while ((int)c->uz_lanes.size() < L) {
        c->uz_lanes.emplace_back(new Lane());
        Lane &ln = *c->uz_lanes.back();
        // the runtime keeps separate hardware queues per stream priority: lanes of different priority never share one
        int plo = 0, phi = 0;
        (void)hipDeviceGetStreamPriorityRange(&plo, &phi);      // (lowest, highest): numerically phi <= plo
        const int idx = (int)c->uz_lanes.size() - 1, span = plo - phi + 1;
        // (highest and lowest first, three lanes each, then the default priority: that class also carries the context's own stream and the
        //  process's null stream -- a fourth lane in one class shares a hardware queue with another and the two serialise)
        int prio = 0;
        if (span > 2) { static const int cls[8] = {0, 1, 0, 1, 0, 1, 2, 2}; const int k = cls[idx & 7]; prio = k == 0 ? phi : k == 1 ? plo : (phi + plo) / 2; }
        else if (span > 1) prio = (idx & 1) ? plo : phi;
        if (hipStreamCreateWithPriority(&ln.st, hipStreamNonBlocking, prio) != hipSuccess || hipEventCreateWithFlags(&ln.done, hipEventDisableTiming) != hipSuccess) return -1;
        size_t off = 0;
        auto take = [&off](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_ubuf = take(c->oc_ubuf.n * 8), o_part = take(c->oc_part.n * 8), o_cbuf = take(c->oc_cbuf.n * 8), o_bar = take(c->oc_bar.n * 4),
                     o_flags = take(c->oc_flags.n * 8), o_scal = take(2 * sizeof(CgScal)), o_cnt = take(c->counters.n * 4),
                     o_b = take(c->n3 * 8), o_x = take(c->n3 * 8), o_u = take(c->n3 * 8);
        // (cleared ON the lane's stream: its first operation makes the runtime create the hardware queue behind it, ~5 ms each -- here, not in the first batch)
        if (ln.slab.alloc(off) != hipSuccess || hipMemsetAsync(ln.slab.p, 0, off, ln.st) != hipSuccess || hipStreamSynchronize(ln.st) != hipSuccess) return -1;
        char *p = ln.slab.p;
        ln.ubuf = (double *)(p + o_ubuf); ln.part = (double *)(p + o_part); ln.cbuf = (double *)(p + o_cbuf); ln.bar = (unsigned *)(p + o_bar);
        ln.flags = (unsigned long long *)(p + o_flags); ln.scal = (CgScal *)(p + o_scal); ln.counters = (int *)(p + o_cnt);
        ln.b = (double *)(p + o_b); ln.x = (double *)(p + o_x); ln.u = (double *)(p + o_u);
    }
    return 0;
}

// Column solves dealt round-robin onto L lanes: fork from the context's stream, three vertices per launch, one `done` event per lane.
// Does NOT wait.  0 ok, -1 error.
int uz_lanes_enqueue(admm_hip_ctx *c, const std::vector<int> &verts, const std::vector<int> &slots, int n_verts, int L, int max_iters, int *launched) {
    typedef admm_hip_ctx::OcLane Lane;
    const int nv = c->nv;
    if (uz_make_lanes(c, L)) return -1;
    if (hipEventRecord(c->uz_fork, c->stream) != hipSuccess) return -1;
    for (int l = 0; l < L; ++l) {
        Lane &ln = *c->uz_lanes[l];
        if (hipStreamWaitEvent(ln.st, c->uz_fork, 0) != hipSuccess) return -1;
        if (hipMemsetAsync(ln.counters, 0, c->counters.n * sizeof(int), ln.st) != hipSuccess || hipMemsetAsync(ln.bar, 0, c->oc_bar.n * sizeof(unsigned), ln.st) != hipSuccess) return -1;
        // the findings that change how k_pcg2 solves (smoother given up, trust revoked) hold for the lanes too
        if (hipMemcpyAsync(ln.counters + kCntSmootherOff, c->counters.p + kCntSmootherOff, (kCntTrustRevoked + 1 - kCntSmootherOff) * sizeof(int), hipMemcpyDeviceToDevice, ln.st) != hipSuccess) return -1;
    }
    int n = 0;
    for (int k = 0; k < n_verts; k += 3, ++n) {
        Lane &ln = *c->uz_lanes[n % L];
        int v[3], sl[3];
        for (int j = 0; j < 3; ++j) { v[j] = k + j < n_verts ? verts[k + j] : -1; sl[j] = v[j] >= 0 ? slots[k + j] : -1; }
        hipLaunchKernelGGL(k_uz_unit_rhs_x0, dim3(blocks_for(c->n3)), dim3(256), 0, ln.st, (int)c->n3, v[0], v[1], v[2], ln.b, ln.x);
        if (launch_pcg2(c, ln.b, ln.x, max_iters, OcRc(), &ln)) return -1;
        hipLaunchKernelGGL(k_uz_store_cols, dim3(blocks_for(nv)), dim3(256), 0, ln.st, nv, ln.x, c->uzc_cols.p, sl[0], sl[1], sl[2]);
        c->uzc_col_solves += 1;
    }
    *launched = n;
    for (int l = 0; l < L; ++l)
        if (hipEventRecord(c->uz_lanes[l]->done, c->uz_lanes[l]->st) != hipSuccess) return -1;
    return 0;
}
int uz_lanes_converged(admm_hip_ctx *c, int L, int *converged) {      // (after the lanes are done) solves that met their tolerance
    int conv = 0;
    for (int l = 0; l < L; ++l) {
        int v = 0;
        if (hipMemcpy(&v, c->uz_lanes[l]->counters + kCntConverged, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        conv += v;
    }
    *converged = conv;
    return 0;
}

// The batch of uz_ensure_columns on L side streams.  *converged = solves that met their tolerance.  0 ok, -1 error.
int uz_columns_on_lanes(admm_hip_ctx *c, const std::vector<int> &miss, const std::vector<int> &slots, int n_missing, int L, int max_iters,
                        int *launched, int *converged) {
    const bool dbg = c->uz_lanes_debug;
    const auto t_enq0 = std::chrono::steady_clock::now();
    if (uz_lanes_enqueue(c, miss, slots, n_missing, L, max_iters, launched)) return -1;
    for (int l = 0; l < L; ++l)
        if (hipStreamWaitEvent(c->stream, c->uz_lanes[l]->done, 0) != hipSuccess) return -1;
    const auto t_enq1 = std::chrono::steady_clock::now();
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (dbg) fprintf(stderr, "[uz_lanes] ctx %p frame %d: %d solves on %d streams: enqueued in %.2f ms, done after %.2f ms\n", (void *)c, c->rc_frame, *launched, L,
                     std::chrono::duration<double, std::milli>(t_enq1 - t_enq0).count(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq0).count());
    if (uz_lanes_converged(c, L, converged)) return -1;
    c->uzc_lane_batches += 1;
    return 0;
}

// Room for `top` columns in uzc_cols (doubling, at least 64 columns, never beyond the cap; the columns move once).  Must not be called
// while lanes are writing columns.  1 ok, 0 no room, -1 error.
int uz_grow_cols(admm_hip_ctx *c, size_t top) {
    const int nv = c->nv;
    if (top * (size_t)nv <= c->uzc_cols.n) return 1;
    const size_t have = c->uzc_cols.n / (size_t)nv, cols = std::min(c->uzc_cap, std::max<size_t>(top, std::max<size_t>(64, 2 * have)));
    if (cols < top) return 0;
    DevBuf<double> nb;
    if (nb.alloc(cols * (size_t)nv) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (c->uzc_n > 0 && hipMemcpy(nb.p, c->uzc_cols.p, sizeof(double) * (size_t)c->uzc_n * nv, hipMemcpyDeviceToDevice) != hipSuccess) return -1;
    c->uzc_cols = std::move(nb);
    return 1;
}

double uz_column_tol(const admm_hip_ctx *c) {      // a hundredth of the solver's own, never looser than 1e-10
    return std::min(0.01 * c->pcg_tol, 1e-10);
}

// LOOK-AHEAD.  The columns in flight are done (block: wait for them): commit their slots, or give the look-ahead up when a solve missed
// its tolerance.  1 = nothing in flight any more, 0 = still running (block == false), -1 error.
int uz_ahead_harvest(admm_hip_ctx *c, bool block) {
    if (c->pf_v.empty()) return 1;
    for (int l = 0; l < c->pf_lanes; ++l) {
        const hipError_t e = block ? hipEventSynchronize(c->uz_lanes[l]->done) : hipEventQuery(c->uz_lanes[l]->done);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
        if (e != hipSuccess) return -1;
    }
    int conv = 0;
    if (uz_lanes_converged(c, c->pf_lanes, &conv)) return -1;
    const bool aborted = c->h_sig && c->h_sig[kSigAbort];
    { if (c->uz_lanes_debug) fprintf(stderr, "[uz_ahead] ctx %p frame %d: harvest (%s) of %d columns: %d of %d launches converged%s\n", (void *)c, c->rc_frame, block ? "waited" : "polled",
                       (int)c->pf_v.size(), conv, c->pf_launched, aborted ? ", ABORTED" : ""); }
    if (!aborted && conv == c->pf_launched) {
        for (size_t k = 0; k < c->pf_v.size(); ++k) c->uzc_slot_h[c->pf_v[k]] = c->pf_slot[k];
        if (hipMemcpy(c->uzc_slot.p, c->uzc_slot_h.data(), sizeof(int) * (size_t)c->nv, hipMemcpyHostToDevice) != hipSuccess) return -1;
        c->pf_columns += (long long)c->pf_v.size();
    } else {      // (their slots stay unused; the vertices get columns the ordinary way when they touch)
        c->pf_on = false;
        if (!aborted) c->uzc_unconverged += c->pf_launched;
    }
    c->pf_v.clear(); c->pf_slot.clear(); c->pf_launched = 0;
    return 1;
}

// Launch the column solves of the `count` vertices k_uz_near listed, on the lanes, WITHOUT waiting: they run beside the ADMM loop
// (lanes + the loop's own k_pcg2 <= what the chip holds).  0 ok (also when there was nothing to do), -1 error.
int uz_ahead_launch(admm_hip_ctx *c, int count) {
    const bool dbg = c->uz_lanes_debug;
    if (count <= 0 || !c->pf_v.empty()) return 0;
    // Fewer lanes than a batch the loop WAITS for: the loop's own persistent kernels (k_pcg2, the Schur CG with up to 100 KB of LDS per
    // block) must find their CUs beside the lanes' blocks.
    constexpr int ahead_lanes = 4;
    const int L = std::min(std::min(c->uz_lanes_cfg > 0 ? c->uz_lanes_cfg : 8, ahead_lanes), uz_lane_fit(c) - 1);
    if (L < 1) { c->pf_on = false; return 0; }
    std::vector<int> list(count);
    if (hipMemcpy(list.data(), c->pf_list.p, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    std::sort(list.begin(), list.end());
    list.erase(std::remove_if(list.begin(), list.end(), [c](int v) { return v < 0 || v >= c->nv || c->uzc_slot_h[v] >= 0; }), list.end());
    const size_t room = c->uzc_cap - (size_t)c->uzc_n;
    const size_t n = std::min(std::min(list.size(), room), (size_t)3 * 512);
    if (n == 0) return 0;
    list.resize(n);
    const int g = uz_grow_cols(c, (size_t)c->uzc_n + n);
    if (g <= 0) return g;       // no room: the look-ahead just does not happen
    std::vector<int> slots(n);
    for (size_t k = 0; k < n; ++k) slots[k] = c->uzc_n + (int)k;
    const double keep_tol = c->pcg_tol;
    c->pcg_tol = uz_column_tol(c);
    int launched = 0;
    const int rc = uz_lanes_enqueue(c, list, slots, (int)n, L, std::max(c->pcg_max_iters, 2000), &launched);
    c->pcg_tol = keep_tol;
    if (rc) return -1;
    c->uzc_n += (int)n;      // (reserved: committed by uz_ahead_harvest)
    c->pf_v = list; c->pf_slot = slots; c->pf_launched = launched; c->pf_lanes = L;
    c->pf_batches += 1;
    if (dbg) fprintf(stderr, "[uz_ahead] ctx %p frame %d: %d columns (%d launches) in flight on %d lanes\n", (void *)c, c->rc_frame, (int)n, launched, L);
    return 0;
}

// Columns of K^-1 for the vertices listed in uzc_miss (n_missing of them): three per PCG launch (one per axis), at a tolerance two
// orders below the context's.  1 = every active vertex now has its column, 0 = the cache is full (this solve uses the PCG), -1 error.
int uz_ensure_columns(admm_hip_ctx *c, int n_missing) {
    if (n_missing <= 0) return 1;
    hipStream_t st = c->stream;
    const int nv = c->nv;
    std::vector<int> miss(n_missing);
    if (hipMemcpy(miss.data(), c->uzc_miss.p, sizeof(int) * (size_t)n_missing, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (!c->pf_v.empty()) {      // columns in flight (look-ahead): wait for them -- some of the missing ones may be among them
        c->pf_waits += 1;
        if (uz_ahead_harvest(c, true) < 0) return -1;
        if (c->h_sig && c->h_sig[kSigAbort]) return -2;
    }
    if (c->pf_batches > 0) {     // (the list was made with the slot table of BEFORE this solve's harvest)
        miss.erase(std::remove_if(miss.begin(), miss.end(), [c](int v) { return c->uzc_slot_h[v] >= 0; }), miss.end());
        n_missing = (int)miss.size();
        if (n_missing == 0) return 1;
    }
    // slots for the new columns: fresh ones while the cache has room; a FULL cache gives up the columns of every vertex that is not
    // active in this solve (contacts that moved on -- a rolling or sliding body -- must not pin the cache for good)
    std::vector<int> slots;
    const size_t fresh = std::min<size_t>((size_t)n_missing, c->uzc_cap - (size_t)c->uzc_n);
    for (size_t k = 0; k < fresh; ++k) slots.push_back(c->uzc_n + (int)k);
    std::vector<int> evicted;       // vertices whose columns are given up (committed only if the solves succeed)
    if (slots.size() < (size_t)n_missing) {
        std::vector<int> act(c->uzc_n_act);
        if (c->uzc_n_act > 0 && hipMemcpy(act.data(), c->uzc_act.p, sizeof(int) * (size_t)c->uzc_n_act, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        std::vector<char> is_act(nv, 0);
        for (int v : act) is_act[v] = 1;
        for (int v = 0; v < nv && slots.size() < (size_t)n_missing; ++v)
            if (c->uzc_slot_h[v] >= 0 && !is_act[v]) { slots.push_back(c->uzc_slot_h[v]); evicted.push_back(v); }
        if (slots.size() < (size_t)n_missing) return 0;      // the active set itself does not fit: this solve uses the PCG
    }
    const size_t top = (size_t)*std::max_element(slots.begin(), slots.end()) + 1;
    { const int g = uz_grow_cols(c, top); if (g <= 0) return g; }      // no room: this solve uses the PCG
    const double keep_tol = c->pcg_tol;
    c->pcg_tol = uz_column_tol(c);
    int rc = 1;
    // the solver's counters before the batch: the solves of this step that met their tolerance -- every column solve must add one --
    // and the totals admm_hip_solve_totals reports, which the column solves must not show up in (the caller's solves only)
    int cnt0[kCntRing], tot0[kCntTotalsLen];
    if (hipMemcpy(cnt0, c->counters.p, sizeof(cnt0), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(tot0, c->counters.p + kCntTotals, sizeof(tot0), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int launched = 0, lane_conv = -1;
    const int max_col_iters = c->uzc_test_iters > 0 ? c->uzc_test_iters : std::max(c->pcg_max_iters, 2000);
    const int lanes = uz_lane_count(c, (n_missing + 2) / 3);
    if (lanes >= 2) { if (uz_columns_on_lanes(c, miss, slots, n_missing, lanes, max_col_iters, &launched, &lane_conv)) rc = -1; }
    else
    for (int k = 0; k < n_missing && rc == 1; k += 3) {
        int v[3], sl[3];
        for (int j = 0; j < 3; ++j) { v[j] = k + j < n_missing ? miss[k + j] : -1; sl[j] = v[j] >= 0 ? slots[k + j] : -1; }
        if (hipMemsetAsync(c->uz_q1.p, 0, c->n3 * sizeof(double), st) != hipSuccess || hipMemsetAsync(c->uz_q2.p, 0, c->n3 * sizeof(double), st) != hipSuccess) { rc = -1; break; }
        hipLaunchKernelGGL(k_uz_unit_rhs, dim3(1), dim3(1), 0, st, v[0], v[1], v[2], c->uz_q1.p);
        if (launch_pcg(c, c->uz_q1.p, c->uz_q2.p, max_col_iters)) { rc = -1; break; }
        hipLaunchKernelGGL(k_uz_store_cols, dim3(blocks_for(nv)), dim3(256), 0, st, nv, c->uz_q2.p, c->uzc_cols.p, sl[0], sl[1], sl[2]);
        c->uzc_col_solves += 1; ++launched;
    }
    c->pcg_tol = keep_tol;
    if (rc == 1 && hipStreamSynchronize(st) != hipSuccess) rc = -1;
    const bool aborted = c->h_sig && c->h_sig[kSigAbort];     // a grid barrier of one of the solves timed out
    // Did every column solve meet its tolerance?  A column that ran out of iterations would be a wrong Schur operator for every later
    // solve: the batch is then not committed and this solve applies A^-1 by inner PCG solves (rc 0), counted in uzc_unconverged.
    bool all_converged = true;
    if (rc == 1 && !aborted && lane_conv >= 0) all_converged = lane_conv == launched;      // (the lanes count in their own counters: nothing to restore)
    else if (rc == 1 && !aborted) {
        int cnt1[kCntRing];
        if (hipMemcpy(cnt1, c->counters.p, sizeof(cnt1), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
        else {
            all_converged = cnt1[kCntConverged] - cnt0[kCntConverged] == launched;
            for (int w : {kCntIters, kCntMaxIters, kCntConverged}) cnt1[w] = cnt0[w];      // the step's own statistics do not count the columns either
            if (hipMemcpy(c->counters.p, cnt1, kCntStepWords * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(c->counters.p + kCntTotals, tot0, sizeof(tot0), hipMemcpyHostToDevice) != hipSuccess) rc = -1;
        }
    }
    // (the evicted vertices' slots may have been overwritten whatever happened: they are given up in every case)
    for (int v : evicted) c->uzc_slot_h[v] = -1;
    if (rc == 1 && !aborted && all_converged) {
        for (int k = 0; k < n_missing; ++k) c->uzc_slot_h[miss[k]] = slots[k];
        c->uzc_n += (int)fresh;
    } else if (rc == 1 && !aborted) { rc = 0; c->uzc_unconverged += launched; }
    else rc = aborted ? -2 : -1;      // -2: the caller takes the recovery path of an aborted on-chip solve (kStepAborted)
    if (hipMemcpy(c->uzc_slot.p, c->uzc_slot_h.data(), sizeof(int) * (size_t)nv, hipMemcpyHostToDevice) != hipSuccess) return -1;
    c->uzc_evictions += (long long)evicted.size();
    return rc;
}

// UzawaCG::solve (src/UzawaCG.hpp:57-125).  The Schur-CG loop is enqueued in chunks, its stop decision is taken on the device; A^-1 of
// every iteration through cached columns of K^-1 (kernels.hpp: k_uz_cols_apply, k_uzc_*) or, without them, an on-chip PCG solve.
// Returns the reference's iteration count via *iters.
int launch_uzawa(admm_hip_ctx *c, const double *b, double *x, int *iters, bool loop = true) {
    hipStream_t st = c->stream;
    const int nv = c->nv, gv = blocks_for(nv);
    *iters = 1;
    int nh = 0;
    const bool dyn = !c->dyn.empty();
    const int *dface = dyn ? c->dyn_face.p : nullptr;
    const double *dbary = dyn ? c->dyn_bary.p : nullptr;
    const int nq = c->n_surf > 0 ? c->n_surf : nv, gq = blocks_for(nq);
    const int *qlist = c->n_surf > 0 ? c->surf_list.p : nullptr;
    if (c->uz_freeze && c->uz_detected) nh = c->uz_last_hits;     // frozen active set: the rows of this step's first detect
    else if (c->obst.n > 0 || dyn) {
        const bool first_detect = !c->uz_detected;
        c->uz_detected = true;
        // Collider::detect at the current iterate + ConstraintSet::make_matrix (ck = sqrt(constraint_w))
        const double ck = std::sqrt(std::max(0.0, c->constraint_w));
        if (c->timing && hipEventRecord(c->ev_coll0, st) != hipSuccess) return -1;
        // (kCntHits: cleared by k_uz_act_compact after it has been read when the column cache is on -- see below)
        if ((!c->uzc_on || !c->uz_hits_cleared) && hipMemsetAsync(c->counters.p + kCntHits, 0, sizeof(int), st) != hipSuccess) return -1;
        c->uz_hits_cleared = false;
        if (c->obst.n > 0)
            hipLaunchKernelGGL(k_uz_detect, dim3(gv), dim3(256), 0, st, nv, x, c->obst, ck, c->uz_cn.p, c->uz_cc.p, c->counters.p + kCntHits,
                               c->n_surf > 0 ? c->surf_mask.p : nullptr);
        else if (hipMemsetAsync(c->uz_cn.p, 0, c->n3 * sizeof(double), st) != hipSuccess ||
                 hipMemsetAsync(c->uz_cc.p, 0, nv * sizeof(double), st) != hipSuccess) return -1;
        if (dyn) {
            if (enqueue_dyn_detect(c, x)) return -1;
            hipLaunchKernelGGL(k_dyn_rows, dim3(gq), dim3(256), 0, st, nq, qlist, ck, c->uz_cn.p, c->uz_cc.p, c->dyn_face.p, c->dyn_n.p,
                               c->counters.p + kCntHits);
        }
        if (c->timing && hipEventRecord(c->ev_coll1, st) != hipSuccess) return -1;
        int info[3] = {0, 0, 0};
        if (c->uzc_on) {   // the vertices C^T touches (ascending), and those without a cached column; the hit count rides along
            if (dyn) {     // (a dynamic row also activates the three vertices of its face: flag pass)
                if (hipMemsetAsync(c->uzc_flag.p, 0, nv, st) != hipSuccess) return -1;
                hipLaunchKernelGGL(k_uz_act_flags, dim3(gv), dim3(256), 0, st, nv, c->uz_cn.p, dface, c->uzc_flag.p);
            }
            const unsigned char *fl = dyn ? c->uzc_flag.p : (const unsigned char *)nullptr;
            const int nbc = (nv + 4095) / 4096;
            if (nbc > c->uzc_one_block_max && c->uzc_counts.n < (size_t)2 * nbc && c->uzc_counts.alloc((size_t)2 * nbc) != hipSuccess) return -1;
            // ascending list of the flagged vertices (flag == nullptr: of the vertices whose row of C is not zero)
            auto list = [&](const unsigned char *flag, int *out, int *miss_out, int *pos_out, int *info_out, int *hits) {
                if (nbc <= c->uzc_one_block_max)
                    hipLaunchKernelGGL(k_uz_act_compact, dim3(1), dim3(1024), 0, st, nv, flag, c->uzc_slot.p, out, miss_out, pos_out, info_out, c->uz_cn.p, hits);
                else {      // many blocks: counts, then placement behind the blocks before (kernels.hpp)
                    hipLaunchKernelGGL(k_uz_act_count, dim3(nbc), dim3(1024), 0, st, nv, flag, c->uzc_slot.p, c->uz_cn.p, c->uzc_counts.p);
                    hipLaunchKernelGGL(k_uz_act_scatter, dim3(nbc), dim3(1024), 0, st, nv, flag, c->uzc_slot.p, c->uz_cn.p, c->uzc_counts.p, out, miss_out, pos_out, info_out, hits);
                }
            };
            list(fl, c->uzc_act.p, c->uzc_miss.p, c->uzc_pos.p, c->uzc_info.p, c->counters.p + kCntHits);
            c->uz_hits_cleared = true;
            if (hipMemcpyAsync(info, c->uzc_info.p, sizeof(info), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
            if (dyn && c->uzp_enabled) {     // the ROWS (vertices that carry a row), for the persistent Schur kernel on coupled rows (k_uzc_schur)
                if (!c->uzp_rowlist.p && (c->uzp_rowlist.alloc((size_t)3 * nv + 8) != hipSuccess)) { (void)hipGetLastError(); c->uzp_enabled = false; }
                else {
                    int *rl = c->uzp_rowlist.p;      // [nv] rows | [nv] scratch (missing) | [nv] scratch (places) | [8] info
                    list(nullptr, rl, rl + nv, rl + 2 * (size_t)nv, rl + 3 * (size_t)nv, nullptr);
                    if (hipMemcpyAsync(c->uzp_rowinfo, rl + 3 * (size_t)nv, 2 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
                }
            }
        } else if (hipMemcpyAsync(&nh, c->counters.p + kCntHits, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
        // LOOK-AHEAD, once per step (its first detect), passive objects: which vertices will touch within pf_frames frames at their current
        // speed and have no column of K^-1?  (c->v: the velocity after the explicit forces of this step.)  Their columns are solved on the
        // lanes while the ADMM loop goes on, so that the touchdown finds them in the cache.
        int pf_count = 0;
        const bool pf_scan = c->uzc_on && c->pf_on && c->in_step && first_detect && c->obst.n > 0 && c->oc_enabled && c->pf_v.empty() && (size_t)c->uzc_n < c->uzc_cap;
        if (pf_scan) {
            if (hipMemsetAsync(c->pf_list.p + nv, 0, sizeof(int), st) != hipSuccess) return -1;
            hipLaunchKernelGGL(k_uz_near, dim3(gv), dim3(256), 0, st, nv, x, c->v.p, c->obst, c->pf_frames * c->dt, c->uzc_slot.p,
                               c->n_surf > 0 ? c->surf_mask.p : nullptr, c->pf_list.p, c->pf_list.p + nv);
            if (hipMemcpyAsync(&pf_count, c->pf_list.p + nv, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
        }
        if (hipStreamSynchronize(st) != hipSuccess) return -1;
        if (c->h_sig && c->h_sig[kSigAbort]) return -2;      // an earlier persistent launch (Schur CG, on-chip PCG) was given up: recovery path
        if (c->uzc_on && first_detect && !c->pf_v.empty() && uz_ahead_harvest(c, false) < 0) return -1;      // (done by now? then commit; never waits here)
        if (c->uzc_on) nh = info[2];
        if (c->uzc_on) {
            c->uzc_n_act = info[0];
            c->uzc_usable = false;
            if (nh > 0) { const int rc = uz_ensure_columns(c, info[1]); if (rc < 0) return rc; c->uzc_usable = rc == 1; }
            if (pf_scan && pf_count > 0 && uz_ahead_launch(c, pf_count) < 0) return -1;
        }
        if (c->timing) { float ms = 0.f; if (hipEventElapsedTime(&ms, c->ev_coll0, c->ev_coll1) == hipSuccess) c->coll_ms_step += ms; }
    }
    c->uz_last_hits = nh; c->uz_rows_total += nh;
    if (nh != c->uz_prev_hits) { // multipliers are kept only while the number of rows is unchanged (UzawaCG.hpp:74)
        if (hipMemsetAsync(c->uz_y.p, 0, nv * sizeof(double), st) != hipSuccess) return -1;
        c->uz_prev_hits = nh;
    }
    if (nh == 0) return launch_pcg_recycled(c, b, x, loop); // no constraints: one prefactored solve (:78-81)
    hipLaunchKernelGGL(k_uz_ct, dim3(gv), dim3(256), 0, st, nv, 0, b, c->uz_cn.p, c->uz_y.p, c->uz_q1.p);       // q1 = b - C^T y
    if (dyn) launch_ct_dyn(c, nq, qlist, 0, c->uz_y.p, dface, dbary, c->uz_q1.p);
    // x = A^-1 q1, warm-started from the current x and -- like the contact-free solves -- projected on the recycled pairs first
    c->defl_start_hold = true;      // (with constraint rows the first solve's right-hand side b - C^T y is the multipliers' kick, not the soft-mode
                                    // transient of the free solve: the step in front buys nothing there -- cube100k_uzawa_floor 1 357 against 1 396)
    const int rc_first = launch_pcg_recycled(c, c->uz_q1.p, x, loop);
    c->defl_start_hold = false;
    if (rc_first) return -1;
    hipLaunchKernelGGL(k_uz_resid, dim3(gv), dim3(256), 0, st, nv, x, c->uz_cn.p, c->uz_cc.p, c->uz_r.p, c->uz_d.p, dface, dbary, c->uz_scal.p);
    const double tol2 = c->uz_tol * c->uz_tol;
    UzScal h{};
    // Schur-complement CG (src/UzawaCG.hpp:92-120).  The stop decision is taken on the device (k_uz_beta / k_uz_alpha set
    // UzScal::stop; every later kernel of the loop -- the inner PCG launch included -- is then a no-op), so the host does
    // not synchronise per iteration: it enqueues as many iterations as the previous solve needed, looks at the flag, and
    // continues two at a time.
    const int *stop_flag = &c->uz_scal.p->stop;
    int launched = 0;
    int chunk = std::max(1, std::min(c->uz_max_iters, c->uz_prev_iters > 0 ? c->uz_prev_iters + 1 : 4));
    // Only the persistent kernel (k_pcg2) and the column kernels honour the device-side stop flag; on the launch-per-iteration
    // inner-solve path an iteration enqueued behind the stop would run a full dead solve: one at a time there.
    const bool use_cols = c->uzc_on && c->uzc_usable;      // every active vertex has its column of K^-1: no inner solves
    // ... and the iterations themselves run on the active vertices only (k_uzc_*): the active x active block of K^-1 is extracted
    // once per solve, x is updated once after the loop from the multiplier update y - y0
    const int n_act = c->uzc_n_act, ldG = (n_act + 63) & ~63;
    bool compact = use_cols && c->uzc_compact && n_act > 0 && n_act <= c->uzc_compact_max;      // (G is n_act^2 doubles: 512 MB at the limit)
    int nseg = 1, seg_len = n_act;
    if (compact) {
        const int nbi = (n_act + 63) / 64;
        nseg = std::max(1, std::min(std::min(16, nbi), 256 / nbi));
        seg_len = (n_act + nseg - 1) / nseg;
        const size_t needG = (size_t)n_act * ldG, needP = (size_t)nseg * n_act * 3;
        if (c->uzc_G.n < needG && c->uzc_G.alloc(needG + needG / 4) != hipSuccess) { (void)hipGetLastError(); compact = false; }
        if (compact && c->uzc_part.n < needP && c->uzc_part.alloc(2 * needP) != hipSuccess) return -1;
        if (compact && c->uzc_gq.n < (size_t)3 * n_act && c->uzc_gq.alloc((size_t)6 * n_act) != hipSuccess) return -1;
    }
    // Passive rows only, <= 1024 active vertices: the whole Schur CG is ONE persistent launch (uz_persist.hpp; ADMM_HIP_UZ_PERSIST=0:
    // two launches per iteration, as before).  Decided before the extraction: the persistent kernel takes S_ij = G_ij (n_i . n_j).
    bool persist_launched = false;
    // n_rows: the rows of the Schur CG -- the active vertices themselves with passive rows only; with dynamic rows (a row couples its hit
    // vertex and the three vertices of a face) the vertices that carry a row, listed next to the active ones in the detect phase
    const int n_rows = dyn ? c->uzp_rowinfo[0] : n_act, ldS = (n_rows + 63) & ~63;
    bool persist = compact && c->uzp_enabled && n_rows > 0 && n_rows <= std::min(kUzpMaxAct, c->uzc_one_max) && c->uz_max_iters > 0 && c->uz_max_iters < 250 &&
                   (!dyn || c->uzp_rowlist.p);
    if (persist) {
        const int R = c->uzp_rows > 0 ? c->uzp_rows : uzp_rows_per_block(n_rows), NB = (n_rows + R - 1) / R;
        if (!c->uzp_dbox.p) {
            if (c->uzp_dbox.alloc(2 * kUzpMaxAct) != hipSuccess || c->uzp_sbox.alloc(2 * kUzpMaxBlocks * 8) != hipSuccess || c->uzp_abort.alloc(1) != hipSuccess ||
                c->uzp_dbox.zero() != hipSuccess || c->uzp_sbox.zero() != hipSuccess || c->uzp_abort.zero() != hipSuccess ||
                hipFuncSetAttribute((const void *)k_uz_persist, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256) != hipSuccess) { (void)hipGetLastError(); persist = false; c->uzp_enabled = false; }
        }
        // (its blocks hand granules to each other: all of them must be resident at once -- one block per CU at this LDS size)
        if (persist && (NB > kUzpMaxBlocks || NB > c->n_cus || uzp_lds_bytes(n_rows, R) > (size_t)(160 * 1024 - 256))) persist = false;
        if (persist && dyn && c->uzp_S.n < (size_t)n_rows * ldS && c->uzp_S.alloc((size_t)n_rows * ldS * 2) != hipSuccess) { (void)hipGetLastError(); persist = false; }
    }
    if (compact) {
        if (hipMemcpyAsync(c->uz_y0.p, c->uz_y.p, nv * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_uzc_extract, dim3((n_act + 255) / 256, n_act), dim3(256), 0, st, nv, n_act, ldG, c->uzc_act.p, c->uzc_slot.p, c->uzc_cols.p, c->uzc_G.p,
                           (persist && !dyn) ? c->uz_cn.p : (const double *)nullptr);
        if (persist && dyn)
            hipLaunchKernelGGL(k_uzc_schur, dim3((n_rows + 255) / 256, n_rows), dim3(256), 0, st, n_rows, ldS, ldG, c->uzp_rowlist.p, c->uzc_pos.p, dface, dbary,
                               c->uz_cn.p, c->uzc_G.p, c->uzp_S.p);
    }
    const bool skip_honoured = use_cols || (c->oc_enabled && c->oc_plan);
    if (!skip_honoured) chunk = 1;
    if (persist) {
        const int R = c->uzp_rows > 0 ? c->uzp_rows : uzp_rows_per_block(n_rows), NB = (n_rows + R - 1) / R;
        const size_t lds = uzp_lds_bytes(n_rows, R);
        {
            UzpArgs ua{};
            ua.n_act = n_rows; ua.ld = dyn ? ldS : ldG; ua.R = R; ua.NB = NB; ua.max_iters = c->uz_max_iters;
            ua.act = dyn ? c->uzp_rowlist.p : c->uzc_act.p; ua.G = dyn ? c->uzp_S.p : c->uzc_G.p;
            ua.d = c->uz_d.p; ua.r = c->uz_r.p; ua.y = c->uz_y.p; ua.q3 = c->uz_q3.p;
            ua.tol2 = tol2; ua.sc = c->uz_scal.p;
            ua.dbox = (v4u *)c->uzp_dbox.p; ua.sbox = (v4u *)c->uzp_sbox.p;
            ua.stamp0 = (++c->uzp_seq) * 1024u;      // (four stamps per iteration, < 250 iterations)
            ua.abort_word = c->uzp_abort.p; ua.sig = c->d_sig;
            ua.iters_step = c->counters.p + kCntSchurIters; ua.applies_total = c->counters.p + kCntSchurProducts;
            if (c->test_abort_uzp > 0 && (int)c->uzp_seq == c->test_abort_uzp)      // test hook: this launch finds its hand-off given up
                (void)hipMemsetAsync(c->uzp_abort.p, 1, sizeof(unsigned), st);
            hipLaunchKernelGGL(k_uz_persist, dim3(NB), dim3(kUzpT), lds, st, ua);
            c->uzp_launches += 1;
            // No synchronisation: the verdict stays on the device, the iteration count goes to kCntSchurIters (read with the step's
            // statistics), a hand-off time-out shows at the next synchronisation like any aborted on-chip solve.
            persist_launched = true;
            launched = c->uz_max_iters;
        }
    }
    while (launched < c->uz_max_iters) {
        const int n = std::min(chunk, c->uz_max_iters - launched);
        for (int it = 0; it < n; ++it) {
            if (compact) {      // one Schur iteration on the active vertices: two launches (+ C^T d by the dense kernels if rows share face vertices)
                if (dyn) {
                    hipLaunchKernelGGL(k_uz_ct, dim3(gv), dim3(256), 0, st, nv, 1, b, c->uz_cn.p, c->uz_d.p, c->uz_q1.p);
                    launch_ct_dyn(c, nq, qlist, 1, c->uz_d.p, dface, dbary, c->uz_q1.p);
                }
                hipLaunchKernelGGL(k_uzc_matvec, dim3((n_act + 63) / 64, nseg), dim3(256), 0, st, n_act, ldG, seg_len, c->uzc_act.p, c->uzc_G.p,
                                   c->uz_cn.p, c->uz_d.p, dyn ? c->uz_q1.p : (const double *)nullptr, c->uzc_part.p, stop_flag);
                if (n_act <= c->uzc_one_max)
                    hipLaunchKernelGGL((k_uzc_rows<true>), dim3(1), dim3(1024), 0, st, n_act, nseg, c->uzc_act.p, c->uzc_pos.p, c->uzc_part.p, c->uzc_gq.p,
                                       c->uz_cn.p, dface, dbary, c->uz_d.p, c->uz_r.p, c->uz_y.p, c->uz_q3.p, tol2, c->uz_scal.p);
                else
                    hipLaunchKernelGGL((k_uzc_rows<false>), dim3(1), dim3(1024), 0, st, n_act, nseg, c->uzc_act.p, c->uzc_pos.p, c->uzc_part.p, c->uzc_gq.p,
                                       c->uz_cn.p, dface, dbary, c->uz_d.p, c->uz_r.p, c->uz_y.p, c->uz_q3.p, tol2, c->uz_scal.p);
                c->uzc_applies += 1;
                continue;
            }
            hipLaunchKernelGGL(k_uz_ct, dim3(gv), dim3(256), 0, st, nv, 1, b, c->uz_cn.p, c->uz_d.p, c->uz_q1.p);   // q1 = C^T d
            if (dyn) launch_ct_dyn(c, nq, qlist, 1, c->uz_d.p, dface, dbary, c->uz_q1.p);
            if (use_cols) {                                                                                          // q2 = A^-1 q1
                hipLaunchKernelGGL(k_uz_cols_apply, dim3((nv + 63) / 64), dim3(256), 0, st, nv, c->uzc_n_act, c->uzc_act.p, c->uzc_slot.p,
                                   c->uzc_cols.p, c->uz_q1.p, c->uz_q2.p, stop_flag);
                c->uzc_applies += 1;
            } else {
                if (hipMemsetAsync(c->uz_q2.p, 0, c->n3 * sizeof(double), st) != hipSuccess) return -1;
                if (launch_pcg(c, c->uz_q1.p, c->uz_q2.p, c->pcg_max_iters, stop_flag)) return -1;
                c->uzc_pcg_solves += 1;
            }
            hipLaunchKernelGGL(k_uz_dots, dim3(c->NBU), dim3(256), 0, st, nv, c->uz_q2.p, c->uz_cn.p, c->uz_d.p, c->uz_r.p, c->uz_q3.p,
                               c->uz_part.p, c->NBU, dface, dbary);
            hipLaunchKernelGGL(k_uz_alpha, dim3(1), dim3(256), 0, st, c->uz_part.p, c->NBU, c->uz_scal.p);
            hipLaunchKernelGGL(k_uz_step, dim3(c->NBU), dim3(256), 0, st, nv, c->uz_scal.p, x, c->uz_q2.p, c->uz_y.p, c->uz_d.p, c->uz_r.p,
                               c->uz_q3.p, c->uz_part.p, c->NBU);
            hipLaunchKernelGGL(k_uz_beta, dim3(1), dim3(256), 0, st, c->uz_part.p, c->NBU, tol2, c->uz_scal.p);
            hipLaunchKernelGGL(k_uz_dir, dim3(gv), dim3(256), 0, st, nv, c->uz_scal.p, c->uz_r.p, c->uz_d.p);
        }
        launched += n;
        if (hipMemcpyAsync(&h, c->uz_scal.p, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
        if (hipStreamSynchronize(st) != hipSuccess) return -1;
        if (h.stop) break;
        chunk = skip_honoured ? 2 : 1;
    }
    if (compact) {      // x = x0 - A^-1 C^T (y - y0): one pass over the full columns
        hipLaunchKernelGGL(k_uzc_dy, dim3(gv), dim3(256), 0, st, nv, c->uz_y.p, c->uz_y0.p, c->uz_q3.p);
        hipLaunchKernelGGL(k_uz_ct, dim3(gv), dim3(256), 0, st, nv, 1, b, c->uz_cn.p, c->uz_q3.p, c->uz_q1.p);
        if (dyn) launch_ct_dyn(c, nq, qlist, 1, c->uz_q3.p, dface, dbary, c->uz_q1.p);
        hipLaunchKernelGGL(k_uz_cols_apply, dim3((nv + 63) / 64), dim3(256), 0, st, nv, n_act, c->uzc_act.p, c->uzc_slot.p, c->uzc_cols.p,
                           c->uz_q1.p, c->uz_q2.p, (const int *)nullptr);
        hipLaunchKernelGGL(k_uzc_xsub, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, x, c->uz_q2.p);
    }
    if (persist_launched) { *iters = 0; return 0; }      // (counted on the device)
    c->uz_prev_iters = h.iters;
    *iters = h.iters;
    return 0;
}

void enqueue_gs(admm_hip_ctx *c, const double *b, double *x) {
    hipStream_t st = c->stream;
    (void)hipMemsetAsync(c->counters.p + kCntGsDone, 0, (kCntGsSweeps + 1 - kCntGsDone) * sizeof(int), st);
    GsArgs a{};
    a.S = sell_arg(c->gs_sell); a.slot_node = c->gs_slot_node.p; a.diag = c->gs_diag.p; a.m = c->m.p; a.b = b; a.x = x;
    a.pin_flag = c->gs_has_pins ? c->gs_pin_flag.p : nullptr; a.pin_xyz = c->gs_pin_xyz.p; a.pin_nrm = c->gs_pin_nrm.p;
    a.omega = c->gs_omega; a.done = c->counters.p + kCntGsDone;
    a.part = c->part.p; a.NBp = c->NB; a.tol2 = c->gs_tol * c->gs_tol; a.sweeps = c->counters.p + kCntGsSweeps; a.total = c->counters.p + kCntIters;
    a.proj = c->gs_proj.p;
    const SellA A = sell_arg(c->A);
    const int check = c->gs_tol > 0.0 ? 1 : 0;
    if (check && c->n_colors == 2 && c->gs_xb.p && c->gs_max_iters > 0) {
        // two colours: the residual test rides on the colour kernels (k_gs_color2), two launches per sweep
        const int s00 = c->gs_color_slice[0], ns0 = c->gs_color_slice[1] - s00, s01 = c->gs_color_slice[1], ns1 = c->gs_color_slice[2] - s01;
        const int nbB = (ns0 + 3) / 4, nbA = (ns1 + 3) / 4;
        Gs2Args a2{a, c->gs_xb.p, c->gs_part2.p, c->gs_part2.p + 4 * (size_t)nbA, nbA, nbB, s00, ns0};
        for (int it = 0; it < c->gs_max_iters; ++it) {
            const int par = it & 1;
            if (it == 0) hipLaunchKernelGGL((k_gs_color2<false, true, false>), dim3(nbB), dim3(256), 0, st, a2, s00, ns0, c->obst, 0, par);
            else hipLaunchKernelGGL((k_gs_color2<true, true, false>), dim3(nbB), dim3(256), 0, st, a2, s00, ns0, c->obst, 0, par);
            hipLaunchKernelGGL((k_gs_color2<false, true, true>), dim3(nbA), dim3(256), 0, st, a2, s01, ns1, c->obst, it /* 0: nothing to settle; else the launch's stamp */, par);
        }
        hipLaunchKernelGGL((k_gs_color2<true, false, false>), dim3(nbB), dim3(256), 0, st, a2, s00, ns0, c->obst, 0, 0);
        hipLaunchKernelGGL(k_gs_check2, dim3(1), dim3(256), 0, st, a2, (c->gs_max_iters - 1) & 1);
        return;
    }
    if (check && c->gs_fusedN && c->gs_max_iters > 0) {
        // three and more colours: the residual test rides on the colour kernels too (k_gs_colorN), one launch per colour and sweep
        const int C = c->n_colors, sL = c->gs_color_slice[C - 1], nsL = c->gs_color_slice[C] - sL, nbL = (nsL + 3) / 4;
        int nE = 0;
        std::vector<int> off(C, 0);
        for (int k = 0; k + 1 < C; ++k) { off[k] = nE; nE += (c->gs_color_slice[k + 1] - c->gs_color_slice[k] + 3) / 4; }
        GsNArgs aN{a, c->gs_xb.p, c->gs_part2.p, c->gs_part2.p + 4 * (size_t)nbL, nbL, nE, c->gs_color_slice[0], sL - c->gs_color_slice[0], c->gs_low.p};
        for (int it = 0; it < c->gs_max_iters; ++it) {
            const int par = it & 1;
            for (int k = 0; k + 1 < C; ++k) {
                const int s0 = c->gs_color_slice[k], ns = c->gs_color_slice[k + 1] - s0, nb = (ns + 3) / 4;
                if (nb == 0) continue;
                if (it == 0) hipLaunchKernelGGL((k_gs_colorN<0, false, true>), dim3(nb), dim3(256), 0, st, aN, s0, ns, c->obst, 0, par, off[k], k);
                else hipLaunchKernelGGL((k_gs_colorN<0, true, true>), dim3(nb), dim3(256), 0, st, aN, s0, ns, c->obst, 0, par, off[k], k);
            }
            hipLaunchKernelGGL((k_gs_colorN<2, false, true>), dim3(nbL), dim3(256), 0, st, aN, sL, nsL, c->obst, it /* the launch's stamp */, par, 0, C - 1);
        }
        // the last sweep: residuals of the earlier colours in one pass (nothing moves any more), then the verdict
        hipLaunchKernelGGL((k_gs_colorN<0, true, false>), dim3(nE), dim3(256), 0, st, aN, aN.s0_early, aN.ns_early, c->obst, 0, 0, 0, 1);
        hipLaunchKernelGGL(k_gs_checkN, dim3(1), dim3(256), 0, st, aN, (c->gs_max_iters - 1) & 1);
        return;
    }
    for (int it = 0; it < c->gs_max_iters; ++it) {
        bool first = true;
        for (int col = 0; col < c->n_colors; ++col) {
            const int s0 = c->gs_color_slice[col], ns = c->gs_color_slice[col + 1] - s0;
            if (ns == 0) continue;
            // the first colour kernel of sweep it >= 1 settles the residual test / sweep count of sweep it-1
            const int decide = (first && it > 0) ? (check ? 2 : 1) : 0;
            hipLaunchKernelGGL(k_gs_color, dim3((ns + 3) / 4), dim3(256), 0, st, a, s0, ns, c->obst, decide);
            first = false;
        }
        if (check)
            hipLaunchKernelGGL(k_gs_resid, dim3(c->NB), dim3(256), 0, st, A, c->m.p, b, x, c->part.p, c->NB, c->counters.p + kCntGsDone,
                               (const unsigned char *)nullptr);
    }
    // the last sweep is settled by a dedicated one-block kernel
    hipLaunchKernelGGL(k_gs_check, dim3(1), dim3(256), 0, st, c->part.p, c->NB, c->gs_tol * c->gs_tol, c->counters.p + kCntGsDone,
                       c->counters.p + kCntGsSweeps, c->counters.p + kCntIters, check);
}

// the whole solve as ONE persistent launch (gs_persist.hpp)
void launch_gs_persist(admm_hip_ctx *c, const double *b, double *x) {
    hipStream_t st = c->stream;
    GspArgs a{};
    a.G = c->gsp_G; a.C = c->gsp_C;
    a.hdr = c->gsp_hdr.p; a.orig = c->gsp_orig.p; a.out_idx = c->gsp_out.p; a.halo_box = c->gsp_hbox.p; a.halo_orig = c->gsp_horig.p;
    a.diag = c->gsp_diag.p; a.vals = c->gsp_vals.p; a.cols = c->gsp_cols.p;
    a.m = c->m.p; a.b = b; a.x = x;
    a.pin_flag = c->gs_has_pins ? c->gs_pin_flag.p : nullptr; a.pin_xyz = c->gs_pin_xyz.p; a.pin_nrm = c->gs_pin_nrm.p;
    a.omega = c->gs_omega; a.tol2 = c->gs_tol * c->gs_tol; a.max_sweeps = c->gs_max_iters; a.check = c->gs_tol > 0.0 ? 1 : 0;
    a.seq = (unsigned)++c->solve_seq;
    a.box = (v4u *)c->gsp_box.p; a.n_box = (int)std::max<int64_t>(c->gsp_stat[4], 1); a.part = (v4u *)c->gsp_part.p; a.meet = (v4u *)c->gsp_meet.p; a.abort_word = c->gsp_abort.p;
    a.done = c->counters.p + kCntGsDone; a.sweeps = c->counters.p + kCntGsSweeps; a.total = c->counters.p + kCntIters; a.sig = c->d_sig;
    a.prof = c->gsp_prof.p; a.prof_block = c->gsp_prof_block;
    a.ob = c->obst_dev.p; a.proj = c->gs_proj.p; a.stop = c->stop_dev;
    if (c->test_abort_seq > 0 && (int)a.seq == c->test_abort_seq)   // test hook: this solve finds its hand-off given up
        (void)hipMemsetAsync(c->gsp_abort.p, 1, sizeof(unsigned), st);
    if (c->stop_dev) hipLaunchKernelGGL(k_gs_persist<true>, dim3(c->gsp_G), dim3(kGspT), c->gsp_lds, st, a);
    else hipLaunchKernelGGL(k_gs_persist<false>, dim3(c->gsp_G), dim3(kGspT), c->gsp_lds, st, a);
    c->gsp_launches += 1;
    if (c->gsp_prof.p && (c->solve_seq % 200) == 0) {     // diagnosis: one block's wall-clock split of the phases since the last print
        unsigned long long h[16];
        if (hipMemcpyAsync(h, c->gsp_prof.p, sizeof(h), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && h[4]) {
            const double k = 0.01 / (double)h[4];      // 100 MHz ticks -> us per phase
            fprintf(stderr, "[gsp_prof] block %d, %llu phases: halo poll %.2f  block barrier %.2f  rows + publish %.2f  verdict etc. %.2f us per phase\n",
                    c->gsp_prof_block, h[4], k * h[0], k * h[1], k * h[2], k * h[3]);
            if (h[6]) fprintf(stderr, "[gsp_prof] shader clock during the solves: %.0f MHz\n", 100.0 * (double)h[5] / (double)h[6]);
            if (h[8]) fprintf(stderr, "[gsp_prof] rows + publish in detail (-DADMM_GSP_PROF_FINE): row sums %.2f  own row's data + residual before %.2f  pin / relax %.2f  stores + granules + residual after %.2f  "
                                      "parked partial + judge %.2f  park %.2f us per phase\n", k * h[8], k * h[9], k * h[10], k * h[11], k * h[12], k * h[13]);
            if (h[14]) { const double ps = k * (double)c->gs_max_iters * (double)c->gsp_C;     // per solve of max_iters sweeps
                         fprintf(stderr, "[gsp_prof] per solve: fill %.2f  phases %.2f  end of the last sweep + verdicts + write-back %.2f us\n", ps * h[14], ps * h[6], ps * ((double)h[15] - (double)h[6])); }
            (void)hipMemsetAsync(c->gsp_prof.p, 0, sizeof(h), st);
        }
    }
}

// Plan + buffers of the persistent GS kernel; leaves gsp_enabled = false when the scene does not fit (the colour kernels serve it).
hipError_t plan_gs_persist(admm_hip_ctx *c) {
    c->gsp_enabled = false;
    if (!env_flag("ADMM_HIP_GS_PERSIST", true)) return hipSuccess;
    static_assert(kGspMaxCK == admm_host::kGspMaxC && kGspHdrK == admm_host::kGspHdr, "gs_persist.hpp and host_setup.hpp disagree on the plan layout");
    if (c->n_colors < 1 || c->n_colors > kGspMaxCK || (int64_t)c->gs_max_iters * c->n_colors >= 2000) return hipSuccess;   // (stamp space of one solve)
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, c->device);
    if (e != hipSuccess) return e;
    const int cus = prop.multiProcessorCount;
    const int lds_max = (int)std::min<size_t>(prop.sharedMemPerBlock, 160 * 1024);
    // (rows per block: 384 through round 5; with the two-granule / whole-sector hand-off of round 6 a phase no longer pays per granule and smaller
    // blocks -- fewer granules to wait for, a shorter fill -- win: cube100k_gs 96 / 128 / 192 / 256 / 320 / 384 / 448 rows = 5 407 / 5 584 / 5 858 /
    // 5 773 / 5 702 / 5 298 / 5 142 ADMM it/s, profiles/r06_gs_rows_per_block.txt; bodies beyond 49 k vertices fill all CUs either way)
    const int rows_target = env_int("ADMM_HIP_GS_ROWS", kGspRowsTarget, 32);
    std::vector<int32_t> col32(c->color_h.begin(), c->color_h.end());
    // Blocks: one per CU.  (Two per CU for bodies with more than cus x rows_target rows was measured in round 6 -- the 200 k-triangle cloth as
    // 512 blocks of 197 rows instead of 256 of 393: 3 452 -> 2 850 ADMM it/s; two waves per SIMD stretch every row's chain and the block barrier
    // (0.03 -> 0.27 us).  profiles/r06_gs_rows_per_block.txt)
    const admm_host::GsPlan P = admm_host::build_gs_plan(c->Ahat, c->n_colors, col32.data(), cus, rows_target, lds_max);
    if (!P.ok) return hipSuccess;
    int per_cu = 0;
    int per_cu_stop = 0;      // (k_gs_persist<true>: the solves of a step with early exit, admm_hip_set_admm_stop)
    if ((e = hipFuncSetAttribute((const void *)k_gs_persist<false>, hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes)) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute((const void *)k_gs_persist<true>, hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gs_persist<false>, kGspT, P.lds_bytes)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_stop, k_gs_persist<true>, kGspT, P.lds_bytes)) != hipSuccess) return e;
    if (per_cu < 1 || per_cu_stop < 1 || P.G > cus) return hipSuccess;      // every block must be resident at once
    if ((e = c->gsp_hdr.upload(std::vector<int>(P.hdr.begin(), P.hdr.end()))) != hipSuccess) return e;
    if ((e = c->gsp_orig.upload(std::vector<int>(P.orig.begin(), P.orig.end()))) != hipSuccess) return e;
    if ((e = c->gsp_out.upload(std::vector<int>(P.out_idx.begin(), P.out_idx.end()))) != hipSuccess) return e;
    if ((e = c->gsp_hbox.upload(std::vector<int>(P.halo_box.begin(), P.halo_box.end()))) != hipSuccess) return e;
    if ((e = c->gsp_horig.upload(std::vector<int>(P.halo_orig.begin(), P.halo_orig.end()))) != hipSuccess) return e;
    if ((e = c->gsp_diag.upload(P.diag)) != hipSuccess) return e;
    if ((e = c->gsp_vals.upload(P.vals)) != hipSuccess) return e;
    if ((e = c->gsp_cols.upload(P.cols)) != hipSuccess) return e;
    if ((e = c->gsp_box.alloc((size_t)std::max(P.ob_total, 1) * 6)) != hipSuccess) return e;
    if ((e = c->gsp_box.zero()) != hipSuccess) return e;
    if ((e = c->gsp_part.alloc((size_t)P.G * 8)) != hipSuccess) return e;
    if ((e = c->gsp_part.zero()) != hipSuccess) return e;
    if ((e = c->gsp_meet.alloc((size_t)P.G)) != hipSuccess) return e;
    if ((e = c->gsp_meet.zero()) != hipSuccess) return e;
    if ((e = c->gsp_abort.alloc(16)) != hipSuccess) return e;
    if ((e = c->gsp_abort.zero()) != hipSuccess) return e;
    if (env_flag("ADMM_HIP_GSP_PROF", false)) {
        if ((e = c->gsp_prof.alloc(16)) != hipSuccess) return e;
        if ((e = c->gsp_prof.zero()) != hipSuccess) return e;
        c->gsp_prof_block = env_int("ADMM_HIP_GSP_PROF_BLOCK", 0);
    }
    c->gsp_G = P.G; c->gsp_C = P.C; c->gsp_lds = (size_t)P.lds_bytes;
    c->gsp_stat[0] = P.G; c->gsp_stat[1] = P.max_rows; c->gsp_stat[2] = P.max_halo; c->gsp_stat[3] = P.max_nbr; c->gsp_stat[4] = P.ob_total; c->gsp_stat[5] = P.lds_bytes;
    if (getenv("ADMM_HIP_OC_DIAG"))
        fprintf(stderr, "[gs_plan] %d blocks x %d threads, <= %d rows and %d halo entries per block, <= %d neighbour blocks, %d outbox nodes, %d bytes of LDS\n",
                P.G, kGspT, P.max_rows, P.max_halo, P.max_nbr, P.ob_total, P.lds_bytes);
    c->gsp_enabled = true;
    c->test_abort_seq = env_int("ADMM_HIP_TEST_ABORT_SOLVE", 0);
    return hipSuccess;
}

void launch_gs(admm_hip_ctx *c, const double *b, double *x) {
    // (the persistent kernel stamps its phases: sweeps x colours of one solve must stay inside the stamp space -- admm_hip_set_solver_params may raise max_iters)
    if (c->gsp_enabled && (int64_t)c->gs_max_iters * c->gsp_C < 2000) { launch_gs_persist(c, b, x); return; }
    if (c->gs_exec && (c->gs_graph_b != b || c->gs_graph_x != x)) { (void)hipGraphExecDestroy(c->gs_exec); c->gs_exec = nullptr; }
    if (!c->gs_exec) {
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            enqueue_gs(c, b, x);
            if (hipStreamEndCapture(c->stream, &g) == hipSuccess && g &&
                hipGraphInstantiate(&c->gs_exec, g, nullptr, nullptr, 0) == hipSuccess) {
                c->gs_graph_b = b; c->gs_graph_x = x;
            } else {
                c->gs_exec = nullptr;
            }
            if (g) (void)hipGraphDestroy(g);
        }
        (void)hipGetLastError();
    }
    if (c->gs_exec && hipGraphLaunch(c->gs_exec, c->stream) == hipSuccess) return;
    enqueue_gs(c, b, x); // capture unavailable: plain launches
}

// NodalMultiColorGS::solve with dynamic hits (src/NodalMultiColorGS.hpp:75-86): detect, and if anything was hit sweep
// A + C^T C -- untouched nodes with the SELL colour kernels (skip mask), touched nodes with k_gs_touched over new colours.
int launch_gs_dynamic(admm_hip_ctx *c, const double *b, double *x) {
    hipStream_t st = c->stream;
    const int nv = c->nv;
    const int nq = c->n_surf > 0 ? c->n_surf : nv;
    const int *qlist = c->n_surf > 0 ? c->surf_list.p : nullptr;
    if (c->timing && hipEventRecord(c->ev_coll0, st) != hipSuccess) return -1;
    if (enqueue_dyn_detect(c, x)) return -1;
    if (hipMemsetAsync(c->counters.p + kCntHits, 0, sizeof(int), st) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_compact, dim3(blocks_for(nq)), dim3(256), 0, st, nq, qlist, c->dyn_face.p, c->dyn_bary.p, c->dyn_n.p,
                       c->gsd_hits.p, (int)c->gsd_hits.n, c->counters.p + kCntHits);
    if (c->timing && hipEventRecord(c->ev_coll1, st) != hipSuccess) return -1;
    int nh = 0;
    if (hipMemcpyAsync(&nh, c->counters.p + kCntHits, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    if (c->timing) { float ms = 0.f; if (hipEventElapsedTime(&ms, c->ev_coll0, c->ev_coll1) == hipSuccess) c->coll_ms_step += ms; }
    c->gsd_last_hits = nh;
    if (nh == 0) { launch_gs(c, b, x); return 0; }
    std::vector<DynHit> hits(nh);
    if (hipMemcpy(hits.data(), c->gsd_hits.p, nh * sizeof(DynHit), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    std::sort(hits.begin(), hits.end(), [](const DynHit &p, const DynHit &q) { return p.v < q.v; });
    // touched nodes and their hits
    std::map<int, int> tix;
    for (const DynHit &h : hits) { const int nd[4] = {h.v, h.f0, h.f1, h.f2}; for (int k = 0; k < 4; ++k) tix.emplace(nd[k], 0); }
    std::vector<int> touched; touched.reserve(tix.size());
    for (auto &kv : tix) { kv.second = (int)touched.size(); touched.push_back(kv.first); }
    const int nt = (int)touched.size();
    std::vector<std::vector<std::pair<int, double> > > inc(nt);
    std::vector<std::vector<int> > adj(nt);
    for (int h = 0; h < nh; ++h) {
        const int nd[4] = {hits[h].v, hits[h].f0, hits[h].f1, hits[h].f2};
        const double cf[4] = {1.0, -hits[h].b[0], -hits[h].b[1], -hits[h].b[2]};
        for (int k = 0; k < 4; ++k) {
            inc[tix[nd[k]]].emplace_back(h, cf[k]);
            for (int l = 0; l < 4; ++l) if (nd[l] != nd[k]) adj[tix[nd[k]]].push_back(tix[nd[l]]);
        }
    }
    for (int t = 0; t < nt; ++t) {
        const int v = touched[t];
        for (int k = c->Ahat.rowptr[v]; k < c->Ahat.rowptr[v + 1]; ++k) {
            const int j = c->Ahat.col[k];
            if (j == v || c->Ahat.val[k] == 0.0) continue;
            auto it = tix.find(j);
            if (it != tix.end()) adj[t].push_back(it->second);
        }
    }
    // first fit over new colours, increasing node order (the rule the oracle restates: oracle.py recolor_touched)
    std::vector<int> extra(nt, -1);
    int n_extra = 0;
    for (int t = 0; t < nt; ++t) {
        std::vector<char> used(n_extra + 1, 0);
        for (int u : adj[t]) if (extra[u] >= 0) used[extra[u]] = 1;
        int e = 0;
        while (used[e]) ++e;
        extra[t] = e; n_extra = std::max(n_extra, e + 1);
    }
    // group by new colour (stable: node order inside a colour)
    std::vector<int> order(nt), cstart(n_extra + 1, 0);
    for (int t = 0; t < nt; ++t) cstart[extra[t] + 1] += 1;
    for (int e = 0; e < n_extra; ++e) cstart[e + 1] += cstart[e];
    { std::vector<int> pos(cstart.begin(), cstart.end() - 1); for (int t = 0; t < nt; ++t) order[pos[extra[t]]++] = t; }
    // flat arrays: [node | rptr | hptr | rcol | hidx] ints, [rval | hcoef | hc | hn] doubles
    std::vector<int> node(nt), rptr(nt + 1, 0), hptr(nt + 1, 0), rcol, hidx;
    std::vector<double> rval, hcoef, hc(4 * (size_t)nh), hn(3 * (size_t)nh);
    std::vector<int4> hnode(nh);
    for (int i = 0; i < nt; ++i) {
        const int t = order[i], v = touched[t];
        node[i] = v;
        for (int k = c->Ahat.rowptr[v]; k < c->Ahat.rowptr[v + 1]; ++k) { rcol.push_back(c->Ahat.col[k]); rval.push_back(c->Ahat.val[k]); }
        rptr[i + 1] = (int)rcol.size();
        for (auto &pr : inc[t]) { hidx.push_back(pr.first); hcoef.push_back(pr.second); }
        hptr[i + 1] = (int)hidx.size();
    }
    for (int h = 0; h < nh; ++h) {
        hnode[h] = make_int4(hits[h].v, hits[h].f0, hits[h].f1, hits[h].f2);
        hc[4 * (size_t)h] = 1.0;
        for (int k = 0; k < 3; ++k) { hc[4 * (size_t)h + 1 + k] = -hits[h].b[k]; hn[3 * (size_t)h + k] = hits[h].n[k]; }
    }
    std::vector<int> ints; ints.reserve(node.size() + rptr.size() + hptr.size() + rcol.size() + hidx.size());
    const size_t o_node = 0, o_rptr = o_node + node.size(), o_hptr = o_rptr + rptr.size(), o_rcol = o_hptr + hptr.size(), o_hidx = o_rcol + rcol.size();
    ints.insert(ints.end(), node.begin(), node.end()); ints.insert(ints.end(), rptr.begin(), rptr.end());
    ints.insert(ints.end(), hptr.begin(), hptr.end()); ints.insert(ints.end(), rcol.begin(), rcol.end()); ints.insert(ints.end(), hidx.begin(), hidx.end());
    std::vector<double> dbl;
    const size_t o_rval = 0, o_hcoef = o_rval + rval.size(), o_hc = o_hcoef + hcoef.size(), o_hn = o_hc + hc.size();
    dbl.insert(dbl.end(), rval.begin(), rval.end()); dbl.insert(dbl.end(), hcoef.begin(), hcoef.end());
    dbl.insert(dbl.end(), hc.begin(), hc.end()); dbl.insert(dbl.end(), hn.begin(), hn.end());
    if (c->gsd_int.n < ints.size() && c->gsd_int.alloc(2 * ints.size()) != hipSuccess) return -1;
    if (c->gsd_dbl.n < dbl.size() && c->gsd_dbl.alloc(2 * dbl.size()) != hipSuccess) return -1;
    if (c->gsd_hnode.n < hnode.size() && c->gsd_hnode.alloc(2 * hnode.size()) != hipSuccess) return -1;
    std::vector<unsigned char> mask(nv, 0);
    for (int v : touched) mask[v] = 1;
    if (hipMemcpyAsync(c->gsd_int.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c->gsd_dbl.p, dbl.data(), dbl.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c->gsd_hnode.p, hnode.data(), hnode.size() * sizeof(int4), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c->gsd_skip.p, mask.data(), nv, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;   // the host vectors die at the end of this function
    GsDyn d{};
    d.n_touched = nt; d.n_hits = nh;
    d.node = c->gsd_int.p + o_node; d.rptr = c->gsd_int.p + o_rptr; d.hptr = c->gsd_int.p + o_hptr; d.rcol = c->gsd_int.p + o_rcol; d.hidx = c->gsd_int.p + o_hidx;
    d.rval = c->gsd_dbl.p + o_rval; d.hcoef = c->gsd_dbl.p + o_hcoef; d.hc = c->gsd_dbl.p + o_hc; d.hn = c->gsd_dbl.p + o_hn;
    d.hnode = c->gsd_hnode.p;
    d.ck2 = std::max(0.0, c->constraint_w);
    // the sweeps (plain launches: the colour structure changes with every solve, so there is nothing to capture)
    (void)hipMemsetAsync(c->counters.p + kCntGsDone, 0, (kCntGsSweeps + 1 - kCntGsDone) * sizeof(int), st);
    const int NBp = c->NB + 1;
    GsArgs a{};
    a.S = sell_arg(c->gs_sell); a.slot_node = c->gs_slot_node.p; a.diag = c->gs_diag.p; a.m = c->m.p; a.b = b; a.x = x;
    a.pin_flag = c->gs_has_pins ? c->gs_pin_flag.p : nullptr; a.pin_xyz = c->gs_pin_xyz.p; a.pin_nrm = c->gs_pin_nrm.p;
    a.omega = c->gs_omega; a.done = c->counters.p + kCntGsDone;
    a.part = c->gsd_part.p; a.NBp = NBp; a.tol2 = c->gs_tol * c->gs_tol; a.sweeps = c->counters.p + kCntGsSweeps; a.total = c->counters.p + kCntIters;
    a.skip = c->gsd_skip.p;
    const SellA A = sell_arg(c->A);
    const int check = c->gs_tol > 0.0 ? 1 : 0;
    for (int it = 0; it < c->gs_max_iters; ++it) {
        bool first = true;
        for (int col = 0; col < c->n_colors; ++col) {
            const int s0 = c->gs_color_slice[col], ns = c->gs_color_slice[col + 1] - s0;
            if (ns == 0) continue;
            const int decide = (first && it > 0) ? (check ? 2 : 1) : 0;
            hipLaunchKernelGGL(k_gs_color, dim3((ns + 3) / 4), dim3(256), 0, st, a, s0, ns, c->obst, decide);
            first = false;
        }
        for (int e = 0; e < n_extra; ++e)
            hipLaunchKernelGGL(k_gs_touched, dim3((cstart[e + 1] - cstart[e] + 63) / 64), dim3(64), 0, st, a, d, cstart[e], cstart[e + 1], c->obst);
        if (check) {
            hipLaunchKernelGGL(k_gs_resid, dim3(c->NB), dim3(256), 0, st, A, c->m.p, b, x, c->gsd_part.p, NBp, c->counters.p + kCntGsDone,
                               (const unsigned char *)c->gsd_skip.p);
            hipLaunchKernelGGL(k_gs_touched_resid, dim3(1), dim3(256), 0, st, a, d, c->gsd_part.p, NBp, c->NB);
        }
    }
    hipLaunchKernelGGL(k_gs_check, dim3(1), dim3(256), 0, st, c->gsd_part.p, NBp, c->gs_tol * c->gs_tol, c->counters.p + kCntGsDone,
                       c->counters.p + kCntGsSweeps, c->counters.p + kCntIters, check);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int validate(const admm_hip_desc *d) {
    if (!d) return fail(ADMM_HIP_ERR_ARG, "desc is NULL");
    if (d->struct_size != (int32_t)sizeof(admm_hip_desc)) return fail(ADMM_HIP_ERR_ARG, "desc.struct_size mismatch");
    if (d->n_verts < 1 || !d->masses) return fail(ADMM_HIP_ERR_ARG, "Problem with node data (Solver.cpp:180-183)");
    if (d->n_tets < 0 || d->n_tris < 0 || d->n_pins < 0) return fail(ADMM_HIP_ERR_ARG, "negative count");
    // the kernels address the per-element SoA arrays and the node vectors with 32-bit byte offsets (buffer instructions):
    // the largest array of a context, cf[12][n + 1] doubles, and the node vectors must stay below 2^31 bytes
    if ((int64_t)128 * ((int64_t)d->n_tets + 1) >= ((int64_t)1 << 31) || (int64_t)96 * ((int64_t)d->n_tris + 1) >= ((int64_t)1 << 31) ||
        (int64_t)24 * d->n_verts >= ((int64_t)1 << 31))
        return fail(ADMM_HIP_ERR_ARG, "scene too large for one context (limit: 16.7 M tets, 22.3 M tris, 89 M vertices per rank)");
    if (d->n_tets && (!d->tet_idx || !d->tet_Binv || !d->tet_weight || !d->tet_kind || !d->tet_mu || !d->tet_lambda || !d->tet_k))
        return fail(ADMM_HIP_ERR_ARG, "tet arrays missing");
    if (d->n_tris && (!d->tri_idx || !d->tri_rest || !d->tri_weight || !d->tri_limit_min || !d->tri_limit_max))
        return fail(ADMM_HIP_ERR_ARG, "tri arrays missing");
    if (d->n_pins && (!d->pin_vert || !d->pin_xyz)) return fail(ADMM_HIP_ERR_ARG, "pin arrays missing");
    if (d->n_bends < 0) return fail(ADMM_HIP_ERR_ARG, "negative count");
    if (d->n_bends && (!d->bend_idx || !d->bend_coef || !d->bend_weight || !d->bend_stiffness)) return fail(ADMM_HIP_ERR_ARG, "bend arrays missing");
    if ((int64_t)96 * ((int64_t)d->n_bends + 1) >= ((int64_t)1 << 31)) return fail(ADMM_HIP_ERR_ARG, "scene too large for one context (limit: 22.3 M bending hinges per rank)");
    for (int64_t i = 0; i < (int64_t)4 * d->n_bends; ++i)
        if (d->bend_idx[i] < 0 || d->bend_idx[i] >= d->n_verts) return fail(ADMM_HIP_ERR_ARG, "bend index out of range");
    for (int i = 0; i < d->n_bends; ++i) {
        if (!(d->bend_weight[i] > 0.0)) return fail(ADMM_HIP_ERR_ARG, "Some weight leq 0 (EnergyTerm.hpp:124-126)");
        if (!(d->bend_stiffness[i] >= 0.0)) return fail(ADMM_HIP_ERR_ARG, "negative bending stiffness");
    }
    if (d->pin_normal)
        for (int64_t i = 0; i < (int64_t)3 * d->n_pins; ++i)
            if (!std::isfinite(d->pin_normal[i])) return fail(ADMM_HIP_ERR_ARG, "non-finite pin normal");
    if (d->linsolver < 0 || d->linsolver > 2) return fail(ADMM_HIP_ERR_ARG, "linsolver must be 0, 1 or 2");
    if (d->n_obstacles < 0 || d->n_obstacles > kMaxObst) return fail(ADMM_HIP_ERR_ARG, "too many obstacles (max 8)");
    if (d->n_obstacles && d->linsolver == 0)
        return fail(ADMM_HIP_ERR_ARG, "No collisions with LDLT solver (Solver.cpp:249-254)");
    for (int j = 0; j < d->n_obstacles; ++j) {
        const int k = d->obstacle_kind[j];
        const double *q = d->obstacle_params + 4 * (size_t)j;
        if (k < ADMM_OBJ_FLOOR || k > ADMM_OBJ_GRID) return fail(ADMM_HIP_ERR_ARG, "unknown obstacle kind");
        if (k == ADMM_OBJ_PLANE && !(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] > 0.0)) return fail(ADMM_HIP_ERR_ARG, "plane obstacle with a zero normal");
        if (k == ADMM_OBJ_GRID) {
            const int g = (int)q[0];
            if (g < 0 || g >= d->n_obstacle_grids || !d->obstacle_grid_meta || !d->obstacle_grid_data) return fail(ADMM_HIP_ERR_ARG, "sampled obstacle: its grid (admm_host_sample_obstacle) is missing");
            const double *m = d->obstacle_grid_meta + 10 * (size_t)g;
            if (!(m[3] > 0.0 && m[4] > 0.0 && m[5] > 0.0 && m[6] >= 2.0 && m[7] >= 2.0 && m[8] >= 2.0 && m[9] >= 0.0)) return fail(ADMM_HIP_ERR_ARG, "sampled obstacle: bad grid description");
        }
    }
    if (d->world_size > 1 && (d->rank < 0 || d->rank >= d->world_size)) return fail(ADMM_HIP_ERR_ARG, "rank out of range");
    for (int i = 0; i < 3 * d->n_verts; ++i)
        if (!(d->masses[i] > 0.0)) return fail(ADMM_HIP_ERR_ARG, "non-positive mass");
    for (int64_t i = 0; i < (int64_t)4 * d->n_tets; ++i)
        if (d->tet_idx[i] < 0 || d->tet_idx[i] >= d->n_verts) return fail(ADMM_HIP_ERR_ARG, "tet index out of range");
    for (int64_t i = 0; i < (int64_t)3 * d->n_tris; ++i)
        if (d->tri_idx[i] < 0 || d->tri_idx[i] >= d->n_verts) return fail(ADMM_HIP_ERR_ARG, "tri index out of range");
    for (int i = 0; i < d->n_tets; ++i) {
        if (!(d->tet_weight[i] > 0.0)) return fail(ADMM_HIP_ERR_ARG, "Some weight leq 0 (EnergyTerm.hpp:124-126)");
        if (d->tet_kind[i] < 0 || d->tet_kind[i] > ADMM_TET_STABLE_NH) return fail(ADMM_HIP_ERR_ARG, "unknown tet kind");
        if (d->tet_kind[i] == ADMM_TET_SPLINE_TABLE &&
            (!d->spline_tables || !d->tet_spline || d->tet_spline[i] < 0 || d->tet_spline[i] >= d->n_spline_tables))
            return fail(ADMM_HIP_ERR_ARG, "SplineTet with a user-defined spline: its table (admm_host_tabulate_spline) is missing");
    }
    for (int i = 0; i < d->n_tris; ++i) {
        if (!(d->tri_weight[i] > 0.0)) return fail(ADMM_HIP_ERR_ARG, "Some weight leq 0 (EnergyTerm.hpp:124-126)");
        if (d->tri_limit_min[i] > 1.0) return fail(ADMM_HIP_ERR_ARG, "Strain limit min should be -inf to 1 (TriEnergyTerm.cpp:32)");
        if (d->tri_limit_max[i] < 1.0) return fail(ADMM_HIP_ERR_ARG, "Strain limit max should be 1 to inf (TriEnergyTerm.cpp:33)");
    }
    for (int i = 0; i < d->n_pins; ++i)
        if (d->pin_vert[i] < 0 || d->pin_vert[i] >= d->n_verts) return fail(ADMM_HIP_ERR_ARG, "pin index out of range");
    return 0;
}

} // namespace

extern "C" {

const char *admm_hip_last_error(void) { return g_last_error.c_str(); }

int admm_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int create_impl(const admm_hip_desc *d, admm_hip_ctx **out);

// world_size > 1: whole bodies per rank when the scene has enough of them (see admm_hip_ctx::CompMode), element blocks otherwise
// (ADMM_HIP_PARTITION=elements forces the latter; =components insists on the former and fails if the scene does not split).
int admm_hip_create(const admm_hip_desc *d, admm_hip_ctx **out) {
    if (!out) return fail(ADMM_HIP_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (int rc = validate(d)) return rc;
    const char *pm = getenv("ADMM_HIP_PARTITION");
    const bool force_el = pm && !strcmp(pm, "elements"), force_co = pm && !strcmp(pm, "components");
    if (d->world_size <= 1 || force_el) return create_impl(d, out);
    const int world = d->world_size, rank = d->rank, nv = d->n_verts;
    std::vector<int32_t> vrank(nv);
    const int32_t ncomp = admm_host::component_partition(nv, d->n_tets, d->tet_idx, d->n_tris, d->tri_idx, world, vrank.data(), d->n_bends, d->bend_idx);
    if (ncomp < world) {
        if (force_co) return fail(ADMM_HIP_ERR_ARG, "ADMM_HIP_PARTITION=components: the scene has fewer connected components (bodies with elements) than ranks");
        return create_impl(d, out);
    }
    if (!force_co) {     // one body that dominates the load (a large mesh + debris): whole bodies per rank would leave ranks idle -- element blocks then
        std::vector<int64_t> load(world, 0);
        for (int32_t t = 0; t < d->n_tets; ++t) load[vrank[d->tet_idx[4 * (size_t)t]]] += 1;
        for (int32_t t = 0; t < d->n_tris; ++t) load[vrank[d->tri_idx[3 * (size_t)t]]] += 1;
        const int64_t total = (int64_t)d->n_tets + d->n_tris, mx = *std::max_element(load.begin(), load.end());
        if (mx * world > 2 * total) return create_impl(d, out);
    }
    // ---- the sub-scene of this rank, locally numbered ----
    std::vector<int32_t> l2g, g2l(nv, -1);
    for (int32_t v = 0; v < nv; ++v) if (vrank[v] == rank) { g2l[v] = (int32_t)l2g.size(); l2g.push_back(v); }
    const int32_t nl = (int32_t)l2g.size();
    std::vector<double> masses(3 * (size_t)nl), xyz;
    for (int32_t i = 0; i < nl; ++i) for (int j = 0; j < 3; ++j) masses[3 * (size_t)i + j] = d->masses[3 * (size_t)l2g[i] + j];
    if (d->vert_xyz) { xyz.resize(3 * (size_t)nl); for (int32_t i = 0; i < nl; ++i) for (int j = 0; j < 3; ++j) xyz[3 * (size_t)i + j] = d->vert_xyz[3 * (size_t)l2g[i] + j]; }
    std::vector<int32_t> t_idx, t_kind, r_idx, p_vert, p_act, colors, t_spl;
    std::vector<double> t_Binv, t_w, t_mu, t_la, t_k, t_kap, r_rest, r_w, r_lmin, r_lmax, p_xyz, p_nrm, h_coef, h_w, h_k;
    std::vector<int32_t> h_idx;
    for (int32_t t = 0; t < d->n_bends; ++t) {
        if (vrank[d->bend_idx[4 * (size_t)t]] != rank) continue;
        for (int k = 0; k < 4; ++k) { h_idx.push_back(g2l[d->bend_idx[4 * (size_t)t + k]]); h_coef.push_back(d->bend_coef[4 * (size_t)t + k]); }
        h_w.push_back(d->bend_weight[t]); h_k.push_back(d->bend_stiffness[t]);
    }
    for (int32_t t = 0; t < d->n_tets; ++t) {
        if (vrank[d->tet_idx[4 * (size_t)t]] != rank) continue;
        for (int k = 0; k < 4; ++k) t_idx.push_back(g2l[d->tet_idx[4 * (size_t)t + k]]);
        for (int k = 0; k < 9; ++k) t_Binv.push_back(d->tet_Binv[9 * (size_t)t + k]);
        t_w.push_back(d->tet_weight[t]); t_kind.push_back(d->tet_kind[t]); t_mu.push_back(d->tet_mu[t]); t_la.push_back(d->tet_lambda[t]); t_k.push_back(d->tet_k[t]);
        if (d->tet_kappa) t_kap.push_back(d->tet_kappa[t]);
        if (d->tet_spline) t_spl.push_back(d->tet_spline[t]);
    }
    for (int32_t t = 0; t < d->n_tris; ++t) {
        if (vrank[d->tri_idx[3 * (size_t)t]] != rank) continue;
        for (int k = 0; k < 3; ++k) r_idx.push_back(g2l[d->tri_idx[3 * (size_t)t + k]]);
        for (int k = 0; k < 4; ++k) r_rest.push_back(d->tri_rest[4 * (size_t)t + k]);
        r_w.push_back(d->tri_weight[t]); r_lmin.push_back(d->tri_limit_min[t]); r_lmax.push_back(d->tri_limit_max[t]);
    }
    for (int32_t p = 0; p < d->n_pins; ++p) {
        if (vrank[d->pin_vert[p]] != rank) continue;
        p_vert.push_back(g2l[d->pin_vert[p]]);
        for (int j = 0; j < 3; ++j) p_xyz.push_back(d->pin_xyz[3 * (size_t)p + j]);
        if (d->pin_active) p_act.push_back(d->pin_active[p]);
        if (d->pin_normal) for (int j = 0; j < 3; ++j) p_nrm.push_back(d->pin_normal[3 * (size_t)p + j]);
    }
    if (d->gs_colors) { colors.resize(nl); for (int32_t i = 0; i < nl; ++i) colors[i] = d->gs_colors[l2g[i]]; }
    admm_hip_desc sub = *d;
    sub.n_verts = nl; sub.masses = masses.data(); sub.vert_xyz = d->vert_xyz ? xyz.data() : nullptr;
    sub.n_tets = (int32_t)t_w.size(); sub.tet_idx = t_idx.data(); sub.tet_Binv = t_Binv.data(); sub.tet_weight = t_w.data(); sub.tet_kind = t_kind.data();
    sub.tet_mu = t_mu.data(); sub.tet_lambda = t_la.data(); sub.tet_k = t_k.data(); sub.tet_kappa = d->tet_kappa ? t_kap.data() : nullptr;
    sub.tet_spline = d->tet_spline ? t_spl.data() : nullptr;
    sub.n_tris = (int32_t)r_w.size(); sub.tri_idx = r_idx.data(); sub.tri_rest = r_rest.data(); sub.tri_weight = r_w.data();
    sub.tri_limit_min = r_lmin.data(); sub.tri_limit_max = r_lmax.data();
    sub.n_pins = (int32_t)p_vert.size(); sub.pin_vert = p_vert.data(); sub.pin_xyz = p_xyz.data(); sub.pin_active = d->pin_active ? p_act.data() : nullptr;
    sub.gs_colors = d->gs_colors ? colors.data() : nullptr;
    sub.pin_normal = d->pin_normal ? p_nrm.data() : nullptr;
    sub.n_bends = (int32_t)h_w.size(); sub.bend_idx = h_idx.data(); sub.bend_coef = h_coef.data(); sub.bend_weight = h_w.data(); sub.bend_stiffness = h_k.data();
    sub.rank = 0; sub.world_size = 0;
    if (int rc = create_impl(&sub, out)) return rc;
    admm_hip_ctx *c = *out;
    c->cm.on = true; c->cm.rank = rank; c->cm.world = world; c->cm.nv_global = nv; c->cm.n_components = ncomp;
    c->cm.l2g = std::move(l2g); c->cm.g2l = std::move(g2l);
    return ADMM_HIP_OK;
}

static int create_impl(const admm_hip_desc *d, admm_hip_ctx **out) {
    if (!out) return fail(ADMM_HIP_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = validate(d);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(ADMM_HIP_ERR_DEVICE, "no HIP device available: the ADMM hot path has no CPU fallback");
    if (d->device < 0 || d->device >= ndev) return fail(ADMM_HIP_ERR_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(d->device));

    admm_hip_ctx *c = new admm_hip_ctx();
    std::unique_ptr<admm_hip_ctx> guard(c);
    c->device = d->device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d->device) == hipSuccess && cus > 0) c->n_cus = cus; }
    c->nv = d->n_verts; c->n3 = 3 * d->n_verts;
    c->dt = d->dt > 0.0 ? d->dt : 1.0 / 24.0;
    c->linsolver = d->linsolver;
    c->pcg_max_iters = d->pcg_max_iters > 0 ? d->pcg_max_iters : 500;
    c->pcg_tol = d->pcg_tol > 0 ? d->pcg_tol : 1e-10;
    c->gs_max_iters = d->gs_max_iters > 0 ? d->gs_max_iters : 30;
    c->gs_tol = d->gs_tol >= 0 ? d->gs_tol : 1e-10;
    c->gs_omega = d->gs_omega > 0 ? d->gs_omega : 1.9;
    c->uz_max_iters = d->uzawa_max_iters > 0 ? d->uzawa_max_iters : 20;
    c->uz_tol = d->uzawa_tol > 0 ? d->uzawa_tol : 1e-10;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev_step0));
    HIP_TRY(hipEventCreate(&c->ev_step1));
    HIP_TRY(hipHostMalloc((void **)&c->h_sig, kSigWords * sizeof(int), hipHostMallocMapped));
    std::memset(c->h_sig, 0, kSigWords * sizeof(int));
    c->stop_host = env_flag("ADMM_HIP_STOP_HOST", false);      // A/B, tests: the early exit of the ADMM loop decided on the host on every path
    HIP_TRY(hipHostGetDevicePointer((void **)&c->d_sig, c->h_sig, 0));

    const double dt2 = c->dt * c->dt;
    const int nv = c->nv;

    // ---- element-block partition (multi-GPU): contiguous blocks of the caller's element order ----
    c->world = d->world_size > 1 ? d->world_size : 1;
    c->rank = d->world_size > 1 ? d->rank : 0;
    int32_t tb = 0, te = d->n_tets, rb = 0, re = d->n_tris, hb = 0, he = d->n_bends;
    if (c->world > 1) {
        admm_host::partition(d->n_tets, c->world, c->rank, &tb, &te);
        admm_host::partition(d->n_tris, c->world, c->rank, &rb, &re);
        admm_host::partition(d->n_bends, c->world, c->rank, &hb, &he);
    }
    c->nt_total = d->n_tets; c->ntri_total = d->n_tris; c->tri_begin = rb; c->nbend_total = d->n_bends; c->bend_begin = hb;
    // rows of the vertex -> (element, corner) incidence lists (k_gather_rhs): by list length inside 512-vertex windows
    std::vector<int32_t> g_order;
    {
        // (this rank's elements only: the lists are built from them)
        g_order = admm_host::incidence_row_order(nv, te - tb, d->tet_idx + 4 * (size_t)tb, re - rb, d->tri_idx + 3 * (size_t)rb, 0);
        HIP_TRY(c->g_order.upload(std::vector<int>(g_order.begin(), g_order.end())));
    }
    // ---- tets: sort by constitutive model (wave-uniform code paths), build the material table ----
    c->nt = te - tb; c->ldt = c->nt + 1;
    if (c->nt > 0) {
        const int nt = c->nt, ld = c->ldt;
        auto kap = [&](int t) { return (d->tet_kappa && d->tet_kind[t] >= ADMM_TET_SPLINE_NH && d->tet_kind[t] <= ADMM_TET_SPLINE_COROTATED) ? d->tet_kappa[t] : 0.0; };
        auto grp_t = [&](int t) {   // xu::NeoHookean / xu::StVK splines with kappa = 0 ARE the NH / StVK models
            const int k = d->tet_kind[t];
            if (kap(t) != 0.0 || k == ADMM_TET_SPLINE_TABLE || k == ADMM_TET_STABLE_NH) return 4;
            return k == ADMM_TET_LINEAR ? 0 : (k == ADMM_TET_STVK || k == ADMM_TET_SPLINE_STVK) ? 2 : k == ADMM_TET_SPLINE_COROTATED ? 3 : 1;
        };
        c->tet_perm.resize(nt);
        std::iota(c->tet_perm.begin(), c->tet_perm.end(), tb);
        // inside a model group: by the lowest vertex index (then the index sum), i.e. in the order their vertices are laid out -- the
        // position gathers of the local step and the corner-force gathers of the RHS then walk memory as coherently as the
        // caller's vertex numbering allows, whatever order the tets arrive in (shuffled tets of the 1 M-tet cube: local step
        // 108 -> 71 us, RHS gather 208 -> 45 us; generator order: unchanged)
        auto vsum = [&](int t) { return (long long)d->tet_idx[4 * (size_t)t] + d->tet_idx[4 * (size_t)t + 1] + d->tet_idx[4 * (size_t)t + 2] + d->tet_idx[4 * (size_t)t + 3]; };
        auto vmin = [&](int t) { return std::min(std::min(d->tet_idx[4 * (size_t)t], d->tet_idx[4 * (size_t)t + 1]), std::min(d->tet_idx[4 * (size_t)t + 2], d->tet_idx[4 * (size_t)t + 3])); };
        std::stable_sort(c->tet_perm.begin(), c->tet_perm.end(), [&](int a, int b) {
            const int ga = grp_t(a), gb = grp_t(b);
            if (ga != gb) return ga < gb;
            const int ma = vmin(a), mb = vmin(b);
            return ma != mb ? ma < mb : vsum(a) < vsum(b);
        });
        int cnt[5] = {0, 0, 0, 0, 0};
        for (int t = tb; t < te; ++t) cnt[grp_t(t)]++;
        c->kind_begin[0] = 0;
        for (int gI = 0; gI < 5; ++gI) c->kind_begin[gI + 1] = c->kind_begin[gI] + cnt[gI];
        std::map<std::tuple<double, double, double, double, int, int>, int> mat_map;
        std::vector<Mat> mats;
        std::vector<int4> idx(nt);
        std::vector<double> Binv((size_t)9 * ld, 0.0), sc(ld, 0.0);
        std::vector<int> mat(nt);
        for (int n = 0; n < nt; ++n) {
            const int o = c->tet_perm[n];
            idx[n] = make_int4(d->tet_idx[4 * o], d->tet_idx[4 * o + 1], d->tet_idx[4 * o + 2], d->tet_idx[4 * o + 3]);
            for (int k = 0; k < 9; ++k) Binv[(size_t)k * ld + n] = d->tet_Binv[9 * (size_t)o + k];
            sc[n] = dt2 * d->tet_weight[o] * d->tet_weight[o];
            const bool tabulated = d->tet_kind[o] == ADMM_TET_SPLINE_TABLE, snh = d->tet_kind[o] == ADMM_TET_STABLE_NH;
            const int stype = tabulated ? 3 : snh ? 4 : d->tet_kind[o] == ADMM_TET_SPLINE_STVK ? 1 : d->tet_kind[o] == ADMM_TET_SPLINE_COROTATED ? 2 : 0;
            const int table = tabulated ? d->tet_spline[o] : 0;
            auto key = std::make_tuple(d->tet_mu[o], d->tet_lambda[o], d->tet_k[o], kap(o), (kap(o) != 0.0 || tabulated || snh) ? stype : 0, table);
            auto it = mat_map.find(key);
            if (it == mat_map.end()) { it = mat_map.emplace(key, (int)mats.size()).first; mats.push_back(Mat{d->tet_mu[o], d->tet_lambda[o], d->tet_k[o], kap(o), stype, table}); }
            mat[n] = it->second;
        }
        HIP_TRY(c->t_idx.upload(idx)); HIP_TRY(c->t_sc.upload(sc));
        {   // Binv: recomputed by the local step from the rest positions when the tets come from one set of positions (they do
            // when TetEnergyTerm's constructor made them), streamed otherwise.  ADMM_HIP_TET_REST=0: always streamed (A/B, tests).
            std::vector<double> x0((size_t)3 * nv);
            c->tet_rest_mode = !env_flag("ADMM_HIP_TET_REST", true) ? 0 : admm_host::tet_rest_positions(nv, nt, d->tet_idx + 4 * (size_t)tb, d->tet_Binv + 9 * (size_t)tb, d->vert_xyz, x0.data());   // (this rank's tets)
            if (c->tet_rest_mode) HIP_TRY(c->t_x0.upload(x0));
            else HIP_TRY(c->t_Binv.upload(Binv));
        }
        HIP_TRY(c->t_mat.upload(mat)); HIP_TRY(c->mats.upload(mats));
        if (d->n_spline_tables > 0 && d->spline_tables) {
            static_assert(kSplineTableDoubles == ADMM_SPLINE_TABLE_DOUBLES && kSplineTableDoubles == admm_host::kSplineTableDoublesH, "spline table layout");
            HIP_TRY(c->spl_tab.upload(std::vector<double>(d->spline_tables, d->spline_tables + (size_t)d->n_spline_tables * ADMM_SPLINE_TABLE_DOUBLES)));
        }
        HIP_TRY(c->t_u.alloc((size_t)9 * ld)); HIP_TRY(c->t_u.zero());
        HIP_TRY(c->t_z.alloc((size_t)9 * ld)); HIP_TRY(c->t_z.zero());
        // the chunks' reduction lists and the vertex -> records incidence, on the permuted numbering
        static_assert(kChunkFanK == admm_host::kChunkFan && kChunkLdK == admm_host::kChunkLd, "kernels.hpp and host_setup.hpp disagree on the chunk layout");
        std::vector<int32_t> pidx((size_t)4 * nt);
        for (int n = 0; n < nt; ++n) { pidx[4 * n] = idx[n].x; pidx[4 * n + 1] = idx[n].y; pidx[4 * n + 2] = idx[n].z; pidx[4 * n + 3] = idx[n].w; }
        const admm_host::TetChunks ch = admm_host::tet_chunks(nt, pidx.data(), c->kind_begin);
        if ((size_t)ch.n_rec * 32 + 32 >= (size_t)1 << 31) return fail(ADMM_HIP_ERR_ARG, "too many corner-force records for 32-bit offsets");
        c->chunk_base[0] = 0;
        for (int gI = 0; gI < 5; ++gI) c->chunk_base[gI + 1] = c->chunk_base[gI] + blocks_for(cnt[gI]);
        HIP_TRY(c->ch_ent.upload(ch.ent)); HIP_TRY(c->ch_group.upload(std::vector<int>(ch.group_base.begin(), ch.group_base.end())));
        HIP_TRY(c->ch_rec.upload(std::vector<int>(ch.rec_base.begin(), ch.rec_base.end())));
        HIP_TRY(c->t_rec.alloc((size_t)4 * (ch.n_rec + 1))); HIP_TRY(c->t_rec.zero());     // record n_rec stays zero: the padding of the incidence lists
        HIP_TRY(c->t_inc.upload(admm_host::record_incidence(nv, ch.n_rec, ch.rec_vertex.data(), ch.n_rec, g_order.data())));
        c->n_rec = ch.n_rec;
    }
    // ---- tris ----
    c->ntri = re - rb; c->ldr = c->ntri + 1;
    if (c->ntri > 0) {
        const int n = c->ntri, ld = c->ldr;
        std::vector<int4> idx(n);
        std::vector<double> rest((size_t)4 * ld, 0.0), sc(ld, 0.0), lmin(ld, -100.0), lmax(ld, 100.0);
        c->tri_perm.resize(n);
        std::iota(c->tri_perm.begin(), c->tri_perm.end(), rb);
        auto rmin = [&](int t) { return std::min(d->tri_idx[3 * (size_t)t], std::min(d->tri_idx[3 * (size_t)t + 1], d->tri_idx[3 * (size_t)t + 2])); };
        auto rsum = [&](int t) { return (long long)d->tri_idx[3 * (size_t)t] + d->tri_idx[3 * (size_t)t + 1] + d->tri_idx[3 * (size_t)t + 2]; };
        std::stable_sort(c->tri_perm.begin(), c->tri_perm.end(), [&](int a, int b) {   // same locality rule as the tets
            const int ma = rmin(a), mb = rmin(b);
            return ma != mb ? ma < mb : rsum(a) < rsum(b);
        });
        std::vector<int32_t> tri_sorted(3 * (size_t)n);
        for (int t = 0; t < n; ++t) {
            const int o = c->tri_perm[t];
            for (int k = 0; k < 3; ++k) tri_sorted[3 * (size_t)t + k] = d->tri_idx[3 * (size_t)o + k];
            idx[t] = make_int4(d->tri_idx[3 * o], d->tri_idx[3 * o + 1], d->tri_idx[3 * o + 2], 0);
            for (int k = 0; k < 4; ++k) rest[(size_t)k * ld + t] = d->tri_rest[4 * (size_t)o + k];
            sc[t] = dt2 * d->tri_weight[o] * d->tri_weight[o];
            lmin[t] = d->tri_limit_min[o]; lmax[t] = d->tri_limit_max[o];
            if (lmin[t] > 0.0 || lmax[t] < 100.0) c->tri_limited = true;
        }
        HIP_TRY(c->r_idx.upload(idx)); HIP_TRY(c->r_rest.upload(rest)); HIP_TRY(c->r_sc.upload(sc));
        HIP_TRY(c->r_lmin.upload(lmin)); HIP_TRY(c->r_lmax.upload(lmax));
        HIP_TRY(c->r_u.alloc((size_t)6 * ld)); HIP_TRY(c->r_u.zero());
        HIP_TRY(c->r_z.alloc((size_t)6 * ld)); HIP_TRY(c->r_z.zero());
        HIP_TRY(c->r_cf.alloc((size_t)12 * ld)); HIP_TRY(c->r_cf.zero());
        HIP_TRY(c->r_inc.upload(admm_host::incidence_sell(nv, n, 3, tri_sorted.data(), n * 4, g_order.data())));
    }
    // ---- bending hinges ----
    c->nbend = he - hb; c->ldb = c->nbend + 1;
    if (c->nbend > 0) {
        const int n = c->nbend, ld = c->ldb;
        c->bend_perm.resize(n);
        std::iota(c->bend_perm.begin(), c->bend_perm.end(), hb);
        auto hmin = [&](int t) { const int32_t *q = d->bend_idx + 4 * (size_t)t; return std::min(std::min(q[0], q[1]), std::min(q[2], q[3])); };
        std::stable_sort(c->bend_perm.begin(), c->bend_perm.end(), [&](int a, int b) { return hmin(a) < hmin(b); });   // same locality rule as the other elements
        std::vector<int4> idx(n);
        std::vector<int32_t> sorted(4 * (size_t)n);
        std::vector<double> coef((size_t)4 * ld, 0.0), sc(ld, 0.0), gam(ld, 0.0);
        for (int t = 0; t < n; ++t) {
            const int o = c->bend_perm[t];
            const int32_t *q = d->bend_idx + 4 * (size_t)o;
            idx[t] = make_int4(q[0], q[1], q[2], q[3]);
            for (int k = 0; k < 4; ++k) { sorted[4 * (size_t)t + k] = q[k]; coef[(size_t)k * ld + t] = d->bend_coef[4 * (size_t)o + k]; }
            const double w2 = d->bend_weight[o] * d->bend_weight[o];
            sc[t] = dt2 * w2; gam[t] = w2 / (d->bend_stiffness[o] + w2);
        }
        HIP_TRY(c->h_idx.upload(idx)); HIP_TRY(c->h_coef.upload(coef)); HIP_TRY(c->h_sc.upload(sc)); HIP_TRY(c->h_gam.upload(gam));
        {   // the hinges' stiffness itself: their energy (monitor.hpp)
            std::vector<double> kst(ld, 0.0);
            for (int t = 0; t < n; ++t) kst[t] = d->bend_stiffness[c->bend_perm[t]];
            HIP_TRY(c->h_kst.upload(kst));
        }
        HIP_TRY(c->h_u.alloc((size_t)3 * ld)); HIP_TRY(c->h_u.zero());
        HIP_TRY(c->h_z.alloc((size_t)3 * ld)); HIP_TRY(c->h_z.zero());
        HIP_TRY(c->h_cf.alloc((size_t)12 * ld)); HIP_TRY(c->h_cf.zero());
        HIP_TRY(c->h_inc.upload(admm_host::incidence_sell(nv, n, 4, sorted.data(), n * 4, g_order.data())));
    }
    // ---- pins ----
    double max_w = 0.0;
    for (int t = 0; t < d->n_tets; ++t) max_w = std::max(max_w, d->tet_weight[t]);
    for (int t = 0; t < d->n_tris; ++t) max_w = std::max(max_w, d->tri_weight[t]);
    for (int t = 0; t < d->n_bends; ++t) max_w = std::max(max_w, d->bend_weight[t]);
    // unit normals of the slide pins (zero = ordinary pin)
    std::vector<double> nrm_pin(3 * (size_t)d->n_pins, 0.0);
    bool any_slide = false;
    if (d->pin_normal)
        for (int p = 0; p < d->n_pins; ++p) {
            const double *q = d->pin_normal + 3 * (size_t)p;
            const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            if (l > 0.0) { for (int j = 0; j < 3; ++j) nrm_pin[3 * (size_t)p + j] = q[j] / l; any_slide = true; }
        }
    {
        double mu, la, k;
        admm_host::lame(10000000.0, 0.499, &mu, &la, &k); // Lame::rubber(), SpringEnergyTerm.hpp:50-51
        c->pin_weight = d->pin_weight > 0 ? d->pin_weight : std::sqrt(k * 2.0);
    }
    const bool pins_as_terms = (d->linsolver == 0 || d->linsolver == 2); // Solver.cpp:190-196
    if (pins_as_terms && d->n_pins > 0) {
        c->npin_terms = d->n_pins;
        max_w = std::max(max_w, c->pin_weight);
        std::vector<int> vp(nv, -1), act(d->n_pins, 1);
        std::vector<double> xyz(d->pin_xyz, d->pin_xyz + 3 * (size_t)d->n_pins);
        for (int p = 0; p < d->n_pins; ++p) {
            if (vp[d->pin_vert[p]] >= 0) return fail(ADMM_HIP_ERR_ARG, "duplicate pin vertex");
            vp[d->pin_vert[p]] = p;
            if (d->pin_active) act[p] = d->pin_active[p] ? 1 : 0;
        }
        c->pin_vert_h.assign(d->pin_vert, d->pin_vert + d->n_pins);
        HIP_TRY(c->pin_vert_d.upload(std::vector<int>(d->pin_vert, d->pin_vert + d->n_pins)));      // (monitor.hpp: pin term -> vertex)
        HIP_TRY(c->vert_pin.upload(vp)); HIP_TRY(c->pin_active.upload(act)); HIP_TRY(c->pin_xyz.upload(xyz));
        HIP_TRY(c->pin_u.alloc(3 * (size_t)d->n_pins)); HIP_TRY(c->pin_u.zero());
        HIP_TRY(c->pin_z.alloc(3 * (size_t)d->n_pins)); HIP_TRY(c->pin_z.zero());
        c->pin_nrm_h = nrm_pin; c->has_slide = any_slide;
        HIP_TRY(c->pin_nrm.upload(nrm_pin));
    }
    if (d->linsolver == 1) {
        std::vector<int> flag(nv, 0);
        std::vector<double> xyz((size_t)3 * nv, 0.0);
        c->pin_nrm_h.assign((size_t)3 * nv, 0.0);      // (per VERTEX with this solver: the pin set is replaced freely)
        for (int p = 0; p < d->n_pins; ++p) {
            if (d->pin_active && !d->pin_active[p]) continue;
            const bool slide = nrm_pin[3 * (size_t)p] != 0.0 || nrm_pin[3 * (size_t)p + 1] != 0.0 || nrm_pin[3 * (size_t)p + 2] != 0.0;
            flag[d->pin_vert[p]] = slide ? 2 : 1;
            for (int j = 0; j < 3; ++j) { xyz[3 * (size_t)d->pin_vert[p] + j] = d->pin_xyz[3 * (size_t)p + j]; c->pin_nrm_h[3 * (size_t)d->pin_vert[p] + j] = nrm_pin[3 * (size_t)p + j]; }
            c->gs_has_pins = true;
        }
        c->has_slide = any_slide;
        HIP_TRY(c->gs_pin_flag.upload(flag)); HIP_TRY(c->gs_pin_xyz.upload(xyz)); HIP_TRY(c->gs_pin_nrm.upload(c->pin_nrm_h));
    }
    // constraint weight: Solver.cpp:235 (GS: 3 max W), :239 (Uzawa: 1), :245 (override)
    c->constraint_w = (d->linsolver == 1) ? 3.0 * max_w : 1.0;
    if (d->constraint_w > 0.0) c->constraint_w = d->constraint_w;
    c->obst.n = d->n_obstacles;
    c->obst.gmeta = nullptr; c->obst.gdata = nullptr;
    for (int j = 0; j < d->n_obstacles; ++j) {
        c->obst.kind[j] = d->obstacle_kind[j];
        for (int k = 0; k < 4; ++k) c->obst.par[j][k] = d->obstacle_params[4 * j + k];
        if (d->obstacle_kind[j] == ADMM_OBJ_PLANE) {      // unit normal, offset scaled with it
            const double il = 1.0 / std::sqrt(c->obst.par[j][0] * c->obst.par[j][0] + c->obst.par[j][1] * c->obst.par[j][1] + c->obst.par[j][2] * c->obst.par[j][2]);
            for (int k = 0; k < 4; ++k) c->obst.par[j][k] *= il;
        }
    }
    if (d->n_obstacle_grids > 0 && d->obstacle_grid_meta && d->obstacle_grid_data) {
        size_t nodes = 0;
        for (int g = 0; g < d->n_obstacle_grids; ++g) {
            const double *m = d->obstacle_grid_meta + 10 * (size_t)g;
            nodes = std::max(nodes, (size_t)m[9] + (size_t)m[6] * (size_t)m[7] * (size_t)m[8]);
        }
        HIP_TRY(c->obst_gmeta.upload(std::vector<double>(d->obstacle_grid_meta, d->obstacle_grid_meta + 10 * (size_t)d->n_obstacle_grids)));
        HIP_TRY(c->obst_gdata.upload(std::vector<double>(d->obstacle_grid_data, d->obstacle_grid_data + 4 * nodes)));
        c->obst.gmeta = c->obst_gmeta.p; c->obst.gdata = c->obst_gdata.p;
    }
    HIP_TRY(c->obst_dev.upload(std::vector<Obstacles>(1, c->obst)));

    // ---- system matrix ----
    c->Ahat = admm_host::assemble_Ahat(nv, c->dt, d->n_tets, d->tet_idx, d->tet_Binv, d->tet_weight, d->n_tris, d->tri_idx,
                                       d->tri_rest, d->tri_weight, pins_as_terms ? d->n_pins : 0, d->pin_vert, c->pin_weight);
    if (d->n_bends > 0) c->Ahat = admm_host::add_stencil_terms(c->Ahat, c->dt, d->n_bends, d->bend_idx, d->bend_coef, d->bend_weight);
    {
        const admm_host::Sell S = admm_host::csr_to_sell(c->Ahat);
        for (int w : S.slice_width) c->A_wmax = std::max(c->A_wmax, w);
        HIP_TRY(c->A.upload(S));
    }
    {
        std::vector<double> mass(d->masses, d->masses + c->n3), dinv(c->n3);
        for (int vtx = 0; vtx < nv; ++vtx) {
            double diag = 0.0;
            for (int k = c->Ahat.rowptr[vtx]; k < c->Ahat.rowptr[vtx + 1]; ++k)
                if (c->Ahat.col[k] == vtx) diag = c->Ahat.val[k];
            for (int j = 0; j < 3; ++j) dinv[3 * (size_t)vtx + j] = 1.0 / (mass[3 * (size_t)vtx + j] + diag);
        }
        HIP_TRY(c->m.upload(mass)); HIP_TRY(c->dinv.upload(dinv));
    }
    HIP_TRY(c->x.alloc(c->n3)); HIP_TRY(c->x.zero());
    HIP_TRY(c->v.alloc(c->n3)); HIP_TRY(c->v.zero());
    HIP_TRY(c->Mxbar.alloc(c->n3)); HIP_TRY(c->Mxbar.zero());
    HIP_TRY(c->curr.alloc(c->n3)); HIP_TRY(c->curr.zero());
    HIP_TRY(c->b.alloc(c->n3)); HIP_TRY(c->b.zero());
    c->NB = std::max(1, (c->A.n_slices + 3) / 4);              // SpMV-type kernels: one SELL slice per wave
    c->NBV = std::max(1, (c->nv + 255) / 256);                  // vector-update kernel: one vertex per thread
    HIP_TRY(c->cg_r.alloc(c->n3)); HIP_TRY(c->cg_u.alloc(c->n3)); HIP_TRY(c->cg_w.alloc(c->n3));
    HIP_TRY(c->cg_p.alloc(c->n3)); HIP_TRY(c->cg_s.alloc(c->n3));
    HIP_TRY(c->cg_p.zero()); HIP_TRY(c->cg_s.zero());
    HIP_TRY(c->part.alloc(6 * (size_t)c->NB)); HIP_TRY(c->part_b.alloc(3 * (size_t)c->NB));
    HIP_TRY(c->cg_scal.alloc(2)); HIP_TRY(c->cg_scal.zero());
    HIP_TRY(c->counters.alloc(kCntWords)); HIP_TRY(c->counters.zero());
    c->create_xyz = d->vert_xyz;
    c->big_allowed = env_flag("ADMM_HIP_BIG", true);
    c->defl_start = env_int("ADMM_HIP_DEFL_START", c->defl_start);
    c->defl_use_resid = env_flag("ADMM_HIP_DEFL_RESID", true);
    c->kernel_clock = env_flag("ADMM_HIP_KERNEL_CLOCK", false);
    c->uz_lanes_debug = env_flag("ADMM_HIP_UZ_LANES_DEBUG", false);
    if (d->vert_xyz) c->tc_xyz_h.assign(d->vert_xyz, d->vert_xyz + c->n3);
    if (d->vert_xyz && d->linsolver != 1) c->xyz_h.assign(d->vert_xyz, d->vert_xyz + c->n3);      // (the launch-path two-level PCG plans lazily)
    {   // distributed solve of ONE body (ADMM_HIP_DIST_SOLVE=1, element-block partition): contiguous vertex rows per rank, 64-aligned
        const bool force_comm = env_flag("ADMM_HIP_FORCE_COMM", false);     // (tests: a world of ONE with a communicator runs the same collectives through RCCL)
        if (env_flag("ADMM_HIP_DIST_SOLVE", false) && (c->world > 1 || force_comm) && d->linsolver != 1) {
            const int ns = (nv + 63) / 64;
            c->row_lo = 64 * (int)((int64_t)ns * c->rank / c->world);
            c->row_hi = c->rank + 1 == c->world ? nv : 64 * (int)((int64_t)ns * (c->rank + 1) / c->world);
            c->dist_solve = true;
        }
    }
    if (d->linsolver != 1 && !c->dist_solve) HIP_TRY(plan_pcg_onchip(c));
    c->create_xyz = nullptr;
    if (d->linsolver != 1) {
        c->rc_enabled = !env_flag("ADMM_HIP_NO_RECYCLE", false);
        // pairs per projection: four until the scene has shown how many iterations its solves need (step_impl).  (Round 6 looked at this
        // test again: it is biased -- the start-up transient decays from frame to frame, so the count measured SECOND looks better, and it
        // picks three on the bench body where four need fewer iterations.  But fewer iterations from a richer basis are not free: see kRcHist.
        // The test stays.)
        c->rc_pairs = kRc;
        c->NBR = std::max(1, std::min((nv + 255) / 256, 256));
        c->n3i = std::max(c->n3, 3 * c->oc_rows);
        if (c->rc_enabled) {
            c->rc_hist = (c->oc_enabled && c->oc_plan) ? 1 : 0;
            HIP_TRY(c->rc_buf.alloc((size_t)(admm_hip_ctx::kRcAllSlots + (c->rc_hist ? admm_hip_ctx::kRcDepth * admm_hip_ctx::kRcHist : 0)) * 2 * c->n3i));
            HIP_TRY(c->rc_r0.alloc(c->n3i)); HIP_TRY(c->rc_xs.alloc(c->n3i));
            HIP_TRY(c->rc_part.alloc((size_t)3 * kRcQ * c->NBR)); HIP_TRY(c->rc_coef.alloc(3 * kRc)); HIP_TRY(c->rc_coef.zero());
        }
    }

    if (d->linsolver == 1) {
        c->color_h.resize(nv);
        if (d->gs_colors) {
            c->n_colors = 0;
            for (int i = 0; i < nv; ++i) {
                if (d->gs_colors[i] < 0) return fail(ADMM_HIP_ERR_ARG, "negative colour");
                c->color_h[i] = d->gs_colors[i];
                c->n_colors = std::max(c->n_colors, d->gs_colors[i] + 1);
            }
            for (int i = 0; i < nv; ++i)
                for (int k = c->Ahat.rowptr[i]; k < c->Ahat.rowptr[i + 1]; ++k)
                    if (c->Ahat.col[k] != i && c->Ahat.val[k] != 0.0 && c->color_h[c->Ahat.col[k]] == c->color_h[i])
                        return fail(ADMM_HIP_ERR_ARG, "gs_colors is not a valid colouring of A");
        } else {
            // colour the graph of NON-ZERO couplings: exact zeros do not couple nodes (the sweep skips them,
            // NodalMultiColorGS.hpp:194) and on structured meshes they would only multiply the colour count
            std::vector<int32_t> rp(nv + 1, 0), ci;
            ci.reserve(c->Ahat.col.size());
            for (int i = 0; i < nv; ++i) {
                for (int k = c->Ahat.rowptr[i]; k < c->Ahat.rowptr[i + 1]; ++k)
                    if (c->Ahat.val[k] != 0.0 || c->Ahat.col[k] == i) ci.push_back(c->Ahat.col[k]);
                rp[i + 1] = (int32_t)ci.size();
            }
            c->n_colors = admm_host::greedy_coloring(nv, rp.data(), ci.data(), c->color_h.data());
        }
        c->color_ptr_h.assign(c->n_colors + 1, 0);
        for (int i = 0; i < nv; ++i) c->color_ptr_h[c->color_h[i] + 1]++;
        for (int k = 0; k < c->n_colors; ++k) c->color_ptr_h[k + 1] += c->color_ptr_h[k];
        std::vector<int> nodes(nv), pos(c->color_ptr_h.begin(), c->color_ptr_h.end() - 1);
        for (int i = 0; i < nv; ++i) nodes[pos[c->color_h[i]]++] = i;
        HIP_TRY(c->color_nodes.upload(nodes));
        {   // colour-ordered SELL of the off-diagonal non-zeros for the sweep kernel
            std::vector<int32_t> col32(c->color_h.begin(), c->color_h.end());
            admm_host::GsSell g = admm_host::build_gs_sell(c->Ahat, c->n_colors, col32);
            HIP_TRY(c->gs_sell.upload(g.sell));
            HIP_TRY(c->gs_slot_node.upload(g.slot_node)); HIP_TRY(c->gs_diag.upload(g.diag));
            c->gs_color_slice.assign(g.color_slice.begin(), g.color_slice.end());
            const bool three_kernels = env_flag("ADMM_HIP_GS_THREE_KERNELS", false);   // A/B switch
            if (c->n_colors == 2 && !three_kernels) {   // two-colour scheme: roll-back copy + partial sums (2 x 2 x nbA last colour, 2 x nbB first colour)
                const int nbB = (c->gs_color_slice[1] - c->gs_color_slice[0] + 3) / 4, nbA = (c->gs_color_slice[2] - c->gs_color_slice[1] + 3) / 4;
                HIP_TRY(c->gs_xb.alloc(c->n3)); HIP_TRY(c->gs_xb.zero());
                HIP_TRY(c->gs_part2.alloc(4 * (size_t)nbA + 2 * (size_t)nbB)); HIP_TRY(c->gs_part2.zero());
            }
            // three colours (triangulated cloth): the same, generalised (k_gs_colorN): no residual SpMV per sweep.  Every colour kernel
            // pays ~1.3 us for its share of the residual, the SpMV launch it replaces cost 5.6 us: beyond three or four colours the plain
            // sequence is faster (ADMM_HIP_GS_FUSED_MAX=n raises the limit: tests).
            const int fused_max = env_int("ADMM_HIP_GS_FUSED_MAX", 3);
            if (c->n_colors >= 3 && c->n_colors <= fused_max && !three_kernels) {
                int nE = 0;
                for (int k = 0; k + 1 < c->n_colors; ++k) nE += (c->gs_color_slice[k + 1] - c->gs_color_slice[k] + 3) / 4;
                const int nbL = (c->gs_color_slice[c->n_colors] - c->gs_color_slice[c->n_colors - 1] + 3) / 4;
                // per SELL entry: is the column's colour below the row's?  (padding entries: no)
                std::vector<unsigned char> low(g.sell.idx.size(), 0);
                for (int32_t sl = 0; sl < g.sell.n_slices; ++sl)
                    for (int l = 0; l < 64; ++l) {
                        const int32_t row = g.slot_node[(size_t)64 * sl + l];
                        if (row < 0) continue;
                        for (int32_t k = 0; k < g.sell.slice_width[sl]; ++k) {
                            const size_t e = (size_t)g.sell.slice_ptr[sl] + 64 * (size_t)k + l;
                            if (g.sell.val[e] != 0.0 && c->color_h[g.sell.idx[e]] < c->color_h[row]) low[e] = 1;
                        }
                    }
                if (nE > 0 && nbL > 0) {
                    HIP_TRY(c->gs_low.upload(low));
                    HIP_TRY(c->gs_xb.alloc(c->n3)); HIP_TRY(c->gs_xb.zero());
                    HIP_TRY(c->gs_part2.alloc(4 * (size_t)nbL + 2 * (size_t)nE)); HIP_TRY(c->gs_part2.zero());
                    c->gs_fusedN = true;
                }
            }
        }
    }
    if (d->linsolver == 1) { HIP_TRY(c->gs_proj.alloc(1)); HIP_TRY(c->gs_proj.zero()); }
    if (d->linsolver == 1) HIP_TRY(plan_gs_persist(c));
    if (d->linsolver == 2) {
        c->uz_freeze = env_flag("ADMM_HIP_UZ_FREEZE", false);
        c->NBU = std::max(1, std::min((nv + 255) / 256, 256));
        HIP_TRY(c->uz_cn.alloc(c->n3)); HIP_TRY(c->uz_cn.zero());
        HIP_TRY(c->uz_q1.alloc(c->n3)); HIP_TRY(c->uz_q2.alloc(c->n3)); HIP_TRY(c->uz_q2.zero());
        HIP_TRY(c->uz_dmax.alloc(2)); HIP_TRY(c->uz_dmax.zero()); HIP_TRY(c->uz_dacc.alloc(c->n3)); HIP_TRY(c->uz_dacc.zero());
        HIP_TRY(c->uz_cc.alloc(nv)); HIP_TRY(c->uz_y.alloc(nv)); HIP_TRY(c->uz_y.zero());
        HIP_TRY(c->uz_r.alloc(nv)); HIP_TRY(c->uz_d.alloc(nv)); HIP_TRY(c->uz_q3.alloc(nv));
        HIP_TRY(c->uz_part.alloc(2 * (size_t)c->NBU)); HIP_TRY(c->uz_scal.alloc(1)); HIP_TRY(c->uz_scal.zero());
        {   // column cache of the Schur iterations: needs A = K (x) I3 (per-vertex masses, which is all the reference has).
            // ADMM_HIP_UZ_CACHE=0 switches it off (every Schur iteration is then an on-chip PCG solve, as in rounds 1-2),
            // ADMM_HIP_UZ_CACHE_MB bounds its HBM (default 16 GiB of the 288; allocated at the first contact).
            const char *mb = getenv("ADMM_HIP_UZ_CACHE_MB");
            bool per_vertex = true;
            for (int v = 0; v < nv && per_vertex; ++v)
                per_vertex = d->masses[3 * (size_t)v] == d->masses[3 * (size_t)v + 1] && d->masses[3 * (size_t)v] == d->masses[3 * (size_t)v + 2];
            const double bytes = (mb ? atof(mb) : 16384.0) * 1048576.0;
            c->uzc_cap = (size_t)std::min<double>((double)nv, std::floor(bytes / (8.0 * nv)));
            c->uzc_on = env_flag("ADMM_HIP_UZ_CACHE", true) && per_vertex && c->uzc_cap >= 3;
            if (c->uzc_on) {
                c->uzc_slot_h.assign(nv, -1);
                HIP_TRY(c->uzc_slot.upload(c->uzc_slot_h)); HIP_TRY(c->uzc_act.alloc(nv)); HIP_TRY(c->uzc_miss.alloc(nv));
                HIP_TRY(c->uzc_info.alloc(4)); HIP_TRY(c->uzc_info.zero()); HIP_TRY(c->uzc_flag.alloc(nv));
                HIP_TRY(c->uzc_pos.alloc(nv)); HIP_TRY(c->uz_y0.alloc(nv));
                c->uzc_test_iters = env_int("ADMM_HIP_TEST_UZ_COL_ITERS", 0);
                c->uzc_compact = env_flag("ADMM_HIP_UZ_COMPACT", true);
                c->uzp_enabled = env_flag("ADMM_HIP_UZ_PERSIST", true);
                c->uzc_one_block_max = env_int("ADMM_HIP_UZ_LIST_BLOCKS", c->uzc_one_block_max, 0);
                c->test_abort_uzp = env_int("ADMM_HIP_TEST_ABORT_SCHUR", 0);
                c->uz_lanes_cfg = env_int("ADMM_HIP_UZ_LANES", 0, 1, 8);      // streams of a batch of column solves (uz_lane_count)
                if (d->n_obstacles > 0) {      // a scene with colliders will need columns: the lanes are set up here, not inside its first touchdown
                    const int L = uz_lane_count(c, 8);
                    if (L >= 2 && uz_make_lanes(c, L)) return fail(ADMM_HIP_ERR_DEVICE, "create: streams / memory of the UzawaCG column lanes");
                    // look-ahead (ADMM_HIP_UZ_AHEAD=f: frames of travel; default 0 = OFF): needs room for the lanes BESIDE the loop's own solve.
                    // Off by default since the batches take 39 ms: constant-velocity prediction lists layers that never touch (a landing body
                    // decelerates) -- 200 frames of cube100k_uzawa_floor: 2 layers needed, 4-5 solved ahead, 1 277-1 300 against 1 311-1 329
                    // ADMM it/s without (profiles/r05_uzawa_look_ahead.txt).  What it buys is the stall: no solve ever waits for a column.
                    const char *ae = getenv("ADMM_HIP_UZ_AHEAD");
                    c->pf_frames = ae ? atof(ae) : 0.0;
                    c->pf_on = L >= 2 && c->pf_frames > 0.0 && uz_lane_fit(c) >= 2;
                    if (c->pf_on) HIP_TRY(c->pf_list.alloc((size_t)nv + 1));
                }
                { const int pr = env_int("ADMM_HIP_UZ_PERSIST_ROWS", 0); c->uzp_rows = (pr == 8 || pr == 16) ? pr : 0; }   // 0: two launches per Schur iteration (A/B, tests)   // 0: full-height column pass in every Schur iteration (A/B)
                c->uzc_one_max = env_int("ADMM_HIP_UZ_ONE_MAX", c->uzc_one_max, 0, 1024);      // test hooks
                c->uzc_compact_max = env_int("ADMM_HIP_UZ_COMPACT_MAX", c->uzc_compact_max, 0);
            }
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    *out = guard.release();
    return ADMM_HIP_OK;
}

void admm_hip_destroy(admm_hip_ctx *ctx) { delete ctx; }

int admm_hip_num_rows(const admm_hip_ctx *c) { return c ? 9 * c->nt_total + 6 * c->ntri_total + 3 * c->nbend_total + 6 * c->npin_terms : 0; }

static int set_state_impl(admm_hip_ctx *c, const double *x, const double *v);
static int get_state_impl(admm_hip_ctx *c, double *x, double *v);

int admm_hip_set_state(admm_hip_ctx *c, const double *x, const double *v) {
    if (!c || !x) return fail(ADMM_HIP_ERR_ARG, "set_state: NULL argument");
    if (!c->cm.on) return set_state_impl(c, x, v);
    // component partition: the caller's arrays are numbered globally; this rank takes its bodies
    std::vector<double> xl(c->n3), vl(v ? c->n3 : 0);
    for (int i = 0; i < c->nv; ++i)
        for (int j = 0; j < 3; ++j) { xl[3 * (size_t)i + j] = x[3 * (size_t)c->cm.l2g[i] + j]; if (v) vl[3 * (size_t)i + j] = v[3 * (size_t)c->cm.l2g[i] + j]; }
    return set_state_impl(c, xl.data(), v ? vl.data() : nullptr);
}

// component partition: this rank's entries go into the caller's globally numbered arrays; with a communicator the parts of all
// ranks are merged (one sum all-reduce of a vector that is zero outside the rank's own entries), without one the other ranks'
// entries are left as they are
int admm_hip_get_state(admm_hip_ctx *c, double *x, double *v) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_state: NULL context");
    if (!c->cm.on) return get_state_impl(c, x, v);
    // With a communicator this call is a COLLECTIVE: every rank runs both merges (x, then v) whatever it asked for, so that ranks
    // passing different NULL-ness cannot dead-lock each other.
    const bool both = c->cm_comm != nullptr;
    std::vector<double> xl((x || both) ? c->n3 : 0), vl((v || both) ? c->n3 : 0);
    if (int rc = get_state_impl(c, (x || both) ? xl.data() : nullptr, (v || both) ? vl.data() : nullptr)) return rc;
    const size_t n3g = 3 * (size_t)c->cm.nv_global;
    std::vector<double> sink;
    for (int pass = 0; pass < 2; ++pass) {
        double *dst = pass == 0 ? x : v;
        const std::vector<double> &src = pass == 0 ? xl : vl;
        if (!dst && both) { sink.resize(n3g); dst = sink.data(); }
        if (!dst) continue;
        if (!c->cm_comm) {
            for (int i = 0; i < c->nv; ++i) for (int j = 0; j < 3; ++j) dst[3 * (size_t)c->cm.l2g[i] + j] = src[3 * (size_t)i + j];
            continue;
        }
        std::vector<double> full(n3g, 0.0);
        for (int i = 0; i < c->nv; ++i) for (int j = 0; j < 3; ++j) full[3 * (size_t)c->cm.l2g[i] + j] = src[3 * (size_t)i + j];
        if (c->cm_buf.n < n3g) HIP_TRY(c->cm_buf.alloc(n3g));
        HIP_TRY(hipMemcpyAsync(c->cm_buf.p, full.data(), n3g * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (g_rccl.AllReduce(c->cm_buf.p, c->cm_buf.p, n3g, ncclDouble, ncclSum, c->cm_comm, c->stream) != ncclSuccess)
            return fail(ADMM_HIP_ERR_COMM, "get_state: ncclAllReduce (merge of the ranks' bodies) failed");
        HIP_TRY(hipMemcpyAsync(dst, c->cm_buf.p, n3g * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ADMM_HIP_OK;
}

static int set_state_impl(admm_hip_ctx *c, const double *x, const double *v) {
    if (!c || !x) return fail(ADMM_HIP_ERR_ARG, "set_state: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->x.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (v) HIP_TRY(hipMemcpyAsync(c->v.p, v, c->n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(hipMemsetAsync(c->v.p, 0, c->n3 * sizeof(double), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_sig && c->h_sig[kSigAbort]) {   // the steps before this call hit a barrier time-out; their result is overwritten anyway
        c->h_sig[kSigAbort] = 0; c->oc_gave_up = true; c->oc_enabled = false; c->gsp_enabled = false; c->uzp_enabled = false; c->rc_iter = 0;
        c->rc_hist = 0; c->rc_prev_valid = 0; c->rc_prev2_valid = 0;   // (pairs half-written by the aborted solve, and in the on-chip row order)
        if (c->oc_bar.p) HIP_TRY(c->oc_bar.zero());
        if (c->gsp_abort.p) HIP_TRY(c->gsp_abort.zero());
        if (c->uzp_abort.p) HIP_TRY(c->uzp_abort.zero());
        HIP_TRY(hipMemcpy(c->x.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice));
        if (v) HIP_TRY(hipMemcpy(c->v.p, v, c->n3 * sizeof(double), hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(c->v.p, 0, c->n3 * sizeof(double)));
    }
    c->pending.clear();
    c->state_set = true;
    c->xbar_of_state = false;
    return ADMM_HIP_OK;
}

static int get_state_impl(admm_hip_ctx *c, double *x, double *v) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_state: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    if (x) HIP_TRY(hipMemcpyAsync(x, c->x.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (v) HIP_TRY(hipMemcpyAsync(v, c->v.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_sig && c->h_sig[kSigAbort]) {   // replay on the launch path, then read the state again
        if (int rc = recover_from_abort(c, nullptr)) return rc;
        if (x) HIP_TRY(hipMemcpy(x, c->x.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost));
        if (v) HIP_TRY(hipMemcpy(v, c->v.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost));
    }
    c->pending.clear();
    return ADMM_HIP_OK;
}

static int set_pins_impl(admm_hip_ctx *c, int32_t n, const int32_t *vert, const double *xyz);
int admm_hip_set_pins(admm_hip_ctx *c, int32_t n, const int32_t *vert, const double *xyz) {
    if (!c || n < 0 || (n > 0 && (!vert || !xyz))) return fail(ADMM_HIP_ERR_ARG, "set_pins: Bad input (Solver.cpp:118-120)");
    if (!c->cm.on) return set_pins_impl(c, n, vert, xyz);
    std::vector<int32_t> vl; std::vector<double> pl;        // component partition: the pins of this rank's bodies
    for (int i = 0; i < n; ++i) {
        if (vert[i] < 0 || vert[i] >= c->cm.nv_global) return fail(ADMM_HIP_ERR_ARG, "set_pins: index out of range");
        const int32_t l = c->cm.g2l[vert[i]];
        if (l < 0) continue;
        vl.push_back(l); for (int j = 0; j < 3; ++j) pl.push_back(xyz[3 * (size_t)i + j]);
    }
    return set_pins_impl(c, (int32_t)vl.size(), vl.data(), pl.data());
}
static int set_pins_impl(admm_hip_ctx *c, int32_t n, const int32_t *vert, const double *xyz) {
    if (!c || n < 0 || (n > 0 && (!vert || !xyz))) return fail(ADMM_HIP_ERR_ARG, "set_pins: Bad input (Solver.cpp:118-120)");
    HIP_TRY(hipSetDevice(c->device));
    // admm_hip_step without stats returns while its kernels are still in flight on the context's (non-blocking)
    // stream: the pin data must not change under them
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;     // (steps still pending are replayed, if need be, with the OLD pins)
    if (c->linsolver == 1) {
        std::vector<int> flag(c->nv, 0);
        std::vector<double> p((size_t)c->n3, 0.0);
        for (int i = 0; i < n; ++i) {
            if (vert[i] < 0 || vert[i] >= c->nv) return fail(ADMM_HIP_ERR_ARG, "set_pins: index out of range");
            const double *q = c->pin_nrm_h.data() + 3 * (size_t)vert[i];      // (a vertex keeps the slide normal it was given)
            flag[vert[i]] = (c->has_slide && (q[0] != 0.0 || q[1] != 0.0 || q[2] != 0.0)) ? 2 : 1;
            for (int j = 0; j < 3; ++j) p[3 * (size_t)vert[i] + j] = xyz[3 * (size_t)i + j];
        }
        c->gs_has_pins = n > 0;
        if (c->has_slide) {      // a vertex that LEFT the pin set loses its slide normal: pinned again later it is an ordinary pin
            bool any = false;
            for (int v = 0; v < c->nv; ++v) {
                double *q = c->pin_nrm_h.data() + 3 * (size_t)v;
                if (!flag[v]) q[0] = q[1] = q[2] = 0.0;
                any = any || q[0] != 0.0 || q[1] != 0.0 || q[2] != 0.0;
            }
            c->has_slide = any;
            HIP_TRY(hipMemcpy(c->gs_pin_nrm.p, c->pin_nrm_h.data(), c->pin_nrm_h.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (c->gs_exec) { (void)hipGraphExecDestroy(c->gs_exec); c->gs_exec = nullptr; } // pin pointer is baked into the graph
        HIP_TRY(hipMemcpy(c->gs_pin_flag.p, flag.data(), flag.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->gs_pin_xyz.p, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
        return ADMM_HIP_OK;
    }
    // energy-based pins: locations may move, the set may only be (de)activated (Solver.cpp:126-156)
    std::vector<int> act(c->npin_terms, 0);
    std::vector<double> p(3 * (size_t)c->npin_terms);
    if (c->npin_terms) HIP_TRY(hipMemcpy(p.data(), c->pin_xyz.p, p.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::map<int, int> term_of;
    for (int i = 0; i < c->npin_terms; ++i) term_of[c->pin_vert_h[i]] = i;
    for (int i = 0; i < n; ++i) {
        auto it = term_of.find(vert[i]);
        if (it == term_of.end())
            return fail(ADMM_HIP_ERR_ARG, "Solver::set_pins Error: Constraint for " + std::to_string(vert[i]) + " not found.");
        act[it->second] = 1;
        for (int j = 0; j < 3; ++j) p[3 * (size_t)it->second + j] = xyz[3 * (size_t)i + j];
    }
    if (c->npin_terms) {
        HIP_TRY(hipMemcpy(c->pin_active.p, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->pin_xyz.p, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return ADMM_HIP_OK;
}

// Solver::ext_forces.push_back(std::make_shared<WindForce>(tris)) + WindForce::direction (src/ExplicitForce.hpp:39-46)
int admm_hip_set_pin_normals(admm_hip_ctx *c, int32_t n, const int32_t *vert, const double *normals) {
    if (!c || n < 0 || (n > 0 && (!vert || !normals))) return fail(ADMM_HIP_ERR_ARG, "set_pin_normals: bad input");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    std::map<int, int> term_of;
    if (c->linsolver != 1) for (int i = 0; i < c->npin_terms; ++i) term_of[c->pin_vert_h[i]] = i;
    std::vector<int> flag;
    if (c->linsolver == 1) { flag.resize(c->nv); HIP_TRY(hipMemcpy(flag.data(), c->gs_pin_flag.p, flag.size() * sizeof(int), hipMemcpyDeviceToHost)); }
    for (int i = 0; i < n; ++i) {
        int32_t v = vert[i];
        if (c->cm.on) { if (v < 0 || v >= c->cm.nv_global) return fail(ADMM_HIP_ERR_ARG, "set_pin_normals: index out of range"); v = c->cm.g2l[v]; if (v < 0) continue; }
        if (v < 0 || v >= c->nv) return fail(ADMM_HIP_ERR_ARG, "set_pin_normals: index out of range");
        const double *q = normals + 3 * (size_t)i;
        const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        if (!std::isfinite(l)) return fail(ADMM_HIP_ERR_ARG, "set_pin_normals: non-finite normal");
        size_t slot;
        if (c->linsolver == 1) {
            if (!flag[v]) return fail(ADMM_HIP_ERR_ARG, "Solver::set_pins Error: Constraint for " + std::to_string(vert[i]) + " not found.");
            slot = (size_t)v; flag[v] = l > 0.0 ? 2 : 1;
        } else {
            auto it = term_of.find(v);
            if (it == term_of.end()) return fail(ADMM_HIP_ERR_ARG, "Solver::set_pins Error: Constraint for " + std::to_string(vert[i]) + " not found.");
            slot = (size_t)it->second;
        }
        for (int j = 0; j < 3; ++j) c->pin_nrm_h[3 * slot + j] = l > 0.0 ? q[j] / l : 0.0;
    }
    c->has_slide = false;
    for (double x : c->pin_nrm_h) if (x != 0.0) { c->has_slide = true; break; }
    if (c->linsolver == 1) {
        if (c->gs_exec) { (void)hipGraphExecDestroy(c->gs_exec); c->gs_exec = nullptr; }
        HIP_TRY(hipMemcpy(c->gs_pin_flag.p, flag.data(), flag.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->gs_pin_nrm.p, c->pin_nrm_h.data(), c->pin_nrm_h.size() * sizeof(double), hipMemcpyHostToDevice));
    } else if (c->npin_terms)
        HIP_TRY(hipMemcpy(c->pin_nrm.p, c->pin_nrm_h.data(), c->pin_nrm_h.size() * sizeof(double), hipMemcpyHostToDevice));
    return ADMM_HIP_OK;
}

static int set_wind_impl(admm_hip_ctx *c, int32_t n_tris, const int32_t *tris, const double *direction);
int admm_hip_set_wind(admm_hip_ctx *c, int32_t n_tris, const int32_t *tris, const double *direction) {
    if (!c || n_tris < 0 || (n_tris > 0 && (!tris || !direction))) return fail(ADMM_HIP_ERR_ARG, "set_wind: bad input");
    if (!c->cm.on) return set_wind_impl(c, n_tris, tris, direction);
    std::vector<int32_t> tl;                                  // component partition: the triangles of this rank's bodies
    for (int64_t t = 0; t < n_tris; ++t) {
        int32_t l[3];
        for (int k = 0; k < 3; ++k) {
            const int32_t g = tris[3 * t + k];
            if (g < 0 || g >= c->cm.nv_global) return fail(ADMM_HIP_ERR_ARG, "set_wind: triangle index out of range");
            l[k] = c->cm.g2l[g];
        }
        if (l[0] >= 0 && l[1] >= 0 && l[2] >= 0) for (int k = 0; k < 3; ++k) tl.push_back(l[k]);
    }
    return set_wind_impl(c, (int32_t)(tl.size() / 3), tl.data(), direction);
}
static int set_wind_impl(admm_hip_ctx *c, int32_t n_tris, const int32_t *tris, const double *direction) {
    if (!c || n_tris < 0 || (n_tris > 0 && (!tris || !direction))) return fail(ADMM_HIP_ERR_ARG, "set_wind: bad input");
    for (int64_t i = 0; i < (int64_t)3 * n_tris; ++i)
        if (tris[i] < 0 || tris[i] >= c->nv) return fail(ADMM_HIP_ERR_ARG, "set_wind: triangle index out of range");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    c->wind_n = n_tris;
    if (n_tris == 0) { c->wind_tris.release(); c->wind_inc = SellDev(); c->wind_force.release(); return ADMM_HIP_OK; }
    for (int j = 0; j < 3; ++j) c->wind_dir[j] = direction[j];
    HIP_TRY(c->wind_tris.upload(std::vector<int>(tris, tris + 3 * (size_t)n_tris)));
    HIP_TRY(c->wind_inc.upload(admm_host::incidence_sell(c->nv, n_tris, 3, tris, n_tris * 4)));
    HIP_TRY(c->wind_force.alloc(3 * ((size_t)n_tris + 1))); HIP_TRY(c->wind_force.zero());
    return ADMM_HIP_OK;
}

// Solver::surface_inds (src/Solver.hpp:70): the vertices Collider::detect looks at (Collider.hpp:157,163)
static int set_surface_inds_impl(admm_hip_ctx *c, int32_t n, const int32_t *inds);
int admm_hip_set_surface_inds(admm_hip_ctx *c, int32_t n, const int32_t *inds) {
    if (!c || n < 0 || (n > 0 && !inds)) return fail(ADMM_HIP_ERR_ARG, "set_surface_inds: bad input");
    if (!c->cm.on) return set_surface_inds_impl(c, n, inds);
    std::vector<int32_t> il;
    for (int i = 0; i < n; ++i) {
        if (inds[i] < 0 || inds[i] >= c->cm.nv_global) return fail(ADMM_HIP_ERR_ARG, "set_surface_inds: index out of range");
        if (c->cm.g2l[inds[i]] >= 0) il.push_back(c->cm.g2l[inds[i]]);
    }
    if (n > 0 && il.empty()) {     // a list none of whose vertices is ours must not turn into "every vertex": an all-zero candidate mask
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = settle(c)) return rc;
        c->n_surf = 1;             // (the list itself only serves the dynamic queries, which a component-partitioned context does not run)
        HIP_TRY(c->surf_list.upload(std::vector<int>(1, 0)));
        HIP_TRY(c->surf_mask.upload(std::vector<unsigned char>(c->nv, 0)));
        return ADMM_HIP_OK;
    }
    return set_surface_inds_impl(c, (int32_t)il.size(), il.data());
}
static int set_surface_inds_impl(admm_hip_ctx *c, int32_t n, const int32_t *inds) {
    if (!c || n < 0 || (n > 0 && !inds)) return fail(ADMM_HIP_ERR_ARG, "set_surface_inds: bad input");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));   // a step may still be in flight (see admm_hip_set_pins)
    if (int rc = settle(c)) return rc;          // (steps that hit a barrier time-out are replayed with the OLD surface list)
    std::vector<int> list;
    std::vector<unsigned char> mask(c->nv, 0);
    for (int i = 0; i < n; ++i) {
        if (inds[i] < 0 || inds[i] >= c->nv) return fail(ADMM_HIP_ERR_ARG, "set_surface_inds: index out of range");
        if (!mask[inds[i]]) list.push_back(inds[i]);   // a vertex is a candidate once
        mask[inds[i]] = 1;
    }
    n = (int32_t)list.size();
    c->surf_list.release(); c->surf_mask.release();
    c->n_surf = n;
    if (n > 0) { HIP_TRY(c->surf_list.upload(list)); HIP_TRY(c->surf_mask.upload(mask)); }
    return ADMM_HIP_OK;
}

// Solver::add_dynamic_collider(TetMeshCollision(mesh, v_offset)) -- src/Solver.cpp:163-165, src/DynamicObject.hpp:45-64
int admm_hip_add_dynamic_tetmesh(admm_hip_ctx *c, int32_t vert_offset, int32_t n_verts, const double *rest_verts,
                                 int32_t n_tets, const int32_t *tets, int32_t n_faces, const int32_t *faces) {
    if (c && c->linsolver == 1 && c->has_slide) return fail(ADMM_HIP_ERR_ARG, "add_dynamic_tetmesh: slide pins inside the sweeps of the dynamic-hit GS path are not supported (use linsolver 2)");
    if (c && c->cm.on) return fail(ADMM_HIP_ERR_STATE, "add_dynamic_tetmesh: dynamic colliders couple the bodies -- create the rank contexts with ADMM_HIP_PARTITION=elements");
    if (!c || !rest_verts || !tets || n_verts <= 0 || n_tets <= 0 || vert_offset < 0 || vert_offset + n_verts > c->nv)
        return fail(ADMM_HIP_ERR_ARG, "add_dynamic_tetmesh: bad input");
    if (n_faces <= 0 || !faces) return fail(ADMM_HIP_ERR_ARG, "**TetMeshCollision Error: TetMesh needs surface faces");
    if (c->linsolver == 0) return fail(ADMM_HIP_ERR_ARG, "**Solver::add_obstacle Error: No collisions with LDLT solver");
    for (int i = 0; i < 4 * n_tets; ++i) if (tets[i] < 0 || tets[i] >= n_verts) return fail(ADMM_HIP_ERR_ARG, "add_dynamic_tetmesh: tet index out of range");
    for (int i = 0; i < 3 * n_faces; ++i) if (faces[i] < 0 || faces[i] >= n_verts) return fail(ADMM_HIP_ERR_ARG, "add_dynamic_tetmesh: face index out of range");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));   // a step may still be in flight (see admm_hip_set_pins)
    if (int rc = settle(c)) return rc;          // (pending steps are replayed, if need be, without the new collider)
    auto fill_levels = [](const admm_host::OctTree &T, OctLevels &L) {
        L.n_levels = T.n_levels;
        for (int l = 0; l < T.n_levels; ++l) { L.off[l] = T.level_off[l]; L.n[l] = T.level_n[l]; }
        L.off[T.n_levels] = T.level_off[T.n_levels];
    };
    std::vector<double> cen(3 * (size_t)n_tets);
    for (int t = 0; t < n_tets; ++t)
        for (int a = 0; a < 3; ++a) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += rest_verts[3 * (size_t)tets[4 * (size_t)t + k] + a];
            cen[3 * (size_t)t + a] = 0.25 * s;
        }
    const admm_host::OctTree TT = admm_host::build_octtree(n_tets, cen.data());
    cen.assign(3 * (size_t)n_faces, 0.0);
    for (int f = 0; f < n_faces; ++f)
        for (int a = 0; a < 3; ++a) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += rest_verts[3 * (size_t)faces[3 * (size_t)f + k] + a];
            cen[3 * (size_t)f + a] = s / 3.0;
        }
    const admm_host::OctTree FT = admm_host::build_octtree(n_faces, cen.data());
    if (TT.n_levels > kOctMaxLevels || FT.n_levels > kOctMaxLevels) return fail(ADMM_HIP_ERR_ARG, "add_dynamic_tetmesh: mesh too large");
    std::vector<int4> tet_s(TT.n_padded, make_int4(-1, -1, -1, -1));
    std::vector<int> tet_id(TT.n_padded, -1), face_s(3 * (size_t)FT.n_padded, -1), face_id(FT.n_padded, -1);
    for (int i = 0; i < TT.n_padded; ++i) {
        const int t = TT.order[i];
        if (t < 0) continue;
        tet_s[i] = make_int4(tets[4 * (size_t)t] + vert_offset, tets[4 * (size_t)t + 1] + vert_offset, tets[4 * (size_t)t + 2] + vert_offset,
                             tets[4 * (size_t)t + 3] + vert_offset);
        tet_id[i] = t;
    }
    for (int i = 0; i < FT.n_padded; ++i) {
        const int f = FT.order[i];
        if (f < 0) continue;
        for (int k = 0; k < 3; ++k) face_s[3 * (size_t)i + k] = faces[3 * (size_t)f + k];
        face_id[i] = f;
    }
    const std::vector<double> fbox = admm_host::octtree_boxes_tris(FT, faces, rest_verts);
    std::unique_ptr<admm_hip_ctx::DynDev> d(new admm_hip_ctx::DynDev());
    HIP_TRY(d->tet.upload(tet_s)); HIP_TRY(d->tet_id.upload(tet_id)); HIP_TRY(d->face.upload(face_s)); HIP_TRY(d->face_id.upload(face_id));
    HIP_TRY(d->f_box.upload(fbox));
    HIP_TRY(d->t_box.alloc(6 * (size_t)TT.level_off[TT.n_levels]));
    HIP_TRY(d->rest.upload(std::vector<double>(rest_verts, rest_verts + 3 * (size_t)n_verts)));
    d->m.vert_offset = vert_offset; d->m.n_verts = n_verts;
    fill_levels(TT, d->m.tt); fill_levels(FT, d->m.ft);
    d->m.tet = d->tet.p; d->m.tet_id = d->tet_id.p; d->m.t_box = d->t_box.p;
    d->m.face = d->face.p; d->m.face_id = d->face_id.p; d->m.f_box = d->f_box.p; d->m.rest = d->rest.p;
    if (c->linsolver == 1 && !c->gsd_skip.p) {
        HIP_TRY(c->gsd_hits.alloc((size_t)c->nv)); HIP_TRY(c->gsd_skip.alloc((size_t)c->nv)); HIP_TRY(c->gsd_skip.zero());
        HIP_TRY(c->gsd_part.alloc(2 * ((size_t)c->NB + 1))); HIP_TRY(c->gsd_part.zero());
    }
    if (!c->dyn_face.p) {
        HIP_TRY(c->dyn_face.alloc(3 * (size_t)c->nv)); HIP_TRY(c->dyn_bary.alloc(c->n3)); HIP_TRY(c->dyn_n.alloc(c->n3));
        HIP_TRY(c->dyn_dx.alloc(c->nv));
        HIP_TRY(c->dyn_bary.zero()); HIP_TRY(c->dyn_n.zero()); HIP_TRY(c->dyn_dx.zero());
    }
    c->dyn.push_back(std::move(d));
    return ADMM_HIP_OK;
}

// Collider::detect for the dynamic objects at x (host vector) -- kernel-level entry point for the parity tests.
// Hits come back in candidate order (surface_inds order, else vertex order).
int admm_hip_detect_dynamic(admm_hip_ctx *c, const double *x, int32_t cap, int32_t *n_hits, int32_t *vert, int32_t *face,
                            double *barys, double *normal, double *dx) {
    if (!c || !x || !n_hits || cap < 0) return fail(ADMM_HIP_ERR_ARG, "detect_dynamic: bad input");
    *n_hits = 0;
    if (c->dyn.empty()) return ADMM_HIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> xd;
    HIP_TRY(xd.alloc(c->n3));
    HIP_TRY(hipMemcpyAsync(xd.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (enqueue_dyn_detect(c, xd.p)) return fail(ADMM_HIP_ERR_DEVICE, "detect_dynamic: launch failed");
    std::vector<int> hf(3 * (size_t)c->nv), list;
    std::vector<double> hb(c->n3), hn(c->n3), hd(c->nv);
    HIP_TRY(hipMemcpyAsync(hf.data(), c->dyn_face.p, hf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hb.data(), c->dyn_bary.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hn.data(), c->dyn_n.p, hn.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hd.data(), c->dyn_dx.p, hd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->n_surf > 0) { list.resize(c->n_surf); HIP_TRY(hipMemcpy(list.data(), c->surf_list.p, list.size() * sizeof(int), hipMemcpyDeviceToHost)); }
    const int nq = c->n_surf > 0 ? c->n_surf : c->nv;
    int n = 0;
    for (int q = 0; q < nq; ++q) {
        const int v = c->n_surf > 0 ? list[q] : q;
        if (hf[3 * (size_t)v] < 0) continue;
        if (n < cap) {
            if (vert) vert[n] = v;
            if (dx) dx[n] = hd[v];
            for (int a = 0; a < 3; ++a) {
                if (face) face[3 * (size_t)n + a] = hf[3 * (size_t)v + a];
                if (barys) barys[3 * (size_t)n + a] = hb[3 * (size_t)v + a];
                if (normal) normal[3 * (size_t)n + a] = hn[3 * (size_t)v + a];
            }
        }
        ++n;
    }
    *n_hits = n;
    return ADMM_HIP_OK;
}

static int launch_global(admm_hip_ctx *c, const double *b, double *x, bool loop = true) {      // loop = false: admm_hip_global_solve (k_pcg2: the generic instance)
    if (c->linsolver == 1) {
        if (!c->dyn.empty()) return launch_gs_dynamic(c, b, x);
        launch_gs(c, b, x); return 0;
    }
    if (c->linsolver == 2) {
        int it = 1;
        const int rc = launch_uzawa(c, b, x, &it, loop);
        c->uz_iters_step += it;
        return rc;
    }
    return launch_pcg_recycled(c, b, x, loop);
}

// true: launch_global(c, c->b.p, c->curr.p) will reach launch_pcg2 with the recycled basis as the FIRST thing that reads b
constexpr int kStepAborted = -100;   // step_impl: a grid barrier of the on-chip PCG timed out (seen at the final synchronisation)
static int step_impl(admm_hip_ctx *c, int32_t admm_iters, double gravity, admm_hip_stats *stats) {
    hipStream_t st = c->stream;
    const bool timed = stats != nullptr;
    if (timed) {
        while ((int)c->ev_phase.size() < 3 * admm_iters + 1) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c->ev_phase.push_back(e);
        }
    }
    c->timing = timed; c->coll_ms_step = 0.0; c->lk_launch = 0;
    // opt-in (ADMM_HIP_KERNEL_CLOCK=1): the stamps themselves cost the local-step launch ~1.4 us (2 %)
    if (timed && c->nt > 0 && c->kernel_clock) {
        const int tsn = 4 * (blocks_for(c->nt) + 4), cap = 2 * admm_iters;
        if (c->lk_tsn != tsn || c->lk_cap < cap) {
            HIP_TRY(c->lk_ts.alloc((size_t)cap * 2 * tsn)); HIP_TRY(c->lk_out.alloc(2 * (size_t)cap));
            c->lk_tsn = tsn; c->lk_cap = cap;
            int khz = 0;
            HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
            c->lk_tick_ms = khz > 0 ? 1.0 / (double)khz : 1e-5;     // wall_clock64 ticks: 100 MHz on gfx950
        }
        HIP_TRY(hipMemsetAsync(c->lk_ts.p, 0, (size_t)cap * 2 * tsn * sizeof(unsigned long long), st));
    }
    if (timed && !c->ev_coll0) { HIP_TRY(hipEventCreate(&c->ev_coll0)); HIP_TRY(hipEventCreate(&c->ev_coll1)); }
    HIP_TRY(hipEventRecord(c->ev_step0, st));
    c->uz_iters_step = 0; c->uz_detected = false;
    struct InStep { admm_hip_ctx *c; ~InStep() { c->in_step = false; } } in_step_guard{c};
    c->in_step = true;
    c->xbar_of_state = false;     // (newton_polish: true again where this step commits its state, below)
    // monitor (admm_hip_set_monitor): one record per ADMM iteration, written on the stream -- nothing here waits for the device
    // early exit (admm_hip_set_admm_stop): the step runs with the monitor (mode max(mode, 1)), k_mon_decide takes the place of k_mon_final,
    // and the iterations behind the stop are either never launched (the host decides: one event synchronisation per iteration) or launched
    // as no-ops (c->stop_dev: every kernel of the loop reads the stop word first)
    const bool stopping = c->stop_tol > 0.0 && admm_iters > 0 && monitor_allowed(c);
    const bool stop_on_dev = stopping && stop_device_ok(c);
    struct StopDev { admm_hip_ctx *c; ~StopDev() { c->stop_dev = nullptr; } } stop_dev_guard{c};
    c->stop_dev = stop_on_dev ? c->counters.p + kCntAdmmStop : nullptr;
    c->stop_last = admm_iters; c->stop_on_dev = 0;
    const int seq0 = c->solve_seq;
    const long long oc_launches0 = c->oc_launches, gsp_launches0 = c->gsp_launches;
    if (stopping) {
        if (!c->ev_stop) HIP_TRY(hipEventCreateWithFlags(&c->ev_stop, hipEventDisableTiming));
        c->h_sig[kSigAdmmStop] = 0; c->h_sig[kSigAdmmIters] = 0;      // (no kernel of an earlier step is still running: see the synchronisation below)
    }
    const bool mon = (c->mon_mode != 0 || stopping) && monitor_allowed(c);
    c->mon_n = 0;
    if (mon) {
        HIP_TRY(mon_ensure(c, true, false));
        if (c->mon_rec.n < (size_t)kMonQ * std::max(1, admm_iters)) HIP_TRY(c->mon_rec.alloc((size_t)kMonQ * std::max(1, admm_iters)));
        launch_monitor_init(c, c->x.p);
        c->mon_n = admm_iters;
    }
    // Anderson acceleration (admm_hip_set_anderson): three more launches behind every global solve, the decisions on the device
    struct AaOn { admm_hip_ctx *c; ~AaOn() { c->aa_on = false; } } aa_on_guard{c};
    c->aa_on = c->aa_window > 0 && admm_iters > 0;
    c->aa_n = 0;
    if (c->aa_on) { HIP_TRY(aa_ensure(c, admm_iters)); c->aa_n = admm_iters; }
    const bool stat = mon && c->mon_mode == 3;      // (mode 3: mode 2 plus the stationarity residual, forces.hpp)
    c->mon_stat_n = 0;
    if (stat) {
        HIP_TRY(force_ensure(c, false, std::max(1, admm_iters)));
        HIP_TRY(hipMemsetAsync(c->f_stat.p, 0, c->f_stat.n * sizeof(double), st));
        c->mon_stat_n = admm_iters;
    }
    c->rc_prev2_valid = c->rc_prev_valid; c->rc_prev_valid = c->rc_iter; c->rc_frame += 1; c->rc_iter = 0;   // this frame's pairs become "previous frame"
    // How many pairs a projection uses is decided ONCE per context, from the scene's own behaviour: four pairs cost ~4 us per solve
    // more than three (8.8 MB of reads, 20 block sums) and pay when solves need many iterations (Kuhn cube: 17.4 -> 13.9 per solve),
    // not when they need few (unstructured body at 1e-8: 4.25 vs 4.35).  Decided from measurement, then fixed: deterministic.
    // Round 4 (tighter bench tolerance, 13 instead of 4 iterations per solve on the body): which count needs fewer iterations is
    // not monotone in the iteration count (body: 12.8 with three pairs, 13.9 with four; cube: the other way round), so BOTH are
    // measured -- frame 3 with four pairs, frame 4 with three -- and the fifth frame starts with the better one (three on a tie within
    // 2 %: they are cheaper).  Three stream synchronisations in the life of a context.
    if (!c->rc_decided && c->linsolver != 1 && c->oc_enabled && c->oc_plan && c->rc_frame >= 3 && c->rc_frame <= 5) {
        int its = 0;
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(&its, c->counters.p + kCntTotalIters, sizeof(its), hipMemcpyDeviceToHost));
        if (c->rc_frame == 3) { c->rc_snap[0] = its; c->rc_pairs = kRc; }
        else if (c->rc_frame == 4) { c->rc_snap[1] = its; c->rc_pairs = 3; }
        else {
            const long long its4 = c->rc_snap[1] - c->rc_snap[0], its3 = its - c->rc_snap[1];
            c->rc_pairs = (its4 > 0 && (double)its3 > 1.02 * (double)its4) ? kRc : 3;
            c->rc_decided = true;
        }
    }
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, kCntStepWords * sizeof(int), st));
    if (c->linsolver == 2) HIP_TRY(hipMemsetAsync(c->counters.p + kCntSchurIters, 0, sizeof(int), st));
    if (stopping) HIP_TRY(hipMemsetAsync(c->counters.p + kCntAdmmStop, 0, 2 * sizeof(int), st));      // (kCntAdmmStop, kCntAdmmIters)
    if (c->wind_n > 0) {   // ExplicitForce::project of the wind, Solver.cpp:54 (before gravity and the prediction)
        hipLaunchKernelGGL(k_wind_tris, dim3(blocks_for(c->wind_n)), dim3(256), 0, st, c->wind_n, c->wind_tris.p, c->x.p, c->v.p,
                           c->wind_dir[0], c->wind_dir[1], c->wind_dir[2], c->dt, c->wind_force.p);
        hipLaunchKernelGGL(k_wind_nodes, dim3((c->wind_inc.n_slices + 3) / 4), dim3(256), 0, st, c->nv, c->wind_n, c->wind_inc.ptr.p,
                           c->wind_inc.w.p, c->wind_inc.idx.p, c->wind_force.p, c->v.p);
    }
    hipLaunchKernelGGL(k_predict, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, c->dt, gravity, c->x.p, c->v.p, c->m.p,
                       c->Mxbar.p, c->curr.p);
    // curr_u = 0 (Solver.cpp:71); curr_z = D x is a dead store in the reference (:70)
    if (c->nt) HIP_TRY(hipMemsetAsync(c->t_u.p, 0, c->t_u.n * sizeof(double), st));
    if (c->ntri) HIP_TRY(hipMemsetAsync(c->r_u.p, 0, c->r_u.n * sizeof(double), st));
    if (c->nbend) HIP_TRY(hipMemsetAsync(c->h_u.p, 0, c->h_u.n * sizeof(double), st));
    if (c->npin_terms) HIP_TRY(hipMemsetAsync(c->pin_u.p, 0, c->pin_u.n * sizeof(double), st));
    if (c->aa_on) launch_aa_init(c);      // s_0 = (x_bar, 0), the ring empty: nothing carries over from the step before
    int n_launched = 0;      // iterations enqueued (all of them, unless the host has seen the stop)
    for (int s = 0; s < admm_iters; ++s) {
        if (timed) HIP_TRY(hipEventRecord(c->ev_phase[3 * s], st));
        n_launched = s + 1;
        const bool lt = !timed && c->lt_on;
        if (lt) {
            while (c->lt_ev.size() < c->lt_used + 2) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); c->lt_ev.push_back(e); }
            if (c->lt_mode == 2) { c->lt_k0 = c->lt_ev[c->lt_used]; c->lt_k1 = c->lt_ev[c->lt_used + 1]; c->lt_taken = false; }
            else HIP_TRY(hipEventRecord(c->lt_ev[c->lt_used], st));
        }
        if (mon) launch_local<true>(c);         // (the monitor reads z: the WRITE_Z instantiations of admm_hip_local_step)
        else launch_local<false>(c);            // Solver.cpp:84-87
        if (lt) {
            if (c->lt_mode == 2) { c->lt_k0 = nullptr; c->lt_k1 = nullptr; }
            else HIP_TRY(hipEventRecord(c->lt_ev[c->lt_used + 1], st));
            if (c->lt_mode != 2 || c->lt_taken) c->lt_used += 2;      // (mode 2: a pair no kernel took was never recorded)
        }
        if (timed) HIP_TRY(hipEventRecord(c->ev_phase[3 * s + 1], st));
        // passive collisions are resolved inside the GS sweeps (linsolver 1, Solver.cpp:76)
        if (int rr = launch_rhs(c))             // Solver.cpp:98
            return fail(rr == -2 ? ADMM_HIP_ERR_STATE : ADMM_HIP_ERR_COMM, rr == -2 ? "step: world_size > 1 but neither admm_hip_comm_init nor admm_hip_set_rhs_allreduce was called" : "all-reduce of the right-hand side failed");
        if (timed) HIP_TRY(hipEventRecord(c->ev_phase[3 * s + 2], st));
        const int grc = launch_global(c, c->b.p, c->curr.p);   // Solver.cpp:99
        if (grc == -2) return kStepAborted;       // a grid barrier timed out in a column solve of UzawaCG: same recovery as any aborted on-chip solve
        if (grc) return fail(ADMM_HIP_ERR_DEVICE, "PCG: the device stopped signalling progress");
        if (stat) launch_stationarity(c, s);
        if (c->aa_on) launch_aa_record(c, s);             // F_k, the safeguard, theta: before the monitor's decision, which a rejection vetoes
        if (mon) launch_monitor_step(c, s, stopping);     // x = x^{s+1}, z = z^{s+1}, z_prev = z^s
        if (stopping && !stop_on_dev) {      // the host decides: wait for the decision, read its pinned copy
            HIP_TRY(hipEventRecord(c->ev_stop, st));
            HIP_TRY(hipEventSynchronize(c->ev_stop));
            if (c->h_sig[kSigAbort]) break;      // (a persistent launch gave up: seen again below)
            if (((volatile int *)c->h_sig)[kSigAdmmStop]) break;
        }
        if (c->aa_on) launch_aa_apply(c, s + 1 == admm_iters);      // s_{k+1} (behind the stop: a no-op, the step's x is the solve's output)
    }
    c->timing = false;
    if (timed) HIP_TRY(hipEventRecord(c->ev_phase[3 * n_launched], st));
    if (timed && c->lk_launch > 0)
        hipLaunchKernelGGL(k_ts_reduce, dim3(c->lk_launch), dim3(256), 0, st, c->lk_ts.p, c->lk_tsn, c->lk_launch, c->lk_out.p);
    hipLaunchKernelGGL(k_finish, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, 1.0 / c->dt, c->x.p, c->v.p, c->curr.p);
    c->xbar_of_state = true;      // x is this step's result and Mxbar its x_bar (newton_polish)
    HIP_TRY(hipEventRecord(c->ev_step1, st));
    HIP_TRY(hipGetLastError());
    int n_exec = admm_iters;      // iterations executed
    if (stopping) {
        // ONE synchronisation ends a step with early exit: the host learns the executed count, and everything that counts the solves of a
        // frame on the host is set from it -- not from the number of launches
        HIP_TRY(hipStreamSynchronize(st));
        if (c->h_sig[kSigAbort]) return kStepAborted;      // (the replay decides again for itself)
        n_exec = std::min(n_launched, std::max(1, (int)((volatile int *)c->h_sig)[kSigAdmmIters]));
        c->stop_last = n_exec; c->stop_on_dev = stop_on_dev ? 1 : 0;
        c->mon_n = n_exec;
        if (c->aa_on) c->aa_n = n_exec;
        if (c->rc_iter > n_exec) c->rc_iter = n_exec;      // the pairs this frame really wrote: next frame's rc_prev_valid, then rc_prev2_valid
        if (stop_on_dev) {      // every skipped iteration took one solve number (and, k_pcg2, one place in the verification sample): give them back
            const int skipped = n_launched - n_exec;
            c->solve_seq = seq0 + n_exec;
            if (c->linsolver != 1) {      // (admm_hip_persistent_launches, admm_hip_pcg_instances: solves, not no-op launches)
                c->oc_launches = oc_launches0 + n_exec;
                c->oc_instance_launches[c->oc_last_instance == 2 ? 0 : 1] -= skipped;
            } else c->gsp_launches = gsp_launches0 + n_exec;
            if (c->linsolver == 2) c->uz_iters_step -= skipped;      // (one per launched iteration on this path: stats->inner_iters counts executed ones)
        }
    }
    if (timed) {
        HIP_TRY(hipEventSynchronize(c->ev_step1));
        if (c->h_sig && c->h_sig[kSigAbort]) return kStepAborted;
        std::memset(stats, 0, sizeof(*stats));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_step0, c->ev_step1));
        stats->step_ms = ms;
        for (int s = 0; s < n_exec; ++s) {      // (executed iterations only; a skipped one costs its empty launches, inside step_ms)
            // local_ms = the prox kernels (the reference's local loop); global_ms = RHS + solve, as in Solver.cpp:97-100
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_phase[3 * s], c->ev_phase[3 * s + 1])); stats->local_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_phase[3 * s + 1], c->ev_phase[3 * s + 2])); stats->rhs_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_phase[3 * s + 1], c->ev_phase[3 * s + 3])); stats->global_ms += ms;
        }
        if (c->lk_launch > 0) {
            std::vector<unsigned long long> tt(2 * (size_t)c->lk_launch);
            HIP_TRY(hipMemcpy(tt.data(), c->lk_out.p, tt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int i = 0; i < c->lk_launch; ++i)
                if (tt[2 * i + 1] > tt[2 * i]) stats->local_kernel_ms += (double)(tt[2 * i + 1] - tt[2 * i]) * c->lk_tick_ms;
        }
        // collision_ms = Collider::detect + constraint rows (Solver.cpp:90-95); it runs inside the global phase here
        stats->collision_ms = c->coll_ms_step;
        stats->global_ms = std::max(0.0, stats->global_ms - c->coll_ms_step);
        int h[kCntRing];
        HIP_TRY(hipMemcpy(h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost));
        CgScal sc[2];
        HIP_TRY(hipMemcpy(sc, c->cg_scal.p, sizeof(sc), hipMemcpyDeviceToHost));
        stats->admm_iters = n_exec;
        if (c->linsolver == 1) { stats->inner_iters = h[kCntIters]; stats->last_solve_converged = h[kCntGsDone] != 0; }   // (the done word carries the stamp of the launch that raised it)
        else if (c->linsolver == 2) {
            stats->inner_iters = c->uz_iters_step + h[kCntSchurIters]; // the reference counts Schur-CG iterations (UzawaCG.hpp:124)
            stats->n_constraints = c->uz_last_hits;
            stats->last_solve_converged = sc[c->last_launched_iters & 1].converged;
            stats->pcg_launched_iters = c->last_launched_iters;
        }
        else {
            stats->inner_iters = h[kCntIters];
            stats->last_solve_converged = sc[c->last_launched_iters & 1].converged;
            stats->unconverged_solves = n_exec - h[kCntConverged];
            {   // iterations of the last (up to 64) solves of this step, oldest first
                int ring[kCntRingLen];
                HIP_TRY(hipMemcpy(ring, c->counters.p + kCntRing, sizeof(ring), hipMemcpyDeviceToHost));
                const int n = std::min(n_exec, kCntRingLen);
                for (int i = 0; i < n; ++i) stats->pcg_iters_per_solve[i] = ring[(c->solve_seq - n + 1 + i) & kCntRingMask];
            }
            stats->pcg_launched_iters = c->last_launched_iters;
        }
    }
    return ADMM_HIP_OK;
}

// The state a replay starts from: positions, velocities and -- UzawaCG -- the multipliers with the row count they belong to (an aborted
// Schur launch leaves them half-updated; a replay that started from those would run its <= 20 Schur iterations from a different point
// than the undisturbed run: 2.6e-6 instead of < 1e-7 in test_persistent_schur_hand_off_timeout_recovers, depending on how far the other
// blocks got before they saw the abort).
static hipError_t backup_state(admm_hip_ctx *c) {
    hipError_t e;
    if (!c->bk_x.p) { if ((e = c->bk_x.alloc(c->n3)) != hipSuccess) return e; if ((e = c->bk_v.alloc(c->n3)) != hipSuccess) return e; }
    if ((e = hipMemcpyAsync(c->bk_x.p, c->x.p, c->n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(c->bk_v.p, c->v.p, c->n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream)) != hipSuccess) return e;
    if (c->linsolver == 2 && c->uz_y.p) {
        if (!c->bk_y.p && (e = c->bk_y.alloc(c->uz_y.n)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(c->bk_y.p, c->uz_y.p, c->uz_y.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream)) != hipSuccess) return e;
        c->bk_prev_hits = c->uz_prev_hits; c->bk_prev_iters = c->uz_prev_iters;
    }
    return hipSuccess;
}
// A timed-out grid barrier was seen after a stream synchronisation: give up the persistent kernel, go back to the last
// good state and replay.  Single-GPU contexts only (a replay on one rank would issue all-reduces the others do not).
static int recover_from_abort(admm_hip_ctx *c, admm_hip_stats *stats_of_last) {
    c->h_sig[kSigAbort] = 0;
    if (c->world > 1 || c->comm || c->ar_fn)     // a replay on one rank would issue all-reduces the other ranks do not: the step is lost, cleanly
        return fail(ADMM_HIP_ERR_COMM, "PCG: a grid barrier of the on-chip solve timed out on a rank of a multi-GPU job; the step cannot be replayed under a "
                                       "communicator -- restore the state on every rank (admm_hip_set_state) and continue");
    if (c->pending.empty() || !c->bk_x.p)
        return fail(ADMM_HIP_ERR_DEVICE, "PCG: a grid barrier of the on-chip solve timed out (is another persistent kernel sharing the GPU?)");
    if (!c->oc_gave_up) fprintf(stderr, "[admm_hip] on-chip PCG: a grid barrier timed out (blocks not co-resident?) -- falling back to the launch-per-iteration PCG and replaying %d step(s)\n", (int)c->pending.size());
    c->oc_gave_up = true; c->oc_enabled = false; c->gsp_enabled = false; c->uzp_enabled = false;
    c->rc_hist = 0; c->rc_prev_valid = 0; c->rc_prev2_valid = 0;   // the history slots may hold pairs half-written by the aborted solve, in the on-chip kernel's row order
    c->defl_fused = false;      // (the end projection on the soft modes goes on as separate launches)
    if (c->gsp_abort.p) HIP_TRY(c->gsp_abort.zero());
    if (c->uzp_abort.p) HIP_TRY(c->uzp_abort.zero());
    c->rc_iter = 0;      // (the stored pairs are in the on-chip kernel's internal row order: the launch path must not project on them)
    if (c->oc_bar.p) HIP_TRY(c->oc_bar.zero());
    HIP_TRY(hipMemcpyAsync(c->x.p, c->bk_x.p, c->n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->v.p, c->bk_v.p, c->n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (c->bk_y.p && c->uz_y.p) {
        HIP_TRY(hipMemcpyAsync(c->uz_y.p, c->bk_y.p, c->uz_y.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        c->uz_prev_hits = c->bk_prev_hits; c->uz_prev_iters = c->bk_prev_iters;
    }
    const std::vector<std::pair<int, double> > todo(c->pending);
    c->pending.clear();
    for (size_t i = 0; i < todo.size(); ++i) {
        const int rc = step_impl(c, todo[i].first, todo[i].second, i + 1 == todo.size() ? stats_of_last : nullptr);
        if (rc) return rc == kStepAborted ? fail(ADMM_HIP_ERR_DEVICE, "PCG: barrier time-out during the replay") : rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ADMM_HIP_OK;
}
// after a stream synchronisation: everything issued so far is known to be good, or is replayed
static int settle(admm_hip_ctx *c) {
    if (c->h_sig && c->h_sig[kSigAbort]) return recover_from_abort(c, nullptr);
    c->pending.clear();
    return ADMM_HIP_OK;
}

int admm_hip_step(admm_hip_ctx *c, int32_t admm_iters, double gravity, admm_hip_stats *stats) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "step: NULL context");
    if (!c->state_set) return fail(ADMM_HIP_ERR_STATE, "step: call admm_hip_set_state first");
    if (admm_iters < 0) return fail(ADMM_HIP_ERR_ARG, "step: admm_iters < 0");
    HIP_TRY(hipSetDevice(c->device));
    if (((c->oc_enabled && c->linsolver != 1) || (c->gsp_enabled && c->linsolver == 1) || (c->uzp_enabled && c->linsolver == 2 && c->uzc_on)) && c->world == 1 && !c->comm && !c->ar_fn) {
        if (c->pending.empty()) HIP_TRY(backup_state(c));   // the state every later replay starts from
        if (c->pending.size() >= 4096) {   // a long chain of unsynchronised steps: settle it
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (int rc = settle(c)) return rc;
            HIP_TRY(backup_state(c));
        }
        c->pending.emplace_back(admm_iters, gravity);
    }
    const int rc = step_impl(c, admm_iters, gravity, stats);
    if (rc == kStepAborted) return recover_from_abort(c, stats);
    if (rc == ADMM_HIP_OK && stats) c->pending.clear();   // a timed step ends with a synchronisation and the check
    return rc;
}

// z/u between the reference row layout (AoS, caller's term order) and the device SoA (sorted tets)
static void rows_to_dev(const admm_hip_ctx *c, const double *rows, std::vector<double> &tu, std::vector<double> &ru, std::vector<double> &pu, std::vector<double> &hu) {
    tu.assign((size_t)9 * c->ldt, 0.0); ru.assign((size_t)6 * c->ldr, 0.0); pu.assign(3 * (size_t)c->npin_terms, 0.0); hu.assign((size_t)3 * c->ldb, 0.0);
    for (int n = 0; n < c->nt; ++n)
        for (int k = 0; k < 9; ++k) tu[(size_t)k * c->ldt + n] = rows[9 * (size_t)c->tet_perm[n] + k];
    const double *r = rows + 9 * (size_t)c->nt_total;
    for (int t = 0; t < c->ntri; ++t)
        for (int k = 0; k < 6; ++k) ru[(size_t)k * c->ldr + t] = r[6 * (size_t)c->tri_perm[t] + k];
    r += 6 * (size_t)c->ntri_total;
    for (int t = 0; t < c->nbend; ++t)
        for (int k = 0; k < 3; ++k) hu[(size_t)k * c->ldb + t] = r[3 * (size_t)c->bend_perm[t] + k];
    r += 3 * (size_t)c->nbend_total;
    for (int p = 0; p < c->npin_terms; ++p)
        for (int k = 0; k < 3; ++k) pu[3 * (size_t)p + k] = r[6 * (size_t)p + k];
}
static void dev_to_rows(const admm_hip_ctx *c, const std::vector<double> &tu, const std::vector<double> &ru, const std::vector<double> &pu, const std::vector<double> &hu, double *rows) {
    for (int n = 0; n < c->nt; ++n)
        for (int k = 0; k < 9; ++k) rows[9 * (size_t)c->tet_perm[n] + k] = tu[(size_t)k * c->ldt + n];
    double *r = rows + 9 * (size_t)c->nt_total;
    for (int t = 0; t < c->ntri; ++t)
        for (int k = 0; k < 6; ++k) r[6 * (size_t)c->tri_perm[t] + k] = ru[(size_t)k * c->ldr + t];
    r += 6 * (size_t)c->ntri_total;
    for (int t = 0; t < c->nbend; ++t)
        for (int k = 0; k < 3; ++k) r[3 * (size_t)c->bend_perm[t] + k] = hu[(size_t)k * c->ldb + t];
    r += 3 * (size_t)c->nbend_total;
    for (int p = 0; p < c->npin_terms; ++p) {
        for (int k = 0; k < 3; ++k) r[6 * (size_t)p + k] = pu[3 * (size_t)p + k];
        for (int k = 3; k < 6; ++k) r[6 * (size_t)p + k] = 0.0; // rows 3..5 of a SpringPin are never populated
    }
}

int admm_hip_local_step(admm_hip_ctx *c, const double *x, double *u_inout, double *z_out, const double *Mxbar, double *b_out) {
    if (!c || !x || !u_inout || !z_out) return fail(ADMM_HIP_ERR_ARG, "local_step: NULL argument");
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, "local_step: kernel-level entry points work on the rows of the whole scene; this context holds only its rank's bodies (ADMM_HIP_PARTITION=elements)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<double> tu, ru, pu, hu;
    rows_to_dev(c, u_inout, tu, ru, pu, hu);
    HIP_TRY(hipMemcpyAsync(c->curr.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->nt) HIP_TRY(hipMemcpyAsync(c->t_u.p, tu.data(), tu.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->ntri) HIP_TRY(hipMemcpyAsync(c->r_u.p, ru.data(), ru.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->npin_terms) HIP_TRY(hipMemcpyAsync(c->pin_u.p, pu.data(), pu.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->nbend) HIP_TRY(hipMemcpyAsync(c->h_u.p, hu.data(), hu.size() * sizeof(double), hipMemcpyHostToDevice, st));
    c->xbar_of_state = false;      // (Mxbar is the caller's from here on, not the last step's: newton_polish refuses)
    if (Mxbar) HIP_TRY(hipMemcpyAsync(c->Mxbar.p, Mxbar, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(c->Mxbar.p, 0, c->n3 * sizeof(double), st));
    launch_local<true>(c);
    // multi-GPU contexts without a communicator return their PARTIAL right-hand side (parity tests sum them)
    if (c->world > 1 && !c->comm && !c->ar_fn) launch_gather(c);
    else if (launch_rhs(c)) return fail(ADMM_HIP_ERR_COMM, "local_step: ncclAllReduce failed");
    HIP_TRY(hipGetLastError());
    std::vector<double> tz((size_t)9 * c->ldt), rz((size_t)6 * c->ldr), pz(3 * (size_t)c->npin_terms), hz((size_t)3 * c->ldb);
    if (c->nbend) {
        HIP_TRY(hipMemcpyAsync(hu.data(), c->h_u.p, hu.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hz.data(), c->h_z.p, hz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (c->nt) {
        HIP_TRY(hipMemcpyAsync(tu.data(), c->t_u.p, tu.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(tz.data(), c->t_z.p, tz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (c->ntri) {
        HIP_TRY(hipMemcpyAsync(ru.data(), c->r_u.p, ru.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(rz.data(), c->r_z.p, rz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (c->npin_terms) {
        HIP_TRY(hipMemcpyAsync(pu.data(), c->pin_u.p, pu.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pz.data(), c->pin_z.p, pz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (b_out) HIP_TRY(hipMemcpyAsync(b_out, c->b.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    dev_to_rows(c, tu, ru, pu, hu, u_inout);
    dev_to_rows(c, tz, rz, pz, hz, z_out);
    return ADMM_HIP_OK;
}

int admm_hip_regather_rhs(admm_hip_ctx *c, const double *u_before, int32_t variant, double *b_out) {
    if (!c || !b_out) return fail(ADMM_HIP_ERR_ARG, "regather_rhs: NULL argument");
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, "regather_rhs: kernel-level entry points work on the rows of the whole scene; this context holds only its rank's bodies (ADMM_HIP_PARTITION=elements)");
    if (variant < 0 || variant > 3) return fail(ADMM_HIP_ERR_ARG, "regather_rhs: variant must be a combination of 1 (reference loop) and 2 (instantiation with the stop word)");
    if (c->world > 1 || c->comm || c->ar_fn) return fail(ADMM_HIP_ERR_ARG, "regather_rhs: single-GPU contexts only");
    if (c->npin_terms && !u_before) return fail(ADMM_HIP_ERR_ARG, "regather_rhs: a scene with pin terms needs u_before (the gather runs their local step)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // the gather runs the local step of the pin terms: start it from the u the measured gather started from, and put back what that one left
    const size_t np3 = 3 * (size_t)c->npin_terms;
    std::vector<double> pu(np3), pu_keep(np3), pz_keep(np3), b_keep((size_t)c->n3);
    if (np3) {
        const double *r = u_before + 9 * (size_t)c->nt_total + 6 * (size_t)c->ntri_total + 3 * (size_t)c->nbend_total;
        for (int p = 0; p < c->npin_terms; ++p)
            for (int k = 0; k < 3; ++k) pu[3 * (size_t)p + k] = r[6 * (size_t)p + k];
        HIP_TRY(hipMemcpyAsync(pu_keep.data(), c->pin_u.p, np3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pz_keep.data(), c->pin_z.p, np3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->pin_u.p, pu.data(), np3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(b_keep.data(), c->b.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    {   // variant & 2: the instantiation a step with the early exit on the device launches, its stop word cleared as at the start of a step
        struct StopDev { admm_hip_ctx *c; ~StopDev() { c->stop_dev = nullptr; } } stop_dev_guard{c};
        if (variant & 2) {
            HIP_TRY(hipMemsetAsync(c->counters.p + kCntAdmmStop, 0, sizeof(int), st));
            c->stop_dev = c->counters.p + kCntAdmmStop;
        }
        if (variant & 1) launch_gather<true>(c);
        else launch_gather<false>(c);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b_out, c->b.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));      // (the pageable copies above are staged: the host buffers are free to reuse)
    HIP_TRY(hipMemcpyAsync(c->b.p, b_keep.data(), c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (np3) {
        HIP_TRY(hipMemcpyAsync(c->pin_u.p, pu_keep.data(), np3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->pin_z.p, pz_keep.data(), np3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}

int admm_hip_global_solve(admm_hip_ctx *c, const double *b, double *x_inout, int32_t *iters) {
    if (!c || !b || !x_inout) return fail(ADMM_HIP_ERR_ARG, "global_solve: NULL argument");
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, "global_solve: kernel-level entry points work on the whole scene; this context holds only its rank's bodies (ADMM_HIP_PARTITION=elements)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(c->b.p, b, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->curr.p, x_inout, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    c->uz_iters_step = 0;
    c->rc_prev_valid = 0; c->rc_prev2_valid = 0; c->rc_frame += 1; c->rc_iter = 0;   // stand-alone solve: nothing to recycle
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, kCntStepWords * sizeof(int), st));
    if (c->linsolver == 2) HIP_TRY(hipMemsetAsync(c->counters.p + kCntSchurIters, 0, sizeof(int), st));
    if (launch_global(c, c->b.p, c->curr.p, false)) return fail(ADMM_HIP_ERR_DEVICE, "PCG: the device stopped signalling progress");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x_inout, c->curr.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    int h[kCntRing];
    HIP_TRY(hipMemcpyAsync(h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->h_sig && c->h_sig[kSigAbort]) { c->h_sig[kSigAbort] = 0; return fail(ADMM_HIP_ERR_DEVICE, "PCG: a grid barrier of the on-chip solve timed out (is another persistent kernel sharing the GPU?)"); }
    if (iters) *iters = (c->linsolver == 1) ? h[kCntGsSweeps] : (c->linsolver == 2 ? c->uz_iters_step + h[kCntSchurIters] : h[kCntIters]);
    return ADMM_HIP_OK;
}

int admm_hip_pcg_instances(admm_hip_ctx *c, int32_t *last, int64_t *launches, int32_t *last_verifications) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "pcg_instances: NULL context");
    if (last) *last = c->oc_last_instance;
    if (launches) for (int i = 0; i < 4; ++i) launches[i] = c->oc_instance_launches[i];
    if (last_verifications) {
        *last_verifications = -1;
        if (c->oc_last_instance) {      // (k_pcg2's report of the solve: alpha[0] = verifications of the true residual it ran)
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            CgScal h;
            HIP_TRY(hipMemcpy(&h, c->cg_scal.p, sizeof(h), hipMemcpyDeviceToHost));
            *last_verifications = (int32_t)h.alpha[0];
        }
    }
    return ADMM_HIP_OK;
}

int admm_hip_solve_totals(admm_hip_ctx *c, int64_t *solves, int64_t *converged, int64_t *inner_iters) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "solve_totals: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    int h[kCntTotalsLen] = {};
    HIP_TRY(hipMemcpy(h, c->counters.p + kCntTotals, sizeof(h), hipMemcpyDeviceToHost));
    const bool counted = (c->oc_enabled && c->oc_plan) || c->big_enabled || (c->linsolver != 1 && !c->oc_enabled && !c->dist_solve && ensure_big_plan(c));     // the on-chip PCG and the launch-path two-level PCG keep these totals
    if (solves) *solves = counted ? h[0] : -1;
    if (converged) *converged = counted ? h[1] : -1;
    if (inner_iters) *inner_iters = counted ? h[2] : -1;
    return ADMM_HIP_OK;
}

// ---- energy / residuals / monitor (monitor.hpp) ----
static int mon_refuse(const admm_hip_ctx *c, const char *who) {
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, std::string(who) + ": this context holds only its rank's bodies; energies and residuals are sums over the whole scene (single-GPU contexts only)");
    if (!monitor_allowed(c)) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": single-GPU contexts only (world_size > 1, a communicator or a caller all-reduce splits the terms over ranks)");
    return ADMM_HIP_OK;
}

// the context's device current, its stream idle, no step pending (settle)
static int quiesce(admm_hip_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return settle(c);
}

// The common entry of energy, forces / stress and stiffness_apply: refuses what mon_refuse refuses and a call without positions, waits for
// the stream, settles and uploads x.  *xd = the positions on the device: the device-resident state, or curr when x is given (curr is scratch
// between steps).
static int eval_begin(admm_hip_ctx *c, const char *who, const double *x, const double **xd) {
    if (int rc = mon_refuse(c, who)) return rc;
    if (!x && !c->state_set) return fail(ADMM_HIP_ERR_STATE, std::string(who) + ": no device-resident state yet (admm_hip_set_state), and x is NULL");
    if (int rc = quiesce(c)) return rc;
    *xd = c->x.p;
    if (x) { HIP_TRY(hipMemcpyAsync(c->curr.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice, c->stream)); *xd = c->curr.p; }
    return ADMM_HIP_OK;
}

// The common entry of the calls that minimise (newton_polish) or differentiate (step_adjoint, step_adjoint_block, adjoint_held) the step's
// objective at the device-resident state: single-GPU contexts only (the rules of energy(), forces() and stiffness_apply()), nothing in the
// scene that the objective leaves out, the stream idle, and a step behind the state (its x_bar)
static int step_problem_begin(admm_hip_ctx *c, const char *who, bool polish) {
    const std::string w(who);
    if (int rc = mon_refuse(c, who)) return rc;
    if (c->obst.n > 0 || !c->dyn.empty())
        return fail(ADMM_HIP_ERR_ARG, w + ": the context has colliders; contact is not part of the " + (polish ? "objective the polish minimises" : "problem the adjoint differentiates"));
    if (c->tri_limited) return fail(ADMM_HIP_ERR_ARG, w + ": the context has strain-limited triangles; the " + (polish ? "energy ignores" : "forces ignore") + " the limits");
    if (c->has_slide) return fail(ADMM_HIP_ERR_ARG, w + ": the context has slide pins");
    if (int rc = quiesce(c)) return rc;
    if (!c->xbar_of_state) return fail(ADMM_HIP_ERR_ARG, w + ": no step has run on this state yet (the " + (polish ? "objective" : "adjoint") + " needs the step's x_bar)");
    return ADMM_HIP_OK;
}

int admm_hip_energy(admm_hip_ctx *c, const double *x, double *totals4, double *per_term) {
    if (!c || !totals4) return fail(ADMM_HIP_ERR_ARG, "energy: NULL argument");
    const double *xd;
    if (int rc = eval_begin(c, "energy", x, &xd)) return rc;
    HIP_TRY(mon_ensure(c, false, per_term != nullptr));
    hipStream_t st = c->stream;
    MonArgs a = mon_args(c, xd, false);
    a.term = per_term ? c->mon_term.p : nullptr;
    launch_monitor<false, true>(c, a, c->mon_out.p);
    HIP_TRY(hipGetLastError());
    double h[kMonQ];
    const size_t nterm = (size_t)c->nt + c->ntri + c->nbend;
    std::vector<double> term(per_term ? nterm : 0);
    HIP_TRY(hipMemcpyAsync(h, c->mon_out.p, sizeof(h), hipMemcpyDeviceToHost, st));
    if (per_term && nterm) HIP_TRY(hipMemcpyAsync(term.data(), c->mon_term.p, nterm * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    totals4[0] = h[4]; totals4[1] = h[5]; totals4[2] = h[6]; totals4[3] = (h[4] + h[5]) + h[6];
    if (per_term) {      // device order (tets sorted by model, every family by its lowest vertex) -> the caller's term order
        for (int n = 0; n < c->nt; ++n) per_term[c->tet_perm[n]] = term[n];
        double *r = per_term + c->nt_total;
        for (int t = 0; t < c->ntri; ++t) r[c->tri_perm[t]] = term[(size_t)c->nt + t];
        r += c->ntri_total;
        for (int t = 0; t < c->nbend; ++t) r[c->bend_perm[t]] = term[(size_t)c->nt + c->ntri + t];
    }
    return ADMM_HIP_OK;
}

// f = -dE/dx and / or the per-tet stress at x (host, or NULL = the device-resident state): one force pass (forces.hpp)
static int forces_impl(admm_hip_ctx *c, const char *who, const double *x, double *f, double *out13) {
    if (!c || (!f && !out13)) return fail(ADMM_HIP_ERR_ARG, std::string(who) + ": NULL argument");
    const double *xd;
    if (int rc = eval_begin(c, who, x, &xd)) return rc;
    HIP_TRY(force_ensure(c, out13 != nullptr, 0));
    hipStream_t st = c->stream;
    launch_forces(c, xd, out13 != nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<double> sd(out13 && c->nt ? (size_t)kStressQ * c->ldt : 0);      // (a scene without tets has no stress)
    if (f && c->n3) HIP_TRY(hipMemcpyAsync(f, c->f_out.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!sd.empty()) HIP_TRY(hipMemcpyAsync(sd.data(), c->f_stress.p, sd.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out13)      // device order (tets sorted by model) -> the caller's tet order
        for (int n = 0; n < c->nt; ++n)
            for (int q = 0; q < kStressQ; ++q) out13[(size_t)kStressQ * c->tet_perm[n] + q] = sd[(size_t)q * c->ldt + n];
    return ADMM_HIP_OK;
}
int admm_hip_forces(admm_hip_ctx *c, const double *x, double *f) { return forces_impl(c, "forces", x, f, nullptr); }
int admm_hip_stress(admm_hip_ctx *c, const double *x, double *out13) { return forces_impl(c, "stress", x, nullptr, out13); }

// out_j = K(x) d_j + shift (m o d_j), K = d2E/dx2 at x (host, or NULL = the device-resident state): one tangent pass (tangent.hpp)
int admm_hip_stiffness_apply(admm_hip_ctx *c, const double *x, int32_t n_vec, const double *d, double shift, double *out) {
    if (!c || !d || !out || n_vec < 1 || n_vec > 65535) return fail(ADMM_HIP_ERR_ARG, "stiffness_apply: NULL argument, n_vec < 1 or n_vec > 65535");
    const double *xd;
    if (int rc = eval_begin(c, "stiffness_apply", x, &xd)) return rc;
    HIP_TRY(tangent_ensure(c, n_vec));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_vec * c->n3;
    if (n) HIP_TRY(hipMemcpyAsync(c->k_d.p, d, n * sizeof(double), hipMemcpyHostToDevice, st));
    launch_tangent(c, xd, n_vec, shift);
    HIP_TRY(hipGetLastError());
    if (n) HIP_TRY(hipMemcpyAsync(out, c->k_out.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}

// ---- frozen tangent, tangent_solve, newton_polish (newton.hpp) ----
// admm_hip_stiffness_apply on the frozen tangent: one setup, then one frozen pass per direction.  flags bit 0: the element tangents are
// projected to their positive semi-definite part; bit 1: pinned vertices are held (their rows are zero, d is ignored there)
int admm_hip_stiffness_apply_ex(admm_hip_ctx *c, const double *x, int32_t n_vec, const double *d, double shift, int32_t flags, double *out) {
    if (!c || !d || !out || n_vec < 1 || n_vec > 65535) return fail(ADMM_HIP_ERR_ARG, "stiffness_apply_ex: NULL argument, n_vec < 1 or n_vec > 65535");
    if (int rc = newton_args_ok("stiffness_apply_ex", shift, flags, 7)) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "stiffness_apply_ex", x, &xd)) return rc;
    HIP_TRY(newton_ensure(c));
    hipStream_t st = c->stream;
    const int *pin = nullptr;
    if (flags & 2) { launch_pin_mask(c); pin = c->nw_pin.p; }
    launch_tangent_setup(c, xd, flags & 1);
    if ((flags & 4) && c->n3) {      // all columns up in one copy, block passes in slabs of kModalNb directions, back in one copy
        const size_t n = (size_t)n_vec * c->n3;
        HIP_TRY(c->bk_el.ensure(c, std::min<int>(n_vec, kModalNb)));
        if (c->bk_d.n < n) HIP_TRY(c->bk_d.alloc_zeroed(n, st));
        if (c->bk_out.n < n) HIP_TRY(c->bk_out.alloc_zeroed(n, st));
        HIP_TRY(hipMemcpyAsync(c->bk_d.p, d, n * sizeof(double), hipMemcpyHostToDevice, st));
        if (pin) hipLaunchKernelGGL(k_nw_mask_block, dim3(nw_blocks(c), n_vec), dim3(256), 0, st, c->nv, (size_t)c->n3, pin, c->bk_d.p);
        for (int j = 0; j < n_vec; j += kModalNb)
            launch_frozen_block(c, c->bk_d.p + (size_t)j * c->n3, c->bk_out.p + (size_t)j * c->n3, std::min<int>(kModalNb, n_vec - j), shift, pin, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, c->bk_out.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ADMM_HIP_OK;
    }
    for (int j = 0; j < n_vec && c->n3; ++j) {
        HIP_TRY(hipMemcpyAsync(c->nw_rhs.p, d + (size_t)j * c->n3, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_nw_mask, dim3(nw_blocks(c)), dim3(256), 0, st, c->nv, pin, c->nw_rhs.p, c->nw_p.p);
        launch_frozen(c, c->nw_p.p, c->nw_ap.p, shift, pin, nullptr);
        HIP_TRY(hipMemcpyAsync(out + (size_t)j * c->n3, c->nw_ap.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}

// (K(x) [projected] + shift M) y = rhs on the free vertices by Jacobi-PCG on the device.  info4: iterations, converged, |r| / |rhs| with
// r = rhs - A y formed once more at the end (not the recursive residual of the stop test), |rhs|
int admm_hip_tangent_solve(admm_hip_ctx *c, const double *x, const double *rhs, double shift, int32_t flags, double tol, int32_t max_iters,
                           double *y, double *info4) {
    if (!c || !rhs || !y || !info4) return fail(ADMM_HIP_ERR_ARG, "tangent_solve: NULL argument");
    if (int rc = newton_args_ok("tangent_solve", shift, flags)) return rc;
    if (int rc = solve_args_ok("tangent_solve", tol, max_iters)) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "tangent_solve", x, &xd)) return rc;
    HIP_TRY(newton_ensure(c));
    hipStream_t st = c->stream;
    if (c->n3) HIP_TRY(hipMemcpyAsync(c->nw_rhs.p, rhs, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (int rc = tangent_solve_device(c, xd, shift, flags, tol, max_iters)) return rc;
    NwCg h;
    double rr_true = 0.0;
    if (c->n3) HIP_TRY(hipMemcpyAsync(y, c->nw_y.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h, c->nw_st.p + 2, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&rr_true, c->nw_part.p + (size_t)3 * nw_blocks(c) + 2, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    fill_solve_info(h, rr_true, info4);
    return ADMM_HIP_OK;
}

// ---- tangent solves for a stack of right-hand sides (newton.hpp: the block PCG) ----

// admm_hip_tangent_solve for k right-hand sides on one frozen operator: one setup, one diagonal, and the block PCG in slabs of
// kNwBlkCols columns.  info: [k][4] as admm_hip_tangent_solve; block_info3: block iterations (the longest column; of the longest slab),
// column passes, blocked 0 / 1
int admm_hip_tangent_solve_block(admm_hip_ctx *c, const double *x, int32_t k, const double *rhs, double shift, int32_t flags, double tol,
                                 int32_t max_iters, double *y, double *info, double *block_info3) {
    if (!c || !rhs || !y || !info || !block_info3) return fail(ADMM_HIP_ERR_ARG, "tangent_solve_block: NULL argument");
    if (k < 1 || k > 65535) return fail(ADMM_HIP_ERR_ARG, "tangent_solve_block: k < 1 or k > 65535");
    if (int rc = newton_args_ok("tangent_solve_block", shift, flags)) return rc;
    if (int rc = solve_args_ok("tangent_solve_block", tol, max_iters)) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "tangent_solve_block", x, &xd)) return rc;
    HIP_TRY(newton_ensure(c));
    HIP_TRY(block_pcg_ensure(c, std::min<int>(k, kNwBlkCols)));
    hipStream_t st = c->stream;
    const size_t n3 = (size_t)c->n3;
    const bool blocked = c->tc_kind == 0;
    const int *pin = nullptr;
    if (blocked)
        if (int rc = tangent_solve_head(c, xd, shift, flags, false, &pin)) return rc;
    std::vector<NwCg> st3;
    BlockVerdict v;
    NwBlockCtl ctl{};
    block_info3[0] = 0.0; block_info3[1] = 0.0; block_info3[2] = blocked ? 1.0 : 0.0;
    for (int j0 = 0; j0 < k; j0 += kNwBlkCols) {
        const int kk = std::min<int>(kNwBlkCols, k - j0);
        if (n3) HIP_TRY(hipMemcpyAsync(c->bp_rhs.p, rhs + (size_t)j0 * n3, (size_t)kk * n3 * sizeof(double), hipMemcpyHostToDevice, st));
        if (int rc = block_solve_slab(c, xd, kk, shift, flags, pin, tol, max_iters, blocked)) return rc;
        if (n3) HIP_TRY(hipMemcpyAsync(y + (size_t)j0 * n3, c->bp_y.p, (size_t)kk * n3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(block_verdict_download(c, kk, blocked, st3, &v, &ctl));
        HIP_TRY(hipStreamSynchronize(st));
        block_verdict_finish(kk, blocked, st3, ctl, &v);
        for (int j = 0; j < kk; ++j) fill_solve_info(v.st[j], v.rr[j], info + (size_t)4 * (j0 + j));
        block_info3[0] = std::max(block_info3[0], (double)v.iters); block_info3[1] += v.passes;
    }
    return ADMM_HIP_OK;
}

// The preconditioner of admm_hip_tangent_solve, admm_hip_newton_polish and admm_hip_step_adjoint
int admm_hip_set_tangent_precond(admm_hip_ctx *c, int32_t kind, int32_t aggregates) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_tangent_precond: NULL context");
    if (kind < 0 || kind > 1) return fail(ADMM_HIP_ERR_ARG, "set_tangent_precond: kind is 0 (Jacobi) or 1 (two-level)");
    if (aggregates < 0 || aggregates > kTcMaxAgg) return fail(ADMM_HIP_ERR_ARG, "set_tangent_precond: aggregates in 0 .. 64 (0: the default)");
    if (int rc = mon_refuse(c, "set_tangent_precond")) return rc;
    if (aggregates > std::max(1, c->nv)) return fail(ADMM_HIP_ERR_ARG, "set_tangent_precond: more aggregates than vertices");
    if (kind == 1 && c->tc_xyz_h.size() != (size_t)c->n3) return fail(ADMM_HIP_ERR_ARG, "set_tangent_precond: the two-level preconditioner needs desc.vert_xyz");
    c->tc_kind = kind; c->tc_aggregates = aggregates;
    return ADMM_HIP_OK;
}
int admm_hip_get_tangent_precond(admm_hip_ctx *c, int32_t *kind, int32_t *aggregates, int32_t *coarse_dim, int32_t *coarse_dropped, int32_t *coarse_ok,
                                 int32_t *setup_passes) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_tangent_precond: NULL context");
    int h[3] = {0, 0, 0};
    if (c->tc_last_nc > 0) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(h, c->tc_info.p, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (kind) *kind = c->tc_kind;
    if (aggregates) *aggregates = c->tc_aggregates;
    if (coarse_dim) *coarse_dim = c->tc_last_nc;
    if (coarse_dropped) *coarse_dropped = h[2];
    if (coarse_ok) *coarse_ok = h[1];
    if (setup_passes) *setup_passes = c->tc_last_passes;
    return ADMM_HIP_OK;
}
// z = M^-1 r of the two-level preconditioner of the tangent frozen at x (tests): the setup of a solve, then its start -- p of iteration 0
int admm_hip_tangent_precond_apply(admm_hip_ctx *c, const double *x, const double *r, double shift, int32_t flags, double *z_out) {
    if (!c || !r || !z_out) return fail(ADMM_HIP_ERR_ARG, "tangent_precond_apply: NULL argument");
    if (int rc = newton_args_ok("tangent_precond_apply", shift, flags)) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "tangent_precond_apply", x, &xd)) return rc;
    HIP_TRY(newton_ensure(c));
    hipStream_t st = c->stream;
    if (c->n3) HIP_TRY(hipMemcpyAsync(c->nw_rhs.p, r, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    const int *pin;
    if (int rc = tangent_solve_head(c, xd, shift, flags, true, &pin)) return rc;
    launch_tc_start(c, pin);
    HIP_TRY(hipGetLastError());
    if (c->n3) HIP_TRY(hipMemcpyAsync(z_out, c->nw_p.p, c->n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}
// The dense inverse behind the two-level preconditioner: 0 one block (k_tc_invert), 1 blocked over the chip (tangent_coarse.hpp)
int admm_hip_set_tangent_coarse(admm_hip_ctx *c, int32_t solver) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_tangent_coarse: NULL context");
    if (solver < 0 || solver > 1) return fail(ADMM_HIP_ERR_ARG, "set_tangent_coarse: solver is 0 (one block) or 1 (blocked)");
    if (int rc = mon_refuse(c, "set_tangent_coarse")) return rc;
    c->tc_coarse_solver = solver;
    return ADMM_HIP_OK;
}
int admm_hip_get_tangent_coarse(admm_hip_ctx *c, int32_t *solver, int32_t *tile, int32_t *last_launches) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_tangent_coarse: NULL context");
    if (solver) *solver = c->tc_coarse_solver;
    if (tile) *tile = admm_dev::kTcbT;
    if (last_launches) *last_launches = c->tc_last_launches;
    return ADMM_HIP_OK;
}
// X = A^-1 by the selected inverse on the device (tests), in scratch of its own: no tc_ buffer of the context is touched
int admm_hip_tangent_coarse_invert(admm_hip_ctx *c, int32_t n, const double *A_host, double *X_host, int32_t *ok, int32_t *dropped) {
    if (!c || !A_host || !X_host || !ok || !dropped) return fail(ADMM_HIP_ERR_ARG, "tangent_coarse_invert: NULL argument");
    if (n < 1 || n > kTcMaxAgg * kTcPer) return fail(ADMM_HIP_ERR_ARG, "tangent_coarse_invert: n in 1 .. 768");
    if (int rc = mon_refuse(c, "tangent_coarse_invert")) return rc;
    if (int rc = quiesce(c)) return rc;
    hipStream_t st = c->stream;
    const size_t nn = (size_t)n * n;
    DevBuf<double> A, X, ds, dl, col, Linv, Wm;
    DevBuf<int> keep, info;
    HIP_TRY(A.alloc(nn)); HIP_TRY(X.alloc_zeroed(nn, st));
    for (DevBuf<double> *b : {&ds, &dl, &col}) HIP_TRY(b->alloc_zeroed((size_t)n, st));
    HIP_TRY(keep.alloc_zeroed((size_t)n, st)); HIP_TRY(info.alloc_zeroed(3, st));
    HIP_TRY(hipMemcpyAsync(A.p, A_host, nn * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->tc_coarse_solver == 1) {
        HIP_TRY(Wm.alloc_zeroed(nn, st));
        HIP_TRY(Linv.alloc_zeroed((size_t)admm_dev::tcb_tiles(n) * admm_dev::kTcbT * admm_dev::kTcbT, st));
        c->tc_last_launches = launch_tcb_invert(st, n, A.p, X.p, ds.p, keep.p, info.p, Linv.p, Wm.p);
    } else {
        hipLaunchKernelGGL(k_tc_invert, dim3(1), dim3(1024), 0, st, n, A.p, X.p, ds.p, dl.p, col.p, keep.p, info.p, info.p + 1);
        c->tc_last_launches = 1;
    }
    HIP_TRY(hipGetLastError());
    int h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(X_host, X.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h, info.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *ok = h[1]; *dropped = h[2];
    return ADMM_HIP_OK;
}
int admm_host_tangent_plan(int32_t n_verts, const double *xyz, int32_t G, int32_t *agg_ptr, int32_t *agg_vert) {
    if (n_verts < 0 || !agg_ptr || (n_verts > 0 && (!xyz || !agg_vert))) return fail(ADMM_HIP_ERR_ARG, "tangent_plan: NULL argument");
    if (G < 1 || G > kTcMaxAgg || G > std::max(1, n_verts)) return fail(ADMM_HIP_ERR_ARG, "tangent_plan: G in 1 .. min(64, n_verts)");
    std::vector<int32_t> ptr, vert;
    if (!admm_host::tangent_plan(n_verts, xyz, G, ptr, vert)) return fail(ADMM_HIP_ERR_ARG, "tangent_plan: no plan");
    std::copy(ptr.begin(), ptr.end(), agg_ptr);
    std::copy(vert.begin(), vert.end(), agg_vert);
    return ADMM_HIP_OK;
}

// The k lowest eigenpairs of K_s phi = theta M phi on the free rows by LOBPCG on the device (modal.hpp); lambda = theta - shift
int admm_hip_modes(admm_hip_ctx *c, const double *x, int32_t k, int32_t guard, double shift, int32_t flags, double tol, int32_t max_iters,
                   const double *init, double *lambda, double *phi, double *info) {
    if (!c || !lambda || !phi || !info) return fail(ADMM_HIP_ERR_ARG, "modes: NULL argument");
    if (int rc = newton_args_ok("modes", shift, flags)) return rc;
    if (k < 1 || guard < 0 || k + guard > kModalNb) return fail(ADMM_HIP_ERR_ARG, "modes: k >= 1, guard >= 0 and k + guard <= 16");
    if (int rc = solve_args_ok("modes", tol, max_iters)) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "modes", x, &xd)) return rc;
    HIP_TRY(newton_ensure(c));
    hipStream_t st = c->stream;
    const int nb = k + guard;
    const int *pin = nullptr;
    long free_rows = c->n3;
    if (flags & 2) {
        launch_pin_mask(c); pin = c->nw_pin.p;
        std::vector<int> hp((size_t)std::max(1, c->nv));
        HIP_TRY(hipMemcpyAsync(hp.data(), c->nw_pin.p, (size_t)c->nv * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int v = 0; v < c->nv; ++v) free_rows -= hp[v] ? 3 : 0;
    }
    if ((long)3 * nb > free_rows) return fail(ADMM_HIP_ERR_ARG, "modes: 3 (k + guard) exceeds the number of free unknowns");
    HIP_TRY(modal_ensure(c));
    const size_t n3 = (size_t)c->n3;
    HIP_TRY(hipMemsetAsync(c->md_S.p, 0, (size_t)kModalCols * n3 * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(c->md_AS.p, 0, (size_t)kModalCols * n3 * sizeof(double), st));
    if (init) HIP_TRY(hipMemcpyAsync(c->md_S.p, init, (size_t)nb * n3 * sizeof(double), hipMemcpyHostToDevice, st));
    const ModalArgs a = modal_args(c, k, nb, tol, max_iters);
    hipLaunchKernelGGL(k_modal_start, dim3(nw_blocks(c)), dim3(256), 0, st, a, pin, init ? 1 : 0);
    if (int rc = modes_device(c, xd, k, nb, shift, flags, tol, max_iters, pin)) return rc;
    ModalSt h;
    const size_t nbk = (size_t)nw_blocks(c);
    std::vector<double> part((size_t)2 * nb * nbk), th((size_t)nb);
    HIP_TRY(hipMemcpyAsync(&h, c->md_st.p + 2, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(part.data(), c->md_rpart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(th.data(), c->md_theta.p, th.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(phi, c->md_S.p, (size_t)k * n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int met = 0;
    for (int i = 0; i < k; ++i) {
        double r2 = 0.0, mx2 = 0.0;
        for (size_t b = 0; b < nbk; ++b) { r2 += part[(size_t)(2 * i) * nbk + b]; mx2 += part[(size_t)(2 * i + 1) * nbk + b]; }
        const double den = std::fabs(th[i]) * std::sqrt(mx2);
        info[4 + i] = den > 0.0 ? std::sqrt(r2) / den : std::sqrt(r2);
        met += info[4 + i] <= tol ? 1 : 0;
        lambda[i] = th[i] - shift;
    }
    const int ended = h.done ? h.ended : 1;
    info[0] = h.it; info[1] = ended == 0 ? k : met; info[2] = h.restarts; info[3] = ended;
    return ADMM_HIP_OK;
}

// Projected Newton on the step's objective Phi(x) = |x - x_bar|_M^2 / (2 dt^2) + E(x), from the device-resident state of the last step.
// records [cap][5]: Phi, |g_free|, the CG iterations and the accepted step length of the step taken from this iterate (0, 0: none), E.
int admm_hip_newton_polish(admm_hip_ctx *c, int32_t max_newton, double grad_tol, double cg_tol, int32_t cg_max, int32_t cap, int32_t *n,
                           double *records) {
    if (!c || !n || cap < 0 || (cap > 0 && !records)) return fail(ADMM_HIP_ERR_ARG, "newton_polish: bad argument");
    if (max_newton < 0 || !(grad_tol >= 0.0) || !(cg_tol >= 0.0) || !std::isfinite(cg_tol) || cg_max < 1)
        return fail(ADMM_HIP_ERR_ARG, "newton_polish: max_newton >= 0, grad_tol >= 0, cg_tol finite and >= 0, cg_max >= 1");
    if (int rc = step_problem_begin(c, "newton_polish", true)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(newton_ensure(c));
    HIP_TRY(force_ensure(c, false, 0));
    HIP_TRY(mon_ensure(c, false, false));
    const int nv = c->nv, nb = nw_blocks(c);
    const double idt2 = 1.0 / (c->dt * c->dt);
    double *sums = c->nw_part.p + (size_t)3 * nb;      // [0] |g|^2, [1] g . delta
    auto objective = [&](const double *xd, double *phi, double *el) -> int {      // (one synchronisation)
        const MonArgs a = mon_args(c, xd, true);
        launch_monitor<false, true>(c, a, c->mon_out.p);
        double h[kMonQ];
        HIP_TRY(hipMemcpyAsync(h, c->mon_out.p, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *el = (h[4] + h[5]) + h[6];
        *phi = *el + 0.5 * idt2 * h[7];
        return ADMM_HIP_OK;
    };
    launch_pin_mask(c);
    double phi = 0.0, el = 0.0;
    if (int rc = objective(c->x.p, &phi, &el)) return rc;
    *n = 0;
    for (int k = 0; ; ++k) {
        launch_state_residual(c, idt2, c->nw_rhs.p);
        double g2 = 0.0;
        HIP_TRY(hipMemcpyAsync(&g2, sums, sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const double gn = std::sqrt(g2);
        double *rec = (*n < cap) ? records + 5 * (size_t)*n : nullptr;
        if (rec) { rec[0] = phi; rec[1] = gn; rec[2] = 0.0; rec[3] = 0.0; rec[4] = el; }
        *n += 1;
        if (!(gn > grad_tol) || k >= max_newton) break;      // (a NaN gradient ends the polish too)
        if (int rc = tangent_solve_device(c, c->x.p, idt2, 3, cg_tol, cg_max)) return rc;
        hipLaunchKernelGGL(k_nw_slope, dim3(nb), dim3(256), 0, st, nv, c->nw_rhs.p, c->nw_y.p, c->nw_part.p);
        hipLaunchKernelGGL(k_stat_final, dim3(1), dim3(256), 0, st, c->nw_part.p, nb, sums + 1, nullptr);
        NwCg h;
        double slope = 0.0;
        HIP_TRY(hipMemcpyAsync(&h, c->nw_st.p + 2, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&slope, sums + 1, sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (rec) rec[2] = h.it;
        double t = 1.0, phi_t = 0.0, el_t = 0.0;
        bool accepted = false;
        for (int trial = 0; trial < 10; ++trial, t *= 0.5) {      // Armijo, c = 1e-4; a non-finite Phi is a rejection
            hipLaunchKernelGGL(k_nw_axpy, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, t, 0.0, c->nw_y.p, c->x.p, c->curr.p, (double *)nullptr);
            if (int rc = objective(c->curr.p, &phi_t, &el_t)) return rc;
            if (std::isfinite(phi_t) && phi_t <= phi + 1e-4 * t * slope) { accepted = true; break; }
        }
        if (!accepted) break;
        hipLaunchKernelGGL(k_nw_axpy, dim3(blocks_for(c->n3)), dim3(256), 0, st, c->n3, t, t / c->dt, c->nw_y.p, c->x.p, c->x.p, c->v.p);
        phi = phi_t; el = el_t;
        if (rec) rec[3] = t;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}

// ---- adjoint of a step (adjoint.hpp) ----
// a_j^T df/dtheta per energy term at x (host, or NULL = the device-resident state): one k_param_sens pass per kSensCols columns
int admm_hip_param_sensitivity(admm_hip_ctx *c, const double *x, int32_t k, const double *a, double *out_tets, double *out_tris, double *out_bends) {
    if (!c || !a || k < 1 || k > 65535) return fail(ADMM_HIP_ERR_ARG, "param_sensitivity: NULL argument, k < 1 or k > 65535");
    const double *xd;
    if (int rc = eval_begin(c, "param_sensitivity", x, &xd)) return rc;
    HIP_TRY(adjoint_ensure(c));
    hipStream_t st = c->stream;
    const size_t n3 = (size_t)c->n3;
    std::vector<double> h(c->adj_ps.n);
    for (int j0 = 0; j0 < k; j0 += kSensCols) {
        const int kk = std::min<int>(kSensCols, k - j0);
        if (n3) HIP_TRY(hipMemcpyAsync(c->adj_a.p, a + (size_t)j0 * n3, (size_t)kk * n3 * sizeof(double), hipMemcpyHostToDevice, st));
        launch_param_sens(c, xd, c->adj_a.p, n3, kk);
        HIP_TRY(hipGetLastError());
        HIP_TRY(param_sens_download(c, h, kk));
        HIP_TRY(hipStreamSynchronize(st));
        param_sens_unpermute(c, h, j0, kk, out_tets, out_tris, out_bends);
    }
    return ADMM_HIP_OK;
}

// The adjoint of the last step at the device-resident state (the formulas: adjoint.hpp).  flags bit 0: the solve uses the projected
// tangent; bit 1: the parameter sensitivities of lambda are wanted.  info6: iterations, converged, |g_x - A lambda| / |g_x| formed once
// more at the end, |g_x|, |r_free| of the state, the shift 1 / dt^2.
int admm_hip_step_adjoint(admm_hip_ctx *c, const double *dL_dx, const double *dL_dv, int32_t flags, double tol, int32_t max_iters, double *out_lambda,
                          double *out_xbar, double *out_xprev, double *out_vprev, double *out_mass, double *out_tets, double *out_tris,
                          double *out_bends, double *info6) {
    if (!c || !dL_dx || !info6) return fail(ADMM_HIP_ERR_ARG, "step_adjoint: NULL argument");
    if (flags < 0 || flags > 3) return fail(ADMM_HIP_ERR_ARG, "step_adjoint: flags must be a combination of 1 (positive semi-definite projection) and 2 (parameter sensitivities)");
    if (int rc = solve_args_ok("step_adjoint", tol, max_iters)) return rc;
    if (int rc = step_problem_begin(c, "step_adjoint", false)) return rc;      // (the rules of newton_polish: the adjoint is of the problem the polish solves)
    HIP_TRY(newton_ensure(c));
    HIP_TRY(force_ensure(c, false, 0));
    HIP_TRY(adjoint_ensure(c));
    hipStream_t st = c->stream;
    const int nv = c->nv, nb = nw_blocks(c);
    const size_t n3 = (size_t)c->n3;
    const double idt = 1.0 / c->dt, idt2 = 1.0 / (c->dt * c->dt);
    const bool params = (flags & 2) != 0;
    double *Lx = c->adj_l.p, *Lv = dL_dv ? c->adj_l.p + std::max<size_t>(1, n3) : nullptr;
    double *sums = c->nw_part.p + (size_t)3 * nb;      // [0] |r_free|^2, [2] the true residual of the solve
    if (n3) {
        HIP_TRY(hipMemcpyAsync(Lx, dL_dx, n3 * sizeof(double), hipMemcpyHostToDevice, st));
        if (Lv) HIP_TRY(hipMemcpyAsync(Lv, dL_dv, n3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    launch_pin_mask(c);
    // |r_free| of the state: the polish's own figure (its kernels, its bits); k_nw_grad's vector goes to adj_out, overwritten below
    launch_state_residual(c, idt2, c->adj_out.p);
    hipLaunchKernelGGL(k_adj_rhs, dim3(nb), dim3(256), 0, st, nv, Lx, Lv, idt, c->nw_pin.p, c->nw_rhs.p);
    if (int rc = tangent_solve_device(c, c->x.p, idt2, (flags & 1) | 2, tol, max_iters)) return rc;
    hipLaunchKernelGGL(k_adj_out, dim3(nb), dim3(256), 0, st, nv, n3, c->nw_y.p, c->m.p, c->Mxbar.p, c->x.p, Lv, idt, c->nw_pin.p, c->adj_out.p);
    if (params) launch_param_sens(c, c->x.p, c->nw_y.p, n3, 1);
    HIP_TRY(hipGetLastError());
    NwCg h;
    double g2 = 0.0, rr_true = 0.0;
    std::vector<double> hp(params ? c->adj_ps.n : 0);
    double *outs[4] = {out_xbar, out_xprev, out_vprev, out_mass};
    if (n3) {
        if (out_lambda) HIP_TRY(hipMemcpyAsync(out_lambda, c->nw_y.p, n3 * sizeof(double), hipMemcpyDeviceToHost, st));
        for (int q = 0; q < 4; ++q)
            if (outs[q]) HIP_TRY(hipMemcpyAsync(outs[q], c->adj_out.p + q * n3, n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (params) HIP_TRY(param_sens_download(c, hp, 1));
    HIP_TRY(hipMemcpyAsync(&h, c->nw_st.p + 2, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&g2, sums, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&rr_true, sums + 2, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (params) param_sens_unpermute(c, hp, 0, 1, out_tets, out_tris, out_bends);
    fill_solve_info(h, rr_true, info6);
    info6[4] = std::sqrt(g2); info6[5] = idt2;
    return ADMM_HIP_OK;
}

// admm_hip_step_adjoint for k losses at the same state: |r_free| once, k_adj_rhs / k_adj_out per column, the solves by the block PCG
// (block_solve_slab), one k_param_sens pass per slab over the stack of lambda.  info: [k][6] as admm_hip_step_adjoint; block_info3 as
// admm_hip_tangent_solve_block
int admm_hip_step_adjoint_block(admm_hip_ctx *c, int32_t k, const double *dL_dx, const double *dL_dv, int32_t flags, double tol, int32_t max_iters,
                                double *out_lambda, double *out_xbar, double *out_xprev, double *out_vprev, double *out_mass, double *out_tets,
                                double *out_tris, double *out_bends, double *info, double *block_info3) {
    if (!c || !dL_dx || !info || !block_info3) return fail(ADMM_HIP_ERR_ARG, "step_adjoint_block: NULL argument");
    if (k < 1 || k > 65535) return fail(ADMM_HIP_ERR_ARG, "step_adjoint_block: k < 1 or k > 65535");
    if (flags < 0 || flags > 3) return fail(ADMM_HIP_ERR_ARG, "step_adjoint_block: flags must be a combination of 1 (positive semi-definite projection) and 2 (parameter sensitivities)");
    if (int rc = solve_args_ok("step_adjoint_block", tol, max_iters)) return rc;
    if (int rc = step_problem_begin(c, "step_adjoint_block", false)) return rc;      // (the rules of step_adjoint)
    HIP_TRY(newton_ensure(c));
    HIP_TRY(force_ensure(c, false, 0));
    HIP_TRY(adjoint_ensure(c));
    const int slab = std::min<int>(k, kNwBlkCols);
    HIP_TRY(block_pcg_ensure(c, slab));
    hipStream_t st = c->stream;
    const int nv = c->nv, nb = nw_blocks(c);
    const size_t n3 = (size_t)c->n3, ld = std::max<size_t>(1, n3);
    if (c->adj_bl.n < 2 * slab * ld) HIP_TRY(c->adj_bl.alloc_zeroed(2 * slab * ld, st));
    if (c->adj_bout.n < 4 * slab * ld) HIP_TRY(c->adj_bout.alloc_zeroed(4 * slab * ld, st));
    const double idt = 1.0 / c->dt, idt2 = 1.0 / (c->dt * c->dt);
    const bool params = (flags & 2) != 0, blocked = c->tc_kind == 0;
    const int sflags = (flags & 1) | 2;
    double *Lx = c->adj_bl.p, *Lv = dL_dv ? c->adj_bl.p + slab * ld : nullptr;
    double *sums = c->nw_part.p + (size_t)3 * nb;      // [0] |r_free|^2
    launch_pin_mask(c);
    // |r_free| of the state, once (admm_hip_step_adjoint: the polish's own figure)
    launch_state_residual(c, idt2, c->adj_out.p);
    double g2 = 0.0;
    HIP_TRY(hipMemcpyAsync(&g2, sums, sizeof(double), hipMemcpyDeviceToHost, st));
    const int *pin = nullptr;
    if (blocked)
        if (int rc = tangent_solve_head(c, c->x.p, idt2, sflags, false, &pin)) return rc;
    std::vector<NwCg> st3;
    std::vector<double> hp(params ? c->adj_ps.n : 0);
    BlockVerdict v;
    NwBlockCtl ctl{};
    double *outs[4] = {out_xbar, out_xprev, out_vprev, out_mass};
    block_info3[0] = 0.0; block_info3[1] = 0.0; block_info3[2] = blocked ? 1.0 : 0.0;
    for (int j0 = 0; j0 < k; j0 += kNwBlkCols) {
        const int kk = std::min<int>(kNwBlkCols, k - j0);
        if (n3) {
            HIP_TRY(hipMemcpyAsync(Lx, dL_dx + (size_t)j0 * n3, (size_t)kk * n3 * sizeof(double), hipMemcpyHostToDevice, st));
            if (Lv) HIP_TRY(hipMemcpyAsync(Lv, dL_dv + (size_t)j0 * n3, (size_t)kk * n3 * sizeof(double), hipMemcpyHostToDevice, st));
        }
        for (int j = 0; j < kk; ++j)
            hipLaunchKernelGGL(k_adj_rhs, dim3(nb), dim3(256), 0, st, nv, Lx + j * n3, Lv ? Lv + j * n3 : nullptr, idt, c->nw_pin.p, c->bp_rhs.p + j * n3);
        if (int rc = block_solve_slab(c, c->x.p, kk, idt2, sflags, pin, tol, max_iters, blocked)) return rc;
        for (int j = 0; j < kk; ++j)
            hipLaunchKernelGGL(k_adj_out, dim3(nb), dim3(256), 0, st, nv, n3, c->bp_y.p + j * n3, c->m.p, c->Mxbar.p, c->x.p, Lv ? Lv + j * n3 : nullptr, idt,
                               c->nw_pin.p, c->adj_bout.p + 4 * j * n3);
        if (params) launch_param_sens(c, c->x.p, c->bp_y.p, n3, kk);
        HIP_TRY(hipGetLastError());
        if (n3) {
            if (out_lambda) HIP_TRY(hipMemcpyAsync(out_lambda + (size_t)j0 * n3, c->bp_y.p, (size_t)kk * n3 * sizeof(double), hipMemcpyDeviceToHost, st));
            for (int q = 0; q < 4; ++q)
                if (outs[q])      // [kk] rows of n3 doubles, 4 n3 apart on the device
                    HIP_TRY(hipMemcpy2DAsync(outs[q] + (size_t)j0 * n3, n3 * sizeof(double), c->adj_bout.p + q * n3, 4 * n3 * sizeof(double), n3 * sizeof(double),
                                             (size_t)kk, hipMemcpyDeviceToHost, st));
        }
        if (params) HIP_TRY(param_sens_download(c, hp, kk));
        HIP_TRY(block_verdict_download(c, kk, blocked, st3, &v, &ctl));
        HIP_TRY(hipStreamSynchronize(st));
        block_verdict_finish(kk, blocked, st3, ctl, &v);
        if (params) param_sens_unpermute(c, hp, j0, kk, out_tets, out_tris, out_bends);
        for (int j = 0; j < kk; ++j) {
            double *i6 = info + (size_t)6 * (j0 + j);
            fill_solve_info(v.st[j], v.rr[j], i6);
            i6[4] = std::sqrt(g2); i6[5] = idt2;
        }
        block_info3[0] = std::max(block_info3[0], (double)v.iters); block_info3[1] += v.passes;
    }
    return ADMM_HIP_OK;
}

// a_j^T df/dX per rest vertex at x (host, or NULL = the device-resident state): one k_rest_sens pass per kSensCols columns
int admm_hip_rest_sensitivity(admm_hip_ctx *c, const double *x, int32_t k, const double *a, double *out) {
    if (!c || !a || !out || k < 1 || k > 65535) return fail(ADMM_HIP_ERR_ARG, "rest_sensitivity: NULL argument, k < 1 or k > 65535");
    if (int rc = mon_refuse(c, "rest_sensitivity")) return rc;
    if (int rc = rest_refuse(c, "rest_sensitivity")) return rc;
    const double *xd;
    if (int rc = eval_begin(c, "rest_sensitivity", x, &xd)) return rc;
    HIP_TRY(adjoint_ensure(c));
    HIP_TRY(rest_sens_ensure(c, std::min<int>(k, kSensCols)));
    hipStream_t st = c->stream;
    const size_t n3 = (size_t)c->n3;
    for (int j0 = 0; j0 < k; j0 += kSensCols) {
        const int kk = std::min<int>(kSensCols, k - j0);
        if (n3) HIP_TRY(hipMemcpyAsync(c->adj_a.p, a + (size_t)j0 * n3, (size_t)kk * n3 * sizeof(double), hipMemcpyHostToDevice, st));
        launch_rest_sens(c, xd, c->adj_a.p, kk);
        HIP_TRY(hipGetLastError());
        if (n3) HIP_TRY(hipMemcpyAsync(out + (size_t)j0 * n3, c->rs_out.p, (size_t)kk * n3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ADMM_HIP_OK;
}

// dL/dx of the held vertices for the multiplier lam of admm_hip_step_adjoint, at the device-resident state: one k_tangent pass on lam
// (the exact tangent, no mass shift, pins not masked), the pin mask, k_adj_held
int admm_hip_adjoint_held(admm_hip_ctx *c, const double *lam, const double *dL_dx, const double *dL_dv, double *out_held) {
    if (!c || !lam || !dL_dx || !out_held) return fail(ADMM_HIP_ERR_ARG, "adjoint_held: NULL argument");
    if (int rc = step_problem_begin(c, "adjoint_held", false)) return rc;      // (the rules of step_adjoint: lam is its multiplier)
    HIP_TRY(newton_ensure(c));
    HIP_TRY(adjoint_ensure(c));
    HIP_TRY(tangent_ensure(c, 1));
    hipStream_t st = c->stream;
    const size_t n3 = (size_t)c->n3, ld = std::max<size_t>(1, n3);
    if (!c->adj_h.p) HIP_TRY(c->adj_h.alloc_zeroed(ld, st));
    double *Lx = c->adj_l.p, *Lv = dL_dv ? c->adj_l.p + ld : nullptr;
    if (n3) {
        HIP_TRY(hipMemcpyAsync(c->k_d.p, lam, n3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Lx, dL_dx, n3 * sizeof(double), hipMemcpyHostToDevice, st));
        if (Lv) HIP_TRY(hipMemcpyAsync(Lv, dL_dv, n3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    launch_pin_mask(c);
    launch_tangent(c, c->x.p, 1, 0.0);
    hipLaunchKernelGGL(k_adj_held, dim3(nw_blocks(c)), dim3(256), 0, st, c->nv, Lx, Lv, 1.0 / c->dt, c->nw_pin.p, c->k_out.p, c->adj_h.p);
    HIP_TRY(hipGetLastError());
    if (n3) HIP_TRY(hipMemcpyAsync(out_held, c->adj_h.p, n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ADMM_HIP_OK;
}

int admm_hip_residuals(admm_hip_ctx *c, const double *x, const double *z, const double *z_prev, double *out4) {
    if (!c || !x || !z || !z_prev || !out4) return fail(ADMM_HIP_ERR_ARG, "residuals: NULL argument");
    if (int rc = mon_refuse(c, "residuals")) return rc;
    if (int rc = quiesce(c)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(mon_ensure(c, true, false));
    if (c->npin_terms && !c->mon_pz6.p) HIP_TRY(c->mon_pz6.alloc((size_t)6 * c->npin_terms));
    std::vector<double> tz, rz, pz, hz, tp, rp, pp, hp;
    rows_to_dev(c, z, tz, rz, pz, hz);
    rows_to_dev(c, z_prev, tp, rp, pp, hp);
    const size_t pin0 = 9 * (size_t)c->nt_total + 6 * (size_t)c->ntri_total + 3 * (size_t)c->nbend_total;      // the pins keep all six rows here
    HIP_TRY(hipMemcpyAsync(c->curr.p, x, c->n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->nt) { HIP_TRY(hipMemcpyAsync(c->t_z.p, tz.data(), tz.size() * sizeof(double), hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(c->mon_tzp.p, tp.data(), tp.size() * sizeof(double), hipMemcpyHostToDevice, st)); }
    if (c->ntri) { HIP_TRY(hipMemcpyAsync(c->r_z.p, rz.data(), rz.size() * sizeof(double), hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(c->mon_rzp.p, rp.data(), rp.size() * sizeof(double), hipMemcpyHostToDevice, st)); }
    if (c->nbend) { HIP_TRY(hipMemcpyAsync(c->h_z.p, hz.data(), hz.size() * sizeof(double), hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(c->mon_hzp.p, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, st)); }
    if (c->npin_terms) {
        HIP_TRY(hipMemcpyAsync(c->mon_pz6.p, z + pin0, (size_t)6 * c->npin_terms * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->mon_pzp.p, z_prev + pin0, (size_t)6 * c->npin_terms * sizeof(double), hipMemcpyHostToDevice, st));
    }
    MonArgs a = mon_args(c, c->curr.p, false);
    a.pin_dim = 6; a.pin_z = c->mon_pz6.p;
    launch_monitor<true, false>(c, a, c->mon_out.p);
    HIP_TRY(hipGetLastError());
    double h[kMonQ];
    HIP_TRY(hipMemcpyAsync(h, c->mon_out.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) out4[i] = std::sqrt(h[i]);
    return ADMM_HIP_OK;
}

int admm_hip_set_monitor(admm_hip_ctx *c, int32_t mode) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_monitor: NULL context");
    if (mode < 0 || mode > 3) return fail(ADMM_HIP_ERR_ARG, "set_monitor: mode must be 0 (off), 1 (residuals), 2 (residuals + objective) or 3 (2 + stationarity)");
    if (mode != 0) { if (int rc = mon_refuse(c, "set_monitor")) return rc; }
    c->mon_mode = mode;
    return ADMM_HIP_OK;
}

int admm_hip_get_monitor(admm_hip_ctx *c, int32_t cap, int32_t *n, double *records) {
    if (!c || !n || cap < 0 || (cap > 0 && !records)) return fail(ADMM_HIP_ERR_ARG, "get_monitor: bad argument");
    if (int rc = mon_refuse(c, "get_monitor")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;      // (a replayed step has rewritten its records)
    *n = c->mon_n;
    const int m = std::min((int)cap, c->mon_n);
    if (m <= 0) return ADMM_HIP_OK;
    std::vector<double> h((size_t)kMonQ * m);
    HIP_TRY(hipMemcpy(h.data(), c->mon_rec.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> hs((size_t)std::min(m, c->mon_stat_n));      // mode 3: the stationarity sums (forces.hpp)
    if (!hs.empty()) HIP_TRY(hipMemcpy(hs.data(), c->f_stat.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double half_idt2 = 0.5 / (c->dt * c->dt);
    for (int s = 0; s < m; ++s) {
        const double *q = h.data() + (size_t)kMonQ * s;
        double *r = records + 8 * (size_t)s;
        for (int i = 0; i < 4; ++i) r[i] = std::sqrt(q[i]);
        r[4] = (q[4] + q[5]) + q[6]; r[5] = half_idt2 * q[7]; r[6] = r[4] + r[5]; r[7] = (size_t)s < hs.size() ? std::sqrt(hs[s]) : 0.0;
    }
    return ADMM_HIP_OK;
}

// ---- early exit of the ADMM loop on the monitor's residuals (monitor.hpp: admm_stop_test, k_mon_decide; step_impl) ----
int admm_hip_set_admm_stop(admm_hip_ctx *c, double tol, int32_t min_iters) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_admm_stop: NULL context");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ADMM_HIP_ERR_ARG, "set_admm_stop: tol must be finite and >= 0 (0 = off)");
    if (min_iters < 1) return fail(ADMM_HIP_ERR_ARG, "set_admm_stop: min_iters must be >= 1");
    if (tol > 0.0) { if (int rc = mon_refuse(c, "set_admm_stop")) return rc; }
    c->stop_tol = tol; c->stop_min = min_iters;
    return ADMM_HIP_OK;
}

int admm_hip_get_admm_stop(admm_hip_ctx *c, double *tol, int32_t *min_iters, int32_t *last_iters, int32_t *on_device) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_admm_stop: NULL context");
    if (tol) *tol = c->stop_tol;
    if (min_iters) *min_iters = c->stop_min;
    if (last_iters || on_device) {      // (a step without early exit may still be running, and may yet be replayed)
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = settle(c)) return rc;
    }
    if (last_iters) *last_iters = c->stop_last;
    if (on_device) *on_device = c->stop_on_dev;
    return ADMM_HIP_OK;
}

// ---- Anderson acceleration of the ADMM loop (anderson.hpp; step_impl) ----
int admm_hip_set_anderson(admm_hip_ctx *c, int32_t window) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_anderson: NULL context");
    if (window < 0 || window > kAaMax) return fail(ADMM_HIP_ERR_ARG, "set_anderson: window must be 0 (off) .. 8");
    if (window > 0) {
        if (!monitor_allowed(c)) return fail(ADMM_HIP_ERR_ARG, "set_anderson: single-GPU contexts only (world_size > 1, a communicator or a caller all-reduce splits the state over ranks)");
        if (c->obst.n > 0 || !c->dyn.empty()) return fail(ADMM_HIP_ERR_ARG, "set_anderson: the context has colliders (obstacles or dynamic meshes); contact is not part of the accelerated fixed-point map");
        if (c->linsolver != 0) return fail(ADMM_HIP_ERR_ARG, "set_anderson: linsolver 1 and 2 are not supported (their inexact sweeps and multiplier updates are another fixed-point map); use linsolver 0");
    }
    c->aa_window = window;
    return ADMM_HIP_OK;
}

int admm_hip_get_anderson(admm_hip_ctx *c, int32_t cap, int32_t *n, double *records) {
    if (!c || !n || cap < 0 || (cap > 0 && !records)) return fail(ADMM_HIP_ERR_ARG, "get_anderson: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;      // (a replayed step has rewritten its records)
    *n = c->aa_n;
    const int m = std::min((int)cap, c->aa_n);
    if (m <= 0) return ADMM_HIP_OK;
    std::vector<double> h((size_t)kAaRec * m);
    HIP_TRY(hipMemcpy(h.data(), c->aa_rec.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < m; ++s) {
        const double *q = h.data() + (size_t)kAaRec * s;
        double *r = records + (size_t)kAaRec * s;
        for (int i = 0; i < kAaRec; ++i) r[i] = q[i];
        r[3] = std::sqrt(q[3]);
    }
    return ADMM_HIP_OK;
}

int admm_host_admm_stop_test(const double *rec8, double tol) { return (rec8 && admm_k::admm_stop_test(rec8, tol)) ? 1 : 0; }

// LinearSolver tuning members changed after Solver::initialize (the reference reads them on every solve: src/NodalMultiColorGS.hpp:40-46,100,
// src/UzawaCG.hpp:44-45,92).  Takes effect from the next solve; nothing is re-planned.
int admm_hip_set_solver_params(admm_hip_ctx *c, int32_t kind, int32_t max_iters, double tol, double omega) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_solver_params: NULL context");
    if (kind == ADMM_LS_NCMCGS) {
        if (c->linsolver != 1) return fail(ADMM_HIP_ERR_ARG, "set_solver_params: this context does not run the multi-colour GS");
        const int it0 = c->gs_max_iters; const double tol0 = c->gs_tol, om0 = c->gs_omega;
        if (max_iters > 0) c->gs_max_iters = max_iters;
        if (tol >= 0.0) c->gs_tol = tol;
        if (omega > 0.0) c->gs_omega = omega;
        if ((it0 != c->gs_max_iters || tol0 != c->gs_tol || om0 != c->gs_omega) && c->gs_exec) {   // the captured colour-kernel sequence holds the old values
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            (void)hipGraphExecDestroy(c->gs_exec); c->gs_exec = nullptr;
        }
        return ADMM_HIP_OK;
    }
    if (kind == ADMM_LS_UZAWACG) {
        if (c->linsolver != 2) return fail(ADMM_HIP_ERR_ARG, "set_solver_params: this context does not run UzawaCG");
        if (max_iters > 0) c->uz_max_iters = max_iters;
        if (tol > 0.0) c->uz_tol = tol;
        return ADMM_HIP_OK;
    }
    if (kind == ADMM_LS_LDLT_AS_PCG) {      // the PCG that stands for the prefactored solve (linsolver 0, and inside UzawaCG)
        if (c->linsolver == 1) return fail(ADMM_HIP_ERR_ARG, "set_solver_params: this context runs no PCG");
        if (max_iters > 0) c->pcg_max_iters = max_iters;
        if (tol > 0.0) c->pcg_tol = tol;
        return ADMM_HIP_OK;
    }
    return fail(ADMM_HIP_ERR_ARG, "set_solver_params: kind must be ADMM_LS_LDLT_AS_PCG, ADMM_LS_NCMCGS or ADMM_LS_UZAWACG");
}

int admm_hip_get_solver_params(const admm_hip_ctx *c, int32_t kind, int32_t *max_iters, double *tol, double *omega) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_solver_params: NULL context");
    int it; double t, o = 0.0;
    if (kind == ADMM_LS_NCMCGS) { it = c->gs_max_iters; t = c->gs_tol; o = c->gs_omega; }
    else if (kind == ADMM_LS_UZAWACG) { it = c->uz_max_iters; t = c->uz_tol; }
    else if (kind == ADMM_LS_LDLT_AS_PCG) { it = c->pcg_max_iters; t = c->pcg_tol; }
    else return fail(ADMM_HIP_ERR_ARG, "get_solver_params: unknown kind");
    if (max_iters) *max_iters = it;
    if (tol) *tol = t;
    if (omega) *omega = o;
    return ADMM_HIP_OK;
}

int admm_hip_set_soft_modes(admm_hip_ctx *c, int32_t k, const double *Z) {
    if (!c || k < 0 || k > kDeflMax || (k > 0 && !Z)) return fail(ADMM_HIP_ERR_ARG, "set_soft_modes: bad input (at most 64 modes)");
    if (c->linsolver == 1) return fail(ADMM_HIP_ERR_ARG, "set_soft_modes: this context runs no PCG");
    // (the distributed solve: every rank holds the whole x and the whole b after a solve -- x is assembled by the solve's last all-reduce, b by the
    // right-hand side's -- and the whole matrix; the Galerkin step on the modes is then the SAME replicated computation on every rank, k_defl_*)
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    c->defl_k = 0;
    if (k == 0) return ADMM_HIP_OK;
    const int nv = c->nv;
    std::vector<double> mass(c->n3);
    HIP_TRY(hipMemcpy(mass.data(), c->m.p, mass.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int v = 0; v < nv; ++v)
        if (mass[3 * (size_t)v] != mass[3 * (size_t)v + 1] || mass[3 * (size_t)v] != mass[3 * (size_t)v + 2]) return fail(ADMM_HIP_ERR_ARG, "set_soft_modes: needs per-vertex masses (A = K (x) I3)");
    // The fused epilogue of k_pcg2 keeps the modes in SINGLE precision (half the bytes of the step's two passes over them).  The step stays an
    // exact Galerkin step because everything below -- K Z, G = Z^T K Z, the copy the separate kernels use -- is formed from the ROUNDED vectors.
    std::vector<double> Zr;
    const bool want_fused = env_flag("ADMM_HIP_DEFL_FUSED", true) && c->oc_enabled && c->oc_plan && k <= kOc2DeflMax && !c->oc_orig_h.empty();
    if (want_fused) { Zr.assign(Z, Z + (size_t)k * nv); for (double &z : Zr) z = (double)(float)z; Z = Zr.data(); }
    // exact pairs: K Z on the host, G = Z^T K Z, its inverse
    std::vector<double> KZ((size_t)k * nv), G((size_t)k * k, 0.0);
    for (int q = 0; q < k; ++q)
        for (int v = 0; v < nv; ++v) {
            double acc = mass[3 * (size_t)v] * Z[(size_t)q * nv + v];
            for (int e = c->Ahat.rowptr[v]; e < c->Ahat.rowptr[v + 1]; ++e) acc += c->Ahat.val[e] * Z[(size_t)q * nv + c->Ahat.col[e]];
            if (!std::isfinite(acc)) return fail(ADMM_HIP_ERR_ARG, "set_soft_modes: non-finite mode");
            KZ[(size_t)q * nv + v] = acc;
        }
    for (int q = 0; q < k; ++q)
        for (int p = 0; p <= q; ++p) {
            double acc = 0.0;
            for (int v = 0; v < nv; ++v) acc += Z[(size_t)q * nv + v] * KZ[(size_t)p * nv + v];
            G[(size_t)q * k + p] = acc; G[(size_t)p * k + q] = acc;
        }
    {   // inverse of the SPD k x k matrix (Gauss-Jordan on the symmetric matrix, pivots checked)
        std::vector<double> a(G), inv((size_t)k * k, 0.0);
        for (int i = 0; i < k; ++i) inv[(size_t)i * k + i] = 1.0;
        for (int i = 0; i < k; ++i) {
            const double piv = a[(size_t)i * k + i];
            if (!(piv > 1e-14 * G[(size_t)i * k + i]) || !(piv > 0.0)) return fail(ADMM_HIP_ERR_ARG, "set_soft_modes: the modes are linearly dependent");
            for (int j = 0; j < k; ++j) { a[(size_t)i * k + j] /= piv; inv[(size_t)i * k + j] /= piv; }
            for (int r = 0; r < k; ++r) {
                if (r == i) continue;
                const double f = a[(size_t)r * k + i];
                if (f == 0.0) continue;
                for (int j = 0; j < k; ++j) { a[(size_t)r * k + j] -= f * a[(size_t)i * k + j]; inv[(size_t)r * k + j] -= f * inv[(size_t)i * k + j]; }
            }
        }
        G = inv;
    }
    HIP_TRY(c->defl_Z.upload(std::vector<double>(Z, Z + (size_t)k * nv)));
    HIP_TRY(c->defl_Ginv.upload(G));
    HIP_TRY(c->defl_part.alloc((size_t)3 * k * c->NB)); HIP_TRY(c->defl_y.alloc((size_t)3 * k));
    c->defl_fused = false;
    if (want_fused) {      // (ADMM_HIP_DEFL_FUSED=0: the separate k_defl_* launches, the A/B and the checker of the fused epilogue)
        std::vector<float> Zi((size_t)k * c->oc_rows, 0.0f);      // [mode][internal row] (pcg_onchip2.hpp)
        for (int q = 0; q < k; ++q)
            for (int r = 0; r < c->oc_rows; ++r) { const int v = c->oc_orig_h[r]; if (v >= 0) Zi[(size_t)q * c->oc_rows + r] = (float)Z[(size_t)q * nv + v]; }
        HIP_TRY(c->defl_Zint.upload(Zi));
        HIP_TRY(c->defl_rec.alloc((size_t)2 * 3 * kOc2DeflMax * c->oc_G)); HIP_TRY(c->defl_rec.zero());
        c->defl_fused = true;
    }
    c->defl_k = k;
    return ADMM_HIP_OK;
}

// The k lowest eigenvectors of K = diag(m) + Ahat by inverse subspace iteration on the context's own PCG (three right-hand sides per solve),
// Rayleigh-Ritz steps on the host; then admm_hip_set_soft_modes.  Deterministic (fixed start vectors).
int admm_hip_compute_soft_modes(admm_hip_ctx *c, int32_t k, int32_t iters) {
    if (!c || k < 0 || k > kDeflMax) return fail(ADMM_HIP_ERR_ARG, "compute_soft_modes: bad input (at most 64 modes)");
    if (k == 0) return admm_hip_set_soft_modes(c, 0, nullptr);
    if (c->linsolver == 1) return fail(ADMM_HIP_ERR_ARG, "compute_soft_modes: this context runs no PCG");
    // multi-rank contexts: the element-block partition replicates the solve (every rank computes the same modes from the same matrix with the
    // same deterministic code, no collective inside a solve), the component partition solves the rank's own bodies.  The DISTRIBUTED solve
    // (round 6): a COLLECTIVE call -- every rank runs the same inverse iteration on the same start vectors, each K^-1 X is one distributed solve
    // whose result every rank receives whole (the solve's closing all-reduce), the Rayleigh-Ritz steps are the same host arithmetic everywhere:
    // identical modes on every rank, no assembly step.
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    if (int rc = admm_hip_set_soft_modes(c, 0, nullptr)) return rc;
    // guard vectors: the wanted modes converge at the rate (lambda_k / lambda_k3)^iters -- half as many again, at least 12 (three more
    // than the wanted ones gave 3.8e-6 of drift and 9.0 iterations per solve on the bench body, 34 more 2.7e-6 and 7.1)
    const int nv = c->nv, k3 = std::min(nv, 3 * ((k + std::max(12, k / 2) + 2) / 3));
    if (k > nv) return fail(ADMM_HIP_ERR_ARG, "compute_soft_modes: more modes than vertices");
    if (iters <= 0) iters = 8;
    std::vector<double> mass(c->n3);
    HIP_TRY(hipMemcpy(mass.data(), c->m.p, mass.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> X((size_t)k3 * nv), Y((size_t)k3 * nv), KQ((size_t)k3 * nv), H((size_t)k3 * k3), V((size_t)k3 * k3), col3((size_t)c->n3);
    {   // deterministic start: a linear congruential sequence
        unsigned long long st = 0x9E3779B97F4A7C15ull;
        for (double &x : X) { st = st * 6364136223846793005ull + 1442695040888963407ull; x = (double)((st >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0 - 0.5; }
    }
    auto mgs = [&](std::vector<double> &A) -> bool {      // modified Gram-Schmidt on the k3 rows of length nv
        for (int i = 0; i < k3; ++i) {
            double *ai = &A[(size_t)i * nv];
            for (int j = 0; j < i; ++j) {
                const double *aj = &A[(size_t)j * nv];
                double d = 0.0;
                for (int v = 0; v < nv; ++v) d += ai[v] * aj[v];
                for (int v = 0; v < nv; ++v) ai[v] -= d * aj[v];
            }
            double n2 = 0.0;
            for (int v = 0; v < nv; ++v) n2 += ai[v] * ai[v];
            if (!(n2 > 0.0) || !std::isfinite(n2)) return false;
            const double il = 1.0 / std::sqrt(n2);
            for (int v = 0; v < nv; ++v) ai[v] *= il;
        }
        return true;
    };
    DevBuf<double> db, dx;
    HIP_TRY(db.alloc(c->n3)); HIP_TRY(dx.alloc(c->n3));
    int rcode = ADMM_HIP_OK;
    // The solves below are not the scene's: from the second round on their right-hand sides are (nearly) eigenvectors, CG ends after one or two steps
    // and runs on into rounding noise, where the recurrences' r . u can turn negative -- which k_pcg2 reads as "the preconditioner is not positive
    // definite" and answers by giving up its block smoother FOR THE CONTEXT (kCntSmootherOff).  Until round 6 that is what happened to every context
    // that computed its modes here: the bench body ran its ADMM loop with S = D^-1 (ADMM_HIP_OC_CHEB=0 and =2 gave the same 8.675 iterations per
    // solve).  What these solves find out about the context (kCntFindings) is put back on every way out, once the stream has drained.
    int found0[kCntFindingsLen] = {};
    HIP_TRY(hipMemcpy(found0, c->counters.p + kCntFindings, sizeof(found0), hipMemcpyDeviceToHost));
    struct PutBack {
        admm_hip_ctx *c; const int *w;
        hipError_t put() {
            const hipError_t e = hipStreamSynchronize(c->stream), e2 = hipMemcpy(c->counters.p + kCntFindings, w, kCntFindingsLen * sizeof(int), hipMemcpyHostToDevice);
            c = nullptr;
            return e != hipSuccess ? e : e2;
        }
        ~PutBack() { if (c) (void)put(); }
    } put_back{c, found0};
    for (int it = 0; it < iters && rcode == ADMM_HIP_OK; ++it) {
        if (!mgs(X)) { rcode = fail(ADMM_HIP_ERR_DEVICE, "compute_soft_modes: the subspace collapsed"); break; }
        for (int c0 = 0; c0 < k3 && rcode == ADMM_HIP_OK; c0 += 3) {      // Y = K^-1 X, three columns = the three axes of one solve
            for (int v = 0; v < nv; ++v) for (int j = 0; j < 3; ++j) col3[3 * (size_t)v + j] = c0 + j < k3 ? X[(size_t)(c0 + j) * nv + v] : 0.0;
            if (hipMemcpyAsync(db.p, col3.data(), col3.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipMemsetAsync(dx.p, 0, col3.size() * sizeof(double), c->stream) != hipSuccess) { rcode = fail(ADMM_HIP_ERR_DEVICE, "compute_soft_modes: copy failed"); break; }
            if (launch_pcg(c, db.p, dx.p, std::max(c->pcg_max_iters, 2000))) { rcode = fail(ADMM_HIP_ERR_DEVICE, "compute_soft_modes: the solve failed"); break; }
            if (hipMemcpyAsync(col3.data(), dx.p, col3.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { rcode = fail(ADMM_HIP_ERR_DEVICE, "compute_soft_modes: copy failed"); break; }
            if (c->h_sig && c->h_sig[kSigAbort]) { rcode = recover_from_abort(c, nullptr); if (rcode == ADMM_HIP_OK) { c0 -= 3; } continue; }
            for (int v = 0; v < nv; ++v) for (int j = 0; j < 3; ++j) if (c0 + j < k3) Y[(size_t)(c0 + j) * nv + v] = col3[3 * (size_t)v + j];
        }
        if (rcode != ADMM_HIP_OK) break;
        if (!mgs(Y)) { rcode = fail(ADMM_HIP_ERR_DEVICE, "compute_soft_modes: the subspace collapsed"); break; }
        for (int q = 0; q < k3; ++q)      // K Q on the host
            for (int v = 0; v < nv; ++v) {
                double acc = mass[3 * (size_t)v] * Y[(size_t)q * nv + v];
                for (int e = c->Ahat.rowptr[v]; e < c->Ahat.rowptr[v + 1]; ++e) acc += c->Ahat.val[e] * Y[(size_t)q * nv + c->Ahat.col[e]];
                KQ[(size_t)q * nv + v] = acc;
            }
        for (int p = 0; p < k3; ++p)
            for (int q = 0; q <= p; ++q) {
                double acc = 0.0;
                for (int v = 0; v < nv; ++v) acc += Y[(size_t)p * nv + v] * KQ[(size_t)q * nv + v];
                H[(size_t)p * k3 + q] = acc; H[(size_t)q * k3 + p] = acc;
            }
        // eigenvectors of the small symmetric matrix: cyclic Jacobi
        for (int i = 0; i < k3; ++i) for (int j = 0; j < k3; ++j) V[(size_t)i * k3 + j] = i == j ? 1.0 : 0.0;
        for (int sweep = 0; sweep < 60; ++sweep) {
            double off = 0.0, dg = 0.0;
            for (int i = 0; i < k3; ++i) for (int j = 0; j < k3; ++j) (i == j ? dg : off) += H[(size_t)i * k3 + j] * H[(size_t)i * k3 + j];
            if (off <= 1e-28 * dg) break;
            for (int p = 0; p < k3; ++p)
                for (int q = p + 1; q < k3; ++q) {
                    const double apq = H[(size_t)p * k3 + q];
                    if (apq == 0.0) continue;
                    const double th = (H[(size_t)q * k3 + q] - H[(size_t)p * k3 + p]) / (2.0 * apq);
                    const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0)), cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                    for (int r = 0; r < k3; ++r) { const double a = H[(size_t)r * k3 + p], b2 = H[(size_t)r * k3 + q]; H[(size_t)r * k3 + p] = cs * a - sn * b2; H[(size_t)r * k3 + q] = sn * a + cs * b2; }
                    for (int r = 0; r < k3; ++r) { const double a = H[(size_t)p * k3 + r], b2 = H[(size_t)q * k3 + r]; H[(size_t)p * k3 + r] = cs * a - sn * b2; H[(size_t)q * k3 + r] = sn * a + cs * b2; }
                    for (int r = 0; r < k3; ++r) { const double a = V[(size_t)r * k3 + p], b2 = V[(size_t)r * k3 + q]; V[(size_t)r * k3 + p] = cs * a - sn * b2; V[(size_t)r * k3 + q] = sn * a + cs * b2; }
                }
        }
        std::vector<int> ord(k3);
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b2) { return H[(size_t)a * k3 + a] < H[(size_t)b2 * k3 + b2]; });
        for (int q = 0; q < k3; ++q) {      // X = Q V, columns by ascending Ritz value
            double *xq = &X[(size_t)q * nv];
            std::fill(xq, xq + nv, 0.0);
            for (int p = 0; p < k3; ++p) {
                const double w = V[(size_t)p * k3 + ord[q]];
                const double *yp = &Y[(size_t)p * nv];
                for (int v = 0; v < nv; ++v) xq[v] += w * yp[v];
            }
        }
    }
    HIP_TRY(put_back.put());
    if (rcode != ADMM_HIP_OK) return rcode;
    c->rc_iter = 0; c->rc_prev_valid = 0; c->rc_prev2_valid = 0;      // (the recycled basis of the ADMM loop starts clean)
    return admm_hip_set_soft_modes(c, k, X.data());
}

int admm_hip_get_soft_modes(admm_hip_ctx *c, int32_t *k, double *Z) {
    if (!c || !k) return fail(ADMM_HIP_ERR_ARG, "get_soft_modes: NULL argument");
    *k = c->defl_k;
    if (Z && c->defl_k > 0) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(Z, c->defl_Z.p, (size_t)c->defl_k * c->nv * sizeof(double), hipMemcpyDeviceToHost));
    }
    return ADMM_HIP_OK;
}

int admm_hip_contact_totals(admm_hip_ctx *c, int64_t *rows) {
    if (!c || !rows) return fail(ADMM_HIP_ERR_ARG, "contact_totals: NULL argument");
    *rows = 0;
    if (c->linsolver == 2) { *rows = c->uz_rows_total; return ADMM_HIP_OK; }
    if (c->linsolver == 1 && c->gs_proj.p) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = settle(c)) return rc;
        unsigned long long h = 0;
        HIP_TRY(hipMemcpy(&h, c->gs_proj.p, sizeof(h), hipMemcpyDeviceToHost));
        *rows = (int64_t)h;
    }
    return ADMM_HIP_OK;
}

int admm_hip_persistent_launches(const admm_hip_ctx *c, int64_t *pcg, int64_t *gs, int64_t *schur) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "persistent_launches: NULL context");
    if (pcg) *pcg = c->oc_launches;
    if (gs) *gs = c->gsp_launches;
    if (schur) *schur = c->uzp_launches;
    return ADMM_HIP_OK;
}

int admm_hip_pcg_plan_info(const admm_hip_ctx *c, int64_t *out) {
    if (!c || !out) return fail(ADMM_HIP_ERR_ARG, "pcg_plan_info: NULL argument");
    const bool planned = c->oc_plan && c->oc_G > 0;      // (a plan the device accepted: oc_G is set behind the occupancy check)
    out[0] = c->oc_enabled ? 1 : 0;
    out[1] = planned ? c->oc_G : 0; out[2] = planned ? c->oc_spb : 0; out[3] = planned ? c->oc_T : 0;
    out[4] = planned && c->oc_coarse ? 1 : 0;
    out[5] = c->oc_nbr.p ? 1 : 0;
    out[6] = planned ? c->oc_nbr_max : 0;
    out[7] = c->oc_gave_up ? 1 : 0;
    return ADMM_HIP_OK;
}

int admm_hip_pcg_findings(admm_hip_ctx *c, int32_t *smoother_given_up, int32_t *trust_revoked, int64_t *failed_checks) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "pcg_findings: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int h[kCntFindingsLen] = {};
    HIP_TRY(hipMemcpy(h, c->counters.p + kCntFindings, sizeof(h), hipMemcpyDeviceToHost));
    if (smoother_given_up) *smoother_given_up = h[0] != 0;
    if (trust_revoked) *trust_revoked = h[1] != 0;
    if (failed_checks) *failed_checks = h[2];
    return ADMM_HIP_OK;
}

int admm_hip_device_buffers(int64_t *buffers, int64_t *bytes) {
    if (buffers) *buffers = g_dev_buffers;
    if (bytes) *bytes = g_dev_bytes;
    return ADMM_HIP_OK;
}
int admm_hip_probe_sync(admm_hip_ctx *c, int32_t n, double *us_all_to_all, double *us_exchange, int64_t *plan_stats) {
    if (!c || n < 1) return fail(ADMM_HIP_ERR_ARG, "probe_sync: bad input");
    if (us_all_to_all) *us_all_to_all = 0.0;
    if (us_exchange) *us_exchange = 0.0;
    if (plan_stats) for (int i = 0; i < 6; ++i) plan_stats[i] = c->oc_stat[i];
    if (!c->oc_enabled || !c->oc_plan || !c->oc_nbr.p) return ADMM_HIP_OK;    // no on-chip plan: nothing to probe
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(st));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    double out[2] = {0.0, 0.0};
    for (int slot = 0; slot < 2; ++slot) {
        const int mode = slot;
        Oc2Args a{};
        a.n_rows = c->oc_rows; a.halo_ptr = c->oc_haloptr.p; a.halo_src = c->oc_halosrc.p; a.vec_len = c->oc_veclen;
        a.ubuf = c->oc_ubuf.p; a.part = c->oc_part.p; a.bar = c->oc_bar.p; a.nbr = c->oc_nbr.p; a.flags = c->oc_flags.p;
        a.sig = c->d_sig; a.spb = c->oc_spb; a.G = c->oc_G;
        for (int rep = 0; rep < 2; ++rep) {     // first launch warms up
            a.seq = ++c->solve_seq;
            HIP_TRY(hipEventRecord(e0, st));
            if (c->oc_T <= 768) hipLaunchKernelGGL((k_sync_probe<768>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a, (int)n, mode, (double *)nullptr);
            else hipLaunchKernelGGL((k_sync_probe<1024>), dim3(c->oc_G), dim3(c->oc_T), c->oc_lds, st, a, (int)n, mode, (double *)nullptr);
            HIP_TRY(hipEventRecord(e1, st));
            HIP_TRY(hipEventSynchronize(e1));
        }
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        out[slot] = 1e3 * (double)ms / (double)n;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (c->h_sig && c->h_sig[kSigAbort]) { c->h_sig[kSigAbort] = 0; return fail(ADMM_HIP_ERR_DEVICE, "probe_sync: a grid barrier timed out"); }
    if (us_all_to_all) *us_all_to_all = out[0];
    if (us_exchange) *us_exchange = out[1];
    return ADMM_HIP_OK;
}

int admm_hip_time_local_launches(admm_hip_ctx *c, int32_t on) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "time_local_launches: NULL context");
    c->lt_on = on != 0;
    c->lt_mode = on == 2 ? 2 : 1;
    return ADMM_HIP_OK;
}

int admm_hip_local_launch_times(admm_hip_ctx *c, int64_t *n_pairs, double *sum_ms) {
    if (!c || !n_pairs || !sum_ms) return fail(ADMM_HIP_ERR_ARG, "local_launch_times: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = settle(c)) return rc;
    double sum = 0.0;
    for (size_t i = 0; i + 1 < c->lt_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->lt_ev[i], c->lt_ev[i + 1]));
        sum += ms;
    }
    *n_pairs = (int64_t)(c->lt_used / 2); *sum_ms = sum;
    c->lt_used = 0;
    return ADMM_HIP_OK;
}

int admm_hip_get_matrix(const admm_hip_ctx *c, int32_t *rowptr, int32_t *col, double *val, int32_t *nnz) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_matrix: NULL context");
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, "get_matrix: this context holds only its rank's bodies (admm_host_assemble_matrix gives the whole matrix)");
    if (nnz) *nnz = (int32_t)c->Ahat.col.size();
    if (rowptr) std::copy(c->Ahat.rowptr.begin(), c->Ahat.rowptr.end(), rowptr);
    if (col) std::copy(c->Ahat.col.begin(), c->Ahat.col.end(), col);
    if (val) std::copy(c->Ahat.val.begin(), c->Ahat.val.end(), val);
    return ADMM_HIP_OK;
}

int admm_hip_get_colors(const admm_hip_ctx *c, int32_t *color, int32_t *n_colors) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "get_colors: NULL context");
    if (c->linsolver != 1) return fail(ADMM_HIP_ERR_STATE, "get_colors: context was not created with linsolver 1");
    if (n_colors) *n_colors = c->n_colors;
    if (color) std::copy(c->color_h.begin(), c->color_h.end(), color);
    return ADMM_HIP_OK;
}

int admm_hip_comm_unique_id(char *id128) {
    if (!id128) return fail(ADMM_HIP_ERR_ARG, "comm_unique_id: NULL buffer");
    if (!g_rccl.load()) return fail(ADMM_HIP_ERR_COMM, "cannot load librccl");
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(ADMM_HIP_ERR_COMM, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof(id));
    return ADMM_HIP_OK;
}

int admm_hip_comm_init(admm_hip_ctx *c, const char *id128, int rank, int world_size) {
    if (!c || !id128) return fail(ADMM_HIP_ERR_ARG, "comm_init: NULL argument");
    if (c->cm.on) {     // component partition: the communicator only merges the ranks' parts in admm_hip_get_state
        if (rank != c->cm.rank || world_size != c->cm.world) return fail(ADMM_HIP_ERR_ARG, "comm_init: rank/world_size differ from the ones the context was created with");
        if (!g_rccl.load()) return fail(ADMM_HIP_ERR_COMM, "cannot load librccl");
        HIP_TRY(hipSetDevice(c->device));
        ncclUniqueId idc;
        std::memcpy(&idc, id128, sizeof(idc));
        ncclResult_t rr = g_rccl.CommInitRank(&c->cm_comm, world_size, idc, rank);
        if (rr != ncclSuccess) return fail(ADMM_HIP_ERR_COMM, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(rr));
        return ADMM_HIP_OK;
    }
    if (rank != c->rank || world_size != c->world)
        return fail(ADMM_HIP_ERR_ARG, "comm_init: rank/world_size differ from the ones the context was created with");
    // a world of one needs no communicator; ADMM_HIP_FORCE_COMM=1 builds (and uses) one anyway so that the RCCL
    // binding, the in-place all-reduce on the context's stream and its ordering against the persistent PCG kernel
    // can be exercised on a single GPU (tests/test_multi_gpu.py)
    if (c->world <= 1 && !env_flag("ADMM_HIP_FORCE_COMM", false)) return ADMM_HIP_OK;
    if (!g_rccl.load()) return fail(ADMM_HIP_ERR_COMM, "cannot load librccl");
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world_size, id, rank);
    if (r != ncclSuccess) return fail(ADMM_HIP_ERR_COMM, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
    return ADMM_HIP_OK;
}

int admm_hip_comm_info(const admm_hip_ctx *c, int32_t *n_ranks, int32_t *rank, char *device_id64) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "comm_info: NULL context");
    ncclComm_t cm = c->comm ? c->comm : c->cm_comm;
    int n = 0, r = -1;
    if (cm && g_rccl.CommCount && g_rccl.CommUserRank) {      // asked of RCCL itself, not echoed from the arguments of comm_init
        if (g_rccl.CommCount(cm, &n) != ncclSuccess || g_rccl.CommUserRank(cm, &r) != ncclSuccess) return fail(ADMM_HIP_ERR_COMM, "comm_info: ncclCommCount / ncclCommUserRank failed");
    }
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    if (device_id64) {
        device_id64[0] = 0;
        hipUUID u;
        char bus[32] = {0};
        (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), c->device);
        std::string sid = "pci ";
        sid += bus;
        if (hipDeviceGetUuid(&u, c->device) == hipSuccess) {
            char hex[40]; int k = 0;
            for (int i = 0; i < 16 && k < 38; ++i) k += snprintf(hex + k, sizeof(hex) - k, "%02x", (unsigned)(unsigned char)u.bytes[i]);
            sid += " uuid "; sid += hex;
        }
        (void)hipGetLastError();
        std::strncpy(device_id64, sid.c_str(), 63); device_id64[63] = 0;
    }
    return ADMM_HIP_OK;
}

int admm_hip_set_rhs_allreduce(admm_hip_ctx *c, admm_allreduce_fn fn, void *user) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "set_rhs_allreduce: NULL context");
    if (c->cm.on) return fail(ADMM_HIP_ERR_STATE, "set_rhs_allreduce: the component partition exchanges nothing inside a step");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fn && !c->ar_host) HIP_TRY(hipHostMalloc((void **)&c->ar_host, (size_t)c->n3 * sizeof(double), hipHostMallocDefault));
    c->ar_fn = fn; c->ar_user = user;
    return ADMM_HIP_OK;
}

// ---- host-only entry points ----
int admm_host_assemble_matrix(const admm_hip_desc *d, int32_t *rowptr, int32_t *col, double *val, int32_t *nnz) {
    int rc = validate(d);
    if (rc) return rc;
    const double dt = d->dt > 0.0 ? d->dt : 1.0 / 24.0;
    double mu, la, k;
    admm_host::lame(10000000.0, 0.499, &mu, &la, &k);
    const double pw = d->pin_weight > 0 ? d->pin_weight : std::sqrt(k * 2.0);
    const bool pins_as_terms = (d->linsolver == 0 || d->linsolver == 2);
    admm_host::Csr A = admm_host::assemble_Ahat(d->n_verts, dt, d->n_tets, d->tet_idx, d->tet_Binv, d->tet_weight, d->n_tris,
                                                d->tri_idx, d->tri_rest, d->tri_weight, pins_as_terms ? d->n_pins : 0, d->pin_vert, pw);
    if (d->n_bends > 0) A = admm_host::add_stencil_terms(A, dt, d->n_bends, d->bend_idx, d->bend_coef, d->bend_weight);
    if (nnz) *nnz = (int32_t)A.col.size();
    if (rowptr) std::copy(A.rowptr.begin(), A.rowptr.end(), rowptr);
    if (col) std::copy(A.col.begin(), A.col.end(), col);
    if (val) std::copy(A.val.begin(), A.val.end(), val);
    return ADMM_HIP_OK;
}
// the plan admm_hip_create would make for this description (admm_host_oc_plan, admm_host_oc_plan_halo)
static int host_oc_plan_of(const admm_hip_desc *d, int32_t n_blocks, int32_t spb, int32_t lds_bytes, bool want_coarse, admm_host::OcPlan &P) {
    int rc = validate(d);
    if (rc) return rc;
    if (n_blocks < 1 || spb < 1 || spb > 16 || (int64_t)n_blocks * spb * 64 < d->n_verts) return fail(ADMM_HIP_ERR_ARG, "oc_plan: blocks x slices do not hold the vertices");
    const double dt = d->dt > 0.0 ? d->dt : 1.0 / 24.0;
    double mu, la, k;
    admm_host::lame(10000000.0, 0.499, &mu, &la, &k);
    const double pw = d->pin_weight > 0 ? d->pin_weight : std::sqrt(k * 2.0);
    const bool pins_as_terms = (d->linsolver == 0 || d->linsolver == 2);
    admm_host::Csr A = admm_host::assemble_Ahat(d->n_verts, dt, d->n_tets, d->tet_idx, d->tet_Binv, d->tet_weight, d->n_tris,
                                                      d->tri_idx, d->tri_rest, d->tri_weight, pins_as_terms ? d->n_pins : 0, d->pin_vert, pw);
    if (d->n_bends > 0) A = admm_host::add_stencil_terms(A, dt, d->n_bends, d->bend_idx, d->bend_coef, d->bend_weight);      // (the matrix admm_hip_create plans for)
    P = admm_host::build_oc_plan(A, d->masses, n_blocks, spb, lds_bytes, want_coarse, d->vert_xyz);
    if (!P.ok) return fail(ADMM_HIP_ERR_ARG, "oc_plan: a block does not fit its slots");
    return ADMM_HIP_OK;
}
int admm_host_oc_plan_halo(const admm_hip_desc *d, int32_t n_blocks, int32_t spb, int32_t lds_bytes, int32_t *halo_ptr, int32_t *halo_src, int32_t *halo_vert) {
    if (!halo_ptr) return fail(ADMM_HIP_ERR_ARG, "oc_plan_halo: halo_ptr is NULL");
    admm_host::OcPlan P;
    const int rc = host_oc_plan_of(d, n_blocks, spb, lds_bytes, false, P);
    if (rc) return rc;
    std::copy(P.halo_ptr.begin(), P.halo_ptr.end(), halo_ptr);
    if (halo_src) std::copy(P.halo_src.begin(), P.halo_src.end(), halo_src);
    if (halo_vert) std::copy(P.halo_vert.begin(), P.halo_vert.end(), halo_vert);
    return ADMM_HIP_OK;
}
int admm_host_oc_plan(const admm_hip_desc *d, int32_t n_blocks, int32_t spb, int32_t lds_bytes, int32_t *row_vertex,
                      int32_t *row_aggregate, double *coarse_inv, int64_t *stats, float *row_weights) {
    admm_host::OcPlan P;
    const int rc = host_oc_plan_of(d, n_blocks, spb, lds_bytes, coarse_inv != nullptr, P);
    if (rc) return rc;
    if (row_vertex) std::copy(P.orig.begin(), P.orig.end(), row_vertex);
    if (row_weights) std::copy(P.cwt.begin(), P.cwt.end(), row_weights);
    if (row_aggregate)
        for (int32_t r = 0; r < P.n_rows; ++r)
            row_aggregate[r] = P.orig[r] < 0 ? -1 : (r / (64 * spb)) * admm_host::kOcSub + P.row_agg[r];
    if (coarse_inv) {
        if (!P.coarse_ok) return fail(ADMM_HIP_ERR_ARG, "oc_plan: no coarse space (masses differ between the axes, or too many blocks)");
        for (int i = 0; i < P.nc; ++i) std::copy(P.ainv.begin() + (size_t)i * P.ncp, P.ainv.begin() + (size_t)i * P.ncp + P.nc, coarse_inv + (size_t)i * P.nc);
    }
    if (stats) {
        stats[0] = P.stat_nnz; stats[1] = P.stat_stored; stats[2] = P.stat_onchip; stats[3] = P.stat_local;
        stats[4] = P.nbr_ok ? P.nbr_max : -1; stats[5] = P.coarse_ok ? P.nc : 0; stats[6] = P.nh_max; stats[7] = P.bcols;
        stats[8] = (int64_t)llround(1e9 * P.lam_bb); stats[9] = (int64_t)llround(1e6 * P.stat_bank_sorted); stats[10] = (int64_t)llround(1e6 * P.stat_bank_placed);
    }
    return ADMM_HIP_OK;
}
int admm_host_big_plan(const admm_hip_desc *d, int32_t max_aggregates, int32_t *stats, int32_t *row_vertex, double *row_weights, float *coarse_inv) {
    int rc = validate(d);
    if (rc) return rc;
    if (!stats) return fail(ADMM_HIP_ERR_ARG, "big_plan: stats is NULL");
    const double dt = d->dt > 0.0 ? d->dt : 1.0 / 24.0;
    double mu, la, k;
    admm_host::lame(10000000.0, 0.499, &mu, &la, &k);
    const double pw = d->pin_weight > 0 ? d->pin_weight : std::sqrt(k * 2.0);
    const bool pins_as_terms = (d->linsolver == 0 || d->linsolver == 2);
    admm_host::Csr A = admm_host::assemble_Ahat(d->n_verts, dt, d->n_tets, d->tet_idx, d->tet_Binv, d->tet_weight, d->n_tris,
                                                d->tri_idx, d->tri_rest, d->tri_weight, pins_as_terms ? d->n_pins : 0, d->pin_vert, pw);
    if (d->n_bends > 0) A = admm_host::add_stencil_terms(A, dt, d->n_bends, d->bend_idx, d->bend_coef, d->bend_weight);      // (the matrix admm_hip_create plans for)
    const admm_host::BigPlan P = admm_host::build_big_plan(A, d->masses, d->vert_xyz, max_aggregates > 0 ? max_aggregates : 1024);
    if (!P.ok) return fail(ADMM_HIP_ERR_ARG, "big_plan: no plan (masses differ between the axes of a vertex)");
    stats[0] = P.G; stats[1] = P.ra; stats[2] = P.n_rows; stats[3] = P.nc; stats[4] = P.ncp; stats[5] = P.A.n_slices;
    if (row_vertex) std::copy(P.orig.begin(), P.orig.end(), row_vertex);
    if (row_weights) std::copy(P.cwt.begin(), P.cwt.end(), row_weights);
    if (coarse_inv) for (int i = 0; i < P.nc; ++i) std::copy(P.ainv.begin() + (size_t)i * P.ncp, P.ainv.begin() + (size_t)i * P.ncp + P.nc, coarse_inv + (size_t)i * P.nc);
    return ADMM_HIP_OK;
}
int admm_host_gs_plan_sweeps(const admm_hip_desc *d, int32_t n_colors, const int32_t *color, int32_t max_blocks, int32_t rows_target,
                             const double *b, double *x, int32_t sweeps, double omega, int32_t *stats) {
    int rc = validate(d);
    if (rc) return rc;
    if (!color || !b || !x || sweeps < 0) return fail(ADMM_HIP_ERR_ARG, "gs_plan_sweeps: NULL argument");
    const double dt = d->dt > 0.0 ? d->dt : 1.0 / 24.0;
    admm_host::Csr A = admm_host::assemble_Ahat(d->n_verts, dt, d->n_tets, d->tet_idx, d->tet_Binv, d->tet_weight, d->n_tris,
                                                d->tri_idx, d->tri_rest, d->tri_weight, 0, d->pin_vert, 0.0);
    if (d->n_bends > 0) A = admm_host::add_stencil_terms(A, dt, d->n_bends, d->bend_idx, d->bend_coef, d->bend_weight);      // (the matrix admm_hip_create plans for)
    const admm_host::GsPlan P = admm_host::build_gs_plan(A, n_colors, color, max_blocks > 0 ? max_blocks : 256, rows_target > 0 ? rows_target : kGspRowsTarget, 160 * 1024);
    if (!P.ok) return fail(ADMM_HIP_ERR_ARG, "gs_plan_sweeps: no plan (too many colours, or a block does not fit the LDS)");
    const int G = P.G, C = P.C, H = admm_host::kGspHdr;
    if (stats) { stats[0] = G; stats[1] = C; stats[2] = P.lds_bytes; stats[3] = P.max_halo; stats[4] = P.max_nbr; stats[5] = P.max_rows; }
    // the kernel's data flow on the host: per block a local vector (own rows, then halo entries), per phase fetch the halo entries of the
    // colour swept in the previous phase from the outbox, sweep the rows of this phase's colour out of the ELL with LOCAL columns, publish
    // the boundary rows.  All blocks finish a phase before the next one starts (the kernel's hand-offs enforce exactly that order).
    std::vector<double> box((size_t)3 * std::max(P.ob_total, 1), 0.0);
    std::vector<std::vector<double> > xl(G);
    for (int g = 0; g < G; ++g) {
        const int32_t *h = &P.hdr[(size_t)g * H];
        xl[g].assign((size_t)3 * (h[0] + h[1]), 0.0);
        for (int i = 0; i < h[0]; ++i) for (int q = 0; q < 3; ++q) xl[g][3 * i + q] = x[3 * (size_t)P.orig[h[2] + i] + q];
        for (int i = 0; i < h[1]; ++i) for (int q = 0; q < 3; ++q) xl[g][3 * (h[0] + i) + q] = x[3 * (size_t)P.halo_orig[h[3] + i] + q];
    }
    auto fetch = [&](int cp) {
        for (int g = 0; g < G; ++g) {
            const int32_t *h = &P.hdr[(size_t)g * H];
            for (int hh = h[21 + cp]; hh < h[21 + cp + 1]; ++hh)
                for (int q = 0; q < 3; ++q) xl[g][3 * (h[0] + hh) + q] = box[3 * (size_t)P.halo_box[h[3] + hh] + q];
        }
    };
    for (int sw = 0; sw < sweeps; ++sw)
        for (int c = 0; c < C; ++c) {
            if (sw > 0 || c > 0) fetch(c > 0 ? c - 1 : C - 1);
            for (int g = 0; g < G; ++g) {
                const int32_t *h = &P.hdr[(size_t)g * H];
                const int r0 = h[8 + c], n_c = h[8 + c + 1] - r0, W = h[34 + c];
                const size_t e0 = (size_t)h[4] + h[46 + c];
                std::vector<double> nx((size_t)3 * std::max(n_c, 1));
                for (int i = 0; i < n_c; ++i) {
                    double acc[3] = {0.0, 0.0, 0.0};
                    for (int k = 0; k < W; ++k) {
                        const int col = P.cols[e0 + (size_t)k * n_c + i] & 0x7fff;
                        const double a = P.vals[e0 + (size_t)k * n_c + i];
                        for (int q = 0; q < 3; ++q) acc[q] = std::fma(a, xl[g][3 * col + q], acc[q]);
                    }
                    const int li = r0 + i, v = P.orig[h[2] + li];
                    for (int q = 0; q < 3; ++q) {
                        const double aii = P.diag[h[2] + li] + d->masses[3 * (size_t)v + q];
                        const double jac = (b[3 * (size_t)v + q] - acc[q]) * (1.0 / aii);
                        nx[3 * i + q] = std::fma(omega, jac, (1.0 - omega) * xl[g][3 * li + q]);
                    }
                }
                for (int i = 0; i < n_c; ++i) {
                    const int li = r0 + i, o = P.out_idx[h[2] + li];
                    for (int q = 0; q < 3; ++q) {
                        xl[g][3 * li + q] = nx[3 * i + q];
                        if (o >= 0) box[3 * (size_t)(h[5] + o) + q] = nx[3 * i + q];
                    }
                }
            }
        }
    for (int g = 0; g < G; ++g) {
        const int32_t *h = &P.hdr[(size_t)g * H];
        for (int i = 0; i < h[0]; ++i) for (int q = 0; q < 3; ++q) x[3 * (size_t)P.orig[h[2] + i] + q] = xl[g][3 * i + q];
    }
    return ADMM_HIP_OK;
}
void admm_host_partition(int32_t n_items, int world_size, int rank, int32_t *begin, int32_t *end) {
    admm_host::partition(n_items, world_size, rank, begin, end);
}
int32_t admm_host_component_partition(const admm_hip_desc *d, int world_size, int32_t *vertex_rank) {
    if (!d || !vertex_rank || d->n_verts < 1) return -1;
    return admm_host::component_partition(d->n_verts, d->n_tets, d->tet_idx, d->n_tris, d->tri_idx, std::max(world_size, 1), vertex_rank, d->n_bends, d->bend_idx);
}
int admm_host_tabulate_spline(admm_spline_fn fn, void *user, double s_min, double s_max, double *table_out) {
    const int r = admm_host::tabulate_spline(fn, user, s_min, s_max, table_out);
    if (r == -1) return fail(ADMM_HIP_ERR_ARG, "tabulate_spline: need a function, a table and 0 < s_min < s_max");
    if (r == -2) return fail(ADMM_HIP_ERR_ARG, "tabulate_spline: the spline returned a non-finite value inside [s_min, s_max] (and their products)");
    return ADMM_HIP_OK;
}
void admm_host_spline_table_eval(const double *table, int which, double x, double *out3) { admm_host::spline_table_eval(table, which, x, out3); }
int admm_host_tet_rest_positions(int32_t n_verts, int32_t n_tets, const int32_t *idx, const double *Binv, const double *candidate, double *x0_out) {
    if (n_verts <= 0 || n_tets < 0 || !idx || !Binv || !x0_out) return -1;
    return admm_host::tet_rest_positions(n_verts, n_tets, idx, Binv, candidate, x0_out);
}
int admm_hip_uzawa_cache_stats(admm_hip_ctx *c, int64_t *columns, int64_t *column_solves, int64_t *schur_from_columns, int64_t *schur_by_pcg,
                               int64_t *evicted) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "uzawa_cache_stats: NULL context");
    if (columns) {
        *columns = -1;
        if (c->uzc_on) { int64_t n = 0; for (int s : c->uzc_slot_h) n += s >= 0 ? 1 : 0; *columns = n; }
    }
    if (column_solves) *column_solves = c->uzc_col_solves;
    if (schur_from_columns) {
        int dev = 0;      // the persistent Schur launches count on the device
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&dev, c->counters.p + kCntSchurProducts, sizeof(int), hipMemcpyDeviceToHost));
        *schur_from_columns = c->uzc_applies + dev;
    }
    if (schur_by_pcg) *schur_by_pcg = c->uzc_pcg_solves;
    if (evicted) *evicted = c->uzc_evictions;
    return ADMM_HIP_OK;
}
int admm_hip_uzawa_column_lanes(admm_hip_ctx *c, int64_t *batches, int *lanes, int64_t *ahead_columns, int64_t *ahead_waits) {
    if (!c) return fail(ADMM_HIP_ERR_ARG, "uzawa_column_lanes: NULL context");
    if (batches) *batches = c->uzc_lane_batches;
    if (lanes) *lanes = (int)c->uz_lanes.size();
    if (ahead_columns) *ahead_columns = c->pf_columns;
    if (ahead_waits) *ahead_waits = c->pf_waits;
    return ADMM_HIP_OK;
}
int admm_hip_uzawa_unconverged_columns(admm_hip_ctx *c, int64_t *n) {
    if (!c || !n) return fail(ADMM_HIP_ERR_ARG, "uzawa_unconverged_columns: NULL argument");
    *n = c->uzc_unconverged;
    return ADMM_HIP_OK;
}
int admm_host_sample_obstacle(admm_obstacle_fn fn, void *user, const double *lo, const double *hi, const int32_t *dims, double *meta, double *data) {
    if (!fn || !lo || !hi || !dims || !meta || !data) return fail(ADMM_HIP_ERR_ARG, "sample_obstacle: NULL argument");
    for (int a = 0; a < 3; ++a) if (dims[a] < 2 || !(hi[a] > lo[a])) return fail(ADMM_HIP_ERR_ARG, "sample_obstacle: need hi > lo and at least two nodes per axis");
    for (int a = 0; a < 3; ++a) { meta[a] = lo[a]; meta[3 + a] = (hi[a] - lo[a]) / (double)(dims[a] - 1); meta[6 + a] = (double)dims[a]; }
    meta[9] = 0.0;
    size_t node = 0;
    for (int k = 0; k < dims[2]; ++k)
        for (int j = 0; j < dims[1]; ++j)
            for (int i = 0; i < dims[0]; ++i, ++node) {
                const double x[3] = {lo[0] + meta[3] * i, lo[1] + meta[4] * j, lo[2] + meta[5] * k};
                double out[7] = {0, 0, 0, 0, 0, 0, 0};
                fn(user, x, out);
                for (int q = 0; q < 7; ++q) if (!std::isfinite(out[q])) return fail(ADMM_HIP_ERR_ARG, "sample_obstacle: the object returned a non-finite value inside the box");
                data[4 * node] = out[0]; data[4 * node + 1] = out[4]; data[4 * node + 2] = out[5]; data[4 * node + 3] = out[6];
            }
    return ADMM_HIP_OK;
}
int admm_hip_tet_rest_mode(const admm_hip_ctx *c) { return c ? c->tet_rest_mode : -1; }
int admm_host_tet_rest(int32_t n, const int32_t *idx, const double *verts, double *Binv, double *vol) {
    int r = admm_host::tet_rest(n, idx, verts, Binv, vol);
    if (r) return fail(ADMM_HIP_ERR_GEOMETRY, "TetEnergyTerm Error: Inverted initial tet " + std::to_string(-r - 1));
    return ADMM_HIP_OK;
}
int32_t admm_host_bend_hinges(int32_t n_verts, int32_t n_tris, const int32_t *tris, const double *verts, int32_t cap, int32_t *hinge_idx, double *coef, double *area) {
    if (n_verts < 0 || n_tris < 0 || (n_tris > 0 && (!tris || !verts))) return -1;
    return admm_host::bend_hinges(n_verts, n_tris, tris, verts, cap, hinge_idx, coef, area);
}
int admm_host_tri_rest(int32_t n, const int32_t *idx, const double *verts, double *rest, double *area) {
    int r = admm_host::tri_rest(n, idx, verts, rest, area);
    if (r) return fail(ADMM_HIP_ERR_GEOMETRY, "TriEnergyTerm Error: Inverted initial pose " + std::to_string(-r - 1));
    return ADMM_HIP_OK;
}
void admm_host_lame(double youngs, double poisson, double *mu, double *lambda, double *bulk) {
    admm_host::lame(youngs, poisson, mu, lambda, bulk);
}
int admm_host_greedy_coloring(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t *color) {
    return admm_host::greedy_coloring(n, rowptr, col, color);
}

void admm_host_block_order(int32_t n_verts, int32_t n_elems, int32_t corners, const int32_t *idx, int32_t leaf, int32_t *new_id) {
    admm_host::block_order(n_verts, n_elems, corners, idx, leaf, new_id);
}

int admm_host_chunk_reduce(int32_t n_verts, int32_t n_tets, const int32_t *tet_idx, const int32_t *kind_begin, const double *corner_forces,
                           double *vertex_sums, int64_t *stats) {
    if (n_verts < 1 || n_tets < 0 || !tet_idx || !kind_begin || !corner_forces || !vertex_sums) return fail(ADMM_HIP_ERR_ARG, "chunk_reduce: bad input");
    const admm_host::TetChunks ch = admm_host::tet_chunks(n_tets, tet_idx, kind_begin);
    const admm_host::Sell inc = admm_host::record_incidence(n_verts, ch.n_rec, ch.rec_vertex.data(), ch.n_rec);
    // the block's LDS image: rows of kChunkLd doubles, row 3 c + j = component j of corner c, column = tet of the chunk, column 256 = 0
    std::vector<double> lds((size_t)12 * admm_host::kChunkLd), rec((size_t)4 * (ch.n_rec + 1), 0.0);
    int32_t chunk = 0;
    int64_t max_groups = 0;
    for (int k = 0; k < 5; ++k)
        for (int32_t t0 = kind_begin[k]; t0 < kind_begin[k + 1]; t0 += 256, ++chunk) {
            std::fill(lds.begin(), lds.end(), 0.0);
            for (int32_t t = t0; t < std::min(kind_begin[k + 1], t0 + 256); ++t)
                for (int c = 0; c < 12; ++c) lds[(size_t)c * admm_host::kChunkLd + (t - t0)] = corner_forces[12 * (size_t)t + c];
            const int32_t nrec = ch.rec_base[chunk + 1] - ch.rec_base[chunk];
            max_groups = std::max<int64_t>(max_groups, ch.group_base[chunk + 1] - ch.group_base[chunk]);
            for (int32_t g = ch.group_base[chunk]; g < ch.group_base[chunk + 1]; ++g)
                for (int tid = 0; tid < 256; ++tid) {
                    double sum[3] = {0.0, 0.0, 0.0};
                    for (int i = 0; i < admm_host::kChunkFan; ++i) {
                        const size_t w = ch.ent[((size_t)g * 256 + tid) * admm_host::kChunkFan + i] / 8;
                        for (int j = 0; j < 3; ++j) sum[j] += lds[w + (size_t)j * admm_host::kChunkLd];
                    }
                    const int32_t j = (g - ch.group_base[chunk]) * 256 + tid;
                    if (j < nrec) for (int q = 0; q < 3; ++q) rec[4 * (size_t)(ch.rec_base[chunk] + j) + q] = sum[q];
                }
        }
    int64_t max_w = 0;
    for (int32_t v = 0; v < n_verts; ++v) {
        const int32_t s = v / 64, l = v % 64;
        double sum[3] = {0.0, 0.0, 0.0};
        for (int32_t kk = 0; kk < inc.slice_width[s]; ++kk) {
            const int32_t e = inc.idx[(size_t)inc.slice_ptr[s] + 64 * kk + l];
            for (int q = 0; q < 3; ++q) sum[q] += rec[4 * (size_t)e + q];
        }
        max_w = std::max<int64_t>(max_w, inc.slice_width[s]);
        for (int q = 0; q < 3; ++q) vertex_sums[3 * (size_t)v + q] = sum[q];
    }
    if (stats) { stats[0] = ch.n_chunks; stats[1] = ch.n_rec; stats[2] = max_groups; stats[3] = max_w; stats[4] = (int64_t)inc.idx.size(); }
    return ADMM_HIP_OK;
}

#ifdef ADMM_LOCAL_PHASES
// experiments only (not declared in include/admm_hip.h): phase ticks of the local-step waves since the last call
int admm_debug_local_phases(unsigned long long *out8) {
    std::vector<unsigned long long> all((size_t)8 * admm_k::kPhaseWaves);
    if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(admm_k::g_local_phase), all.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    for (size_t i = 0; i < all.size(); ++i) out8[i & 7] += all[i];
    std::fill(all.begin(), all.end(), 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(admm_k::g_local_phase), all.data(), all.size() * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

void admm_host_locality_order(int32_t n_verts, int32_t n_elems, int32_t corners, const int32_t *idx, int32_t *new_id,
                              double *span_before, double *span_after) {
    admm_host::locality_order(n_verts, n_elems, corners, idx, new_id, span_before, span_after);
}

} // extern "C"
