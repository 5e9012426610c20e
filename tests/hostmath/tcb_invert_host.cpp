// The blocked dense inverse of the two-level tangent preconditioner (csrc/tangent_coarse.hpp: the routines the k_tcb_ kernels call)
// compiled for the host: ONE thread walks the blocks of every launch and the items of every phase in the device's launch order
// (admm_hip.hip: launch_tcb_invert), the barrier is empty and the LDS tiles are ordinary arrays -- the device's arithmetic entry for
// entry, up to the compilers' contraction of a * b + c (tests/test_tangent_coarse_host.py builds this with g++ -I tests/hostmath, as
// tests/test_tangent_precond_host.py builds tc_invert_host.cpp).
#include "../../admm-elastic_amd/csrc/tangent_coarse.hpp"
#include <vector>
using namespace admm_dev;
namespace {
struct NoSync { void operator()() const {} };
}
extern "C" {
// A [n][n] row-major (left as it is) -> X [n][n]; returns the verdict (1: X is the inverse of A without its dropped columns; 0: X = 0),
// *dropped = the columns dropped
int hm_tcb_invert(int n, const double *A, double *X, int *dropped) {
    constexpr int T = kTcbT;
    const int ntile = tcb_tiles(n);
    std::vector<double> a(A, A + (size_t)n * n), ds((size_t)n), linv((size_t)ntile * T * T), w((size_t)n * n);
    std::vector<double> Ta((size_t)T * T), Tb((size_t)T * T), Ws((size_t)T * kTcbStrip), Sg((size_t)T * kTcbStrip);
    std::vector<int> keep((size_t)n);
    int flag = 0, ok = 0;
    double rd = 0.0;
    int ri = 0;
    tcb_scan(n, a.data(), ds.data(), keep.data(), &flag, dropped, &rd, &ri, 0, 1, NoSync());
    tcb_scale(n, a.data(), ds.data(), keep.data(), &flag, 0, 1, 0, 1);
    for (int k = 0; k < ntile; ++k) {
        const int m = ntile - k - 1;
        tcb_potrf(n, k, a.data(), linv.data(), &flag, Ta.data(), Tb.data(), 0, 1, NoSync());
        if (!m) break;
        for (int b = 0; b < m; ++b) tcb_panel(n, k, k + 1 + b, a.data(), linv.data(), &flag, Ta.data(), Tb.data(), 0, 1, NoSync());
        for (int b = 0; b < m * (m + 1) / 2; ++b) {
            int i, j;
            tcb_lower_tile(b, &i, &j);
            tcb_update(n, k, k + 1 + i, k + 1 + j, a.data(), &flag, Ta.data(), Tb.data(), 0, 1, NoSync());
        }
    }
    for (int j = 0; j < ntile; ++j)
        for (int s = 0; s < T / kTcbStrip; ++s) tcb_winv(n, j, s, a.data(), linv.data(), w.data(), &flag, Ta.data(), Ws.data(), Sg.data(), 0, 1, NoSync());
    for (int b = 0; b < ntile * (ntile + 1) / 2; ++b) {
        int i, j;
        tcb_lower_tile(b, &i, &j);
        tcb_wtw(n, i, j, w.data(), X, &flag, Ta.data(), Tb.data(), 0, 1, NoSync());
    }
    tcb_unscale(n, X, ds.data(), keep.data(), &flag, 0, 1, 0, 1);
    tcb_final(n, X, &flag, &ok, 0, 1, 0, 1);
    return ok;
}
int hm_tcb_tile() { return kTcbT; }
}
