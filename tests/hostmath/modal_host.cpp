// The dense Rayleigh-Ritz of the block eigensolver (csrc/device_math.hpp: modal_geneig, modal_rr -- the functions k_modal_rr calls)
// compiled for the host: ONE thread walks every phase's items in order and the barrier is empty, which is the device's arithmetic entry
// for entry (tests/test_modes_host.py builds this with g++ -I tests/hostmath).
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
namespace {
struct NoSync { void operator()() const {} };
struct Work {
    double A[kModalMax * kModalLd], M[kModalMax * kModalLd], Q[kModalMax * kModalLd];
    double ds[kModalMax], dl[kModalMax], ev[kModalMax], cs[kModalMax + 2];
    int perm[kModalMax], ok[2];
    ModalWork view() { return ModalWork{A, M, Q, ds, dl, ev, cs, perm, ok}; }
};
}
extern "C" {
// G_A, G_M [n][n] row-major -> ev [n] ascending, C [n][n] row-major (column r = the r-th vector); 1 = success, 0 = failure (ev, C zero)
int hm_sym_geneig(int n, const double *GA, const double *GM, double *ev, double *C) {
    for (int i = 0; i < n * n; ++i) C[i] = 0.0;
    for (int i = 0; i < n; ++i) ev[i] = 0.0;
    if (n < 1 || n > kModalMax) return 0;
    static Work w;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) { w.A[i * kModalLd + j] = GA[i * n + j]; w.M[i * kModalLd + j] = GM[i * n + j]; }
    if (!modal_geneig(n, w.view(), 0, 1, NoSync())) return 0;
    for (int r = 0; r < n; ++r) {
        ev[r] = w.ev[w.perm[r]];
        for (int i = 0; i < n; ++i) C[i * n + r] = w.A[i * kModalLd + r];
    }
    return 1;
}
// the Rayleigh-Ritz of an iteration with its restart rule: GA, GM [3 nb][3 nb] row-major, m = 3 nb or 2 nb columns in use -> th [nb],
// C [3 nb][nb]; returns the columns used (0: failure), *restarted = 1 when P was dropped
int hm_modal_rr(int nb, int m, const double *GA, const double *GM, double *th, double *C, int *restarted) {
    static Work w;
    return modal_rr(nb, m, GA, GM, w.view(), th, C, restarted, 0, 1, NoSync());
}
double hm_modal_pivot() { return kModalPivot; }
int hm_modal_sweeps() { return kModalSweeps; }
double hm_modal_start(unsigned col, unsigned vertex, unsigned axis) { return modal_start(col, vertex, axis); }
}
