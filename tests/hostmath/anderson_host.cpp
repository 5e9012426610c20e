// The small regularised solve of the Anderson acceleration (csrc/device_math.hpp: aa_small_solve) compiled for the host
// (tests/test_anderson_host.py builds this with g++ -I tests/hostmath, as tests/test_newton_host.py builds tangent_psd_host.cpp)
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
extern "C" {
// H [n][n] row-major, b [n] -> theta [8]; returns 1 when the solve succeeded, 0 when the caller has to clear its history
int hm_aa_small_solve(int n, const double *H, const double *b, double *theta) {
    double Hm[kAaMax * kAaMax], work[kAaWork];
    for (int i = 0; i < kAaMax * kAaMax; ++i) Hm[i] = 0.0;
    for (int i = 0; i < n && i < kAaMax; ++i)
        for (int j = 0; j < n && j < kAaMax; ++j) Hm[i * kAaMax + j] = H[i * n + j];
    return aa_small_solve(n, Hm, b, theta, work) ? 1 : 0;
}
double hm_aa_reg() { return kAaReg; }
}
