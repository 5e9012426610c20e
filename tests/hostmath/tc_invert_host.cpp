// The dense inverse of the two-level tangent preconditioner (csrc/device_math.hpp: tc_invert -- the function k_tc_invert calls) compiled
// for the host: ONE thread walks every phase's items in order and the barrier is empty, which is the device's arithmetic entry for entry
// (tests/test_tangent_precond_host.py builds this with g++ -I tests/hostmath, as tests/test_modes_host.py builds modal_host.cpp).
#include "../../admm-elastic_amd/csrc/device_math.hpp"
#include <vector>
using namespace admm_dev;
namespace {
struct NoSync { void operator()() const {} };
}
extern "C" {
// A [n][n] row-major (left as it is) -> X [n][n]; returns the verdict (1: X is the inverse of A without its dropped columns; 0: X = 0),
// *dropped = the columns dropped
int hm_tc_invert(int n, const double *A, double *X, int *dropped) {
    std::vector<double> a(A, A + (size_t)n * n), ds((size_t)n), dl((size_t)n), col((size_t)n);
    std::vector<int> keep((size_t)n);
    int flag = 0;
    return tc_invert(n, a.data(), X, ds.data(), dl.data(), col.data(), keep.data(), &flag, dropped, 0, 1, NoSync());
}
double hm_tc_drop() { return kTcDrop; }
}
