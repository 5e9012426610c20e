// The per-element parameter derivative (csrc/device_math.hpp: tet_param_grad) compiled for the host (tests/test_adjoint_host.py builds
// this with g++ -I tests/hostmath, as tests/test_newton_host.py builds tangent_psd_host.cpp)
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
extern "C" {
// n tets of one model at F [n][9] (column-major).  S [n][3]: the signed stretches of this call's SVD; sg [n][3] and dsg [n][9] as
// tet_param_grad returns them; fd [n][9]: central differences of the host's own tet_energy_grad in theta_p = (mu, la, kappa) with the
// steps h [3], at the same stretches.
void hm_tet_param_grad(int n, int grp, int type, double mu, double la, double k, double kappa, const double *tab, const double *F,
                       const double *h, double *S, double *sg, double *dsg, double *fd) {
    for (int i = 0; i < n; ++i) {
        double U[9], V[9], *s = S + 3 * i;
        signed_svd3(F + 9 * i, U, s, V);
        tet_param_grad(grp, type, mu, la, k, kappa, tab, s, sg + 3 * i, dsg + 9 * i);
        for (int p = 0; p < 3; ++p) {
            double hi[3], lo[3];
            const double d = h[p];
            (void)tet_energy_grad(grp, type, mu + (p == 0 ? d : 0.0), la + (p == 1 ? d : 0.0), k, kappa + (p == 2 ? d : 0.0), tab, s, hi);
            (void)tet_energy_grad(grp, type, mu - (p == 0 ? d : 0.0), la - (p == 1 ? d : 0.0), k, kappa - (p == 2 ? d : 0.0), tab, s, lo);
            for (int j = 0; j < 3; ++j) fd[9 * i + 3 * p + j] = (hi[j] - lo[j]) / (2.0 * d);
        }
    }
}
}
