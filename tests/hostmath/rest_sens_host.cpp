// The per-element rest-shape derivative (csrc/device_math.hpp: tet_rest_grad) compiled for the host (tests/test_rest_sens_host.py builds
// this with g++ -I tests/hostmath, as tests/test_adjoint_host.py builds param_sens_host.cpp)
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
extern "C" {
// n tets of one model at F [n][9] with nd multipliers A = Ds(a) Binv [n][nd][9] (column-major) and the volumes vol [n].  Out: S [n][3]
// the signed stretches of this call's SVD, P [n][9] = U diag(sg) V^T from tet_energy_grad, T [n][nd][9] = H[A] by tet_tangent_apply,
// Gs [n][nd][9] as tet_rest_grad returns it, s [n][nd] = -vol P : A (the quantity Gs Binv^T is the derivative of).
void hm_tet_rest_grad(int n, int nd, int grp, int type, double mu, double la, double k, double kappa, const double *tab, const double *F,
                      const double *A, const double *vol, double *S, double *P, double *T, double *Gs, double *s) {
    for (int i = 0; i < n; ++i) {
        double U[9], V[9], sg[3], Hs[6], al[3], be[3], a[3], b[3], *Si = S + 3 * i;
        signed_svd3(F + 9 * i, U, Si, V);
        (void)tet_energy_grad(grp, type, mu, la, k, kappa, tab, Si, sg);
        usvt(U, sg, V, P + 9 * i);
        tet_tangent_coef(grp, type, mu, la, k, kappa, tab, Si, Hs, al, be);
        for (int q = 0; q < 3; ++q) { a[q] = 0.5 * (al[q] + be[q]); b[q] = 0.5 * (al[q] - be[q]); }
        for (int j = 0; j < nd; ++j) {
            const size_t o = (size_t)i * nd + j;
            tet_tangent_apply(U, V, Hs, a, b, A + 9 * o, T + 9 * o);
            tet_rest_grad(U, V, Si, sg, Hs, a, b, A + 9 * o, vol[i], Gs + 9 * o);
            double pa = 0.0;
            for (int c = 0; c < 9; ++c) pa += P[9 * i + c] * A[9 * o + c];
            s[o] = -vol[i] * pa;
        }
    }
}
}
