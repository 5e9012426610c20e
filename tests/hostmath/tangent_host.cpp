// The per-element tangent of csrc/device_math.hpp compiled for the host (tests/test_stiffness.py builds this with g++ -I tests/hostmath,
// as tests/test_device_math_host.py builds hostmath.cpp)
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
extern "C" {
// n tets of one model.  F [n][9] column-major, dF and dP [n][nd][9] column-major; coef [n][12] = Hs (6), al (3), be (3) in the frame of
// the signed SVD; S [n][3] its signed stretches.  grp / type as kernels.hpp: Mat; tab: the tabulated spline's table or NULL.
void hm_tet_tangent(int n, int nd, int grp, int type, double mu, double la, double k, double kappa, const double *tab, const double *F,
                    const double *dF, double *dP, double *coef, double *S) {
    for (int i = 0; i < n; ++i) {
        double U[9], V[9], Hs[6], al[3], be[3], a[3], b[3];
        signed_svd3(F + 9 * i, U, S + 3 * i, V);
        tet_tangent_coef(grp, type, mu, la, k, kappa, tab, S + 3 * i, Hs, al, be);
        for (int q = 0; q < 6; ++q) coef[12 * i + q] = Hs[q];
        for (int q = 0; q < 3; ++q) { coef[12 * i + 6 + q] = al[q]; coef[12 * i + 9 + q] = be[q]; a[q] = 0.5 * (al[q] + be[q]); b[q] = 0.5 * (al[q] - be[q]); }
        for (int j = 0; j < nd; ++j) tet_tangent_apply(U, V, Hs, a, b, dF + 9 * ((size_t)i * nd + j), dP + 9 * ((size_t)i * nd + j));
    }
}
// n stretch triples of one model, taken as they are (no SVD): S [n][3] signed -> psi [n] the density, sg [n][3] the diagonal of dpsi/dF in
// the frame of the signed SVD (device_math.hpp: tet_energy_grad, the one dispatch under energy() and forces())
void hm_tet_energy_grad(int n, int grp, int type, double mu, double la, double k, double kappa, const double *tab, const double *S,
                        double *psi, double *sg) {
    for (int i = 0; i < n; ++i) psi[i] = tet_energy_grad(grp, type, mu, la, k, kappa, tab, S + 3 * i, sg + 3 * i);
}
// n triangles: F [n][6] (3x2 column-major), dF and out [n][nd][6]; out = dF - dQ (the caller scales by w^2)
void hm_tri_tangent(int n, int nd, const double *F, const double *dF, double *out) {
    for (int i = 0; i < n; ++i) {
        double Q[6], Si[3], itr;
        tri_tangent_frame(F + 6 * i, Q, Si, itr);
        for (int j = 0; j < nd; ++j) tri_tangent_apply(Q, Si, itr, dF + 6 * ((size_t)i * nd + j), out + 6 * ((size_t)i * nd + j));
    }
}
}
