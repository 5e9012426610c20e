// The positive semi-definite projection of the per-element tangent (csrc/device_math.hpp: tet_tangent_psd, tri_tangent_apply_psd)
// compiled for the host (tests/test_newton_host.py builds this with g++ -I tests/hostmath, as tests/test_stiffness.py builds
// tangent_host.cpp)
#include "../../admm-elastic_amd/csrc/device_math.hpp"
using namespace admm_dev;
extern "C" {
// n tets of one model, as hm_tet_tangent of tangent_host.cpp; psd != 0: the coefficients go through tet_tangent_psd first.
// coef [n][12] = Hs (6), al (3), be (3) as applied, raw [n][12] = the same before the projection (from the same SVD).
void hm_tet_tangent_psd(int n, int nd, int psd, int grp, int type, double mu, double la, double k, double kappa, const double *tab,
                        const double *F, const double *dF, double *dP, double *coef, double *raw) {
    for (int i = 0; i < n; ++i) {
        double U[9], V[9], S[3], Hs[6], al[3], be[3], a[3], b[3];
        signed_svd3(F + 9 * i, U, S, V);
        tet_tangent_coef(grp, type, mu, la, k, kappa, tab, S, Hs, al, be);
        for (int q = 0; q < 6; ++q) raw[12 * i + q] = Hs[q];
        for (int q = 0; q < 3; ++q) { raw[12 * i + 6 + q] = al[q]; raw[12 * i + 9 + q] = be[q]; }
        if (psd) tet_tangent_psd(Hs, al, be);
        for (int q = 0; q < 6; ++q) coef[12 * i + q] = Hs[q];
        for (int q = 0; q < 3; ++q) { coef[12 * i + 6 + q] = al[q]; coef[12 * i + 9 + q] = be[q]; a[q] = 0.5 * (al[q] + be[q]); b[q] = 0.5 * (al[q] - be[q]); }
        for (int j = 0; j < nd; ++j) tet_tangent_apply(U, V, Hs, a, b, dF + 9 * ((size_t)i * nd + j), dP + 9 * ((size_t)i * nd + j));
    }
}
// n triangles, as hm_tri_tangent; psd != 0: tri_tangent_apply_psd.  frame [n][4] = Si (3), itr as applied, raw [n][4] before the projection.
void hm_tri_tangent_psd(int n, int nd, int psd, const double *F, const double *dF, double *out, double *frame, double *raw) {
    for (int i = 0; i < n; ++i) {
        double Q[6], Si[3], itr;
        tri_tangent_frame(F + 6 * i, Q, Si, itr);
        for (int j = 0; j < nd; ++j) {
            if (psd) tri_tangent_apply_psd(Q, Si, itr, dF + 6 * ((size_t)i * nd + j), out + 6 * ((size_t)i * nd + j));
            else tri_tangent_apply(Q, Si, itr, dF + 6 * ((size_t)i * nd + j), out + 6 * ((size_t)i * nd + j));
        }
        for (int q = 0; q < 3; ++q) raw[4 * i + q] = Si[q];
        raw[4 * i + 3] = itr;
        if (psd) tri_tangent_psd(Si, itr);
        for (int q = 0; q < 3; ++q) frame[4 * i + q] = Si[q];
        frame[4 * i + 3] = itr;
    }
}
}
