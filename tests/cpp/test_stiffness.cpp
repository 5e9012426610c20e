// The tangent stiffness on the C++ mirror (tests/test_stiffness.py).
//
// The 48-tet Neo-Hookean Kuhn cube (2 x 2 x 2 cells) at a smooth stretch with a ripple:
//   Solver::stiffness_apply(d, x, shift) equals admm_hip_stiffness_apply on the solver's own context bit for bit, shift = 0 and 1 / dt^2;
//   symmetry: |d1 . K d2 - d2 . K d1| <= 1e-12 |d1| |d2| sum_v scale_v, scale_v = sum over the incident tets of w_i^2 |Binv_i|_F^2
//   (w^2 = k vol: the per-vertex scale of tests/test_stiffness.py with the term's k for the size of its tangent);
//   K d is finite and not zero.  Prints SUCCESS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"
#include "../../include/admm_hip.h"

using namespace admm;

namespace {

int run() {
    const int n = 2;
    const double h = 0.5;
    std::vector<double> verts;
    std::vector<int> tets;
    auto vid = [&](int i, int j, int k) { return (i * (n + 1) + j) * (n + 1) + k; };
    for (int i = 0; i <= n; ++i) for (int j = 0; j <= n; ++j) for (int k = 0; k <= n; ++k) { verts.push_back(h * i); verts.push_back(h * j); verts.push_back(h * k); }
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) for (int k = 0; k < n; ++k)
        for (int p = 0; p < 6; ++p) {
            int c[3] = {i, j, k}, id[4];
            id[0] = vid(c[0], c[1], c[2]);
            for (int q = 0; q < 3; ++q) { c[perms[p][q]] += 1; id[q + 1] = vid(c[0], c[1], c[2]); }
            if (p == 1 || p == 2 || p == 5) std::swap(id[2], id[3]);
            for (int q = 0; q < 4; ++q) tets.push_back(id[q]);
        }
    const int nv = (int)verts.size() / 3, nt = (int)tets.size() / 4;
    if (nt != 48) { fprintf(stderr, "FAILURE: %d tets\n", nt); return 1; }
    Solver solver;
    std::vector<double> m(verts.size(), 0.05);
    solver.add_nodes(verts.data(), m.data(), nv);
    const Lame lame(1.0e6, 0.35);
    for (int t = 0; t < nt; ++t) {
        const Vec4i tet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3]);
        std::vector<Vec3> tv;
        for (int c = 0; c < 4; ++c) tv.push_back(Vec3(verts[3 * tet[c]], verts[3 * tet[c] + 1], verts[3 * tet[c] + 2]));
        solver.energyterms.push_back(std::make_shared<NeoHookeanTet>(tet, tv, lame));
    }
    Solver::Settings st; st.verbose = 0; st.admm_iters = 5; st.linsolver = 0;
    if (!solver.initialize(st)) return 2;
    VecX x(verts.size()), d1(verts.size()), d2(verts.size());
    for (int v = 0; v < nv; ++v) {
        const double p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
        x[3 * v] = 1.25 * p[0] + 0.02 * std::sin(5.0 * p[1] + 3.0 * p[2]);
        x[3 * v + 1] = 0.85 * p[1] + 0.03 * std::sin(4.0 * p[0] + 2.0 * p[2]);
        x[3 * v + 2] = 1.10 * p[2] + 0.02 * std::cos(6.0 * p[0] + 3.0 * p[1]);
        for (int a = 0; a < 3; ++a) {
            d1[3 * v + a] = std::sin(1.0 + 7.0 * v + 3.0 * a);
            d2[3 * v + a] = std::cos(2.0 + 5.0 * v - 4.0 * a);
        }
    }
    int failures = 0;
    const double shifts[2] = {0.0, 1.0 / (st.timestep_s * st.timestep_s)};
    for (int k = 0; k < 2; ++k) {
        const VecX a = solver.stiffness_apply(d1, x, shifts[k]);
        std::vector<double> b(verts.size(), 0.0);
        if (admm_hip_stiffness_apply((admm_hip_ctx *)solver.context(), x.data(), 1, d1.data(), shifts[k], b.data()) != ADMM_HIP_OK) {
            fprintf(stderr, "FAILURE: admm_hip_stiffness_apply: %s\n", admm_hip_last_error()); return 1;
        }
        if (a.rows() != x.rows() || std::memcmp(a.data(), b.data(), b.size() * sizeof(double)) != 0) {
            fprintf(stderr, "FAILURE: Solver::stiffness_apply differs from the C ABI (shift %g)\n", shifts[k]); ++failures;
        }
    }
    const VecX K1 = solver.stiffness_apply(d1, x), K2 = solver.stiffness_apply(d2, x);
    std::vector<double> vscale(nv, 0.0);
    for (int t = 0; t < nt; ++t) {
        const int *id = &tets[4 * t];
        double e[3][3];      // Gram matrix of the rest edges: |Binv|_F^2 = trace of its inverse
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {
            e[a][b] = 0.0;
            for (int j = 0; j < 3; ++j) e[a][b] += (verts[3 * id[a + 1] + j] - verts[3 * id[0] + j]) * (verts[3 * id[b + 1] + j] - verts[3 * id[0] + j]);
        }
        const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) + e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
        const double tr = ((e[1][1] * e[2][2] - e[1][2] * e[2][1]) + (e[0][0] * e[2][2] - e[0][2] * e[2][0]) + (e[0][0] * e[1][1] - e[0][1] * e[1][0])) / det;
        const double w = solver.energyterms[t]->get_weight();
        for (int c = 0; c < 4; ++c) vscale[id[c]] += w * w * tr;
    }
    double s12 = 0.0, s21 = 0.0, n1 = 0.0, n2 = 0.0, scale = 0.0, big = 0.0;
    bool finite = true;
    for (int i = 0; i < (int)verts.size(); ++i) {
        s12 += d1[i] * K2[i]; s21 += d2[i] * K1[i]; n1 += d1[i] * d1[i]; n2 += d2[i] * d2[i];
        finite = finite && std::isfinite(K1[i]) && std::isfinite(K2[i]);
        big = std::max(big, std::fabs(K1[i]));
    }
    for (int v = 0; v < nv; ++v) scale += vscale[v];
    const double bar = 1e-12 * std::sqrt(n1) * std::sqrt(n2) * scale;
    printf("symmetry: d1 . K d2 = %.15e, d2 . K d1 = %.15e, difference %.3e (allowed %.3e), largest |K d1| %.3e\n", s12, s21, std::fabs(s12 - s21), bar, big);
    if (!finite || !(big > 0.0)) { fprintf(stderr, "FAILURE: K d is not finite or zero\n"); ++failures; }
    if (!(std::fabs(s12 - s21) <= bar)) { fprintf(stderr, "FAILURE: K is not symmetric\n"); ++failures; }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main() { return run(); }
