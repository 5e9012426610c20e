// Modal analysis on the C++ mirror (tests/test_modes_cpp.py).
//
// The 48-tet Neo-Hookean Kuhn cube, the face x = 0 pinned, at a compressed state: Solver::modes(k = 4, tol = 1e-8).
//   the run ends by its tolerance; the eigenvalues ascend and are positive (the projected tangent with a held face);
//   per mode |A phi - lambda M phi| / (lambda |M phi|) recomputed through Solver::stiffness_apply(psd, hold_pins) is <= 2 tol, through the
//   single pass and through the block pass, whose results are the same bytes;
//   Phi^T M Phi = I to 1e-12 (48 free unknowns: rounding of the last Rayleigh-Ritz); phi = 0 on the pinned vertices.
// Prints SUCCESS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"

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
    const int nv = (int)verts.size() / 3, nt = (int)tets.size() / 4, n3 = 3 * nv;
    Solver solver;
    std::vector<double> m(verts.size());
    for (int i = 0; i < n3; ++i) m[i] = 0.04 + 0.01 * ((i / 3) % 3);
    solver.add_nodes(verts.data(), m.data(), nv);
    const Lame lame(1.0e5, 0.35);
    for (int t = 0; t < nt; ++t) {
        const Vec4i tet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3]);
        std::vector<Vec3> tv;
        for (int c = 0; c < 4; ++c) tv.push_back(Vec3(verts[3 * tet[c]], verts[3 * tet[c] + 1], verts[3 * tet[c] + 2]));
        solver.energyterms.push_back(std::make_shared<NeoHookeanTet>(tet, tv, lame));
    }
    std::vector<int> pins;
    std::vector<bool> held(nv, false);
    for (int v = 0; v < nv; ++v) if (verts[3 * v] < 1e-9) { pins.push_back(v); held[v] = true; }
    solver.set_pins(pins);
    Solver::Settings st; st.verbose = 0; st.admm_iters = 5; st.linsolver = 0;
    if (!solver.initialize(st)) return 2;
    VecX x = solver.m_x;
    for (int v = 0; v < nv; ++v) {      // compressed along y and z, sheared; the pinned face keeps its x
        x[3 * v + 1] = 0.8 * x[3 * v + 1] + 0.05 * x[3 * v];
        x[3 * v + 2] = 0.9 * x[3 * v + 2];
    }
    const int k = 4;
    const double tol = 1e-8;
    Solver::ModesInfo info;
    const std::vector<VecX> phi = solver.modes(k, x, &info, 0.0, true, true, tol, 2000);
    int failures = 0;
    printf("modes: %d iterations, %d converged, %d restarts, ended by %d\n", info.iterations, info.converged_modes, info.restarts, info.ended_by);
    if ((int)phi.size() != k || info.ended_by != 0 || info.converged_modes != k) { fprintf(stderr, "FAILURE: the run did not end by its tolerance\n"); ++failures; }
    for (int i = 0; i < k && i < (int)phi.size(); ++i) {
        const double lam = info.lambda[i];
        const VecX Kp = solver.stiffness_apply(phi[i], x, 0.0, true, true), Kb = solver.stiffness_apply(phi[i], x, 0.0, true, true, true);
        if (std::memcmp(Kp.data(), Kb.data(), sizeof(double) * n3) != 0) { fprintf(stderr, "FAILURE: the block pass differs from the single pass\n"); ++failures; }
        double rr = 0.0, mm = 0.0;
        for (int r = 0; r < n3; ++r) {
            const double mp = m[r] * phi[i][r], res = Kp[r] - lam * mp;
            rr += res * res; mm += mp * mp;
            if (held[r / 3] && phi[i][r] != 0.0) { fprintf(stderr, "FAILURE: phi on a pinned vertex\n"); ++failures; break; }
        }
        const double rel = std::sqrt(rr) / (std::fabs(lam) * std::sqrt(mm));
        printf("mode %d: lambda %.9e, residual reported %.3e, recomputed %.3e\n", i, lam, info.residual[i], rel);
        if (!(rel <= 2.0 * tol)) { fprintf(stderr, "FAILURE: residual of mode %d\n", i); ++failures; }
        if (!(lam > 0.0) || (i > 0 && !(lam >= info.lambda[i - 1]))) { fprintf(stderr, "FAILURE: eigenvalue order\n"); ++failures; }
        for (int j = 0; j <= i; ++j) {
            double g = 0.0;
            for (int r = 0; r < n3; ++r) g += phi[i][r] * m[r] * phi[j][r];
            if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-12)) { fprintf(stderr, "FAILURE: Phi^T M Phi (%d, %d) = %.17g\n", i, j, g); ++failures; }
        }
    }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main() { return run(); }
