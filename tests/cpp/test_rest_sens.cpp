// The rest-shape and held-vertex gradients on the C++ mirror (tests/test_rest_sens_cpp.py).
//
// The scene of test_adjoint.cpp -- the 48-tet Neo-Hookean Kuhn cube, the face x = 0 pinned in the sweeps (linsolver 1), one step() of 5
// ADMM iterations, Solver::newton_polish to 1e-8 |m g|, Solver::step_adjoint with dL/dx_i = sin(1 + 3 i), dL/dv_i = cos(2 + 5 i) -- then
// Solver::rest_sensitivity on the multiplier at the state and Solver::adjoint_held.  lam, rest and held are written to the file named by
// argv[1], one value per line as %.17g, for the Python side to hold against its own binding on the same scene.  Checked here: held is 0
// on the free vertices, rest sums to 0 over the vertices to rounding.  Prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"

using namespace admm;

namespace {

int run(const char *path) {
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
    std::vector<double> m(verts.size(), 0.05);
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
    Solver::Settings st; st.verbose = 0; st.admm_iters = 5; st.linsolver = 1;      // (the pins of the sweeps: held exactly, the same problem on both faces)
    if (!solver.initialize(st)) return 2;
    solver.step();
    double mg = 0.0;
    for (int i = 0; i < n3; ++i) if (!held[i / 3] && i % 3 == 1) mg += (m[i] * st.gravity) * (m[i] * st.gravity);
    const std::vector<Solver::NewtonRecord> rec = solver.newton_polish(20, 1e-8 * std::sqrt(mg), 1e-10, 2000);
    if (rec.empty()) { fprintf(stderr, "FAILURE: no records\n"); return 1; }
    VecX Lx(n3), Lv(n3);
    for (int i = 0; i < n3; ++i) { Lx[i] = std::sin(1.0 + 3.0 * i); Lv[i] = std::cos(2.0 + 5.0 * i); }
    const Solver::StepAdjoint a = solver.step_adjoint(Lx, Lv, false, 1e-12, 4000, false);
    const VecX rest = solver.rest_sensitivity(a.lam, solver.m_x);
    const VecX hd = solver.adjoint_held(a.lam, Lx, Lv);
    int failures = 0;
    if (!a.converged) { fprintf(stderr, "FAILURE: the adjoint solve did not converge\n"); ++failures; }
    double sum[3] = {0.0, 0.0, 0.0}, mag = 0.0;
    for (int i = 0; i < n3; ++i) { sum[i % 3] += rest[i]; mag += std::fabs(rest[i]); }
    printf("rest_sensitivity: |sum over the vertices| = %.3e %.3e %.3e, sum |entries| = %.6e\n", std::fabs(sum[0]), std::fabs(sum[1]), std::fabs(sum[2]), mag);
    for (int j = 0; j < 3; ++j) if (!(std::fabs(sum[j]) <= 1e-12 * mag)) { fprintf(stderr, "FAILURE: rest does not sum to 0 over the vertices\n"); ++failures; break; }
    if (!(mag > 0.0)) { fprintf(stderr, "FAILURE: rest is all zero\n"); ++failures; }
    for (int i = 0; i < n3; ++i) if (!held[i / 3] && hd[i] != 0.0) { fprintf(stderr, "FAILURE: held on a free vertex\n"); ++failures; break; }
    FILE *f = fopen(path, "w");
    if (!f) { fprintf(stderr, "FAILURE: cannot write %s\n", path); return 1; }
    const VecX *vecs[3] = {&a.lam, &rest, &hd};
    for (const VecX *v : vecs) for (int i = 0; i < n3; ++i) fprintf(f, "%.17g\n", (*v)[i]);
    fclose(f);
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: test_rest_sens <output file>\n"); return 2; }
    return run(argv[1]);
}
