// Early exit of the ADMM loop on the C++ mirror (tests/test_admm_stop.py): Settings::parse_args reads -tol, and a pinned body at rest
// without gravity ends its step after one iteration instead of Settings::admm_iters.
//
//   test_admm_stop -tol 1e-12 -it 12      GPU; prints SUCCESS.
//
// The scene: three Kuhn cells in a row (18 Neo-Hookean tets), the x = 0 face pinned, no gravity.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"

using namespace admm;

int main(int argc, char **argv) {
    Solver::Settings st;
    st.verbose = 0; st.linsolver = 0; st.gravity = 0.0;
    if (st.parse_args(argc, argv)) return 2;
    int failures = 0;
    if (!(st.admm_tol == 1e-12) || st.admm_iters != 12 || st.admm_min_iters != 1) {
        fprintf(stderr, "FAILURE: parse_args left admm_tol %.3e, admm_iters %d, admm_min_iters %d\n", st.admm_tol, st.admm_iters, st.admm_min_iters);
        ++failures;
    }
    std::vector<double> verts;
    std::vector<int> tets;
    const int nx = 3;
    const double h = 0.25;
    auto vid = [&](int i, int j, int k) { return (i * 2 + j) * 2 + k; };
    for (int i = 0; i <= nx; ++i) for (int j = 0; j <= 1; ++j) for (int k = 0; k <= 1; ++k) { verts.push_back(h * i); verts.push_back(h * j); verts.push_back(h * k); }
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int i = 0; i < nx; ++i)
        for (int p = 0; p < 6; ++p) {
            int c[3] = {i, 0, 0}, id[4];
            id[0] = vid(c[0], c[1], c[2]);
            for (int q = 0; q < 3; ++q) { c[perms[p][q]] += 1; id[q + 1] = vid(c[0], c[1], c[2]); }
            if (p == 1 || p == 2 || p == 5) std::swap(id[2], id[3]);
            for (int q = 0; q < 4; ++q) tets.push_back(id[q]);
        }
    const int nv = (int)verts.size() / 3;
    Solver solver;
    std::vector<double> m(verts.size(), 0.05);
    solver.add_nodes(verts.data(), m.data(), nv);
    const Lame lame(1.0e6, 0.3);
    for (size_t t = 0; t < tets.size() / 4; ++t) {
        const Vec4i tet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3]);
        std::vector<Vec3> tv;
        for (int c = 0; c < 4; ++c) tv.push_back(Vec3(verts[3 * tet[c]], verts[3 * tet[c] + 1], verts[3 * tet[c] + 2]));
        solver.energyterms.push_back(std::make_shared<NeoHookeanTet>(tet, tv, lame));
    }
    std::vector<int> pins;
    for (int v = 0; v < nv; ++v) if (verts[3 * v] < 1e-9) pins.push_back(v);
    solver.set_pins(pins);
    if (!solver.initialize(st)) return 2;
    const VecX x0 = solver.m_x;
    solver.step();
    const int executed = solver.runtime_data().admm_iters;
    printf("admm_iters %d, executed %d, records %d\n", st.admm_iters, executed, (int)solver.admm_history().size());
    if (!(executed >= 1 && executed < st.admm_iters)) { fprintf(stderr, "FAILURE: the body at rest executed %d of %d iterations\n", executed, st.admm_iters); ++failures; }
    if ((int)solver.admm_history().size() != executed) { fprintf(stderr, "FAILURE: admm_history() has %d records, %d iterations were executed\n", (int)solver.admm_history().size(), executed); ++failures; }
    double d = 0.0;
    for (int i = 0; i < (int)x0.size(); ++i) d = std::max(d, std::fabs(solver.m_x[i] - x0[i]));
    if (!(d <= 1e-13)) { fprintf(stderr, "FAILURE: the body at rest moved by %.3e\n", d); ++failures; }
    // switched off again: all iterations, no records
    solver.set_admm_stop(0.0);
    solver.step();
    if (solver.runtime_data().admm_iters != st.admm_iters || !solver.admm_history().empty()) {
        fprintf(stderr, "FAILURE: with tol = 0 the step executed %d of %d iterations and left %d records\n", solver.runtime_data().admm_iters, st.admm_iters, (int)solver.admm_history().size());
        ++failures;
    }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}
