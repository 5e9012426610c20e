// Anderson acceleration of the ADMM loop on the C++ mirror (tests/test_anderson_cpp.py): Settings::parse_args reads -aa,
// Solver::anderson_history() returns one record per iteration, and the accelerated step ends nearer to the converged one than the plain step.
//
//   test_anderson -aa 3 -it 20      GPU; prints SUCCESS.
//
// The scene: three Kuhn cells in a row (18 Neo-Hookean tets), the x = 0 face pinned, under gravity.
#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"

using namespace admm;

static bool build(Solver &solver, const Solver::Settings &st) {
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
    std::vector<double> m(verts.size(), 0.05);
    solver.add_nodes(verts.data(), m.data(), nv);
    const Lame lame(1.0e5, 0.3);
    for (size_t t = 0; t < tets.size() / 4; ++t) {
        const Vec4i tet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3]);
        std::vector<Vec3> tv;
        for (int c = 0; c < 4; ++c) tv.push_back(Vec3(verts[3 * tet[c]], verts[3 * tet[c] + 1], verts[3 * tet[c] + 2]));
        solver.energyterms.push_back(std::make_shared<NeoHookeanTet>(tet, tv, lame));
    }
    std::vector<int> pins;
    for (int v = 0; v < nv; ++v) if (verts[3 * v] < 1e-9) pins.push_back(v);
    solver.set_pins(pins);
    return solver.initialize(st);
}

static double dist(const VecX &a, const VecX &b) {
    double d = 0.0;
    for (int i = 0; i < (int)a.size(); ++i) d = std::max(d, std::fabs(a[i] - b[i]));
    return d;
}

int main(int argc, char **argv) {
    Solver::Settings st;
    st.verbose = 0; st.linsolver = 0;
    if (st.parse_args(argc, argv)) return 2;
    int failures = 0;
    if (st.anderson != 3 || st.admm_iters != 20) { fprintf(stderr, "FAILURE: parse_args left anderson %d, admm_iters %d\n", st.anderson, st.admm_iters); ++failures; }
    Solver::Settings plain = st, conv = st;
    plain.anderson = 0; conv.anderson = 0; conv.admm_iters = 600;
    Solver sa, sp, sc;
    if (!build(sa, st) || !build(sp, plain) || !build(sc, conv)) return 2;
    sa.step(); sp.step(); sc.step();
    const std::vector<Solver::AndersonRecord> h = sa.anderson_history();
    const double ea = dist(sa.m_x, sc.m_x), ep = dist(sp.m_x, sc.m_x);
    int n_accel = 0, n_rej = 0;
    for (const Solver::AndersonRecord &r : h) { n_accel += r.accelerated ? 1 : 0; n_rej += r.accepted ? 0 : 1; }
    printf("records %d, accelerated %d, rejected %d; to the converged step: plain %.3e, accelerated %.3e\n", (int)h.size(), n_accel, n_rej, ep, ea);
    if ((int)h.size() != st.admm_iters) { fprintf(stderr, "FAILURE: anderson_history() has %d records, the step ran %d iterations\n", (int)h.size(), st.admm_iters); ++failures; }
    if (!h.empty() && !(h[0].accepted && !h[0].accelerated && h[0].entries == 1 && h[0].resid > 0.0)) { fprintf(stderr, "FAILURE: the first evaluation is not a plain accepted one\n"); ++failures; }
    if (n_accel < 1) { fprintf(stderr, "FAILURE: no iteration started from an extrapolated state\n"); ++failures; }
    if (!(ea < ep)) { fprintf(stderr, "FAILURE: the accelerated step is not nearer to the converged one (%.3e against %.3e)\n", ea, ep); ++failures; }
    if (!sp.anderson_history().empty()) { fprintf(stderr, "FAILURE: the plain solver has Anderson records\n"); ++failures; }
    // a window outside 0 .. 8 is refused, and the setting stays
    bool threw = false;
    try { sa.set_anderson(9); } catch (const std::exception &) { threw = true; }
    if (!threw || sa.settings().anderson != 3) { fprintf(stderr, "FAILURE: set_anderson(9) was not refused\n"); ++failures; }
    // switched off again: no records
    sa.set_anderson(0);
    sa.step();
    if (!sa.anderson_history().empty()) { fprintf(stderr, "FAILURE: with the window 0 the step left %d records\n", (int)sa.anderson_history().size()); ++failures; }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}
