// EnergyTerm::energy and the ADMM monitor on the C++ mirror (tests/test_energy_monitor.py).
//
// The fixed scene: three Kuhn cells in a row (18 tets) whose tets cycle through all eight tet kinds, one material per kind -- linear,
// NeoHookeanTet, StVKTet, SplineTet with xu::NeoHookean (kappa 0), xu::StVK and xu::CoRotated with a compression term, a user-defined
// xu::Spline (tabulated on the device) and StableNeoHookeanTet -- plus a cloth of 4 x 4 cells (32 triangles) beside it.
//
//   test_energy --host   no GPU: prints the scene and, for the states "rest", "rotated" and "deformed", the mirror's HOST
//                        EnergyTerm::energy(D, x) of every term; the Python test restates them in numpy (src/TetEnergyTerm.cpp:94-100,
//                        138-149, src/TriEnergyTerm.cpp:104-114: 0 at rest and after a rotation).
//   test_energy          GPU: Solver::energy(x) (the device reduction) against the sum of those host energies, and a step with
//                        Settings::monitor = 1; prints SUCCESS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "Solver.hpp"
#include "TetEnergyTerm.hpp"
#include "TriEnergyTerm.hpp"

using namespace admm;

namespace {

// a spline that is none of the three named ones: f = a (s - 1)^2, g = b (p - 1)^2, h = c (J - 1)^2
struct QuadSpline : xu::Spline {
    double a, b, c;
    QuadSpline(double a_, double b_, double c_) : a(a_), b(b_), c(c_) {}
    double f(double x) const { return a * (x - 1.0) * (x - 1.0); }
    double g(double x) const { return b * (x - 1.0) * (x - 1.0); }
    double h(double x) const { return c * (x - 1.0) * (x - 1.0); }
    double df(double x) const { return 2.0 * a * (x - 1.0); }
    double dg(double x) const { return 2.0 * b * (x - 1.0); }
    double dh(double x) const { return 2.0 * c * (x - 1.0); }
};

struct SceneData {
    std::vector<double> verts;            // rest positions
    std::vector<int> tets, tet_kind, tris;
    std::vector<Lame> tet_lame;           // the tet's own Lame (its bulk modulus is the term's k)
    std::vector<double> tet_kappa;
    Lame tri_lame;
    int nv() const { return (int)verts.size() / 3; }
    int nt() const { return (int)tets.size() / 4; }
    int ntri() const { return (int)tris.size() / 3; }
};

Lame kind_lame(int kind) { return Lame(1.0e6 * (1.0 + kind), 0.30 + 0.02 * kind); }
double kind_kappa(int kind) { return kind == 4 ? 2.0e5 : kind == 5 ? 1.0e5 : 0.0; }

SceneData make_scene() {
    SceneData s;
    const int nx = 3;
    const double h = 0.25;
    auto vid = [&](int i, int j, int k) { return (i * 2 + j) * 2 + k; };
    for (int i = 0; i <= nx; ++i) for (int j = 0; j <= 1; ++j) for (int k = 0; k <= 1; ++k) { s.verts.push_back(h * i); s.verts.push_back(h * j); s.verts.push_back(h * k); }
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int i = 0; i < nx; ++i)
        for (int p = 0; p < 6; ++p) {
            int c[3] = {i, 0, 0}, id[4];
            id[0] = vid(c[0], c[1], c[2]);
            for (int q = 0; q < 3; ++q) { c[perms[p][q]] += 1; id[q + 1] = vid(c[0], c[1], c[2]); }
            if (p == 1 || p == 2 || p == 5) std::swap(id[2], id[3]);
            const int kind = (int)(s.tets.size() / 4) % 8;
            for (int q = 0; q < 4; ++q) s.tets.push_back(id[q]);
            s.tet_kind.push_back(kind); s.tet_lame.push_back(kind_lame(kind)); s.tet_kappa.push_back(kind_kappa(kind));
        }
    const int base = s.nv(), nc = 4;
    for (int i = 0; i <= nc; ++i) for (int j = 0; j <= nc; ++j) { s.verts.push_back(1.2 + 0.2 * i); s.verts.push_back(0.3); s.verts.push_back(0.2 * j); }
    auto cid = [&](int i, int j) { return base + i * (nc + 1) + j; };
    for (int i = 0; i < nc; ++i) for (int j = 0; j < nc; ++j) {
        const int t[6] = {cid(i, j), cid(i, j + 1), cid(i + 1, j), cid(i + 1, j), cid(i, j + 1), cid(i + 1, j + 1)};      // (normal +y)
        for (int q = 0; q < 6; ++q) s.tris.push_back(t[q]);
    }
    s.tri_lame = Lame(2.0e5, 0.3);
    return s;
}

std::shared_ptr<EnergyTerm> make_tet(const SceneData &s, int t) {
    const Vec4i tet(s.tets[4 * t], s.tets[4 * t + 1], s.tets[4 * t + 2], s.tets[4 * t + 3]);
    std::vector<Vec3> tv;
    for (int c = 0; c < 4; ++c) tv.push_back(Vec3(s.verts[3 * tet[c]], s.verts[3 * tet[c] + 1], s.verts[3 * tet[c] + 2]));
    const Lame &l = s.tet_lame[t];
    switch (s.tet_kind[t]) {
        case 0: return std::make_shared<TetEnergyTerm>(tet, tv, l);
        case 1: return std::make_shared<NeoHookeanTet>(tet, tv, l);
        case 2: return std::make_shared<StVKTet>(tet, tv, l);
        case 3: return std::make_shared<SplineTet>(tet, tv, l);
        case 4: return std::make_shared<SplineTet>(tet, tv, l, std::make_shared<xu::StVK>(l.mu, l.lambda, s.tet_kappa[t]));
        case 5: return std::make_shared<SplineTet>(tet, tv, l, std::make_shared<xu::CoRotated>(l.mu, l.lambda, s.tet_kappa[t]));
        case 6: return std::make_shared<SplineTet>(tet, tv, l, std::make_shared<QuadSpline>(l.mu, 0.25 * l.lambda, 0.5 * l.lambda));
        default: return std::make_shared<StableNeoHookeanTet>(tet, tv, l);
    }
}

void add_terms(const SceneData &s, std::vector<std::shared_ptr<EnergyTerm> > &terms) {
    for (int t = 0; t < s.nt(); ++t) terms.push_back(make_tet(s, t));
    create_tris_from_mesh<double, TriEnergyTerm>(terms, s.verts.data(), s.tris.data(), s.ntri(), s.tri_lame, 0);
}

// the three states: rest, a rigid rotation + translation of it, a smooth stretch with a ripple (stretches within [0.6, 1.5])
VecX make_state(const SceneData &s, int which) {
    VecX x(s.verts.size());
    const double c = std::cos(0.7), sn = std::sin(0.7);
    for (int v = 0; v < s.nv(); ++v) {
        const double p[3] = {s.verts[3 * v], s.verts[3 * v + 1], s.verts[3 * v + 2]};
        if (which == 0) { for (int a = 0; a < 3; ++a) x[3 * v + a] = p[a]; }
        else if (which == 1) { x[3 * v] = c * p[0] - sn * p[2] + 0.1; x[3 * v + 1] = p[1] - 0.2; x[3 * v + 2] = sn * p[0] + c * p[2] + 0.3; }
        else {
            x[3 * v] = 1.25 * p[0] + 0.02 * std::sin(5.0 * p[1] + 3.0 * p[2]);
            x[3 * v + 1] = 0.85 * p[1] + 0.03 * std::sin(4.0 * p[0] + 2.0 * p[2]);
            x[3 * v + 2] = 1.10 * p[2] + 0.02 * std::cos(6.0 * p[0] + 3.0 * p[1]);
        }
    }
    return x;
}

SparseMat reduction_matrix(std::vector<std::shared_ptr<EnergyTerm> > &terms, int dof) {
    std::vector<Triplet> triplets; std::vector<double> weights;
    for (auto &t : terms) t->get_reduction(triplets, weights);
    SparseMat D;
    D.resize((int)weights.size(), dof);
    D.setFromTriplets(triplets.begin(), triplets.end());
    return D;
}

int host_mode() {
    const SceneData s = make_scene();
    std::vector<std::shared_ptr<EnergyTerm> > terms;
    add_terms(s, terms);
    SparseMat D = reduction_matrix(terms, 3 * s.nv());
    printf("NV %d\n", s.nv());
    for (int v = 0; v < s.nv(); ++v) printf("V %.17g %.17g %.17g\n", s.verts[3 * v], s.verts[3 * v + 1], s.verts[3 * v + 2]);
    printf("NT %d\n", s.nt());
    for (int t = 0; t < s.nt(); ++t)
        printf("T %d %d %d %d %d %.17g %.17g %.17g\n", s.tets[4 * t], s.tets[4 * t + 1], s.tets[4 * t + 2], s.tets[4 * t + 3], s.tet_kind[t], s.tet_lame[t].mu,
               s.tet_lame[t].lambda, s.tet_kappa[t]);
    printf("NR %d %.17g %.17g\n", s.ntri(), s.tri_lame.mu, s.tri_lame.lambda);
    for (int t = 0; t < s.ntri(); ++t) printf("R %d %d %d\n", s.tris[3 * t], s.tris[3 * t + 1], s.tris[3 * t + 2]);
    const char *names[3] = {"rest", "rotated", "deformed"};
    for (int w = 0; w < 3; ++w) {
        const VecX x = make_state(s, w);
        printf("STATE %s\n", names[w]);
        for (int v = 0; v < s.nv(); ++v) printf("X %.17g %.17g %.17g\n", x[3 * v], x[3 * v + 1], x[3 * v + 2]);
        for (size_t i = 0; i < terms.size(); ++i) printf("E %.17g\n", terms[i]->energy(D, x));
    }
    return 0;
}

int gpu_mode() {
    SceneData s = make_scene();
    int failures = 0;
    Solver solver;
    std::vector<double> m(s.verts.size(), 0.05);
    solver.add_nodes(s.verts.data(), m.data(), s.nv());
    add_terms(s, solver.energyterms);
    // host energies through a reduction matrix of our own (Solver::m_D is protected), on separate term objects
    std::vector<std::shared_ptr<EnergyTerm> > host_terms;
    add_terms(s, host_terms);
    SparseMat D = reduction_matrix(host_terms, 3 * s.nv());
    Solver::Settings st; st.verbose = 0; st.admm_iters = 6; st.linsolver = 0; st.monitor = 1;
    if (!solver.initialize(st)) return 2;
    for (int w = 0; w < 3; ++w) {
        const VecX x = make_state(s, w);
        double sum = 0.0, tol = 0.0;
        for (auto &t : host_terms) {
            const double e = t->energy(D, x);
            sum += e; tol += 1e-9 * (std::fabs(e) + t->get_weight() * t->get_weight());      // w^2 = k vol (k area): the bar of the per-term parity test
        }
        const double dev = solver.energy(x);
        printf("state %d: Solver::energy %.12e, sum of the host terms %.12e, |difference| %.3e (allowed %.3e)\n", w, dev, sum, std::fabs(dev - sum), tol);
        if (!(std::fabs(dev - sum) <= tol)) { fprintf(stderr, "FAILURE: Solver::energy differs from the host terms in state %d\n", w); ++failures; }
    }
    solver.m_x = make_state(s, 2);      // start the step from the deformed state: the residuals are far from zero
    solver.step();
    const std::vector<Solver::AdmmRecord> &hist = solver.admm_history();
    if ((int)hist.size() != st.admm_iters) { fprintf(stderr, "FAILURE: admm_history() has %d records, admm_iters is %d\n", (int)hist.size(), st.admm_iters); ++failures; }
    for (size_t i = 0; i < hist.size(); ++i) {
        printf("iteration %d: primal %.6e dz %.6e\n", (int)i, hist[i].primal, hist[i].dz);
        if (!(std::isfinite(hist[i].primal) && hist[i].primal > 0.0)) { fprintf(stderr, "FAILURE: primal residual of iteration %d is not finite and positive\n", (int)i); ++failures; }
        if (hist[i].energy != 0.0 || hist[i].objective != 0.0) { fprintf(stderr, "FAILURE: monitor = 1 filled the objective slots\n"); ++failures; }
    }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) return host_mode();
    return gpu_mode();
}
