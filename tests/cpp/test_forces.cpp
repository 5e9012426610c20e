// Internal forces and the stationarity residual on the C++ mirror (tests/test_forces.py).
//
// The fixed scene of test_energy.cpp: three Kuhn cells in a row (18 tets) whose tets cycle through all eight tet kinds, one material per
// kind, plus a cloth of 4 x 4 cells (32 triangles) beside it.
//
//   Solver::forces(x) at the deformed state: sum f = 0 and sum x cross f = 0 to 1e-12 sum |f_v| (1 + |x_v|) -- a corner force dropped or
//   counted twice breaks them -- and f = 0 at rest and after a rigid motion to 1e-12 of the per-vertex scale sum w_i^2 |Binv_i|_F.
//   Solver::stress(x): one entry per tet, finite, von Mises > 0 at the deformed state.
//   A step of 50 iterations with Settings::monitor = 3: finite, positive stationarity that falls.  Prints SUCCESS.
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

int run() {
    SceneData s = make_scene();
    int failures = 0;
    Solver solver;
    std::vector<double> m(s.verts.size(), 0.05);
    solver.add_nodes(s.verts.data(), m.data(), s.nv());
    add_terms(s, solver.energyterms);
    Solver::Settings st; st.verbose = 0; st.admm_iters = 50; st.linsolver = 0; st.monitor = 3;
    if (!solver.initialize(st)) return 2;
    // the deformed state: momentum balances
    const VecX x = make_state(s, 2);
    const VecX f = solver.forces(x);
    if (f.rows() != x.rows()) { fprintf(stderr, "FAILURE: Solver::forces returned %d values for %d\n", (int)f.rows(), (int)x.rows()); return 1; }
    double lin[3] = {0.0, 0.0, 0.0}, ang[3] = {0.0, 0.0, 0.0}, scale = 0.0, fmax = 0.0;
    for (int v = 0; v < s.nv(); ++v) {
        const double *p = x.data() + 3 * v, *q = f.data() + 3 * v;
        for (int a = 0; a < 3; ++a) lin[a] += q[a];
        ang[0] += p[1] * q[2] - p[2] * q[1]; ang[1] += p[2] * q[0] - p[0] * q[2]; ang[2] += p[0] * q[1] - p[1] * q[0];
        const double fn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), xn = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        scale += fn * (1.0 + xn); fmax = std::max(fmax, fn);
    }
    const double worst = std::max(std::max(std::fabs(lin[0]), std::fabs(lin[1])), std::max(std::max(std::fabs(lin[2]), std::fabs(ang[0])), std::max(std::fabs(ang[1]), std::fabs(ang[2]))));
    printf("deformed: |sum f|, |sum x cross f| <= %.3e (allowed %.3e), largest |f_v| %.3e\n", worst, 1e-12 * scale, fmax);
    if (!(fmax > 0.0) || !(worst <= 1e-12 * scale)) { fprintf(stderr, "FAILURE: the forces of the deformed state do not balance\n"); ++failures; }
    // rest and a rigid motion: no force, to 1e-12 of the per-vertex scale of tests/test_forces.py: sum over the incident terms of
    // w^2 |Binv|_F (w^2 = k vol; triangles: k area and the inverse of the rest edge matrix in a frame of the triangle)
    std::vector<double> vscale(s.nv(), 0.0);
    for (int t = 0; t < s.nt(); ++t) {
        const int *id = &s.tets[4 * t];
        double e[3][3], tr = 0.0;      // Gram matrix of the rest edges: |Binv|_F^2 = trace of its inverse
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {
            e[a][b] = 0.0;
            for (int j = 0; j < 3; ++j) e[a][b] += (s.verts[3 * id[a + 1] + j] - s.verts[3 * id[0] + j]) * (s.verts[3 * id[b + 1] + j] - s.verts[3 * id[0] + j]);
        }
        const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) + e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
        tr = ((e[1][1] * e[2][2] - e[1][2] * e[2][1]) + (e[0][0] * e[2][2] - e[0][2] * e[2][0]) + (e[0][0] * e[1][1] - e[0][1] * e[1][0])) / det;
        const double w = solver.energyterms[t]->get_weight();
        for (int c = 0; c < 4; ++c) vscale[id[c]] += w * w * std::sqrt(tr);
    }
    for (int t = 0; t < s.ntri(); ++t) {
        const int *id = &s.tris[3 * t];
        double g00 = 0.0, g01 = 0.0, g11 = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double a = s.verts[3 * id[1] + j] - s.verts[3 * id[0] + j], b = s.verts[3 * id[2] + j] - s.verts[3 * id[0] + j];
            g00 += a * a; g01 += a * b; g11 += b * b;
        }
        const double w = solver.energyterms[s.nt() + t]->get_weight();
        for (int c = 0; c < 3; ++c) vscale[id[c]] += w * w * std::sqrt((g00 + g11) / (g00 * g11 - g01 * g01));
    }
    for (int w = 0; w < 2; ++w) {
        const VecX f0 = solver.forces(make_state(s, w));
        double big = 0.0;
        for (int v = 0; v < s.nv(); ++v)
            big = std::max(big, std::sqrt(f0[3 * v] * f0[3 * v] + f0[3 * v + 1] * f0[3 * v + 1] + f0[3 * v + 2] * f0[3 * v + 2]) / vscale[v]);
        printf("state %d: largest |f_v| / scale_v %.3e (allowed 1e-12)\n", w, big);
        if (!(big <= 1e-12)) { fprintf(stderr, "FAILURE: a rigid motion produces forces (state %d)\n", w); ++failures; }
    }
    const std::vector<Solver::TetStress> sig = solver.stress(x);
    if ((int)sig.size() != s.nt()) { fprintf(stderr, "FAILURE: Solver::stress returned %d entries for %d tets\n", (int)sig.size(), s.nt()); ++failures; }
    for (size_t t = 0; t < sig.size(); ++t)
        if (!(std::isfinite(sig[t].von_mises) && sig[t].von_mises > 0.0 && sig[t].stretches[0] > 0.0)) { fprintf(stderr, "FAILURE: stress of tet %d\n", (int)t); ++failures; }
    // monitor = 3
    solver.m_x = x;
    solver.step();
    const std::vector<Solver::AdmmRecord> &hist = solver.admm_history();
    if ((int)hist.size() != st.admm_iters) { fprintf(stderr, "FAILURE: admm_history() has %d records, admm_iters is %d\n", (int)hist.size(), st.admm_iters); return 1; }
    for (size_t i = 0; i < hist.size(); ++i)
        if (!(std::isfinite(hist[i].stationarity) && hist[i].stationarity > 0.0)) { fprintf(stderr, "FAILURE: stationarity of iteration %d is not finite and positive\n", (int)i); ++failures; }
    printf("stationarity: %.6e (iteration 0) .. %.6e (iteration %d)\n", hist.front().stationarity, hist.back().stationarity, (int)hist.size() - 1);
    if (!(hist.back().stationarity < hist.front().stationarity)) { fprintf(stderr, "FAILURE: the stationarity residual does not fall\n"); ++failures; }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main() { return run(); }
