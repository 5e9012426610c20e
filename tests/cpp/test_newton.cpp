// The Newton polish on the C++ mirror (tests/test_newton_cpp.py).
//
// The 48-tet Neo-Hookean Kuhn cube, the face x = 0 pinned, under gravity: one step() of 5 ADMM iterations, then Solver::newton_polish.
//   the objective does not increase along the records and the polish reaches grad_tol = 1e-8 |m g| within 10 iterations;
//   |g_free| recomputed from Solver::forces, m_x, the masses and the step's x_bar is <= grad_tol, and far below the step's own;
//   m_v = (m_x - x_prev) / dt to rounding; the pinned vertices have not moved;
//   Solver::tangent_solve at the polished state: the residual recomputed with Solver::stiffness_apply(psd, hold_pins) is <= 2 tol |rhs|.
// Prints SUCCESS.
#include <algorithm>
#include <cmath>
#include <cstdio>
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
    Solver::Settings st; st.verbose = 0; st.admm_iters = 5; st.linsolver = 0;
    if (!solver.initialize(st)) return 2;
    const double dt = st.timestep_s;
    const VecX x_prev = solver.m_x;
    VecX xbar = x_prev;
    for (int v = 0; v < nv; ++v) xbar[3 * v + 1] += dt * dt * st.gravity;
    solver.step();
    const VecX x_admm = solver.m_x;
    auto gnorm = [&](const VecX &x) {
        const VecX f = solver.forces(x);
        double s = 0.0;
        for (int i = 0; i < n3; ++i) if (!held[i / 3]) { const double g = m[i] * (x[i] - xbar[i]) / (dt * dt) - f[i]; s += g * g; }
        return std::sqrt(s);
    };
    double mg = 0.0;
    for (int i = 0; i < n3; ++i) if (!held[i / 3] && i % 3 == 1) mg += (m[i] * st.gravity) * (m[i] * st.gravity);
    const double grad_tol = 1e-8 * std::sqrt(mg), g_admm = gnorm(x_admm);
    const std::vector<Solver::NewtonRecord> rec = solver.newton_polish(10, grad_tol, 1e-10, 2000);
    int failures = 0;
    if (rec.empty()) { fprintf(stderr, "FAILURE: no records\n"); return 1; }
    for (size_t i = 0; i < rec.size(); ++i)
        printf("iterate %d: objective %.15e, |g| %.3e, CG iterations %d, step %g\n", (int)i, rec[i].objective, rec[i].grad_norm, (int)rec[i].cg_iterations, rec[i].step);
    for (size_t i = 1; i < rec.size(); ++i) if (!(rec[i].objective <= rec[i - 1].objective)) { fprintf(stderr, "FAILURE: the objective rose\n"); ++failures; }
    const double g_pol = gnorm(solver.m_x);
    printf("|g_free| after 5 ADMM iterations %.3e, after the polish %.3e (grad_tol %.3e)\n", g_admm, g_pol, grad_tol);
    if (!(rec.back().grad_norm <= grad_tol) || !(g_pol <= grad_tol)) { fprintf(stderr, "FAILURE: grad_tol not reached\n"); ++failures; }
    if (!(std::fabs(rec[0].grad_norm - g_admm) <= 1e-9 * g_admm)) { fprintf(stderr, "FAILURE: the first record is not the step's stationarity\n"); ++failures; }
    double verr = 0.0, vmax = 0.0;
    for (int i = 0; i < n3; ++i) {
        const double vr = (solver.m_x[i] - x_prev[i]) / dt;
        verr = std::max(verr, std::fabs(solver.m_v[i] - vr)); vmax = std::max(vmax, std::max(std::fabs(vr), std::fabs(solver.m_x[i]) / dt));
        if (held[i / 3] && solver.m_x[i] != x_admm[i]) { fprintf(stderr, "FAILURE: a pinned vertex moved\n"); ++failures; break; }
    }
    if (!(verr <= 1e-14 * vmax)) { fprintf(stderr, "FAILURE: v is not (x - x_prev) / dt: %.3e of %.3e\n", verr, vmax); ++failures; }
    VecX rhs(n3);
    for (int i = 0; i < n3; ++i) rhs[i] = std::sin(1.0 + 3.0 * i);
    Solver::SolveInfo info;
    const double tol = 1e-12, shift = 1.0 / (dt * dt);
    const VecX y = solver.tangent_solve(rhs, solver.m_x, &info, -1.0, true, true, tol, 2000);
    const VecX Ky = solver.stiffness_apply(y, solver.m_x, shift, true, true);
    double rr = 0.0, bb = 0.0;
    for (int i = 0; i < n3; ++i) if (!held[i / 3]) { rr += (rhs[i] - Ky[i]) * (rhs[i] - Ky[i]); bb += rhs[i] * rhs[i]; } else if (y[i] != 0.0) { fprintf(stderr, "FAILURE: y on a pinned vertex\n"); ++failures; break; }
    printf("tangent_solve: %d iterations, converged %d, |r| / |rhs| reported %.3e, recomputed %.3e\n", info.iterations, (int)info.converged, info.residual, std::sqrt(rr / bb));
    if (!info.converged || !(std::sqrt(rr / bb) <= 2.0 * tol)) { fprintf(stderr, "FAILURE: tangent_solve\n"); ++failures; }
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main() { return run(); }
