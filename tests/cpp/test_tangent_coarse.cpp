// The blocked coarse inverse of the two-level tangent preconditioner on the C++ mirror (tests/test_tangent_coarse_cpp.py).
//
// The scene of test_tangent_precond.cpp: the 48-tet Neo-Hookean Kuhn cube with the edge x = y = 0 pinned, at a compressed, sheared state.
// Solver::tangent_solve with set_tangent_precond(TwoLevel, 2) and the default coarse inverse, then with
// Solver::set_tangent_coarse(Blocked), then with OneBlock again:
//   the blocked solve converges within 2 iterations of the one-block solve, its residual recomputed with
//   Solver::stiffness_apply(psd, hold_pins) is <= 2 tol |rhs|, Solver::tangent_coarse reports Blocked, tile 64 and the 7 launches of a
//   one-tile chain (OneBlock and 1 launch before and after), Solver::tangent_precond reports what it reported with the one-block inverse;
//   the one-block solve after it has the bits of the one before.
// The blocked y and the one-block y are written to the file named by argv[1], one value per line as %.17g, for the Python side to hold
// against its own binding on the same scene.  Prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    for (int v = 0; v < nv; ++v) if (verts[3 * v] < 1e-9 && verts[3 * v + 1] < 1e-9) { pins.push_back(v); held[v] = true; }
    solver.set_pins(pins);
    Solver::Settings st; st.verbose = 0; st.admm_iters = 5; st.linsolver = 0;
    if (!solver.initialize(st)) return 2;
    const double dt = st.timestep_s;
    VecX x(n3), rhs(n3);
    for (int v = 0; v < nv; ++v) {      // compressed and sheared
        x[3 * v] = 0.9 * verts[3 * v]; x[3 * v + 1] = 0.8 * verts[3 * v + 1] + 0.1 * verts[3 * v]; x[3 * v + 2] = 0.85 * verts[3 * v + 2];
    }
    for (int i = 0; i < n3; ++i) rhs[i] = std::sin(1.0 + 3.0 * i);
    const double tol = 1e-12, shift = 1.0 / (dt * dt);
    int failures = 0;
    Solver::SolveInfo io, ib, io2;
    solver.set_tangent_precond(Solver::TangentPrecond::TwoLevel, 2);
    const Solver::TangentCoarseInfo c0 = solver.tangent_coarse();
    const VecX yo = solver.tangent_solve(rhs, x, &io, -1.0, true, true, tol, 2000);
    const Solver::TangentPrecondInfo po = solver.tangent_precond();
    const Solver::TangentCoarseInfo c1 = solver.tangent_coarse();
    solver.set_tangent_coarse(Solver::TangentCoarse::Blocked);
    const VecX yb = solver.tangent_solve(rhs, x, &ib, -1.0, true, true, tol, 2000);
    const Solver::TangentPrecondInfo pb = solver.tangent_precond();
    const Solver::TangentCoarseInfo c2 = solver.tangent_coarse();
    solver.set_tangent_coarse(Solver::TangentCoarse::OneBlock);
    const VecX yo2 = solver.tangent_solve(rhs, x, &io2, -1.0, true, true, tol, 2000);
    const Solver::TangentCoarseInfo c3 = solver.tangent_coarse();
    printf("one-block: %d iterations, converged %d; blocked: %d iterations, converged %d; tile %d, launches %d; coarse_dim %d, dropped %d, ok %d\n", io.iterations,
           (int)io.converged, ib.iterations, (int)ib.converged, c2.tile, c2.launches, pb.coarse_dim, pb.coarse_dropped, (int)pb.coarse_ok);
    if (!io.converged || !ib.converged || std::abs(ib.iterations - io.iterations) > 2) { fprintf(stderr, "FAILURE: iterations\n"); ++failures; }
    if (c0.solver != Solver::TangentCoarse::OneBlock || c0.tile != 64 || c0.launches != 0 || c1.solver != Solver::TangentCoarse::OneBlock || c1.launches != 1 ||
        c2.solver != Solver::TangentCoarse::Blocked || c2.tile != 64 || c2.launches != 7 || c3.solver != Solver::TangentCoarse::OneBlock || c3.launches != 1) {
        fprintf(stderr, "FAILURE: tangent_coarse()\n"); ++failures;
    }
    if (pb.kind != po.kind || pb.aggregates != po.aggregates || pb.coarse_dim != 24 || po.coarse_dim != 24 || pb.coarse_dropped != 0 || po.coarse_dropped != 0 ||
        !pb.coarse_ok || !po.coarse_ok || pb.setup_passes != po.setup_passes) {
        fprintf(stderr, "FAILURE: tangent_precond() with the blocked inverse\n"); ++failures;
    }
    const VecX Ky = solver.stiffness_apply(yb, x, shift, true, true);
    double rr = 0.0, bb = 0.0;
    for (int i = 0; i < n3; ++i) if (!held[i / 3]) { rr += (rhs[i] - Ky[i]) * (rhs[i] - Ky[i]); bb += rhs[i] * rhs[i]; } else if (yb[i] != 0.0) { fprintf(stderr, "FAILURE: y on a pinned vertex\n"); ++failures; break; }
    printf("blocked: |r| / |rhs| reported %.3e, recomputed %.3e\n", ib.residual, std::sqrt(rr / bb));
    if (!(std::sqrt(rr / bb) <= 2.0 * tol)) { fprintf(stderr, "FAILURE: the residual\n"); ++failures; }
    if (std::memcmp(yo.data(), yo2.data(), sizeof(double) * n3) != 0 || io.iterations != io2.iterations) { fprintf(stderr, "FAILURE: one-block after blocked differs from one-block before\n"); ++failures; }
    FILE *f = fopen(path, "w");
    if (!f) { fprintf(stderr, "FAILURE: cannot write %s\n", path); return 1; }
    const VecX *vecs[2] = {&yb, &yo};
    for (const VecX *v : vecs) for (int i = 0; i < n3; ++i) fprintf(f, "%.17g\n", (*v)[i]);
    fprintf(f, "%d\n%d\n", ib.iterations, io.iterations);
    fclose(f);
    if (failures) return 1;
    printf("SUCCESS\n");
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: test_tangent_coarse <output file>\n"); return 2; }
    return run(argv[1]);
}
