// Solver.hpp -- admm::Solver of the MI355X build (reference: src/Solver.hpp:32-124).
// Same public surface; initialize() flattens the scene into an admm_hip_desc and step() runs the whole
// ADMM loop on the GPU through include/admm_hip.h.  m_x / m_v stay valid host-side after every step.
#ifndef ADMM_SOLVER_HPP
#define ADMM_SOLVER_HPP 1

#include <string>
#include <unordered_map>
#include "ConstraintSet.hpp"
#include "EnergyTerm.hpp"
#include "SpringEnergyTerm.hpp"
#include "BendEnergyTerm.hpp"
#include "ExplicitForce.hpp"
#include "LinearSolver.hpp"
#include "PassiveObject.hpp"

namespace admm {

namespace solver_detail {

// Solver::Settings (src/Solver.hpp:39-50): command-line switches in the comments
struct SolverSettings {
    SolverSettings() : timestep_s(1.0 / 24.0), verbose(1), admm_iters(10), gravity(-9.8), linsolver(0), constraint_w(-1), soft_modes(0), monitor(0), admm_tol(0.0), admm_min_iters(1), anderson(0) {}
    double timestep_s;   // -dt
    int verbose;         // -v
    int admm_iters;      // -it
    double gravity;      // -g
    int linsolver;       // -ls  0 = LDLT (here: GPU PCG), 1 = NCMCGS, 2 = UzawaCG
    double constraint_w; // -ck  (-1 = automatic)
    int soft_modes;      // -sm  (GPU build, appended: the reference's fields keep their order) every PCG solve ends with an exact Galerkin step on
                         //      the k softest modes of the system matrix (admm_hip_compute_soft_modes at initialize); 0 = off
    int monitor;         //      (GPU build, appended) ADMM monitor of every step (admm_hip_set_monitor): 0 off, 1 residuals, 2 residuals + objective,
                         //      3 = 2 + stationarity; -monitor
    double admm_tol;     // -tol (GPU build, appended) early exit of a step's ADMM loop (admm_hip_set_admm_stop): the loop stops after the iteration whose
                         //      residuals meet  |W(Dx - z)| <= tol max(|W z|, |W D x|)  and  |W(z - z_prev)| <= tol |W z|; 0 = off
    int admm_min_iters;  //      (GPU build, appended) ... but not before this many iterations (>= 1)
    int anderson;        // -aa  (GPU build, appended) Anderson acceleration of a step's ADMM loop (admm_hip_set_anderson): window 0 (off) .. 8
    void help();
    bool parse_args(int argc, char **argv);   // true when help() was printed
};

// Solver::RuntimeData (src/Solver.hpp:54-61): filled from admm_hip_stats after every step
struct SolverRuntimeData {
    SolverRuntimeData() : global_ms(0), local_ms(0), collision_ms(0), inner_iters(0), admm_iters(0) {}
    double global_ms, local_ms, collision_ms;
    int inner_iters;
    int admm_iters;      // (GPU build, appended) ADMM iterations the step executed: Settings::admm_iters, fewer with Settings::admm_tol > 0
    void print(const SolverSettings &settings);
};

// One ADMM iteration of the last step as the monitor recorded it (Settings::monitor; include/admm_hip.h: admm_hip_get_monitor), taken after
// the iteration's global solve: primal = |W(Dx - z)|, dz = |W(z - z_prev)|, wz = |W z|, wdx = |W D x|; elastic energy, inertia term
// 1/(2 dt^2) |x - x_bar|^2_M and their sum, the objective (the last three 0 with monitor = 1); stationarity = |(M (x - x_bar) / dt^2 +
// grad E(x))_free| over the nodes without an active pin (monitor = 3, else 0).
struct AdmmRecord { double primal, dz, wz, wdx, energy, inertia, objective, stationarity; };
// One ADMM iteration of the last step as the Anderson acceleration decided it (Settings::anderson; include/admm_hip.h: admm_hip_get_anderson):
// the evaluation was accepted; it started from an extrapolated state; entries in the ring after it (0 after a rejection or a cleared
// ring); |F_k|; theta (zeros beyond entries - 1).
struct AndersonRecord { bool accepted, accelerated; int entries; double resid, theta[8]; };
// Stress of one tet (include/admm_hip.h: admm_hip_stress): first Piola-Kirchhoff stress P = dpsi/dF column-major, the signed stretches, the von
// Mises stress of the Cauchy stress P F^T / J (at J -> 0: what the arithmetic gives)
struct TetStress { double P[9], stretches[3], von_mises; };

} // namespace solver_detail

class Solver {
public:
    typedef solver_detail::SolverSettings Settings;
    typedef solver_detail::SolverRuntimeData RuntimeData;
    typedef solver_detail::AndersonRecord AndersonRecord;
    typedef solver_detail::AdmmRecord AdmmRecord;
    typedef solver_detail::TetStress TetStress;

    Solver();
    virtual ~Solver();

    // ---- scene data the callers fill directly (src/Solver.hpp:66-73) ----
    VecX m_x, m_v, m_masses;                                      // three entries per node
    std::vector<std::shared_ptr<EnergyTerm> > energyterms;
    std::vector<std::shared_ptr<ExplicitForce> > ext_forces;
    std::vector<int> surface_inds;                                // collision candidates (empty = every node)

    // ---- the life cycle (all virtual in the reference as well) ----
    virtual bool initialize(const Settings &settings_ = Settings());
    virtual void step();
    virtual void set_pins(const std::vector<int> &inds, const std::vector<Vec3> &points = std::vector<Vec3>());
    // Slide constraints (README.md:23-28 TODO of the reference; the counterpart of set_pins for normal-only constraints): node inds[i] may move
    // in the plane through points[i] with normal normals[i].  Replaces the current set; after initialize() only nodes that had a slide
    // constraint at initialize() may be given again (like pins with linsolver 0 / 2, src/Solver.cpp:147-151).
    virtual void set_slide_pins(const std::vector<int> &inds, const std::vector<Vec3> &points, const std::vector<Vec3> &normals);
    virtual void add_obstacle(std::shared_ptr<PassiveCollision> obj);
    virtual void add_dynamic_collider(std::shared_ptr<DynamicCollision> obj);
    virtual void save_matrix(const std::string &filename);
    virtual const RuntimeData &runtime_data() { return m_runtime; }
    const Settings &settings() { return m_settings; }

    // appends n_verts nodes (positions x, masses m, three values each); returns the new node count (src/Solver.hpp:127-141)
    template <typename T> int add_nodes(T *x, T *m, int n_verts) {
        const int old_size = m_x.size(), extra = 3 * n_verts;
        m_x.conservativeResize(old_size + extra);
        m_v.conservativeResize(old_size + extra);
        m_masses.conservativeResize(old_size + extra);
        for (int i = 0; i < extra; ++i) { m_x[old_size + i] = x[i]; m_masses[old_size + i] = m[i]; m_v[old_size + i] = 0.0; }
        return (old_size + extra) / 3;
    }

    // ---- additions of the GPU build ----
    int device;                                                   // HIP device ordinal used by initialize() (default 0)
    // User-defined PassiveCollision subclasses are sampled at initialize() on obstacle_grid_nodes^3 nodes over the box
    // [obstacle_grid_lo, obstacle_grid_hi]; an empty box (lo >= hi, the default) = the bounding box of m_x grown by half its diagonal.
    int obstacle_grid_nodes; Vec3 obstacle_grid_lo, obstacle_grid_hi;
    bool build_global_matrices;                                   // initialize() fills m_D / m_Dt / m_W_diag / solver_Dt_Wt_W (default true, like
                                                                  // the reference; the GPU path itself never reads them -- switch off for very large scenes)
    std::shared_ptr<LinearSolver> linear_solver() { return m_linsolver; }
    // Sum of EnergyTerm::energy(D, x) over all terms (pins have none), reduced on the device (admm_hip_energy); after initialize()
    double energy(const VecX &x);
    // Internal forces f = -dE/dx of that energy, three values per node, and the stress of every tet term in the order of energyterms
    // (admm_hip_forces, admm_hip_stress); after initialize()
    VecX forces(const VecX &x);
    std::vector<TetStress> stress(const VecX &x);
    // K(x) d + shift (m o d), K = d2E/dx2 = -d forces / dx the exact tangent stiffness of that energy at x, m the nodal masses
    // (admm_hip_stiffness_apply); shift = 1 / dt^2: the Jacobian of the implicit-Euler residual.  Pins are not masked; after initialize()
    VecX stiffness_apply(const VecX &d, const VecX &x, double shift = 0.0);
    // The same from the tangent frozen at x (admm_hip_stiffness_apply_ex): psd projects every element tangent to its nearest positive
    // semi-definite one, hold_pins holds the pinned vertices (their rows are 0, d is ignored there)
    // block: through the block pass (ADMM_HIP_TANGENT_BLOCK), the same bits
    VecX stiffness_apply(const VecX &d, const VecX &x, double shift, bool psd, bool hold_pins, bool block = false);
    // The k lowest eigenpairs of (K(x) + shift M) phi = theta M phi on the free vertices by LOBPCG on the device (admm_hip_modes):
    // returns phi, column i = mode i (three values per node, M-orthonormal, 0 on held vertices); info->lambda = theta - shift ascending.
    // guard < 0 means min(4, 16 - k).  A body without held vertices needs shift > 0
    struct ModesInfo { int iterations, converged_modes, restarts, ended_by; std::vector<double> lambda, residual; };
    std::vector<VecX> modes(int k, const VecX &x, ModesInfo *info = nullptr, double shift = 0.0, bool psd = true, bool hold_pins = true,
                            double tol = 1e-8, int max_iters = 2000, int guard = -1);
    // y with (K(x) + shift M) y = rhs on the free vertices: Jacobi-PCG on the device (admm_hip_tangent_solve); shift < 0 means 1 / dt^2
    struct SolveInfo { int iterations; bool converged; double residual, rhs_norm; };
    VecX tangent_solve(const VecX &rhs, const VecX &x, SolveInfo *info = nullptr, double shift = -1.0, bool psd = true, bool hold_pins = true,
                       double tol = 1e-10, int max_iters = 1000);
    // tangent_solve for a stack of right-hand sides on the same frozen operator (admm_hip_tangent_solve_block): one setup, k independent
    // CG recurrences that share every launch; y[j] and info->columns[j] have the bits of tangent_solve(rhs[j]).  block_iterations: of
    // the longest column; column_passes: the columns applied over all iterations; blocked: false with the two-level preconditioner
    struct BlockSolveInfo { std::vector<SolveInfo> columns; int block_iterations, column_passes; bool blocked; };
    std::vector<VecX> tangent_solve_block(const std::vector<VecX> &rhs, const VecX &x, BlockSolveInfo *info = nullptr, double shift = -1.0, bool psd = true,
                                          bool hold_pins = true, double tol = 1e-10, int max_iters = 1000);
    // The preconditioner of the CG behind tangent_solve, newton_polish and step_adjoint (admm_hip_set_tangent_precond): Jacobi (the
    // default), or two-level with the affine displacements of `aggregates` compact aggregates (0: n_verts / 256 in 1 .. 64) as coarse space
    enum class TangentPrecond { Jacobi = 0, TwoLevel = 1 };
    struct TangentPrecondInfo { TangentPrecond kind; int aggregates, coarse_dim, coarse_dropped; bool coarse_ok; int setup_passes; };      // the last four: of the last solve
    void set_tangent_precond(TangentPrecond kind, int aggregates = 0);
    TangentPrecondInfo tangent_precond();
    // The dense inverse of the coarse matrix behind the two-level preconditioner (admm_hip_set_tangent_coarse): one workgroup (the
    // default), or blocked in 64 x 64 tiles over the chip; launches: of the last inverse
    enum class TangentCoarse { OneBlock = 0, Blocked = 1 };
    struct TangentCoarseInfo { TangentCoarse solver; int tile, launches; };
    void set_tangent_coarse(TangentCoarse solver);
    TangentCoarseInfo tangent_coarse();
    // Projected Newton with a backtracking line search on the objective of the last step(), applied to its result; m_x and m_v are
    // updated (admm_hip_newton_polish).  One record per iterate, the first is the state the step left
    struct NewtonRecord { double objective, grad_norm, cg_iterations, step, energy; };
    std::vector<NewtonRecord> newton_polish(int max_iters = 10, double grad_tol = 1e-8, double cg_tol = 1e-8, int cg_max = 500);
    // a^T d forces / d theta per energy term at x (admm_hip_param_sensitivity): tets [n_tets][4] = (d_mu, d_la, d_kappa, d_scale) in the
    // order of energyterms, tris [n_tris], hinges [n_hinges]; d_scale, tris and hinges: the derivative in a factor on the term's energy
    struct ParamSensitivity { std::vector<double> tets, tris, hinges; };
    ParamSensitivity param_sensitivity(const VecX &a, const VecX &x);
    // The adjoint of the last step() at its result (admm_hip_step_adjoint): for a loss L(x, v) with dL_dx, dL_dv (empty: 0) the
    // multiplier lam of (K(x) + M / dt^2) lam = dL_dx + dL_dv / dt on the free rows and the gradients dL/dx_bar, dL/dx_prev, dL/dv_prev,
    // dL/dm (per degree of freedom) and, with params, lam^T d forces / d theta.  x_prev and v_prev are the dL_dx and dL_dv
    // contributions of the step before: several steps chain through them.  stationarity: |r_free| of the state
    struct StepAdjoint {
        VecX lam, xbar, x_prev, v_prev, masses; ParamSensitivity params;
        int iterations; bool converged; double residual, rhs_norm, stationarity, shift;
    };
    StepAdjoint step_adjoint(const VecX &dL_dx, const VecX &dL_dv = VecX(), bool psd = false, double tol = 1e-10, int max_iters = 2000,
                             bool params = true);
    // step_adjoint for k losses at the same state (admm_hip_step_adjoint_block): dL_dv empty or one vector per loss; entry j has the
    // bits of step_adjoint(dL_dx[j], dL_dv[j]); the solves are tangent_solve_block's
    struct StepAdjointBlock { std::vector<StepAdjoint> columns; int block_iterations, column_passes; bool blocked; };
    StepAdjointBlock step_adjoint_block(const std::vector<VecX> &dL_dx, const std::vector<VecX> &dL_dv = std::vector<VecX>(), bool psd = false,
                                        double tol = 1e-10, int max_iters = 2000, bool params = true);
    // d(a . forces)/dX per rest vertex at x, X the rest positions of the tets, masses and material constants held fixed
    // (admm_hip_rest_sensitivity); three values per node.  Refused for scenes with triangles or hinges
    VecX rest_sensitivity(const VecX &a, const VecX &x);
    // dL/dx of the held vertices for the multiplier lam of step_adjoint with the same dL_dx, dL_dv (admm_hip_adjoint_held):
    // (dL_dx + dL_dv / dt) - K(x) lam on the held rows, 0 on the free ones, at the result of the last step()
    VecX adjoint_held(const VecX &lam, const VecX &dL_dx, const VecX &dL_dv = VecX());
    // the records of the last step(), one per EXECUTED ADMM iteration; empty with Settings::monitor = 0 and early exit off
    const std::vector<AdmmRecord> &admm_history() { return m_history; }
    // admm_hip_set_admm_stop after initialize(): in effect from the next step (tol = 0: off)
    void set_admm_stop(double tol, int min_iters = 1);
    // admm_hip_set_anderson after initialize(): in effect from the next step (window 0: off)
    void set_anderson(int window);
    // the records of the last step(), one per EXECUTED ADMM iteration; empty with Settings::anderson = 0
    std::vector<AndersonRecord> anderson_history();
    void *context() { return m_ctx; }                             // the admm_hip_ctx behind this solver (include/admm_hip.h), for the C ABI's extras

protected:
    void release();
    void *m_ctx;                                                  // admm_hip_ctx
    bool initialized;
    int m_n_tets;                                                 // tet terms handed to the context at initialize()
    int m_n_tris = 0, m_n_bends = 0;                              // triangle and hinge terms
    Settings m_settings;
    RuntimeData m_runtime;
    std::vector<AdmmRecord> m_history;
    // Global matrices of src/Solver.hpp:115-121, for subclasses that read them (the reference's own step() is their only other user;
    // here the device holds its own copies in kernel layouts): reduction matrix D (rows x dof) and its transpose, the weights W,
    // dt^2 D^T W^T W (dof x rows).
    SparseMat m_D, m_Dt;
    VecX m_W_diag;
    SparseMat solver_Dt_Wt_W;
    SparseMat solver_termA;                                       // Ahat (n_verts x n_verts): the reference's solver_termA = diag(m) + Ahat (x) I3
    std::shared_ptr<ConstraintSet> m_constraints;
    std::shared_ptr<LinearSolver> m_linsolver;
    std::unordered_map<int, std::shared_ptr<SpringPin> > m_pin_energies;
    std::unordered_map<int, std::shared_ptr<SlidePin> > m_slide_energies;
    void push_pins();                                            // pins + slide constraints -> the context
};

} // namespace admm
#endif
