/*
 * admm_hip.h -- C ABI of the MI355X-native ADMM elastic hot path (libadmm_hip.so).
 *
 * The reference (mattoverby/admm-elastic) has no FFI of its own: its extension points are the C++
 * classes admm::Solver / EnergyTerm / LinearSolver.  This header is the boundary those classes'
 * MI355X-native re-implementation (admm-elastic_amd/host/) sits on, and the only thing the Python
 * harness binds (ctypes).  Plain pointers and sizes, no C++/torch types.  Each entry point cites the
 * reference interface it replaces (file:line relative to the reference repo root).
 *
 * Conventions
 *   - all floating point data is FP64, all indices int32
 *   - node vectors (x, v, b, masses) are [3*n_verts], interleaved xyz, exactly like Solver::m_x
 *     (src/Solver.hpp:66-68)
 *   - 3x3 / 2x2 matrices are column-major (Eigen default)
 *   - energy-term order inside a context is: tets (given order), then tris, then bending hinges, then pins; the ADMM
 *     vectors z,u use the reference's row layout (9 rows per tet, 6 per tri, 3 per hinge, 6 per pin:
 *     src/TetEnergyTerm.hpp:68, src/TriEnergyTerm.hpp:66, src/SpringEnergyTerm.hpp:42)
 *   - every function returns 0 on success or a negative admm_hip_status; the message of the last
 *     failure on the calling thread is available from admm_hip_last_error()
 *   - a context is bound to one HIP device, owns all of its device memory, is not thread-safe
 *   - functions named admm_host_* do not touch the GPU (set-up arithmetic shared by every caller)
 */
#ifndef ADMM_HIP_H
#define ADMM_HIP_H 1

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ADMM_HIP_OK = 0,
    ADMM_HIP_ERR_ARG = -1,      /* bad argument / inconsistent description  (reference: std::runtime_error) */
    ADMM_HIP_ERR_DEVICE = -2,   /* no usable HIP device, or a HIP runtime call failed */
    ADMM_HIP_ERR_GEOMETRY = -3, /* inverted rest element (src/TetEnergyTerm.cpp:42-44, TriEnergyTerm.cpp:45-47) */
    ADMM_HIP_ERR_STATE = -4,    /* call out of order (e.g. step before set_state) */
    ADMM_HIP_ERR_COMM = -5      /* RCCL failure */
} admm_hip_status;

/* tet constitutive models -- src/TetEnergyTerm.hpp:57 (linear), :116 (NeoHookean), :142 (StVK), :176 (SplineTet).
 * SplineTet carries an xu::Spline (src/XuSpline.hpp); the three splines the reference ships are accepted with
 * : xu::NeoHookean (the default; with kappa = 0 algebraically the NH model), xu::StVK (with kappa = 0 algebraically the
 * StVK model) and xu::CoRotated (co-rotated linear: mu sum (s_i-1)^2 + lambda/2 (sum s_i - 3)^2).  tet_mu / tet_lambda are
 * the SPLINE's constants, tet_kappa its compression term (src/XuSpline.hpp:44-45; 0 = none), tet_k the tet's bulk modulus
 * (src/TetEnergyTerm.hpp:192-204).  User-defined splines have no kernel. */
enum { ADMM_TET_LINEAR = 0, ADMM_TET_NEOHOOKEAN = 1, ADMM_TET_STVK = 2, ADMM_TET_SPLINE_NH = 3, ADMM_TET_SPLINE_STVK = 4,
       ADMM_TET_SPLINE_COROTATED = 5,
       ADMM_TET_SPLINE_TABLE = 6,     /* SplineTet with a USER-DEFINED xu::Spline (src/TetEnergyTerm.hpp:197-204, src/XuSpline.hpp:34-46):
                                       * the spline's six functions sampled by admm_host_tabulate_spline, desc.tet_spline = its table */
       ADMM_TET_STABLE_NH = 7 };      /* stable Neo-Hookean (README.md:23-28 lists it as a TODO the reference never shipped; it would sit beside
                                       * NeoHookeanTet, src/TetEnergyTerm.hpp:116-136, as one more HyperElasticTet): Smith, de Goes, Kim 2018,
                                       * Psi = mu_s/2 (I_C - 3) + la_s/2 (J - alpha)^2 - mu_s/2 log(I_C + 1) with mu_s = 4/3 mu, la_s = lambda + 5/6 mu,
                                       * alpha = 1 + 3 mu_s / (4 la_s) from the tet's tet_mu / tet_lambda; finite for inverted elements */
#define ADMM_SPLINE_TABLE_DOUBLES 9228   /* doubles of one table: 3 functions x (4 header + 3 x 1024 node values) */

/* global solvers -- Solver::Settings::linsolver, src/Solver.hpp:46 ("0=LDLT, 1=NCMCGS, 2=UzawaCG").
 * 0: the prefactored LDLT (src/LinearSolver.hpp:59-92) is replaced by a preconditioned CG (Jacobi, or a block-local
 *    symmetric Gauss-Seidel sweep on 2-colourable meshes) on
 *    the GPU iterated to pcg_tol; 1: nodal multi-colour SOR (src/NodalMultiColorGS.hpp); 2: Schur-
 *    complement CG (src/UzawaCG.hpp) whose inner LDLT solves are the same GPU PCG. */
enum { ADMM_LS_LDLT_AS_PCG = 0, ADMM_LS_NCMCGS = 1, ADMM_LS_UZAWACG = 2 };

/* passive obstacles -- src/PassiveObject.hpp:32-45 (Floor: params[0]=y), :48-64 (Sphere: cx,cy,cz,r).
 * User-defined PassiveCollision subclasses (src/Collider.hpp:66-83 is an interface of one virtual function) reach the kernels in two
 * forms: ADMM_OBJ_PLANE, the half space n.x < d (params nx, ny, nz, d; n is normalised by the library; signed distance n.x - d, contact
 * point x - dx n), and ADMM_OBJ_GRID, ANY object sampled at Solver::initialize (params[0] = index of its grid in
 * desc.obstacle_grid_meta; admm_host_sample_obstacle fills the grid from the object's own signed_distance): the kernels interpolate
 * distance and normal trilinearly and take the contact point as x - dx n (exact for a true signed distance function, O(h^2)
 * otherwise); outside its grid an object is never hit. */
enum { ADMM_OBJ_FLOOR = 0, ADMM_OBJ_SPHERE = 1, ADMM_OBJ_PLANE = 2, ADMM_OBJ_GRID = 3 };

typedef struct admm_hip_ctx admm_hip_ctx;

/* Everything Solver::initialize (src/Solver.cpp:167-261) consumes, flattened to arrays. */
typedef struct {
    int32_t struct_size;          /* = sizeof(admm_hip_desc), for forward compatibility */
    int32_t device;               /* HIP device ordinal */

    int32_t n_verts;
    const double *masses;         /* [3*n_verts]  Solver::m_masses (src/Solver.hpp:68) */
    double dt;                    /* Settings::timestep_s (src/Solver.hpp:42); <=0 -> 1/24 like Solver.cpp:175-179 */

    /* TetEnergyTerm family (src/TetEnergyTerm.cpp:31-71) */
    int32_t n_tets;
    const int32_t *tet_idx;       /* [4*n_tets] */
    const double *tet_Binv;       /* [9*n_tets] edges_inv, column-major */
    const double *tet_weight;     /* [n_tets]   w = sqrt(k*vol) */
    const int32_t *tet_kind;      /* [n_tets]   ADMM_TET_* */
    const double *tet_mu;         /* [n_tets]   Lame::mu */
    const double *tet_lambda;     /* [n_tets]   Lame::lambda */
    const double *tet_k;          /* [n_tets]   Lame::bulk_modulus() */

    /* TriEnergyTerm (src/TriEnergyTerm.cpp:29-101) */
    int32_t n_tris;
    const int32_t *tri_idx;       /* [3*n_tris] */
    const double *tri_rest;       /* [4*n_tris] rest_pose (2x2, column-major) */
    const double *tri_weight;     /* [n_tris] */
    const double *tri_limit_min;  /* [n_tris] Lame::limit_min */
    const double *tri_limit_max;  /* [n_tris] Lame::limit_max */

    /* Pins.  linsolver 0/2: every pin becomes a SpringPin energy term (src/Solver.cpp:190-196,
     * src/SpringEnergyTerm.hpp:31-73) with weight pin_weight (<=0 -> sqrt(2*k_rubber)).
     * linsolver 1: pins are applied inside the GS sweeps (src/NodalMultiColorGS.hpp:111-117). */
    int32_t n_pins;
    const int32_t *pin_vert;      /* [n_pins] */
    const double *pin_xyz;        /* [3*n_pins] */
    const int32_t *pin_active;    /* [n_pins] or NULL (= all active) */
    double pin_weight;

    int32_t linsolver;            /* ADMM_LS_* */
    double constraint_w;          /* Settings::constraint_w; <=0 -> auto (src/Solver.cpp:235,239,245) */

    int32_t pcg_max_iters;        /* <=0 -> 500.  Iterations are launched in chunks, one chunk ahead of the GPU,
                                   * and stop as soon as the device signals convergence (no stream sync). */
    double pcg_tol;               /* relative residual of the (Jacobi-scaled) system; <=0 -> 1e-10 */
    int32_t gs_max_iters;         /* <=0 -> 30   (NodalMultiColorGS::max_iters, NodalMultiColorGS.hpp:45-46) */
    double gs_tol;                /* <0 -> 1e-10 (m_tol); 0 disables the residual test like the reference */
    double gs_omega;              /* <=0 -> 1.9  (m_omega) */
    int32_t uzawa_max_iters;      /* <=0 -> 20   (UzawaCG::max_iters, UzawaCG.hpp:44-45) */
    double uzawa_tol;             /* <=0 -> 1e-10 */

    int32_t n_obstacles;          /* Solver::add_obstacle (src/Solver.cpp:159-161); needs linsolver 1 or 2 */
    const int32_t *obstacle_kind; /* [n_obstacles] ADMM_OBJ_* */
    const double *obstacle_params;/* [4*n_obstacles] */

    const int32_t *gs_colors;     /* optional [n_verts] colour per node; NULL -> greedy (admm_host_greedy_coloring) */

    /* multi-GPU: this context is rank `rank` of `world_size` (0 or 1 = single GPU).  Every rank is
     * given the FULL description; the library keeps the element block admm_host_partition assigns to
     * the rank (tets and tris separately), assembles the full matrix, and replicates the global solve. */
    int32_t rank;
    int32_t world_size;

    /* SplineTet with a spline constructed with a compression term (src/XuSpline.hpp:43-45, the `kappa` of xu::NeoHookean /
     * xu::StVK / xu::CoRotated): [n_tets] or NULL (= 0 everywhere, what the reference's own SplineTet constructors pass,
     * src/TetEnergyTerm.hpp:194).  Read for the ADMM_TET_SPLINE_* kinds only. */
    const double *tet_kappa;

    /* Optional [3 * n_verts]: any SMOOTH coordinates of the vertices -- Solver::m_x as it stands at Solver::initialize
     * (src/Solver.cpp:167), which is what both host mirrors pass.  Used ONLY to build the coarse space of the on-chip PCG's
     * two-level preconditioner: with coordinates every block carries the four functions {1, x, y, z} (the low-energy modes of
     * the Laplacian-like Ahat) instead of four piecewise-constant aggregates -- same 4 unknowns per block, the smooth error
     * modes that dominate the POSITION error of an iterate are represented to second order.  NULL = piecewise constants.
     * The solution of the system does not depend on it (a preconditioner). */
    const double *vert_xyz;

    /* Tabulated user splines (ADMM_TET_SPLINE_TABLE): n_spline_tables tables of ADMM_SPLINE_TABLE_DOUBLES doubles each, made by
     * admm_host_tabulate_spline; tet_spline [n_tets]: table of every tet (read for that kind only).  tet_mu / tet_lambda of such
     * tets are not used; tet_k is the tet's bulk modulus as for every kind. */
    int32_t n_spline_tables;
    const double *spline_tables;
    const int32_t *tet_spline;

    /* Sampled obstacles (ADMM_OBJ_GRID): obstacle_grid_meta [10 * n_obstacle_grids] = origin xyz, spacing xyz, nodes nx ny nz
     * (each >= 2), index of the grid's first node in obstacle_grid_data; obstacle_grid_data [4 per node, x fastest] = signed
     * distance, normal xyz.  Both made by admm_host_sample_obstacle. */
    int32_t n_obstacle_grids;
    const double *obstacle_grid_meta;
    const double *obstacle_grid_data;

    /* SLIDE constraints (README.md:23-28 lists them as a TODO the reference never shipped; no reference code).  [3*n_pins] or NULL:
     * a pin with a non-zero normal n (normalised by the library) constrains only n . (x - pin_xyz) = 0 -- the vertex slides in the
     * plane through the pin's point.  linsolver 0 / 2: a SpringPin term (src/SpringEnergyTerm.hpp:31-73: same D-block I3, same
     * weight) whose prox projects q = D x + u onto that plane instead of onto the point (:61); linsolver 1: inside the sweeps
     * (src/NodalMultiColorGS.hpp:111-117) the node takes the plane-constrained Jacobi value of :218-262 on its own plane.  A zero
     * normal = an ordinary pin.  admm_hip_set_pins moves the points and keeps the normals; admm_hip_set_pin_normals changes them. */
    const double *pin_normal;

    /* BENDING terms for cloth (README.md:23-28 TODO "bending force"; no reference code).  One EnergyTerm per hinge -- an interior edge
     * (v0, v1) and the two vertices v2, v3 opposite to it -- beside TriEnergyTerm (src/TriEnergyTerm.cpp:54-101): dim 3, D-block =
     * (c0, c1, c2, c3) (x) I3, i.e. D_i x = sum_k c_k x_{v_k} (the discrete mean-curvature normal of the hinge, Bergou et al. 2006, "A
     * Quadratic Bending Model for Inextensible Surfaces"), energy E(z) = bend_stiffness / 2 |z|^2, weight bend_weight, so that
     * prox(q) = q w^2 / (stiffness + w^2).  bend_idx [4*n_bends], bend_coef [4*n_bends], bend_weight [n_bends] (> 0), bend_stiffness
     * [n_bends] (>= 0).  admm_host_bend_hinges builds idx / coef / rest areas from a triangle mesh; the mirrors then use
     * stiffness = k_bend * 3 / area and weight = sqrt(stiffness) (prox = q / 2, the idiom of src/TriEnergyTerm.cpp:77-83).
     * Rows of z / u: after the triangles, before the pins, 3 per hinge. */
    int32_t n_bends;
    const int32_t *bend_idx;
    const double *bend_coef;
    const double *bend_weight;
    const double *bend_stiffness;
} admm_hip_desc;

/* Maps 1:1 onto Solver::RuntimeData (src/Solver.hpp:54-61) plus GPU-side extras. */
typedef struct {
    double global_ms;
    double local_ms;              /* the per-element prox kernels only (HIP events on the context's stream) */
    double collision_ms;
    int32_t inner_iters;
    int32_t admm_iters;
    double step_ms;               /* whole step, HIP events */
    int32_t last_solve_converged; /* PCG: residual test met within pcg_max_iters in the last ADMM iteration */
    int32_t n_constraints;        /* rows of C in the last ADMM iteration (UzawaCG) */
    double rhs_ms;                /* part of global_ms spent assembling b = M x_bar + dt^2 D^T W^2 (z-u) */
    int32_t unconverged_solves;   /* PCG solves of this step that did not meet pcg_tol (0 = every solve converged) */
    int32_t pcg_launched_iters;   /* PCG iterations launched for the last solve (converged ones exit early on the device) */
    int32_t pcg_iters_per_solve[64]; /* linsolver 0: PCG iterations of each ADMM iteration's solve (first 64) */
    double local_kernel_ms;       /* sum of the tet local-step KERNEL durations of this step, from the device wall clock
                                   * (every wave stamps its entry and, after its stores have drained, its exit; duration =
                                   * max exit - min entry): what rocprofv3 --kernel-trace reports.  local_ms above is the
                                   * PHASE between two event records, dispatch gaps included.  Opt-in (ADMM_HIP_KERNEL_CLOCK=1:
                                   * the stamps cost the launch ~2 %); 0 otherwise, or when there are no tets. */
} admm_hip_stats;

const char *admm_hip_last_error(void);

/* Number of visible HIP devices (0 when there is no GPU / no driver). Never fails. */
int admm_hip_device_count(void);

/* Solver::initialize (src/Solver.cpp:167-261): validates, uploads, assembles D / W / A on the host,
 * builds the SpMV / gather structures, colours the graph (linsolver 1). */
int admm_hip_create(const admm_hip_desc *desc, admm_hip_ctx **out);
void admm_hip_destroy(admm_hip_ctx *ctx);

/* Solver::m_x / m_v access (src/Solver.hpp:66-67).  Host <-> device copies. */
int admm_hip_set_state(admm_hip_ctx *ctx, const double *x, const double *v);
int admm_hip_get_state(admm_hip_ctx *ctx, double *x, double *v);

/* Solver::set_pins after initialize (src/Solver.cpp:113-157): move / activate / deactivate pins.
 * linsolver 0/2: idx must be among the pins given at create (else ADMM_HIP_ERR_ARG, like the throw
 * at Solver.cpp:147-151); all other pins become inactive.  linsolver 1: the set is replaced freely. */
int admm_hip_set_pins(admm_hip_ctx *ctx, int32_t n, const int32_t *vert, const double *xyz);

/* Slide pins after initialize (see desc.pin_normal): normals [3*n] of the pins at `vert` (a zero normal makes it an ordinary pin again).
 * linsolver 0 / 2: vert must be among the pins given at create; linsolver 1: among the current pins.  Points and activation are
 * admm_hip_set_pins' business. */
int admm_hip_set_pin_normals(admm_hip_ctx *ctx, int32_t n, const int32_t *vert, const double *normals);

/* Solver::ext_forces with a WindForce (src/ExplicitForce.hpp:39-46, src/ExplicitForce.cpp:47-104), applied on the DEVICE at the
 * start of every admm_hip_step, where Solver::step calls ExplicitForce::project (src/Solver.cpp:54): tris [3*n_tris] = the node
 * indices of the triangles the wind acts on (WindForce's constructor argument), direction [3] = WindForce::direction.  Every
 * triangle sees the velocities of the start of the step (the reference's OpenMP loop reads whatever its critical sections have
 * already written).  n_tris = 0 removes the force.  For callers that keep m_x / m_v on the host the C++ mirror applies the same
 * force on the host, like the reference. */
int admm_hip_set_wind(admm_hip_ctx *ctx, int32_t n_tris, const int32_t *tris, const double *direction);

/* Solver::surface_inds (src/Solver.hpp:70; filled by binding::add_tetmesh, samples/utils/AddMeshes.hpp:131-137): the
 * vertices Collider::detect tests (src/Collider.hpp:157,163).  n = 0 -> every vertex (the reference's rule for an
 * empty list).  Applies to passive detection of the UzawaCG path and to dynamic detection. */
int admm_hip_set_surface_inds(admm_hip_ctx *ctx, int32_t n, const int32_t *inds);

/* Solver::add_dynamic_collider(std::make_shared<TetMeshCollision>(mesh, vert_offset)) -- src/Solver.cpp:163-165,
 * src/DynamicObject.hpp:45-64.  rest_verts [3*n_verts], tets [4*n_tets] and faces [3*n_faces] (the surface
 * triangles, outward) index the mesh's OWN vertices; node id = local id + vert_offset.  At every ADMM iteration
 * Collider::detect (src/Collider.hpp:166-168,192-201) refits the tet tree and runs TetMeshCollision::signed_distance
 * (src/DynamicObject.hpp:72-119) for every candidate vertex; hits become the dynamic rows of
 * ConstraintSet::make_matrix (src/ConstraintSet.hpp:92-110): hard constraints of the Schur CG with linsolver 2
 * (src/UzawaCG.hpp), the penalty A + C^T C swept by the multi-colour GS with linsolver 1
 * (src/NodalMultiColorGS.hpp:75-86; the matrix is not formed and not re-coloured as a whole: only the nodes of the
 * hits are re-coloured, see csrc/dyn_collide.hpp).  linsolver 0 fails with the reference's "No collisions with LDLT
 * solver" (src/Solver.cpp:249-254).  Call after admm_hip_create, in add_dynamic_collider order. */
int admm_hip_add_dynamic_tetmesh(admm_hip_ctx *ctx, int32_t vert_offset, int32_t n_verts, const double *rest_verts,
                                 int32_t n_tets, const int32_t *tets, int32_t n_faces, const int32_t *faces);

/* Kernel-level entry point (parity tests): Collider::detect of the dynamic objects at x [3*n_verts] (host).
 * Up to cap hits are written in candidate order: vert[h], face[3h] (node ids), barys[3h], normal[3h], dx[h]
 * = DynamicCollision::Payload (src/Collider.hpp:40-53); *n_hits = number found (may exceed cap). */
int admm_hip_detect_dynamic(admm_hip_ctx *ctx, const double *x, int32_t cap, int32_t *n_hits, int32_t *vert, int32_t *face,
                            double *barys, double *normal, double *dx);

/* Solver::step (src/Solver.cpp:35-110) on the device-resident state: gravity, x_bar, admm_iters x
 * {local step, collision detection, RHS, global solve}, velocity update.  No host<->device traffic
 * besides the launch stream; stats may be NULL. */
int admm_hip_step(admm_hip_ctx *ctx, int32_t admm_iters, double gravity, admm_hip_stats *stats);

/* Kernel-level entry points (parity tests).
 * local step = the OpenMP loop at src/Solver.cpp:84-87 over EnergyTerm::update
 * (src/EnergyTerm.hpp:130-140): given x and u (in/out) produce z, u in the reference row layout.
 * If Mxbar and b_out are non-NULL also returns b = Mxbar + dt^2 D^T W^2 (z-u) (src/Solver.cpp:98).
 * Multi-GPU contexts fill only the rows of their own element block; before admm_hip_comm_init they
 * return their partial b (rank 0 carries Mxbar and the pin terms), afterwards the all-reduced one. */
int admm_hip_local_step(admm_hip_ctx *ctx, const double *x, double *u_inout, double *z_out,
                        const double *Mxbar, double *b_out);
/* LinearSolver::solve (src/LinearSolver.hpp:46): x is in/out (warm start), returns inner iterations
 * through *iters.  Uses the context's linsolver, pins and obstacles. */
int admm_hip_global_solve(admm_hip_ctx *ctx, const double *b, double *x_inout, int32_t *iters);
/* Runs the gather of the right-hand side AGAIN on what the last admm_hip_local_step left on the device (no reference counterpart;
 * tests): b = Mxbar + dt^2 D^T W^2 (z-u) into b_out [3 n_verts].  variant: 0 the kernel the step launches; | 1 its reference
 * instantiation, which loads the records of a vertex four at a time and waits for each four -- the order of the sums is the same,
 * so the two must agree bit for bit; | 2 the instantiations a step with the early exit on the device takes (they read the stop word
 * of the ADMM loop, cleared here as at the start of a step).  The gather also runs the local step of the pin terms: u_before
 * (the u handed to that admm_hip_local_step, reference row layout; may be NULL without pin terms) is where it starts from again.
 * The context's own b, pin u and pin z are put back.  Single-GPU contexts only. */
int admm_hip_regather_rhs(admm_hip_ctx *ctx, const double *u_before, int32_t variant, double *b_out);

/* Totals of the on-chip PCG since admm_hip_create (no reference counterpart): solves launched, solves that met pcg_tol,
 * inner iterations.  Synchronises the context's stream.  Lets a caller run admm_hip_step WITHOUT per-step statistics
 * (asynchronously, no events between the kernels) and still check afterwards that every solve converged.  -1 when the context
 * does not use the general-mesh on-chip PCG. */
int admm_hip_solve_totals(admm_hip_ctx *ctx, int64_t *solves, int64_t *converged, int64_t *inner_iters);   /* returns ADMM_HIP_OK; the three values are -1 when this context's solver keeps no totals */

/* EnergyTerm::energy (src/EnergyTerm.hpp:82,142-147; src/TetEnergyTerm.cpp:94-100,138-149; src/TriEnergyTerm.cpp:104-114) of every term at x, on
 * the device.  x [3*n_verts] host, or NULL = the device-resident state.  totals[4] = tets, tris, hinges, their sum.  per_term: NULL or
 * [n_tets + n_tris + n_bends] in the CALLER's term order (not the library's kind-sorted order).  Pins have no energy (the reference throws,
 * src/SpringEnergyTerm.hpp:63-66).  Every tet kind of ADMM_TET_*; triangles ignore their strain limits like the reference.  The sums are
 * bit-reproducible from run to run (no floating-point atomics).  Single-GPU contexts only.  Synchronises the stream. */
int admm_hip_energy(admm_hip_ctx *ctx, const double *x, double *totals4, double *per_term);

/* Internal forces f = -dE/dx of the energy admm_hip_energy sums (the same sign rules, triangles without their strain limits, hinges; pins
 * add nothing), and the per-tet stress from the same pass.  No reference code exists (TetEnergyTerm::gradient and TriEnergyTerm::gradient
 * throw): the forces are the gradient of the energies.  out13 [13 n_tets]: per tet the first Piola-Kirchhoff stress P = dpsi/dF column-major
 * (9), the signed stretches (3), the von Mises stress of the Cauchy stress P F^T / J (1).  Limits: at a stretch of exactly 0 the kinds
 * evaluated at |sigma| (linear, Neo-Hookean, every SplineTet) have a kink and the force is a one-sided derivative; at J -> 0 the Cauchy
 * stress, and for a collapsed triangle its force, are what the arithmetic gives (inf / NaN), nothing is clamped.  Bit-reproducible from run
 * to run.  Single-GPU contexts only.  Both synchronise the stream. */
int admm_hip_forces(admm_hip_ctx *ctx, const double *x, double *f);      /* x [3 n_verts] host or NULL = device-resident state; f [3 n_verts] = -dE/dx */
int admm_hip_stress(admm_hip_ctx *ctx, const double *x, double *out13);  /* [13 n_tets], the CALLER's tet order (tet_perm, as energy's per_term) */

/* Tangent stiffness K(x) = d2E/dx2 = -df/dx of the same energy, applied to n_vec directions: out_j = K(x) d_j + shift (m o d_j), m the
 * nodal masses.  x [3 n_verts] host or NULL = the device-resident state; d and out [n_vec][3 n_verts] host, 1 <= n_vec <= 65535.  shift = 0: the pure tangent
 * stiffness; shift = 1 / dt^2: the Jacobian of the implicit-Euler residual whose squares monitor mode 3 sums.  Pins carry no energy and
 * are not masked: the caller masks them.  K is the exact second derivative (the equal-stretch and equal-and-inverted cases in closed
 * form), NOT projected to a positive semi-definite matrix and not ADMM's constant surrogate.  Limits as for the forces: kinks at a stretch
 * of exactly 0, the log barrier of the Neo-Hookean kinds at J -> 0, a collapsed triangle -- what the arithmetic gives.  Every column is
 * bit-identical to the same direction applied alone, and from run to run.  Single-GPU contexts only.  Synchronises the stream. */
int admm_hip_stiffness_apply(admm_hip_ctx *ctx, const double *x, int32_t n_vec, const double *d, double shift, double *out);

/* The same operator from a tangent FROZEN at x (csrc/newton.hpp): one setup pass runs the SVD and the coefficients of every tet once and
 * stores a 30-double frame, every direction is then one frozen pass.  flags: ADMM_HIP_TANGENT_PSD -- every element tangent is replaced by
 * its Frobenius-nearest positive semi-definite one (tets: the twist and flip eigenvalues clamped at 0, the 3x3 block of the stretches by
 * its positive part; triangles: the twist and the two out-of-plane eigenvalues; hinges are positive semi-definite already); an element that
 * is positive semi-definite keeps its bits (eigenvalues above -2^-44 of the element's largest coefficient count as zero: the rotation
 * modes of an element at rest).  ADMM_HIP_TANGENT_HOLD_PINS -- pinned vertices (the rule of `stationarity`: active pin terms, or the pins
 * of the sweeps under linsolver 1) are held: their rows of out are 0 and d is ignored there.  flags = 0 is admm_hip_stiffness_apply in
 * another summation order (measured: <= 2e-16 of its per-vertex scale).  Bit-reproducible; a column does not depend on the others.
 * Single-GPU contexts only.  Synchronises the stream.
 * ADMM_HIP_TANGENT_BLOCK (this entry point only) -- all columns go up in one copy, through one setup and block passes of up to 16
 * directions each (an element's frame is read once per pass, not once per direction), and come back in one copy.  Every column has the
 * bits of the call without the flag. */
#define ADMM_HIP_TANGENT_PSD 1
#define ADMM_HIP_TANGENT_HOLD_PINS 2
#define ADMM_HIP_TANGENT_BLOCK 4
int admm_hip_stiffness_apply_ex(admm_hip_ctx *ctx, const double *x, int32_t n_vec, const double *d, double shift, int32_t flags, double *out);

/* Modal analysis at a deformed state: the k lowest eigenpairs of K_s phi = theta M phi on the free rows, K_s = K_frozen(x) + shift M with
 * the frozen tangent of admm_hip_stiffness_apply_ex (flags: ADMM_HIP_TANGENT_PSD, ADMM_HIP_TANGENT_HOLD_PINS), M = diag(m); held vertices
 * are dropped as row and column.  lambda = theta - shift.  LOBPCG with the Jacobi preconditioner on a block of k + guard <= 16 columns
 * (guard >= 0; a few guard columns speed up the k-th mode), all on the device (csrc/modal.hpp): per iteration a residual pass, ONE block
 * frozen pass, the Gram matrices of [X W P] by per-block partials summed in a fixed order, a one-block dense Rayleigh-Ritz (Cholesky +
 * parallel cyclic Jacobi) and the block update; iterations are enqueued in chunks of 8, the host reads one pinned word per chunk.  No
 * floating-point atomics: bit-reproducible.  Stops when the columns 0 .. k-1 meet |A x_i - theta_i M x_i| <= tol |theta_i| |M x_i|, or
 * after max_iters iterations.  A Cholesky pivot of the scaled Gram matrix that is not finite or below 64 eps is a restart (P dropped);
 * a failure on [X W] as well ends the run (breakdown) with the last X.
 * x: host positions, or NULL for the device-resident state.  init: NULL (a fixed integer hash of (column, vertex, axis): every caller
 * starts identically) or [k + guard][3 n_verts].  lambda [k] ascending; phi [k][3 n_verts], M-orthonormal (the returned block passes a last
 * Rayleigh-Ritz), 0 on held vertices; info [4 + k]: iterations, converged modes (k when the run ended by tol, else how many of the true
 * residuals meet tol), restarts, ended-by (0 tol, 1 max_iters, 2 breakdown), then per mode the TRUE residual
 * |A x_i - theta_i M x_i| / (|theta_i| |M x_i|) from one more block pass on the returned X.
 * Without ADMM_HIP_TANGENT_PSD the operator may be indefinite (M is positive definite): the lowest eigenvalues are then the negative
 * ones.  A body without held vertices needs shift > 0: its six rigid modes have theta = shift, and the relative stop test needs
 * theta != 0.  Refused (ADMM_HIP_ERR_ARG): multi-GPU contexts, k < 1, guard < 0, k + guard > 16, 3 (k + guard) above the number of free
 * unknowns, a non-finite shift or tol, tol < 0, max_iters < 1.  Synchronises the stream. */
int admm_hip_modes(admm_hip_ctx *ctx, const double *x, int32_t k, int32_t guard, double shift, int32_t flags, double tol, int32_t max_iters,
                   const double *init, double *lambda, double *phi, double *info);

/* Solves (K(x) + shift M) y = rhs on the free vertices by Jacobi-preconditioned CG, matrix-free on the frozen tangent, on the context's
 * stream.  x as above; rhs and y [3 n_verts] host; flags as above (on held vertices y = 0 and rhs is ignored).  Stops at
 * |r| <= tol |rhs| (2-norms over the free rows, r the recursive residual) or after max_iters iterations.  alpha, beta and the stop
 * decision live on the device: iterations are enqueued in chunks of 8 (four launches each), the host reads one pinned word per chunk
 * and synchronises once at the end; no grid barrier, no persistent kernel, no floating-point atomics: bit-reproducible.
 * info4 = {iterations, converged (0 / 1), |rhs - A y| / |rhs| of the returned y, |rhs|}: the residual is formed once more at the end (one
 * more application); the recursive one of the stop test drifts from it by about eps cond(A) |rhs|, 7e-4 of a residual of 1e-12 |rhs|.  Without ADMM_HIP_TANGENT_PSD the operator can be indefinite and CG can
 * break down: the solve then ends with converged = 0 at the first p.Ap <= 0 or non-finite scalar and returns the iterate before it.
 * Single-GPU contexts only (tabulated-spline tets need the context's table, which admm_hip_create already demands). */
int admm_hip_tangent_solve(admm_hip_ctx *ctx, const double *x, const double *rhs, double shift, int32_t flags, double tol, int32_t max_iters,
                           double *y, double *info4);

/* admm_hip_tangent_solve for a STACK of k >= 1 right-hand sides rhs [k][3 n_verts] on the same frozen operator (host; y [k][3 n_verts]):
 * one setup and one diagonal per call, then k INDEPENDENT CG recurrences that share every launch (csrc/newton.hpp: the block PCG; not a
 * block-Krylov method).  Each column keeps its own alpha, beta, stop decision and breakdown rule: column j is the single solve of rhs_j,
 * bit for bit -- y, and info [k][4], laid out per column as info4 above.  A column that has ended drops out of the launches from the
 * next iteration on (a column list kept on the device); one stop word ends the solve with its last column; chunks of 8 iterations, one
 * pinned word per chunk, one synchronisation per slab: no host decision inside the solve.  More than 16 columns run in slabs of 16.
 * block_info3 = {block iterations: those of the longest column (of the longest slab), column_passes: the columns applied over all
 * iterations, counted on the device (sum_j iterations_j, + 1 for a column that ended in a breakdown), blocked (1)}.
 * With the two-level preconditioner selected (admm_hip_set_tangent_precond) the columns are solved one after the other as
 * admm_hip_tangent_solve solves them -- the two-level preconditioner has no block form -- and blocked = 0 (block iterations: the longest
 * column's, column_passes: their sum).  Refused as admm_hip_tangent_solve, with the same codes, and for k < 1. */
int admm_hip_tangent_solve_block(admm_hip_ctx *ctx, const double *x, int32_t k, const double *rhs, double shift, int32_t flags, double tol,
                                 int32_t max_iters, double *y, double *info, double *block_info3);

/* The preconditioner of the CG behind admm_hip_tangent_solve, admm_hip_newton_polish and admm_hip_step_adjoint, in effect from the next
 * solve.  kind 0 (the default): Jacobi, D^-1 with D the diagonal of A = K(x) + shift M.  kind 1: two-level, M^-1 = D^-1 + P (P^T A P)^-1 P^T
 * with P the affine displacements {1, (x - mean) / h} (x) {e_x, e_y, e_z} of `aggregates` compact aggregates of vertices (12 columns each;
 * zero on held vertices), the aggregates cut once by recursive coordinate bisection of desc.vert_xyz, the functions taken at the x the
 * tangent is frozen at.  P^T A P is formed matrix-free at the start of every solve (ceil(12 aggregates / 16) block passes of the frozen
 * tangent) and inverted on the device.  A column whose diagonal is <= 2^-40 of the largest is DROPPED (an aggregate held entirely; a flat
 * cloth); a coarse matrix that is otherwise not positive definite (no ADMM_HIP_TANGENT_PSD at a compressed state; shift 0 with nothing
 * held) switches the coarse term off for that solve, on the device: the solve is then Jacobi-PCG.  Six launches per iteration instead of
 * four; bit-reproducible.  aggregates 0 means clamp(n_verts / 256, 1, 64).  With kind 0 every call returns the bits it returned before
 * this entry point existed.  Refused (ADMM_HIP_ERR_ARG): kind outside 0 .. 1, aggregates outside 0 .. 64 or above n_verts, kind 1 on a
 * context created without desc.vert_xyz, multi-GPU contexts. */
int admm_hip_set_tangent_precond(admm_hip_ctx *ctx, int32_t kind, int32_t aggregates);
/* The setting, and of the LAST solve: coarse_dim = 12 aggregates (0: it ran with Jacobi), the columns dropped, coarse_ok (1: the coarse
 * term was used; 0: switched off), the block passes of its setup.  Any pointer may be NULL.  Synchronises the stream. */
int admm_hip_get_tangent_precond(admm_hip_ctx *ctx, int32_t *kind, int32_t *aggregates, int32_t *coarse_dim, int32_t *coarse_dropped, int32_t *coarse_ok,
                                 int32_t *setup_passes);
/* Tests: z = M^-1 r of the two-level preconditioner (whatever kind is set; the aggregates as set) of the tangent frozen at x -- the setup
 * of a solve, then one application.  x, shift, flags as admm_hip_tangent_solve; r, z_out [3 n_verts] host (r is ignored and z is 0 on
 * held vertices).  admm_hip_get_tangent_precond then describes this setup. */
int admm_hip_tangent_precond_apply(admm_hip_ctx *ctx, const double *x, const double *r, double shift, int32_t flags, double *z_out);
/* The dense inverse of the coarse matrix P^T A P behind the two-level preconditioner, in effect from the next solve.  solver 0 (the
 * default): one workgroup on the matrix in global memory.  solver 1: BLOCKED, a tiled Cholesky and a tiled L^-T L^-1 in 64 x 64 tiles
 * held in LDS, one launch per phase spread over the chip (about 40 launches at 64 aggregates), with the same rules for dropped columns
 * and for a matrix that is not positive definite; the two inverses differ by rounding.  Bit-reproducible; with solver 0 every call
 * returns the bits it returned before this entry point existed.  Refused (ADMM_HIP_ERR_ARG): solver outside 0 .. 1, multi-GPU contexts. */
int admm_hip_set_tangent_coarse(admm_hip_ctx *ctx, int32_t solver);
/* The setting, the tile size of the blocked inverse, and the kernel launches of the LAST inverse (1 with solver 0; 0 before the first).
 * The last inverse is the setup of the last two-level solve or application, OR a later call of admm_hip_tangent_coarse_invert: the test
 * hook counts here too.  Any pointer may be NULL. */
int admm_hip_get_tangent_coarse(admm_hip_ctx *ctx, int32_t *solver, int32_t *tile, int32_t *last_launches);
/* Tests: X = A^-1 by the selected inverse, on the device, of a caller's symmetric A [n][n] (host, row-major), 1 <= n <= 768 (n need not be
 * a multiple of 12 or of the tile).  *ok = 1 and *dropped = the columns with a diagonal <= 2^-40 of the largest (their rows and columns
 * of X are zero, the rest is the inverse of the rest), or *ok = 0 and X = 0 for a matrix that is not positive definite or not finite.
 * Runs in scratch of its own: a tangent solve after it returns the bits it would have returned without it.  Synchronises the stream. */
int admm_hip_tangent_coarse_invert(admm_hip_ctx *ctx, int32_t n, const double *A_host, double *X_host, int32_t *ok, int32_t *dropped);

/* Projected Newton on the objective of the LAST step, Phi(x) = |x - x_bar|_M^2 / (2 dt^2) + E(x) (what monitor mode 2 sums), applied to
 * the device-resident state: per iteration g = (m o x - M x_bar) / dt^2 - f(x) with the pinned rows zeroed; stop at |g| <= grad_tol;
 * else (K_psd(x) + M / dt^2) delta = -g by admm_hip_tangent_solve (both flags, cg_tol, cg_max), Armijo backtracking on Phi (c = 1e-4,
 * halving, at most 10 trials, a non-finite Phi is a rejection); x += t delta, v += t delta / dt.  Without an accepted trial the polish
 * ends with the last accepted iterate.  At most max_newton steps.  records [cap][5], *n of them written (one per iterate, the first is
 * the state the step left): Phi, |g_free|, the CG iterations and the accepted step length of the step taken FROM that iterate (0, 0: none
 * -- converged, max_newton reached or no trial accepted), the elastic energy E.  One host synchronisation per Newton iteration and per
 * line-search trial, none inside a solve.  Refused (ADMM_HIP_ERR_ARG): multi-GPU contexts, contexts with colliders, with strain-limited
 * triangles (a limit min > 0 or max < 100) or with slide pins, and a state no step has run on (admm_hip_set_state resets that). */
int admm_hip_newton_polish(admm_hip_ctx *ctx, int32_t max_newton, double grad_tol, double cg_tol, int32_t cg_max, int32_t cap, int32_t *n,
                           double *records);

/* The derivative of the internal forces in what a user tunes, contracted with k vectors a [k][3 n_verts] (host): out = a_j^T df/dtheta
 * per ENERGY TERM at x (host positions, or NULL for the device-resident state), in the order the terms were added (csrc/adjoint.hpp:
 * k_param_sens; one pass per 16 columns, the SVD of a tet runs once per pass).
 *   out_tets  [k][n_tets][4] = (d_mu, d_la, d_kappa, d_scale): the derivative in the tet's Lame constants and kappa AS THE LIBRARY STORES
 *             THEM (tet_mu, tet_lambda, tet_kappa of the description) and in a factor on the tet's energy, d_scale = a . f_e.  With
 *             F = U diag(sigma) V^T, sg_i = s_i dpsi/de_i and A^ = U^T Ds(a) Binv V:  d_scale = -vol sum_i sg_i A^_ii,
 *             d_theta = -vol sum_i (d sg_i / d theta) A^_ii.  Every density's sg is linear in (mu, la, kappa), so for the six kinds with
 *             such constants mu d_mu + la d_la + kappa d_kappa = d_scale.  The linear tet and the tabulated spline have none on the
 *             device: their three columns are exactly 0 and d_scale carries everything (linear tet: d/dk_bulk = d_scale / k).
 *   out_tris  [k][n_tris], out_bends [k][n_bends]: sum_c a_c . f_{e,c}, the derivative in a factor on the term's energy (w^2 of a
 *             triangle, the stiffness of a hinge).
 * Any output pointer may be NULL.  Sums over groups of terms (one mu per material) are the caller's.  Column j of a stack has the bits
 * of a_j alone; no atomics: bit-reproducible.  Limits as admm_hip_forces (kinks of the |sigma| kinds, J -> 0, strain limits ignored).
 * Single-GPU contexts only.  Synchronises the stream. */
int admm_hip_param_sensitivity(admm_hip_ctx *ctx, const double *x, int32_t k, const double *a, double *out_tets, double *out_tris,
                               double *out_bends);

/* The adjoint of the LAST implicit-Euler step at the device-resident state x.  A converged step satisfies on the free rows (the rule of
 * `stationarity`; held vertices do not move)  r = m o (x - x_bar) / dt^2 - f(x; theta) = 0,  x_bar = x_prev + dt v_prev + dt^2 a_ext,
 * v = (x - x_prev) / dt.  For a scalar loss L(x, v) with dL_dx = dL/dx and dL_dv = dL/dv (NULL: 0), all [3 n_verts] host:
 *     g_x = dL_dx + dL_dv / dt (held rows 0);   A lambda = g_x,  A = K(x) + M / dt^2 on the free rows, lambda = 0 on held rows
 *     out_xbar  = dL/dx_bar  = m o lambda / dt^2            out_xprev = dL/dx_prev = m o lambda / dt^2 - dL_dv / dt (held rows 0)
 *     out_vprev = dL/dv_prev = m o lambda / dt              out_mass  = dL/dm = -lambda o (x - x_bar) / dt^2 per degree of freedom (x_bar fixed)
 *     out_tets, out_tris, out_bends = lambda^T df/dtheta as admm_hip_param_sensitivity lays them out (k = 1)
 * out_xprev and out_vprev are the dL_dx and dL_dv contributions of the step BEFORE: several steps chain backwards through them.
 * The solve is admm_hip_tangent_solve's (tol, max_iters; shift 1 / dt^2, pins held); flags: ADMM_HIP_ADJOINT_PSD -- the projected tangent
 * (default off: the exact tangent is the Jacobian, positive definite on the free rows at a minimum; a CG breakdown ends with converged
 * = 0); ADMM_HIP_ADJOINT_PARAMS -- the parameter outputs are computed (else untouched).  Any output pointer may be NULL.
 * info6 = {iterations, converged, |g_x - A lambda| / |g_x| formed once more at the end, |g_x|, |r_free| of the state (the figure of
 * `stationarity` and of the polish: an adjoint means something at a converged state only), the shift used}.  The state is not changed;
 * one host synchronisation, at the end.  Refused like admm_hip_newton_polish (ADMM_HIP_ERR_ARG): multi-GPU contexts, contexts with
 * colliders, with strain-limited triangles or with slide pins, and a state no step has run on. */
#define ADMM_HIP_ADJOINT_PSD 1
#define ADMM_HIP_ADJOINT_PARAMS 2
int admm_hip_step_adjoint(admm_hip_ctx *ctx, const double *dL_dx, const double *dL_dv, int32_t flags, double tol, int32_t max_iters,
                          double *out_lambda, double *out_xbar, double *out_xprev, double *out_vprev, double *out_mass, double *out_tets,
                          double *out_tris, double *out_bends, double *info6);
/* admm_hip_step_adjoint for k >= 1 losses at the same state: dL_dx, dL_dv (NULL: 0) and the five vector outputs are [k][3 n_verts],
 * out_tets [k][n_tets][4], out_tris [k][n_tris], out_bends [k][n_bends], info [k][6] laid out per column as info6 above.  |r_free| of
 * the state is formed once; the right-hand sides and the outputs are formed per column with the single call's arithmetic; the k solves
 * are admm_hip_tangent_solve_block's (block_info3 as there; the same fallback with the two-level preconditioner); the parameter
 * sensitivities come from one pass over the stack of lambda per slab of 16.  Column j has the bits of admm_hip_step_adjoint on loss j.
 * Refused as admm_hip_step_adjoint, and for k < 1. */
int admm_hip_step_adjoint_block(admm_hip_ctx *ctx, int32_t k, const double *dL_dx, const double *dL_dv, int32_t flags, double tol,
                                int32_t max_iters, double *out_lambda, double *out_xbar, double *out_xprev, double *out_vprev, double *out_mass,
                                double *out_tets, double *out_tris, double *out_bends, double *info, double *block_info3);

/* The derivative of the internal forces in the REST positions X of the tets (the verts behind add_tets), contracted with k vectors
 * a [k][3 n_verts] (host): out [k][3 n_verts] = d(a_j . f)/dX per rest vertex at x (host positions, or NULL for the device-resident
 * state), masses and material constants held fixed (csrc/adjoint.hpp: k_rest_sens; one pass per 16 columns, the SVD of a tet runs once
 * per pass).  Per tet, with Binv = Dm^-1, vol, F = Ds(x) Binv, P = dpsi/dF, A = Ds(a) Binv and T = H[A] (the exact element tangent):
 *     d(a . f_e)/dDm = Gs Binv^T,   Gs = -vol [ (P : A) I - F^T T - A^T P ];   rest corner m + 1 gets column m, corner 0 minus their sum.
 * With a = lambda of admm_hip_step_adjoint this is dL/dX, the gradient of inverse design.  A caller whose masses are lumped from the
 * rest volumes adds the chain through out_mass.  Column j of a stack has the bits of a_j alone; no atomics: bit-reproducible.  Limits as
 * admm_hip_stiffness_apply.  Refused (ADMM_HIP_ERR_ARG): multi-GPU contexts, and contexts that hold triangles or hinges -- the library is
 * handed a triangle's rest matrix and a hinge's stencil, not the rest positions behind them, and a partial gradient is not returned.
 * Synchronises the stream. */
int admm_hip_rest_sensitivity(admm_hip_ctx *ctx, const double *x, int32_t k, const double *a, double *out);

/* The gradient of admm_hip_step_adjoint's loss in the positions of the HELD vertices (where the pins hold them), at the device-resident
 * state: with lam = out_lambda of admm_hip_step_adjoint for the same dL_dx, dL_dv (NULL: 0),
 *     out_held = (dL_dx + dL_dv / dt) - K(x) lam   on the held rows,  0 on the free rows    ([3 n_verts], host)
 * K the exact tangent of all terms without the mass shift (one admm_hip_stiffness_apply pass).  Refused exactly where
 * admm_hip_step_adjoint is.  The state is not changed.  Synchronises the stream. */
int admm_hip_adjoint_held(admm_hip_ctx *ctx, const double *lam, const double *dL_dx, const double *dL_dv, double *out_held);

/* Kernel-level entry point (parity tests): x [3*n_verts], z and z_prev [admm_hip_num_rows] in the reference row layout (host).
 * out4 = |W(Dx - z)|, |W(z - z_prev)|, |W z|, |W D x|   (2-norms over all rows, pins included).  Single-GPU contexts only. */
int admm_hip_residuals(admm_hip_ctx *ctx, const double *x, const double *z, const double *z_prev, double *out4);

/* Monitor of admm_hip_step: 0 off (default), 1 residuals, 2 residuals + objective, 3 = 2 + the stationarity residual of implicit Euler,
 * |(M (x - x_bar) / dt^2 + grad E(x))_free| over the vertices without an active pin (one force pass more per iteration; contact reactions
 * are not subtracted, so with colliders the figure contains them).  In effect from the next step.  Off, a step is what it
 * was: no launch more, no kernel changed.  On, the local step also stores z and one reduction over the terms follows every global solve, on
 * the context's stream, without any host synchronisation.  Single-GPU contexts only. */
int admm_hip_set_monitor(admm_hip_ctx *ctx, int32_t mode);
/* Records of the LAST step, one per ADMM iteration s, taken after that iteration's global solve with x = x^{s+1}, z = z^{s+1},
 * z_prev = z^{s} (z^0 = D m_x at step entry, src/Solver.cpp:70).  records [cap][8]: the four norms above, elastic energy,
 * inertia term 1/(2 dt^2) |x - x_bar|^2_M, their sum (the objective; the last three 0 in mode 1), the stationarity residual (mode 3; 0 otherwise).
 * *n = iterations recorded (may exceed cap; 0 when the last step ran with the monitor off).  Synchronises the stream. */
int admm_hip_get_monitor(admm_hip_ctx *ctx, int32_t cap, int32_t *n, double *records);

/* EARLY EXIT of a step's ADMM loop on the monitor's residuals.  With the record of iteration s as admm_hip_get_monitor returns it
 * (primal = |W(Dx - z)|, dz = |W(z - z_prev)|, wz = |W z|, wdx = |W D x|) the loop stops AFTER iteration s when
 *     s + 1 >= min_iters   and   primal <= tol * max(wz, wdx)   and   dz <= tol * wz
 * (compared in this product form: 0 <= 0 stops, a NaN never does).  tol = 0 (default) switches it off: a step is then exactly what it
 * was -- the same kernels, the same bits.  tol >= 0 and finite, min_iters >= 1, else ADMM_HIP_ERR_ARG; in effect from the next step;
 * single-GPU contexts only (refused with tol > 0 where admm_hip_set_monitor is).  While tol > 0:
 *   - a step runs with the monitor in mode max(mode, 1); admm_hip_get_monitor returns exactly the executed iterations' records, with
 *     the bits a step of that many iterations records;
 *   - admm_hip_stats::admm_iters is the EXECUTED count; unconverged_solves, inner_iters, pcg_iters_per_solve and the per-phase times
 *     describe the executed iterations only;
 *   - the decision is taken ON THE DEVICE, and the iterations behind it are skipped there (launched ahead as before, every kernel
 *     returns at once), on contexts whose global solve is the on-chip PCG or the persistent Gauss-Seidel sweep, without colliders that
 *     need the host.  The step then ends with ONE stream synchronisation (the host learns the count) and has none inside the loop;
 *   - everywhere else -- bodies beyond the chip (launch-path PCG), UzawaCG with passive or dynamic colliders, the Gauss-Seidel
 *     colour-kernel fall-backs, dynamic colliders, contexts that gave up their persistent kernels, ADMM_HIP_STOP_HOST=1 (read at
 *     create) -- the host takes the same decision: ONE EVENT SYNCHRONISATION PER ADMM ITERATION, then the one at the end.  Same rule,
 *     same count;
 *   - admm_hip_persistent_launches, admm_hip_pcg_instances and admm_hip_solve_totals count executed solves, not the no-op launches
 *     behind the stop.  The opt-in launch diagnostics do include them where the device skips: the event pairs of
 *     admm_hip_time_local_launches also time the empty local-step launches, and under ADMM_HIP_KERNEL_CLOCK=1 a skipped launch leaves
 *     its stamps zero and adds nothing to local_kernel_ms. */
int admm_hip_set_admm_stop(admm_hip_ctx *ctx, double tol, int32_t min_iters);
/* The values in effect and, of the LAST step: the ADMM iterations it executed (= its admm_iters with tol = 0) and whether the
 * remaining ones were skipped on the device (1) or never launched because the host decided (0; also 0 with tol = 0).  Pointers may be
 * NULL; asking for last_iters or on_device synchronises the stream. */
int admm_hip_get_admm_stop(admm_hip_ctx *ctx, double *tol, int32_t *min_iters, int32_t *last_iters, int32_t *on_device);
/* The stop test itself on one record (rec8 as admm_hip_get_monitor returns it; entries 0..3 are read): 1 = stop.  Host code, no GPU:
 * the same inline function the device decision calls. */
int admm_host_admm_stop_test(const double *rec8, double tol);

/* ANDERSON ACCELERATION of a step's ADMM loop (Zhang, Peng, Ouyang, Deng 2019).  The fixed-point map G takes the state s = (x, u) an
 * iteration starts from to g = (x after the global solve, u after the local step); F = g - s, measured in
 * <a, b> = sum_v m_v / dt^2 a_x b_x + sum_rows w^2 a_u b_u.  A ring keeps the newest window + 1 accepted pairs (g_j, F_j); it is empty
 * and r_acc = +inf at the start of EVERY step.  After the global solve of iteration k:
 *   - s_k was extrapolated and |F_k|^2 > r_acc: the evaluation is REJECTED -- the next state is the g of the last accepted evaluation,
 *     the ring is cleared, r_acc stays; the evaluation that follows is accepted whatever its residual;
 *   - otherwise ACCEPTED: r_acc = |F_k|^2, (g_k, F_k) is pushed, and with p >= 2 entries theta solves
 *     (H + 1e-10 (tr H / (p - 1)) I) theta = dF^T F_k, H = dF^T dF over the differences of consecutive entries (FP64 Cholesky);
 *     s_{k+1} = g_k - sum_j theta_j (g_{j+1} - g_j).  A pivot that is not positive and finite or a theta that is not finite clears the
 *     ring, s_{k+1} = g_k; so does p < 2 without clearing;
 *   - nothing is extrapolated behind the last iteration: the step's x is the solve output of the last accepted evaluation;
 *   - with admm_hip_set_admm_stop, a rejected evaluation cannot end the step.
 * Every decision is taken on the device; the host enqueues three launches more per iteration and never waits.  window = 0 (default)
 * switches it off: a step is then exactly what it was -- the same kernels, the same bits.  In effect from the next step.  Refused
 * (ADMM_HIP_ERR_ARG): a window outside 0..8, and with window > 0 multi-GPU contexts, contexts with colliders (obstacles or dynamic meshes)
 * and linsolver 1 and 2. */
int admm_hip_set_anderson(admm_hip_ctx *ctx, int32_t window);
/* Records of the LAST step, one per executed ADMM iteration k (none when it ran with window 0).  records [cap][12]: accepted (1 / 0),
 * accelerated (s_k was an extrapolated state), entries (the ring after this evaluation: p; 0 after a rejection or a cleared ring),
 * |F_k|, theta [8] (zeros beyond p - 1; computed and recorded at the step's last iteration too, where it is not applied).
 * *n = iterations recorded (may exceed cap).  Synchronises the stream. */
int admm_hip_get_anderson(admm_hip_ctx *ctx, int32_t cap, int32_t *n, double *records);

/* The LinearSolver objects' public tuning members, changed AFTER Solver::initialize.  The reference reads them on every solve --
 * NodalMultiColorGS::max_iters / m_tol / m_omega (src/NodalMultiColorGS.hpp:40-46, used at :100 and :136-140), UzawaCG::max_iters /
 * m_tol (src/UzawaCG.hpp:44-45, used at :92 and :109) -- so a caller may cast Solver::m_linsolver and change them between steps.
 * kind = ADMM_LS_NCMCGS (max_iters, tol, omega), ADMM_LS_UZAWACG (max_iters, tol) or ADMM_LS_LDLT_AS_PCG (max_iters, tol of the GPU
 * PCG that stands for the prefactored solve, with linsolver 0 or 2); ADMM_HIP_ERR_ARG when the context does not run that solver.
 * max_iters <= 0, tol < 0 (GS: tol = 0 switches the residual test off, like the reference; the others: tol <= 0) and omega <= 0 keep
 * the current value.  In effect from the next solve.  admm_hip_get_solver_params reads the values in effect (pointers may be NULL). */
int admm_hip_set_solver_params(admm_hip_ctx *ctx, int32_t kind, int32_t max_iters, double tol, double omega);
int admm_hip_get_solver_params(const admm_hip_ctx *ctx, int32_t kind, int32_t *max_iters, double *tol, double *omega);

/* End projection of every PCG solve on SOFT MODES (linsolver 0 / 2; no reference counterpart -- the reference solves exactly).  Z [k][n_verts]:
 * k <= 64 smooth scalar fields, normally the lowest eigenvectors of K = diag(m) + Ahat (one field serves the three axes).  After every solve
 * of the ADMM loop the iterate is corrected by the exact Galerkin step x += Z (Z^T K Z)^-1 Z^T (b - A x), which removes the error a
 * residual-norm stop leaves in span(Z) -- the soft modes in which the error of an inexact solve is largest and accumulates from frame to
 * frame.  The same step is also taken IN FRONT of the second solve of every frame (ADMM's transient: what the recycled warm start leaves of its
 * entry error lies in these modes; ADMM_HIP_DEFL_START=mask at create chooses other solves, 0 none).  The result of a converged solve changes
 * only within the solver's tolerance.  k = 0 removes the modes. */
int admm_hip_set_soft_modes(admm_hip_ctx *ctx, int32_t k, const double *Z);
/* ... with the modes computed by the library: the k lowest eigenvectors of K by `iters` (<= 0: 8) steps of inverse subspace iteration on
 * the context's own PCG (a few seconds at 1 M tets, once per scene -- A never changes after Solver::initialize, src/Solver.cpp:225-226).
 * With the on-chip PCG and k <= 32 the projection is part of the solve's one persistent launch (one more all-to-all).  Multi-rank contexts:
 * every rank computes the modes of the system it solves (element blocks: the replicated system; components: its own bodies); refused with the
 * distributed solve (ADMM_HIP_DIST_SOLVE=1). */
int admm_hip_compute_soft_modes(admm_hip_ctx *ctx, int32_t k, int32_t iters);
/* the modes in effect: *k, and Z [k][n_verts] when Z is not NULL */
int admm_hip_get_soft_modes(admm_hip_ctx *ctx, int32_t *k, double *Z);

/* Contact work since admm_hip_create (measurement: that a timed region really exercised the collision path).  linsolver 2: rows of C
 * (ConstraintSet::make_matrix, src/ConstraintSet.hpp:59-116) summed over all UzawaCG solves; linsolver 1: node updates replaced by the
 * plane-constrained update of src/NodalMultiColorGS.hpp:218-262 (a row projected onto a passive obstacle), summed over all sweeps
 * (passive obstacles; dynamic hits of the GS path are penalty rows and not counted); linsolver 0: 0.  Synchronises the stream (GS). */
int admm_hip_contact_totals(admm_hip_ctx *ctx, int64_t *rows);

/* Launches of the three persistent solver kernels since admm_hip_create (no reference counterpart): the on-chip PCG (one per solve of
 * linsolver 0 / 2 and per batch of K^-1 columns), the multi-colour GS, the Schur CG of UzawaCG.  After a barrier / hand-off time-out
 * the context falls back to the launch-per-iteration kernels for good: the counts then stop growing (tests). */
int admm_hip_persistent_launches(const admm_hip_ctx *ctx, int64_t *pcg, int64_t *gs, int64_t *schur);

/* What the on-chip PCG (k_pcg2) has found out about this context since admm_hip_create and acts on for good (no reference counterpart; diagnostics,
 * tests): *smoother_given_up -- a pipelined pass broke off with negative or non-finite sums far from convergence, later solves run with the Jacobi
 * smoother instead of the block-local Chebyshev polynomial (slower, as exact); *trust_revoked -- a sampled verification of a short first pass
 * failed, every later solve verifies its residual; *failed_checks -- how many such checks failed.  Any pointer may be NULL.  The solves of
 * admm_hip_compute_soft_modes (right-hand sides that are nearly eigenvectors) do not count: their findings are put back (round 6: until then
 * they switched the smoother off for every context that computed its modes).  Synchronises the stream. */
int admm_hip_pcg_findings(admm_hip_ctx *ctx, int32_t *smoother_given_up, int32_t *trust_revoked, int64_t *failed_checks);

/* Which instance of the on-chip PCG kernel served this context's solves (no reference counterpart; diagnostics, tests).  k_pcg2 exists twice per
 * block size: a generic instance, and a hot one with the configuration of the ADMM loop's solves fixed at compile time (same arithmetic, same
 * results; ADMM_HIP_OC_GENERIC=1 forces the generic one).  *last: the instance of the last solve launched on the context's own stream -- 0 none
 * yet, 1 generic, 2 hot; launches[4]: launches since admm_hip_create of the hot and of the generic instance, and how many of each ran on
 * UzawaCG's column lanes (the hot one never does); *last_verifications: how often that last solve left its pipelined iteration to verify the
 * true residual -- the rare path both instances keep behind the iteration loop (-1: no on-chip solve yet; asking for it synchronises the
 * stream).  Any pointer may be NULL. */
int admm_hip_pcg_instances(admm_hip_ctx *ctx, int32_t *last, int64_t *launches, int32_t *last_verifications);

/* What the on-chip PCG (k_pcg2) of this context runs on, as admm_hip_create planned it (no reference counterpart; diagnostics, tests).  out[8]:
 * [0] the on-chip solver serves the context's solves (0: no plan, the launch path was asked for, or the context gave it up); [1] blocks G,
 * [2] waves per block, [3] threads per block T of the plan (0 without one; kept after a give-up); [4] 1 the two-level preconditioner, 0 the
 * block smoother alone; [5] 1 the vector exchanges are ordered by the neighbour hand-off lists, 0 by grid barriers -- a plan in which a block
 * has more than 64 neighbour blocks has no lists, and ADMM_HIP_OC_HANDOFF=0 at create leaves them out of any plan (a test switch: same
 * arithmetic, same bits, generic instance only); [6] most neighbour blocks of a block of the plan, -1 when one has more than 64; [7] 1 after a
 * grid barrier or hand-off timed out and the context gave the persistent kernels up for good (seen at the synchronisation behind it). */
int admm_hip_pcg_plan_info(const admm_hip_ctx *ctx, int64_t *out);

/* Device memory the library holds in this process (no reference counterpart; diagnostics, tests): the number of live device buffers of all
 * contexts and their total size in bytes.  A destroyed context leaves none of its own behind.  Any pointer may be NULL. */
int admm_hip_device_buffers(int64_t *buffers, int64_t *bytes);

/* Diagnostics of the on-chip PCG (linsolver 0 / 2; no reference counterpart): the latency floor of the two
 * synchronisations one CG iteration consists of, measured on this context's grid with the kernel's own primitives and
 * payloads but no arithmetic, as microseconds per repetition over n repetitions: the all-to-all (block record -> grid barrier
 * -> every block reads every record) and the vector exchange (publish 32 B per row -> neighbour flags -> halo fetch).  0 when
 * the context has no on-chip plan.  plan_stats [6] (may be NULL): off-diagonal non-zeros, stored SELL entries, entries held in
 * LDS, block-local non-zeros, most neighbour blocks of a block, coarse unknowns of the two-level preconditioner. */
int admm_hip_probe_sync(admm_hip_ctx *ctx, int32_t n, double *us_all_to_all, double *us_exchange, int64_t *plan_stats);

/* Measurement only (bench.py `roofline`; no counterpart in the reference, whose MicroTimer brackets the whole local loop,
 * src/Solver.cpp:83-88).  on = 1: every later admm_hip_step WITHOUT statistics records a hipEvent pair around the launches of
 * its local step (all constitutive models of one ADMM iteration) on the context's stream -- nothing else changes, no
 * synchronisation is added.  admm_hip_local_launch_times synchronises the stream and returns the number of pairs recorded since
 * the last call and the sum of their intervals in milliseconds (kernel + the two dispatch gaps of the pair).
 * on = 2: the pair is attached to the dispatch of the dominant local-step kernel instead (hipExtLaunchKernelGGL start / stop events:
 * the kernel's own begin and end time stamps, the duration a profiler reports for it). */
int admm_hip_time_local_launches(admm_hip_ctx *ctx, int32_t on);
int admm_hip_local_launch_times(admm_hip_ctx *ctx, int64_t *n_pairs, double *sum_ms);

/* Sizes: R = rows of D (9*n_tets + 6*n_tris + 6*n_pin_terms).  A context of the component partition (whole bodies per rank) holds
 * only its rank's bodies: it returns the rows of THOSE (the kernel-level entry points that use this layout refuse such a context);
 * step statistics are per rank as well. */
int admm_hip_num_rows(const admm_hip_ctx *ctx);

/* The assembled scalar system matrix Ahat (A = M + Ahat (x) I3, src/Solver.cpp:225-226 with the
 * x/y/z replication of src/TetEnergyTerm.cpp:66-68 factored out), CSR with sorted columns.
 * Pass NULL pointers to query nnz only. */
int admm_hip_get_matrix(const admm_hip_ctx *ctx, int32_t *rowptr, int32_t *col, double *val, int32_t *nnz);
/* colour per node used by linsolver 1 */
int admm_hip_get_colors(const admm_hip_ctx *ctx, int32_t *color, int32_t *n_colors);

/* ---- multi-GPU (one context per rank; new work, no reference counterpart -- SURVEY.md 8e) ----
 * Element-block partition: rank r owns the contiguous block of tets/tris admm_host_partition gives
 * it; every rank holds all vertices and replicates the global solve; the only exchange is one RCCL
 * sum all-reduce of the [3*n_verts] partial right-hand side per ADMM iteration. */
int admm_hip_comm_unique_id(char *id128);                                   /* ncclGetUniqueId */
int admm_hip_comm_init(admm_hip_ctx *ctx, const char *id128, int rank, int world_size);
/* What the context's RCCL communicator says about itself (ncclCommCount / ncclCommUserRank: 0 / -1 without a communicator) and which
 * device the context sits on (device_id64: at least 64 chars, "pci <bus id> uuid <hex>") -- printed by bench.py in its N > 1 line so
 * that a scaling run can be checked for N distinct devices in ONE communicator.  Pointers may be NULL. */
int admm_hip_comm_info(const admm_hip_ctx *ctx, int32_t *n_ranks, int32_t *rank, char *device_id64);
/* The same exchange over the CALLER's transport instead of RCCL (MPI, gloo, a test harness that puts several ranks on one device
 * -- which RCCL refuses): once per ADMM iteration the library copies the partial right-hand side to pinned host memory, calls
 * fn(user, host_buf, 3 * n_verts) -- which must sum host_buf in place over all ranks and return 0 -- and copies the result back.
 * Two PCIe copies and one stream synchronisation per ADMM iteration: a functional path, not the fast one.  A context with a
 * communicator (admm_hip_comm_init) ignores it.  fn = NULL removes it. */
typedef int (*admm_allreduce_fn)(void *user, double *host_buf, int64_t n);
int admm_hip_set_rhs_allreduce(admm_hip_ctx *ctx, admm_allreduce_fn fn, void *user);
void admm_host_partition(int32_t n_items, int world_size, int rank, int32_t *begin, int32_t *end);

/* A user-defined xu::Spline on the device (src/XuSpline.hpp:34-46 is an interface of six virtual functions; the reference calls them
 * inside its L-BFGS, src/TetEnergyTerm.cpp:243-265).  `fn(user, which, x)` returns f, g, h, df, dg, dh (which = 0..5) at x > 0;
 * the functions are sampled over stretches in [s_min, s_max] (f), their pairwise products (g) and triple products (h) on grids
 * uniform in ln x, second derivatives by central differences of df / dg / dh, into table_out [ADMM_SPLINE_TABLE_DOUBLES].  The
 * kernels evaluate the C2 quintic Hermite interpolant (relative error of the energy gradient ~1e-10 for splines as smooth as
 * the reference's).  Returns ADMM_HIP_ERR_ARG for a bad range or a non-finite sample.  admm_host_spline_table_eval evaluates a
 * table as the device does: out3 = {F, F', F''} of function which (0 f, 1 g, 2 h) at x (tests). */
typedef double (*admm_spline_fn)(void *user, int which, double x);
int admm_host_tabulate_spline(admm_spline_fn fn, void *user, double s_min, double s_max, double *table_out);
void admm_host_spline_table_eval(const double *table, int which, double x, double *out3);

/* Multi-GPU, component-aware partition (the reference has no distributed layer).  When a scene has at least
 * world_size connected components (bodies that share no vertex), admm_hip_create gives every rank WHOLE bodies: its context
 * holds only them, renumbered locally, and steps them like a single-GPU scene -- no exchange inside a step, the global solve
 * is the rank's block of the block-diagonal system matrix.  The caller keeps the global numbering (set_state / get_state /
 * set_pins translate; admm_hip_get_state merges the ranks' parts over RCCL when admm_hip_comm_init was called -- it is then a
 * COLLECTIVE call: every rank must make it, each runs both merges whatever pointers it passes).  Loose vertices (no element) are not
 * bodies; a scene whose largest body holds more than twice a rank's fair share of the elements uses element blocks instead.  Components go
 * to ranks by decreasing element count, each to the least loaded rank so far.  Otherwise (a single body, or
 * ADMM_HIP_PARTITION=elements) the element-block partition above is used.  This host-only function returns the number of
 * components and, in vertex_rank [n_verts], the rank that would own every vertex. */
int32_t admm_host_component_partition(const admm_hip_desc *desc, int world_size, int32_t *vertex_rank);

/* ---- host-side set-up arithmetic (no GPU) ---- */
/* The matrix admm_hip_create would assemble for this description (same code path), without a GPU:
 * Ahat in CSR (see admm_hip_get_matrix).  Pass NULL arrays to query nnz. */
int admm_host_assemble_matrix(const admm_hip_desc *desc, int32_t *rowptr, int32_t *col, double *val, int32_t *nnz);
/* TetEnergyTerm ctor (src/TetEnergyTerm.cpp:31-48): Binv [9*n], vol [n]; ADMM_HIP_ERR_GEOMETRY if a
 * rest volume is negative.  verts [3*nv], idx [4*n]. */
int admm_host_tet_rest(int32_t n, const int32_t *idx, const double *verts, double *Binv, double *vol);
/* Rest positions behind a set of edges_inv (no reference counterpart; src/TetEnergyTerm.cpp:31-48 builds every Binv from the
 * vertex positions it is handed).  admm_hip_create calls this on the tets it is given: when ONE set of vertex positions
 * reproduces every tet's Binv to 1e-11, the local step gathers those positions (vertex data, cache-resident) and recomputes
 * Binv instead of streaming 72 bytes per tet and launch.  candidate [3*n_verts] or NULL is tried first (admm_hip_create
 * passes desc.vert_xyz); otherwise positions are propagated from tet to tet through inv(Binv), one translation per connected
 * component.  Returns 1 (candidate), 2 (propagated), 0 (the tets do not share one set of rest positions: Binv is streamed),
 * -1 bad arguments; x0_out [3*n_verts].  ADMM_HIP_TET_REST=0 in the environment keeps Binv streamed (A/B, tests). */
int admm_host_tet_rest_positions(int32_t n_verts, int32_t n_tets, const int32_t *idx, const double *Binv,
                                 const double *candidate, double *x0_out);
/* UzawaCG's Schur iterations (src/UzawaCG.hpp:92-120) apply A^-1 to C^T d.  A never changes after initialize and C^T d is
 * non-zero only at constrained vertices, so the library keeps the columns of K^-1 (A = K (x) I3) of every vertex that has ever
 * carried a constraint row: solved once by the on-chip PCG at 1e-2 x pcg_tol (<= 1e-10), three per launch, kept in HBM
 * (grown on demand up to ADMM_HIP_UZ_CACHE_MB, default 16384).  The Schur iterations then run on the active vertices only (the
 * active x active block of K^-1; ADMM_HIP_UZ_COMPACT=0: one pass over the full-height active columns per iteration) and x is
 * updated once from the multiplier update.  ADMM_HIP_UZ_CACHE=0: every Schur iteration is a PCG solve.  columns: cached columns (-1: cache off); column_solves: PCG
 * launches spent on columns; schur_from_columns / schur_by_pcg: Schur iterations served either way since create; evicted:
 * columns given up because the cache was full (it then drops the columns of every vertex that is not active in the current solve). */
int admm_hip_uzawa_cache_stats(admm_hip_ctx *ctx, int64_t *columns, int64_t *column_solves, int64_t *schur_from_columns,
                               int64_t *schur_by_pcg, int64_t *evicted);
/* Column solves that did NOT meet their tolerance within max(pcg_max_iters, 2000) iterations since create: their batch is not cached
 * (an inexact column would be a wrong Schur operator for every later solve), the solve that asked for them applies A^-1 by inner PCG
 * solves instead.  0 in every healthy run. */
int admm_hip_uzawa_unconverged_columns(admm_hip_ctx *ctx, int64_t *n);
/* The column solves of a batch run side by side on up to 8 streams when several instances of the on-chip PCG kernel fit the chip at
 * once (small bodies: the kernel of a 20 k-vertex body holds 77 of 256 CUs and is bound by its grid barrier's latency).  The count is
 * the occupancy of the kernel, never more; ADMM_HIP_UZ_LANES=n (1..8) lowers it, 1 = the main stream only.  batches: batches solved on
 * more than one stream since create; lanes: streams set up (at create for scenes with colliders, else by the first such batch).
 * LOOK-AHEAD (opt-in: ADMM_HIP_UZ_AHEAD=frames, e.g. 4; default 0 = off; admm_hip_step, passive objects, bodies that leave room for the
 * lanes beside the loop's own solve): in the first solve of a step the vertices that would reach an object within that many frames at their current speed get their
 * columns solved on the lanes WHILE the ADMM loop goes on; they are committed when done, a touchdown that needs one still in flight
 * waits for it.  ahead_columns: columns committed that way; ahead_waits: solves that had to wait.  Same columns to the tolerance of a
 * column (the three vertices of a launch share its iteration count), same active sets.  Trades throughput (columns of vertices that never
 * touch: -2 % over 200 frames of the bench's contact scene) for the absence of a stall in the touchdown frame. */
int admm_hip_uzawa_column_lanes(admm_hip_ctx *ctx, int64_t *batches, int *lanes, int64_t *ahead_columns, int64_t *ahead_waits);
/* A user-defined PassiveCollision on the device (src/Collider.hpp:66-83; the reference calls signed_distance per vertex inside
 * Collider::detect_passive, :137-150).  fn(user, x, out7) evaluates the object at x on a FRESH payload: out7 = signed distance, contact
 * point xyz, normal xyz.  Sampled at the nx x ny x nz nodes of the box [lo, hi] (each n >= 2) into meta10_out (node offset 0: the
 * caller adds the offset of the grid inside its obstacle_grid_data) and data_out [4 * nx * ny * nz].  Returns ADMM_HIP_ERR_ARG for a bad
 * box or a non-finite sample. */
typedef void (*admm_obstacle_fn)(void *user, const double *x3, double *out7);
int admm_host_sample_obstacle(admm_obstacle_fn fn, void *user, const double *lo3, const double *hi3, const int32_t *dims3, double *meta10_out,
                              double *data_out);
/* which of the above this context's local step uses: 0 streamed Binv, 1 / 2 rest positions; -1 NULL context */
int admm_hip_tet_rest_mode(const admm_hip_ctx *ctx);
/* TriEnergyTerm ctor (src/TriEnergyTerm.cpp:29-52): rest [4*n], area [n]. */
int admm_host_tri_rest(int32_t n, const int32_t *idx, const double *verts, double *rest, double *area);
/* Bending hinges of a triangle mesh (desc.bend_*; no reference counterpart): every interior edge shared by exactly two triangles gives
 * one hinge (v0 < v1 the edge, v2 / v3 the opposite vertices of the first / second triangle in index order), hinges sorted by (v0, v1).
 * coef = (c03 + c04, c01 + c02, -(c01 + c03), -(c02 + c04)) with the cotangents of the REST angles at v0 (c01 in the first triangle, c02 in
 * the second) and at v1 (c03, c04): sum_k coef_k x_k = 0 for any flat configuration; area = rest area of the two triangles.
 * Returns the number of hinges (may exceed cap: then only cap are written; NULL arrays to count). */
int32_t admm_host_bend_hinges(int32_t n_verts, int32_t n_tris, const int32_t *tris, const double *verts, int32_t cap,
                              int32_t *hinge_idx, double *coef, double *area);
/* Lame (src/EnergyTerm.hpp:34-59) */
void admm_host_lame(double youngs, double poisson, double *mu, double *lambda, double *bulk);
/* Greedy nodal colouring on a CSR pattern (role of the absent mcl::graphcolor::color_matrix,
 * src/NodalMultiColorGS.hpp:57): the better of first-fit in index order and DSATUR; deterministic; returns the
 * number of colours. */
int admm_host_greedy_coloring(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t *color);
/* Mesh preprocessing (no counterpart in the reference, whose CPU solvers do not care): a vertex numbering with locality.
 * The kernels gather positions, corner forces and matrix rows by vertex index, and the on-chip PCG hands vector slices
 * between the blocks that own neighbouring index ranges, so the numbering a mesh arrives with decides how coherent all of
 * that is (1 M-tet cube: lexicographic numbering 1.37 ms per ADMM iteration, randomly renumbered 3.57 ms).  Reverse
 * Cuthill-McKee on the element graph; idx = [corners * n_elems] vertex ids (corners 3 or 4); new_id[v] = new index of
 * vertex v; span_before / span_after (may be NULL) = mean |i - j| over element edges, the figure to decide by.  The
 * caller renumbers its mesh (vertices, elements, pins) BEFORE building the solver: the library never renumbers behind
 * the API (m_x keeps the caller's order). */
void admm_host_locality_order(int32_t n_verts, int32_t n_elems, int32_t corners, const int32_t *idx, int32_t *new_id,
                              double *span_before, double *span_after);

/* The plan admm_hip_create makes for the on-chip PCG of linsolver 0 / 2 (the GPU replacement of LDLTSolver::solve,
 * src/LinearSolver.hpp:87-90), without a GPU -- diagnostics and tests.  The solve renumbers the rows internally (the
 * caller's numbering is kept at the API): n_blocks compact blocks (one per CU) of slices_per_block wavefronts, every block
 * split into 4 compact aggregates that carry the coarse space of the two-level preconditioner
 * M^-1 = D^-1 + P (P^T A P)^-1 P^T.  row_vertex [64 * n_blocks * slices_per_block]: vertex of every internal row (-1 =
 * unused slot); row_aggregate (same length): coarse unknown of the row (block * 4 + aggregate); row_weights (NULL to skip)
 * [4 * rows]: the row's weights in the four coarse functions of its block, i.e. row r of P -- one-hot on the aggregate
 * without desc.vert_xyz, (1, x, y, z) centred and scaled per block with it; coarse_inv [nc * nc], nc =
 * 4 * n_blocks: (P^T A P)^-1, row-major (NULL to skip); stats [11]: off-diagonal non-zeros, stored SELL entries, entries
 * held in LDS, block-local non-zeros, most neighbour blocks of a block (-1: more than 64), coarse unknowns (0 = two-level
 * off), largest halo list, LDS slab columns used, 1e9 x the estimate of lambda_max(D^-1 A_bb) the block-local smoother is built
 * on (A_bb = entries of M + Ahat inside one block), 1e6 x the lanes on the busiest LDS bank pair per half-wavefront column with the
 * entries in index order / as placed.  lds_bytes = LDS a block may spend on its local vector and matrix slab. */
int admm_host_oc_plan(const admm_hip_desc *desc, int32_t n_blocks, int32_t slices_per_block, int32_t lds_bytes,
                      int32_t *row_vertex, int32_t *row_aggregate, double *coarse_inv, int64_t *stats, float *row_weights);
/* The halo lists of the same plan (same arguments), no GPU -- tests.  halo_ptr [n_blocks + 1]: offsets of the blocks' lists; halo_src and
 * halo_vert [halo_ptr[n_blocks]] (either may be NULL: call once for halo_ptr, the sizes): the internal row of every halo entry, and its
 * vertex -- what the on-chip kernel reads the halo of a solve's entry x through. */
int admm_host_oc_plan_halo(const admm_hip_desc *desc, int32_t n_blocks, int32_t slices_per_block, int32_t lds_bytes,
                           int32_t *halo_ptr, int32_t *halo_src, int32_t *halo_vert);

/* The plan of the LAUNCH-PATH two-level PCG (csrc/pcg_big.hpp; csrc/oc_plan.cpp: build_big_plan) for this scene, no GPU -- bodies beyond the
 * chip's LDS and the fall-back of the on-chip solver; replaces the same prefactored solve, src/LinearSolver.hpp:87-90.  The vertices are
 * dealt to G compact aggregates of `ra` rows each (at most max_aggregates, <= 0: 1024); stats [6]: G, ra, rows (G ra), coarse unknowns nc
 * = 4 G, their padded count, SELL slices.  row_vertex [rows] (-1 = unused slot), row_weights [4 rows] (row r of P, energy-orthonormal per
 * aggregate), coarse_inv [nc nc] = (P^T A P)^-1 in single precision; any of the three may be NULL (call once for the sizes). */
int admm_host_big_plan(const admm_hip_desc *desc, int32_t max_aggregates, int32_t *stats, int32_t *row_vertex, double *row_weights, float *coarse_inv);
/* The aggregates of the two-level tangent preconditioner (admm_hip_set_tangent_precond), no GPU: the n_verts vertices at xyz [3 n_verts]
 * in G parts (1 .. min(64, n_verts)) by recursive coordinate bisection -- the longest extent, cut at the median in a stable order.
 * agg_ptr [G + 1], agg_vert [n_verts]: the vertices grouped by aggregate, ascending within one. */
int admm_host_tangent_plan(int32_t n_verts, const double *xyz, int32_t G, int32_t *agg_ptr, int32_t *agg_vert);

/* The plan of the PERSISTENT multi-colour Gauss-Seidel kernel (csrc/gs_persist.hpp; csrc/oc_plan.cpp: build_gs_plan) run ON THE HOST, no
 * GPU (tests): `sweeps` plain SOR sweeps (src/NodalMultiColorGS.hpp:180-216, no pins, no obstacles) over the plan's own data -- blocks, the ELL of
 * every (block, colour) with local columns, halo lists, outbox nodes -- in the kernel's order of phases, x [3 n_verts] in and out.  A plan that
 * drops or misroutes an entry, a halo value or a boundary row gives another x than the sweeps on the assembled matrix.  color [n_verts] as
 * from admm_host_greedy_coloring; max_blocks / rows_target <= 0: 256 / 384; stats [6] (may be NULL): blocks, colours, LDS bytes of the fullest
 * block, largest halo list, most neighbour blocks, most rows of a block. */
int admm_host_gs_plan_sweeps(const admm_hip_desc *desc, int32_t n_colors, const int32_t *color, int32_t max_blocks, int32_t rows_target,
                             const double *b, double *x, int32_t sweeps, double omega, int32_t *stats);

/* Mesh preprocessing, second ordering (no counterpart in the reference): hierarchical BLOCK order.  The vertices are split
 * into compact leaves of about `leaf` vertices by recursive graph bisection (the method the on-chip PCG uses for its blocks),
 * leaves numbered in recursion-tree order, vertices breadth-first inside a leaf.  Reverse Cuthill-McKee minimises the
 * bandwidth, i.e. the index distance of neighbours; this order minimises the ACTIVE WINDOW of the per-vertex gathers (corner
 * forces, positions): on an unstructured 1 M-tet body the right-hand-side gather fetches 2x less.  Same contract as
 * admm_host_locality_order: new_id[v] = new index of vertex v, the caller renumbers its mesh before building the solver. */
void admm_host_block_order(int32_t n_verts, int32_t n_elems, int32_t corners, const int32_t *idx, int32_t leaf, int32_t *new_id);

/* Test hook for the host-side plan of the local step's block-level reduction (csrc/host_setup.hpp: TetChunks; no counterpart
 * in the reference, whose right-hand side is the sparse product D^T W^2 (z - u), src/Solver.cpp:98).  Runs the plan on the host
 * exactly as the kernels do: every chunk of 256 consecutive tets (chunks do not straddle kind_begin[k], the starts of the five
 * constitutive-model groups, kind_begin[5] = n_tets) sums its corner forces [n_tets][4][3] per vertex into records of at most 8
 * corner forces, the per-vertex lists of records are summed into vertex_sums [n_verts][3].
 * stats[0..4] = chunks, records, most 256-record passes of a chunk, widest record list, stored list entries. */
int admm_host_chunk_reduce(int32_t n_verts, int32_t n_tets, const int32_t *tet_idx, const int32_t *kind_begin, const double *corner_forces,
                           double *vertex_sums, int64_t *stats);

#ifdef __cplusplus
}
#endif
#endif /* ADMM_HIP_H */
