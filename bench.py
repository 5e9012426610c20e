"""bench.py -- ADMM iterations/sec of the MI355X-native hot path (Solver::step) on synthetic tet meshes.

A "step" = one Solver::step() (one frame) = `admm_iters` ADMM iterations {local step, RHS gather,
global solve} on a device-resident state (no host<->device traffic inside the timed region).

  python bench.py --gpus 1 --steps K --warmup W [--workload blob1m_mix|cube1m_mix|cube1m_nh|cube100k_gs|...] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline (metric, value, unit, higher_is_better, dtype,
ms_per_step, with the run's configuration).  --full adds everything else: statistics frames behind the timed ones (phase
split, iteration counts, convergence and finiteness checks), the contact leg, the PCIe-inclusive rate, the weak leg of an
N-GPU line, the roofline figures and the CPU baselines.  --dump-outputs DIR writes the state the last timed step computed
(m_x, m_v: what a caller of Solver::step receives) as DIR/<name>.npy.

Workloads (BASELINE.json `configs`):
  blob1m_mix   configs[2] as named ("1M-tet synthetic bunny/dragon, StVK + Neo-Hookean mix"): the DEFAULT.  Unstructured
               body (meshes.unstructured_blob, 1 012 608 tets / 183 844 verts, valences 3..26), soft rubber, feet pinned,
               g=-9.8, dt=1/24, 20 ADMM iters/step, global solve = UzawaCG (linsolver 2; no obstacle in the scene, so every
               solve is the prefactored solve of src/UzawaCG.hpp:78-81 = the recycled on-chip PCG).  With --gpus N > 1 the SAME
               body at fixed tet count: element-block partition, one RCCL all-reduce of the right-hand side per ADMM iteration
               (BASELINE configs[3], "scaling": "strong"); the weak series (one body per GPU) rides along as `weak_value`
  cube1m_mix   the same config on the n=55 Kuhn cube (998 250 tets; round 1's headline mesh), x=0 face pinned
  cube1m_nh    same mesh, all Neo-Hookean (the north-star's target mesh)
  cube100k_gs  configs[1]: n=26 (105 456 tets), Neo-Hookean, multi-colour GS global step

Prints ONE JSON line (rank 0).  value = ADMM iterations/sec over the whole job.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# Tolerance of the GPU PCG that replaces the reference's exact (prefactored LDLT) solves.  Chosen by the parity bar, not by speed:
# the loosest value at which blob1m_mix stays within 1e-5 of the bounding box of the converged trajectory (same path at 1e-12,
# every pass verified) at EVERY one of the driver's 25 frames, with margin (tests/test_bench_parity.py).  Round 3's 1e-8 met the bar
# for two frames and drifted to 4.6e-4 by frame 21 (profiles/r04_drift_tolerance_study.txt: 1e-9 6.5e-6 at 25 frames but 1.7e-5 at
# 50, 7e-10 8.6e-6 at 50, 5e-10 2.9e-6 at 50).
PCG_TOL = 7e-10
# Round 5: the 200-frame drift record (tests/test_bench_parity.py, profiles/r05_drift_tolerance_200_frames.txt) put round 4's 5e-10 at 1.06e-5 --
# over the bar at frame 192 (25 frames: 2.1e-6, 50: 4.1e-6, 100: 9.0e-6) -- 4e-10 at 9.1e-6, 3e-10 at 8.0e-6, 2e-10 at 3.1e-6, 1e-10 at 1.4e-6.  What
# the error consists of is the part of every solve's residual that lives in the body's soft modes, so the bench now ends every solve with the
# exact Galerkin projection of its residual on the 24 lowest modes of the system matrix (admm_hip_compute_soft_modes; inside the persistent
# launch): 3.9e-6 over 200 frames at 7e-10 (32 modes: 4.4e-6; 5e-10 + 32: 2.8e-6; 1e-9 + 32: 9.0e-6).  In the driver's window (20 frames after
# 5) 7e-10 + 24 modes runs 2 333 ADMM it/s against 2 030 at the plain tolerance that meets the same bar (2e-10), 2 555 at round 4's 5e-10.
SOFT_MODES = 24

# Round 6: EVERY quoted workload carries the settings its own 200-frame drift record supports (`workload_settings`; records under profiles/,
# asserted by tests/test_bench_parity.py).  The Kuhn cubes (one face pinned: no soft global modes) sit at 5e-9 of the bounding box over 200 frames at
# the blob's settings -- three decades inside the bar -- and hold 1.3e-6 at pcg_tol 1e-7 without any soft-mode step (profiles/r06_drift_cubes.txt:
# 2e-9 3.8e-8, 1e-8 2.2e-7, 5e-8 8.2e-7, 1e-7 1.26e-6 -- the largest value is frame 0's, i.e. the solves' own error, not drift).
CUBE_PCG_TOL = 1e-7

WORKLOADS = {
    "cube1m_mix": dict(n=55, kinds="mix", linsolver=0, admm_iters=20, pcg_tol=CUBE_PCG_TOL, soft_modes=0),
    "cube1m_nh": dict(n=55, kinds="nh", linsolver=0, admm_iters=20, pcg_tol=CUBE_PCG_TOL, soft_modes=0),
    "cube100k_gs": dict(n=26, kinds="nh", linsolver=1, admm_iters=20),
    # configs[4]: 316 x 316-cell cloth (199 712 tris), Lame(100, 0.1) with strain limits 0.95/1.05, two corner
    # pins, Floor, multi-colour GS with in-sweep pins and plane projection, 10 ADMM iters/step
    "cloth200k_gs_floor": dict(n=316, kinds="cloth", linsolver=1, admm_iters=10),
    # configs[2] as named ("synthetic bunny/dragon"): unstructured body (meshes.unstructured_blob: jittered lattice, random
    # pulling triangulation, carved by an implicit bunny-like surface; valences 3..26), randomly numbered like a mesh file
    # and renumbered by renumber_for_locality like the samples do; NH / StVK by slab, feet pinned
    # BASELINE configs[2] names "UzawaCG global step": linsolver 2.  The scene has no obstacle, so every UzawaCG::solve is the one
    # prefactored solve of src/UzawaCG.hpp:78-81 -- on the GPU the recycled on-chip PCG (equality with linsolver 0 at full size:
    # tests/test_gpu_parity.py::test_big_blob_onchip_pcg_residual_and_uzawa_frame)
    "blob1m_mix": dict(n=118, kinds="blob", linsolver=2, admm_iters=20),
    # UzawaCG with ACTIVE constraints at scale (src/UzawaCG.hpp:92-120): the n=26 cube (105 456 tets, NH) dropped on a Floor,
    # no pins; every ADMM iteration detects, builds C and runs the Schur-complement CG whose every iteration is one on-chip
    # PCG solve.  Steady contact: ~700 constrained vertices.
    "cube100k_uzawa_floor": dict(n=26, kinds="nh_floor", linsolver=2, admm_iters=20),
    # WEAK scaling (the multi-GPU default): N separate 1 M-tet bodies of the blob1m_mix kind in one Solver, one per GPU.  The scene has
    # N connected components, so admm_hip_create gives every rank a whole body (component-aware partition): no exchange inside a
    # step, the rank's solve is its block of the block-diagonal system.  At N = 1 this IS blob1m_mix.
    "blobs_1m_per_gpu": dict(n=118, kinds="blobs", linsolver=0, admm_iters=20),
    "cube1m_linear": dict(n=55, kinds="linear", linsolver=0, admm_iters=20),   # diagnostic: cheapest prox
    "cube1m_stvk": dict(n=55, kinds="stvk", linsolver=0, admm_iters=20),
}


def workload_settings(name):
    """(pcg_tol, soft_modes) a workload is benchmarked AND parity-tested at: its own entry, else the blob's (PCG_TOL, SOFT_MODES)."""
    w = WORKLOADS[name]
    return w.get("pcg_tol", PCG_TOL), w.get("soft_modes", SOFT_MODES)


def build_scene(w, n_override=None, copies=1):
    import admm_elastic_amd as pkg
    from admm_elastic_amd import meshes
    from admm_elastic_amd.solver import Lame
    import scenes
    n = n_override or w["n"]
    if w["kinds"] == "blobs":      # `copies` bodies side by side (2 m apart): the same body, translated
        one = scenes.blob_scene(n, admm_iters=w["admm_iters"], linsolver=w["linsolver"], order=os.environ.get("ADMM_BENCH_ORDER", "rcm"))
        sc = scenes.Scene()
        nv1 = len(one.x)
        for i in range(copies):
            shift = np.array([2.0 * i, 0.0, 0.0])
            for verts, tets, lame, kind, off in one.tets:
                sc.tets.append((verts + shift, tets, lame, kind, off + i * nv1))
            for k, p in one.pins.items():
                sc.pins[k + i * nv1] = p + shift
        sc.x = np.concatenate([one.x + np.array([2.0 * i, 0.0, 0.0]) for i in range(copies)])
        sc.m = np.tile(one.m, copies)
        sc.settings.update(one.settings)
        return sc, copies * sum(len(t[1]) for t in one.tets), len(sc.x)
    if w["kinds"] == "cloth":
        sc = scenes.cloth_scene(n, limits=(0.95, 1.05), floor=0.3, admm_iters=w["admm_iters"], linsolver=w["linsolver"])
        return sc, len(sc.tris[0][1]), len(sc.x)
    if w["kinds"] == "blob":
        sc = scenes.blob_scene(n, admm_iters=w["admm_iters"], linsolver=w["linsolver"], order=os.environ.get("ADMM_BENCH_ORDER", "rcm"))
        return sc, sum(len(t[1]) for t in sc.tets), len(sc.x)
    if w["kinds"] == "nh_floor":
        sc = scenes.cube_scene(n, pkg.TET_NEOHOOKEAN, pin_face=False, admm_iters=w["admm_iters"], linsolver=w["linsolver"])
        sc.pins.clear()
        sc.obstacles.append((0, [-0.02, 0.0, 0.0, 0.0]))
        sc.settings.update(gravity=-9.8, timestep_s=1.0 / 24.0)
        return sc, len(sc.tets[0][1]), len(sc.x)
    verts, tets = meshes.kuhn_cube(n)
    sc = scenes.Scene()
    sc.x = verts
    sc.m = meshes.lumped_masses_tets(verts, tets)
    lame = Lame.soft_rubber()
    if w["kinds"] == "mix":
        cz = verts[tets].mean(axis=1)[:, 2]
        slab = (cz * 8).astype(int) % 2
        sc.tets.append((verts, tets[slab == 0], lame, pkg.TET_NEOHOOKEAN, 0))
        sc.tets.append((verts, tets[slab == 1], lame, pkg.TET_STVK, 0))
    else:
        kind = {"nh": pkg.TET_NEOHOOKEAN, "linear": pkg.TET_LINEAR, "stvk": pkg.TET_STVK}[w["kinds"]]
        sc.tets.append((verts, tets, lame, kind, 0))
    for i in np.nonzero(verts[:, 0] < 1e-9)[0]:
        sc.pins[int(i)] = verts[i].copy()
    sc.settings.update(admm_iters=w["admm_iters"], linsolver=w["linsolver"], gravity=-9.8, timestep_s=1.0 / 24.0)
    return sc, len(tets), len(verts)


def cpu_baseline(w, budget_s=12.0):
    """The oracle (CPU restatement, OpenMP local step + exact sparse solve / GS) timed on this box's
    host cores on a bounded sample: the same scene shape at reduced size, a few ADMM iterations.
    The OpenMP thread count is calibrated (8/16/32/64, never oversubscribed -- SURVEY appendix A)."""
    import ctypes
    from oracle import oracle as orc
    import scenes  # noqa: F401
    cores = os.cpu_count() or 1
    n_s = min(w["n"], {"cloth": 100, "blob": 44}.get(w["kinds"], 20))  # the sample: 48 000 tets (cube) / 52 000 (body) / 20 000 tris
    sc, nt, nv = build_scene(w, n_override=n_s)
    sc.settings["admm_iters"] = 5
    colors = None
    if w["linsolver"] == 1:
        from admm_elastic_amd import capi
        s = sc.make_solver(init=False)
        rp, ci, _ = s.host_matrix(sc.product_settings)
        colors, _ = capi.greedy_coloring(rp, ci)
    o = sc.make_oracle(mode=0, gs_colors=colors, big=True)
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
    except OSError:
        gomp = None
    best = (None, 0.0)
    for th in [t for t in (8, 16, 32, 64) if t <= cores] or [1]:
        if gomp is not None:
            gomp.omp_set_num_threads(th)
        o.step()
        t0 = time.perf_counter(); o.step(); dt1 = time.perf_counter() - t0
        if best[0] is None or o.admm_iters / dt1 > best[1]:
            best = (th, o.admm_iters / dt1)
        if gomp is None:
            break
    threads = best[0]
    if gomp is not None:
        gomp.omp_set_num_threads(threads)
    t0 = time.perf_counter(); iters = 0
    while time.perf_counter() - t0 < budget_s and iters < 5000:
        o.step(); iters += o.admm_iters
    dt = time.perf_counter() - t0
    its = iters / dt
    shape = "unstructured body" if w["kinds"] == "blob" else "cloth" if w["kinds"] == "cloth" else "Kuhn cube"
    solver = "30 multi-colour SOR sweeps" if w["linsolver"] == 1 else "SuperLU direct solve (prefactored)"
    return dict(value=its * nt / 1e6, unit="M element-ADMM-iterations/s", admm_iters_per_s_at_sample=its, cores=threads, kind="port",
                sample="%d-element %s (n=%d), same materials/solver family, %d ADMM iterations in %.1f s; oracle = OpenMP local step "
                       "(L-BFGS, reference stop rule) + %s; host has %d hardware threads" % (nt, shape, n_s, iters, dt, solver, cores))


def cpu_baseline_full_size(w, threads, budget_s=8.0):
    """The CPU leg AT THE BENCHMARKED SIZE, with the solver family that is the fair CPU baseline there (at
    1 M tets the reference's LDLT needs a 31-minute factorisation and then 0.47 ADMM it/s, its multi-colour GS 2.0-2.4 with no
    set-up): the oracle's OpenMP local step + 30 SOR sweeps on the full mesh, `threads` OpenMP threads, whole ADMM iterations
    timed until the budget is spent (at least two)."""
    import ctypes
    from admm_elastic_amd import capi
    wf = dict(w, linsolver=1)
    t0 = time.perf_counter()
    sc, nt, nv = build_scene(wf)
    sc.settings["admm_iters"] = 1
    s = sc.make_solver(init=False)
    rp, ci, _ = s.host_matrix(sc.product_settings)
    colors, nc = capi.greedy_coloring(rp, ci)
    o = sc.make_oracle(mode=0, gs_colors=colors, big=True)
    setup_s = time.perf_counter() - t0
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(threads)
    except OSError:
        pass
    o.step()                                   # (first touch)
    t0 = time.perf_counter(); n = 0
    while n < 2 or (time.perf_counter() - t0 < budget_s and n < 200):
        o.step(); n += 1
    dt = time.perf_counter() - t0
    return dict(admm_iters_per_s=n / dt, elements=nt, colours=nc, cores=threads, admm_iterations_timed=n, seconds=dt, setup_seconds=setup_s,
                what="oracle (port) at the benchmarked size: OpenMP local step (L-BFGS, reference stop rule) + 30 multi-colour SOR sweeps "
                     "(src/NodalMultiColorGS.hpp; tol 1e-10 is never met, like the reference's 600 inner iterations per frame)")


CALIBRATION_FILE = os.path.join(ROOT, "profiles", "r06_cpu_calibration.json")      # (refreshed on the current oracle port every round the port changes; r03_: rounds 3-5)


def cpu_calibration(out_path=CALIBRATION_FILE):
    """the oracle PORT (what `cpu_baseline` times on the GPU box, where /root/reference does not exist) against
    the REAL reference code that compiles here (oracle/_ref: TriEnergyTerm.cpp + EnergyTerm::update, Eigen::SimplicialLDLT as
    LDLTSolver uses it), same inputs, same host, same thread count -- so that "x the port" can be read as "x the reference".
    Run in the build container (`python bench.py --calibrate-cpu-baseline`); the result is committed under profiles/ and quoted
    by `cpu_baseline.calibration`.  The tet prox of the reference needs the absent mcloptlib and cannot be timed."""
    import ctypes
    import platform
    from oracle import oracle as orc
    import scenes
    R = orc.ref_lib()
    if R is None or not hasattr(R, "ref_time_tri_local_step"):
        raise SystemExit("calibration needs oracle/_ref built from /root/reference (make -C oracle)")
    L = orc.lib()
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or (os.cpu_count() or 1)
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(threads)
    except OSError:
        pass
    res = {"host": platform.processor() or platform.machine(), "hardware_threads": os.cpu_count(), "omp_threads": threads, "cases": []}
    # (1) triangle local step: the cloth of configs[4] at 200 x 200 cells (80 000 triangles), strain limits on
    sc = scenes.cloth_scene(200, limits=(0.95, 1.05), admm_iters=5, linsolver=0)
    o = sc.make_oracle(mode=0, big=True)
    verts, tris, lame, off = sc.tris[0]
    rng = np.random.default_rng(0)
    x = (sc.x + 0.01 * rng.standard_normal(sc.x.shape)).ravel()
    idx = np.ascontiguousarray(tris, dtype=np.int32)
    t_ref = R.ref_time_tri_local_step(len(idx), orc._i(idx), len(sc.x), orc._p(np.ascontiguousarray(verts, dtype=np.float64)),
                                      lame.mu, lame.lambda_, lame.limit_min, lame.limit_max, orc._p(np.ascontiguousarray(x)), 5)
    z = np.zeros(o.R); u = np.zeros(o.R)
    t_port = 1e300
    for _ in range(5):
        t0 = time.perf_counter(); o.local_step(x, z, u); t_port = min(t_port, time.perf_counter() - t0)
    res["cases"].append({"what": "triangle local step (TriEnergyTerm::update over all terms, src/Solver.cpp:84-87), %d triangles, strain limits 0.95/1.05" % len(idx),
                         "reference_s": t_ref, "port_s": t_port, "reference_over_port": t_ref / t_port})
    # (2) prefactored solve: the bench's CPU sample (48 000-tet cube, 27 783 dof) and the 105 456-tet cube of configs[1]
    for n in (20, 26):
        scn = scenes.cube_scene(n, pkg_kind("neohookean"), admm_iters=5, linsolver=0)
        on = scn.make_oracle(mode=0, big=True)
        Ah = on.A[0::3, :][:, 0::3].tocsr(); Ah.sort_indices()
        m3 = np.ascontiguousarray(on.m)
        Ahat = (Ah - __import__("scipy.sparse", fromlist=["diags"]).diags(m3[0::3])).tocsr(); Ahat.sort_indices()
        b = np.ascontiguousarray(on.A @ rng.standard_normal(on.dof))
        fs, ss = ctypes.c_double(0), ctypes.c_double(0)
        rc = R.ref_time_ldlt(on.nv, orc._i(np.ascontiguousarray(Ahat.indptr, dtype=np.int32)), orc._i(np.ascontiguousarray(Ahat.indices, dtype=np.int32)),
                             orc._p(np.ascontiguousarray(Ahat.data)), orc._p(m3), orc._p(b), 3, ctypes.byref(fs), ctypes.byref(ss))
        assert rc == 0, rc
        t_port = 1e300
        for _ in range(3):
            t0 = time.perf_counter(); on.solve_ldlt(b); t_port = min(t_port, time.perf_counter() - t0)
        res["cases"].append({"what": "one prefactored solve (Eigen::SimplicialLDLT as LDLTSolver, src/LinearSolver.hpp:79-90, vs the port's SuperLU), Kuhn cube n=%d, %d dof" % (n, on.dof),
                             "reference_s": ss.value, "reference_factor_s": fs.value, "port_s": t_port, "reference_over_port": ss.value / t_port})
    res["summary"] = {"local_step_reference_over_port": res["cases"][0]["reference_over_port"],
                      "solve_reference_over_port": res["cases"][1]["reference_over_port"],
                      "note": "reference_over_port = time of the REAL reference code / time of the oracle port, same inputs, host, threads.  < 1: the reference is FASTER than the port, so x-the-port OVERSTATES x-the-reference by 1 / ratio; the "
                              "reference's tet prox (mcloptlib L-BFGS, absent) is not timed -- the port runs the reference's stop rule with its own minimiser"}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"]))
    return res


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out_dir, arrays, limit_bytes=DUMP_LIMIT_BYTES, seed=0):
    """Write `arrays` (name -> array with one row per vertex) as out_dir/<name>.npy in float64.  When the files would exceed
    `limit_bytes` in all, every array keeps the same fixed, seeded sample of rows (in row order).  Returns the kept rows (None: all)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in arrays.items()}
    rows = {a.shape[0] for a in arrays.values()}
    assert len(rows) == 1, "dump_outputs: arrays differ in their number of rows"
    rows = rows.pop()
    keep = None
    header = 256 * len(arrays)            # (np.save: a header of at most a few hundred bytes per file)
    if sum(a.nbytes for a in arrays.values()) + header > limit_bytes:
        per_row = sum(a.nbytes for a in arrays.values()) // max(rows, 1)
        keep = np.sort(np.random.default_rng(seed).choice(rows, size=(limit_bytes - header) // per_row, replace=False))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a if keep is None else a[keep])
    return keep


def pkg_kind(name):
    import admm_elastic_amd as pkg
    return {"neohookean": pkg.TET_NEOHOOKEAN, "linear": pkg.TET_LINEAR, "stvk": pkg.TET_STVK}[name]


def pmc_traffic(workload, key="local_step_bytes_per_launch"):
    """HBM/fabric bytes per launch of the local-step kernels from the committed rocprofv3 PMC passes
    (profiles/*pmc*.json: --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate runs; FETCH_SIZE doubled per
    MI355X_MICROARCH.md, calibrated on k_predict/k_finish).  None when no profile of this workload exists."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc*.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload") != workload or key not in d:
            continue
        best = d[key]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)     # (the recycled projection settles its pair count in frames 3-4)
    ap.add_argument("--workload", default=None, choices=list(WORKLOADS),
                    help="default: blob1m_mix -- on several GPUs the same body at fixed tet count (strong scaling, BASELINE configs[3]); "
                         "blobs_1m_per_gpu = one 1 M-tet body per GPU (weak scaling) as the whole line")
    ap.add_argument("--n", type=int, default=0, help="override cells per edge (testing only)")
    ap.add_argument("--pcg-tol", type=float, default=None, help="default: the workload's own parity-backed setting (workload_settings)")
    ap.add_argument("--pcg-max-iters", type=int, default=600)
    ap.add_argument("--soft-modes", type=int, default=None, help="default: the workload's own setting; end projection of every PCG solve on this many lowest modes (0: off); PCG workloads")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--calibrate-cpu-baseline", action="store_true", help="build container only: time the oracle port against the compiled reference pieces -> profiles/")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: statistics frames, contact leg, PCIe-inclusive rate, weak leg (N GPUs), roofline, "
                         "CPU baselines (--no-cpu-baseline / --no-roofline drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the state the last timed step computed (m_x, m_v; rank 0's copy) as DIR/<name>.npy, float64, <= 64 MB in all")
    args = ap.parse_args()
    if not args.n and os.environ.get("ADMM_BENCH_N"):      # (tests: the launcher's own parser trips over `--n`)
        args.n = int(os.environ["ADMM_BENCH_N"])
    default_workload = args.workload is None
    if args.workload is None:
        args.workload = "blob1m_mix"
    if args.calibrate_cpu_baseline:
        cpu_calibration()
        return
    wl_tol, wl_soft = workload_settings(args.workload)
    if args.pcg_tol is None:
        args.pcg_tol = wl_tol
    if args.soft_modes is None:
        args.soft_modes = wl_soft

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks here, exactly as the driver's
        # `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` line does (one process per GPU, RCCL)
        import socket
        import subprocess
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:      # (before the heavy imports: a rank that dies early must not hide that the others were started)
        print("bench.py: rank %s of %s started (local rank %s)" % (os.environ.get("RANK", "0"), os.environ["WORLD_SIZE"], os.environ.get("LOCAL_RANK", "0")),
              file=sys.stderr, flush=True)
    import torch
    import admm_elastic_amd as pkg
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1):
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # Functional check of the N-rank code path on a ONE-GPU box (tests/test_multi_gpu.py; never a performance number): every rank
    # uses device 0, the process group is gloo, no RCCL communicator (the component partition needs none inside a step).
    share = os.environ.get("ADMM_BENCH_SHARE_GPU") == "1" and world > 1
    if share:
        local_rank = 0
    if pkg.device_count() < (local_rank + 1 if world > 1 else 1):
        raise SystemExit("bench.py: rank %d needs HIP device %d, %d visible (the hot path has no CPU fallback)" % (rank, local_rank, pkg.device_count()))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    pkg.build_library()
    w = WORKLOADS[args.workload]
    sc, nt, nv = build_scene(w, args.n or None, copies=world)
    iters = w["admm_iters"]
    weak = w["kinds"] == "blobs"
    soft = args.soft_modes if w["linsolver"] != 1 else 0      # (every rank computes the modes of the system it solves; the distributed solve: collectively)
    s = sc.make_solver(device=local_rank, pcg_tol=args.pcg_tol, pcg_max_iters=args.pcg_max_iters, rank=rank, world_size=world, soft_modes=soft)
    if world > 1 and not share:
        s.comm_init(dist)
    elif world > 1 and not weak:
        # one-GPU functional check of the element partition: RCCL cannot put two ranks on one device, so the partial right-hand
        # sides are summed by the caller's own transport (admm_hip_set_rhs_allreduce: here gloo on a host buffer)
        s.set_rhs_allreduce(lambda buf: dist.all_reduce(torch.from_numpy(buf)))
    s.upload()

    def sync():
        torch.cuda.synchronize(local_rank)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(local_rank)

    for _ in range(args.warmup):
        s.step_device(stats=True)
    sync()
    # Timed region: EXACTLY `steps` frames.  With the on-chip PCG the frames are issued without per-step statistics (no
    # events between the kernels, no host synchronisation between frames: +2-3 %) and the solver's own totals say afterwards
    # whether every solve of the region converged; the per-phase split, the event-pair duration of the prox kernels and the
    # iteration counts then come from `steps` more frames run with statistics OUTSIDE the timed region.  Other solvers: the
    # statistics frames are the timed ones, as in round 1.
    local_ms = rhs_ms = global_ms = lk_ms = 0.0
    inner = unconv = 0
    inner_timed = None
    # contact-free scenes on the on-chip PCG (linsolver 0, or UzawaCG without obstacles: one prefactored solve per ADMM iteration)
    contact_free = w["linsolver"] == 0 or (w["linsolver"] == 2 and not sc.obstacles and not sc.dynamic)
    tot0 = s.solve_totals() if contact_free else (-1, -1, -1)
    lean = tot0[0] >= 0
    lt_pairs, lt_ms = 0, 0.0       # the local-step launches of the TIMED region: event pairs, read after it
    if lean:
        # a hipEvent pair attached to the dispatch of every local-step kernel of the timed region (ADMM_BENCH_LOCAL_EVENTS=0 / 1: none /
        # hipEventRecords around the launch -- same-box A/B of what the instrumentation costs, experiments/r06_a.sh).  Only `roofline`
        # (--full) reads them, but a plain run attaches them too: its timed frames stay the very frames every earlier line timed, so
        # `value` stays comparable with those lines and with the --full line of the same build.
        s.time_local_launches(int(os.environ.get("ADMM_BENCH_LOCAL_EVENTS", "2")))
        s.local_launch_times()     # (clears what the warm-up recorded)
    uz0 = s.uzawa_cache_stats() if args.full and w["linsolver"] == 2 else None
    has_contact = bool(sc.obstacles or sc.dynamic) and w["linsolver"] != 0
    ct0 = s.contact_totals() if args.full and has_contact else 0       # rows of C (UzawaCG) / rows projected inside the sweeps (GS) so far
    frame_ms = []                                        # HIP-event time of every statistics frame (median: SURVEY 8d)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s.step_device(stats=not lean)
        if not lean:
            rd = s.runtime_data()
            local_ms += rd.local_ms; rhs_ms += rd.rhs_ms; global_ms += rd.global_ms; inner += rd.inner_iters
            lk_ms += rd.local_kernel_ms
            unconv += rd.unconverged_solves
            frame_ms.append(rd.step_ms)
    sync()
    elapsed = time.perf_counter() - t0
    stats_elapsed = elapsed
    if args.dump_outputs:
        # every rank downloads: under the component partition with a communicator admm_hip_get_state is a collective (include/admm_hip.h)
        if share:
            # no communicator: a rank's download fills only the vertices it owns, so the ranks' parts are merged here (NaN = not filled)
            s.m_x[:] = np.nan; s.m_v[:] = np.nan
            s.download()
            parts = [None] * world
            dist.all_gather_object(parts, (s.m_x, s.m_v))
            for k in (0, 1):
                merged = parts[0][k].copy()
                for p in parts[1:]:
                    merged = np.where(np.isnan(merged), p[k], merged)
                (s.m_x if k == 0 else s.m_v)[:] = merged
        else:
            s.download()
        if rank == 0:
            dump_outputs(args.dump_outputs, {"m_x": s.m_x.reshape(-1, 3), "m_v": s.m_v.reshape(-1, 3)})
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if share else "cuda:%d" % local_rank)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / max(args.steps, 1)
    # weak scaling: every rank steps its own body, the job's rate is the bodies' ADMM iterations per second, summed
    value = (world if weak else 1) * iters * args.steps / elapsed
    out = {
        "metric": "ADMM iterations/sec", "value": value, "unit": "ADMM it/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        # the DEFAULT lines of --gpus 1, 2, 4, 8 are BASELINE's series: ONE 1 M-tet body at fixed tet count (configs[3]); the weak
        # series (one such body per GPU) is `weak_value` of the same lines (--full)
        "scaling": "weak" if weak else "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "soft_modes": soft, "pcg_tol": args.pcg_tol,
        "config": {"workload": args.workload + (" (n=%d override)" % args.n if args.n else ""), "elements": nt, "verts": nv,
                   "admm_iters_per_step": iters, "global_solver": "multicolor-GS(30 sweeps)" if w["linsolver"] == 1 else
                   ("UzawaCG, no active constraints: every solve is the prefactored solve (src/UzawaCG.hpp:78-81) = one persistent on-chip two-level pipelined PCG launch, tol=%g max=%d" % (args.pcg_tol, args.pcg_max_iters)
                    if contact_free else "UzawaCG (Schur-complement CG, <= 20 iterations, stop decided on the device) over the on-chip PCG tol=%g" % args.pcg_tol) if w["linsolver"] == 2 else
                   "PCG (one persistent on-chip launch per solve: two-level preconditioned pipelined CG, matrix and vectors in LDS) tol=%g max=%d" % (args.pcg_tol, args.pcg_max_iters),
                   "parallelism": ("whole bodies per rank x%d (component-aware partition, no exchange inside a step)" % world if weak else
                                   "element-block x%d (RCCL all-reduce of the right-hand side, %s)" % (world,
                                       "DISTRIBUTED solve: launch-path Jacobi PCG, rows split over the ranks, two all-reduces per PCG iteration (ADMM_HIP_DIST_SOLVE=1)"
                                       if os.environ.get("ADMM_HIP_DIST_SOLVE") == "1" and not weak else "replicated solve")) if world > 1 else "single-gpu"},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if dist is not None:
            dist.destroy_process_group()
        return
    ct1 = s.contact_totals() if has_contact else 0
    uz1 = s.uzawa_cache_stats() if w["linsolver"] == 2 else None
    if lean:
        lt_pairs, lt_ms = s.local_launch_times()
        s.time_local_launches(False)
        tot1 = s.solve_totals()
        unconv = (tot1[0] - tot0[0]) - (tot1[1] - tot0[1])
        assert tot1[0] - tot0[0] == iters * args.steps, (tot0, tot1)
        inner_timed = tot1[2] - tot0[2]      # PCG iterations of the TIMED frames themselves (the solver's own device-side totals)
        t1s = time.perf_counter()
        for _ in range(args.steps):
            s.step_device(stats=True)
            rd = s.runtime_data()
            local_ms += rd.local_ms; rhs_ms += rd.rhs_ms; global_ms += rd.global_ms
            lk_ms += rd.local_kernel_ms
            frame_ms.append(rd.step_ms)
        sync()
        stats_elapsed = time.perf_counter() - t1s
        tot2 = s.solve_totals()
        inner = tot2[2] - tot1[2]            # PCG iterations of the statistics frames (UzawaCG's own count is 1 per contact-free solve)
        unconv += (tot2[0] - tot1[0]) - (tot2[1] - tot1[1])
    else:
        lt_pairs, lt_ms = iters * args.steps, local_ms
    # The WEAK series rides along on the strong default line (`weak_value`): every rank steps ONE whole body of its own (a
    # single-GPU context of the same scene -- what blobs_1m_per_gpu gives each rank), same warm-up, same K frames, barriers,
    # max over ranks; N bodies' ADMM iterations per second, summed.
    weak_value = weak_ms = one = None
    if world > 1 and not weak and default_workload:
        sw = sc.make_solver(device=local_rank, pcg_tol=args.pcg_tol, pcg_max_iters=args.pcg_max_iters)
        sw.upload()
        for _ in range(args.warmup):
            sw.step_device(stats=True)
        sync()
        tw = time.perf_counter()
        for _ in range(args.steps):
            sw.step_device(stats=False)
        sync()
        tw = time.perf_counter() - tw
        t = torch.tensor([tw], dtype=torch.float64, device="cpu" if share else "cuda:%d" % local_rank)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        weak_ms = 1e3 * float(t.item()) / max(args.steps, 1)
        weak_value = world * iters * args.steps / float(t.item())
        one = [0.0, 0.0, 0.0]                # split of the single-GPU context (three statistics frames): the inputs of `expected_speedup`
        for _ in range(3):
            sw.step_device(stats=True)
            r1 = sw.runtime_data()
            one[0] += r1.local_ms / (3 * iters); one[1] += r1.rhs_ms / (3 * iters); one[2] += r1.global_ms / (3 * iters)
        sw.close()

    # BASELINE configs[4] names "floor-collision ConstraintSet, dynamic constraints": the cloth of the bench scene swings on its two pins
    # and reaches the floor only around frame 29, AFTER the default timed frames -- so the same run goes on until rows are being projected
    # inside the sweeps (admm_hip_contact_totals moves) and times `steps` more frames there.  Both regimes are quoted.
    contact_leg = None
    if has_contact and w["linsolver"] == 1 and world == 1 and os.environ.get("ADMM_BENCH_CONTACT_LEG", "1") != "0":
        waited, c_prev = 0, s.contact_totals()
        in_contact = ct1 > ct0
        while not in_contact and waited < 120:
            s.step_device(stats=False); waited += 1
            c_now = s.contact_totals(); in_contact = c_now > c_prev; c_prev = c_now
        if in_contact:
            for _ in range(2):
                s.step_device(stats=False)
            sync()
            c_a = s.contact_totals(); fm = []
            tc = time.perf_counter()
            for _ in range(args.steps):
                s.step_device(stats=True); fm.append(s.runtime_data().step_ms)
            sync()
            tc = time.perf_counter() - tc
            c_b = s.contact_totals()
            contact_leg = {"what": "the same run continued until the cloth lies on the floor (%d more frames), then %d frames timed with per-step statistics" % (waited + 2, args.steps),
                           "value": iters * args.steps / tc, "unit": "ADMM it/s", "ms_per_step": 1e3 * tc / max(args.steps, 1),
                           "median_ms_per_frame": float(np.median(fm)), "rows_projected_in_timed_region": c_b - c_a,
                           "rows_projected_per_sweep": (c_b - c_a) / max(1, args.steps * iters * 30)}
    rd = s.runtime_data()
    s.download()
    finite = bool(np.isfinite(s.m_x).all())
    # PCIe-inclusive rate (never `value`): the reference-style Solver::step() with m_x/m_v on the host,
    # i.e. upload + step + download per frame.
    pcie_value = None
    if world == 1:
        t1 = time.perf_counter()
        for _ in range(2):
            s.step()
        pcie_value = iters * 2 / (time.perf_counter() - t1)

    out.update({
        "ms_per_frame": ms_per_step,
        "split_ms_per_admm_iter": {"local": local_ms / (iters * args.steps), "rhs": rhs_ms / (iters * args.steps),
                                   "global": global_ms / (iters * args.steps)},
        # of the TIMED frames (admm_hip_solve_totals before / after them); the statistics frames that follow have their own count
        "inner_iters_per_admm_iter": (inner_timed if inner_timed is not None else inner) / (iters * args.steps),
        "inner_iters_per_admm_iter_statistics_frames": inner / (iters * args.steps) if lean else None,
        "unconverged_solves_in_timed_region": unconv,
        # what the on-chip PCG holds against this context (admm_hip_pcg_findings): until round 6's last session the soft-mode computation left every
        # context that used it with `smoother_given_up` -- the headline ran with a Jacobi smoother.  All false / 0 is the healthy state.
        "pcg_findings": (s.pcg_findings() if w["linsolver"] != 1 else None),
        "timed_region": ("frames issued without per-step statistics (one hipEvent pair around every local-step launch is the only instrumentation: "
                         "`roofline`); split / iteration counts from as many STATISTICS FRAMES right after, which take %.3f x the time of the timed ones "
                         "(`stats_frames_ms_per_step`)" % (stats_elapsed / elapsed)) if lean else "frames with per-step statistics",
        "stats_frames_ms_per_step": 1e3 * stats_elapsed / max(args.steps, 1),
        # "time >= 20 frames, report median": HIP-event time of each statistics frame (`value` stays the contract's K frames / wall clock)
        "median_ms_per_frame_statistics_frames": float(np.median(frame_ms)) if frame_ms else None,
        "median_admm_it_per_s_statistics_frames": (1e3 * iters / float(np.median(frame_ms))) if frame_ms else None,
        # contact work inside the timed region (admm_hip_contact_totals): rows of C summed over the UzawaCG solves / rows projected onto an
        # obstacle summed over the GS sweeps.  0 = the timed frames were contact-free (see `contact_regime`)
        "rows_projected_in_timed_region": (ct1 - ct0) if has_contact else None,
        "contact_regime": contact_leg,
        # UzawaCG: how the Schur iterations of the timed region applied A^-1 (cached columns of K^-1 / inner PCG solves), and the
        # PCG launches the region spent on new columns (vertices that touched an obstacle for the first time)
        "uzawa": None if uz0 is None else {"cached_columns": uz1["columns"],
                                           "schur_iterations_from_columns": uz1["schur_from_columns"] - uz0["schur_from_columns"],
                                           "schur_iterations_by_pcg": uz1["schur_by_pcg"] - uz0["schur_by_pcg"],
                                           "column_solves_in_timed_region": uz1["column_solves"] - uz0["column_solves"],
                                           # ... of which look-ahead (solved on side streams beside the ADMM loop, before the vertex touches):
                                           "columns_committed_ahead_of_contact": uz1.get("ahead_columns", 0) - uz0.get("ahead_columns", 0),
                                           "solves_that_waited_for_a_column": uz1.get("ahead_waits", 0) - uz0.get("ahead_waits", 0),
                                           "column_lanes": uz1.get("lanes", 0)},
        # mean time of one inner (PCG / GS) iteration incl. the per-solve overheads: (global - rhs) / inner iterations.
        # The PCG kernel keeps matrix and vectors on chip; its iteration is bound by one grid barrier, not by HBM.
        "us_per_inner_iter": 1e3 * (global_ms - rhs_ms) / max(inner, 1),
        "finite": finite, "pcie_inclusive_admm_it_per_s": pcie_value,
    })
    if weak_value is not None:
        out["weak_value"] = weak_value
        out["weak"] = {"workload": "one blob1m_mix body per GPU (what --workload blobs_1m_per_gpu runs as its whole line)", "ms_per_step": weak_ms,
                       "unit": "ADMM it/s summed over the %d bodies" % world, "expected_vs_one_gpu": float(world)}
    elif world == 1 and default_workload:
        out["weak_value"] = value            # N = 1: the same body, the same number
    if world > 1:
        # so that a scaling run can be CHECKED: the rank count RCCL itself reports for the context's communicator, and every rank's device
        info = s.comm_info()
        infos = [None] * world
        dist.all_gather_object(infos, info)
        out["rccl"] = {"communicator_ranks": info["n_ranks"], "devices": [i["device"] for i in infos],
                       "distinct_devices": len({i["device"] for i in infos}), "ranks_reporting": [i["rank"] for i in infos]}
    if share:
        out["shared_gpu_functional_test"] = "ADMM_BENCH_SHARE_GPU=1: %d ranks time-share ONE device -- a check that the N-rank path runs, not a measurement" % world
    if world > 1 and not weak:
        # stated BEFORE any curve is measured: only local step + RHS shard, the solve is replicated, the all-reduce adds ~0.04 ms
        # inputs: this rank's SINGLE-GPU context of the same body when the weak leg ran (`one`), else the N-rank split scaled back
        loc, rhs, glo = one if one is not None else (out["split_ms_per_admm_iter"]["local"] * world, out["split_ms_per_admm_iter"]["rhs"] * world,
                                                     out["split_ms_per_admm_iter"]["global"] + out["split_ms_per_admm_iter"]["rhs"] * (world - 1))
        out["expected_speedup"] = {"model": "t_N = (local + rhs) / N + solve + 0.04 ms all-reduce (4.4 MB over xGMI); the solve (one persistent on-chip launch, latency-bound) is replicated",
                                   "single_gpu_ms_per_admm_iter": {"local": loc, "rhs": rhs, "solve": glo - rhs},
                                   "vs_one_gpu": (loc + glo) / ((loc + rhs) / world + (glo - rhs) + 0.04)}
    if world > 1 and not weak:
        # The ONE-body configuration that can scale: N M tets on N GPUs, rows of the launch-path two-level PCG split over the ranks
        # (ADMM_HIP_DIST_SOLVE=1).  No multi-GPU node has been available to this repository: the model below is arithmetic on single-GPU kernel
        # times (profiles/r05_size_curve.txt, r04_dist_solve_cost.txt), stated so that the first real run can be CHECKED against it.
        def _dist(n):
            stream = 58.0 * (n / 2.0) / n            # k_big_spmv + k_big_vec, us per iteration: (33 + 25) at 2 M tets, by size / ranks
            coarse = 36.0 / n                        # dense coarse rows of the rank's own aggregates (923 aggregates at 4-8 M tets)
            coll = 3 * 13.0                          # three latency-bound all-reduces per iteration over xGMI (12-15 us each)
            per_solve = 14.0 * (stream + coarse + coll) + 500.0      # ~14 iterations with the soft-mode steps + entry / recycling / soft-mode kernels
            return 1e6 / (per_solve + 75.0 / 1.0 + 40.0)             # + local step and gather of 1 M tets per rank + the right-hand side's all-reduce
        out["distributed_solve_model"] = {"what": "ONE body of N M tets on N GPUs, ADMM_HIP_DIST_SOLVE=1 (not what this line ran): expected ADMM it/s",
                                          "admm_it_per_s": {"2": _dist(2), "4": _dist(4), "8": _dist(8)},
                                          "single_gpu_measured": {"2 M tets": 537, "4 M tets": 293}}
    if weak and world > 1:
        out["expected_speedup"] = {"model": "N independent bodies, no exchange inside a step: N x the single-GPU rate of one body", "vs_one_gpu": float(world)}
    if rank == 0:
        if w["kinds"] != "cloth":
            from admm_elastic_amd import meshes as _m
            tets_all = np.concatenate([t[1] + t[4] for t in sc.tets])
            out["config"]["vertex_valence"] = _m.valence_stats(nv, tets_all)   # edges per vertex (row of Ahat = valence + 1)
        if not args.no_roofline and contact_free and lean and world == 1:
            # The time-dominant kernel: the whole PCG solve is ONE persistent launch whose matrix and vectors stay in LDS /
            # registers, so it has no HBM roofline; an iteration is two dependent synchronisations -- the vector exchange
            # between neighbour blocks and the all-to-all of the block records behind one grid barrier.  Their latency floor
            # is measured live on the same grid with the kernel's own primitives (admm_hip_probe_sync).
            a2a, xch, pst = s.probe_sync(200)
            n_solves = iters * args.steps
            it_stats = inner / max(n_solves, 1)
            solve_us_stats = 1e3 * (global_ms - rhs_ms) / max(n_solves, 1)
            # The TIMED frames carry no events between their kernels, so their solve time is what is left of a timed ADMM iteration after the
            # local step and the right-hand side (statistics frames' durations; launch gaps stay inside: an upper bound), and the iteration
            # count is the timed frames' own.  The statistics frames' pair of numbers rides along.
            it_per_solve = (inner_timed if inner_timed is not None else inner) / max(n_solves, 1)
            solve_us = 1e3 * ms_per_step / iters - 1e3 * (local_ms + rhs_ms) / max(n_solves, 1)
            us_it = solve_us / max(it_per_solve, 1e-9)
            out["roofline_global"] = {
                "role": "TIME-DOMINANT kernel: %.0f %% of a statistics frame" % (100.0 * (global_ms - rhs_ms) / max(local_ms + global_ms, 1e-30)),
                "measured_in": "the TIMED frames: iterations from the solver's totals around them, `solve_us` = timed ADMM iteration - local step - right-hand side "
                               "(launch gaps included); the statistics frames' event-pair figures in `statistics_frames`",
                "statistics_frames": {"iterations_per_solve": it_stats, "solve_us": solve_us_stats},
                "kernel": "k_pcg2 (whole two-level PCG solve, one persistent launch per ADMM iteration)",
                "bound": "synchronisation latency (grid barrier + neighbour exchange); data on chip",
                "iterations_per_solve": it_per_solve, "solve_us": solve_us, "us_per_iteration_incl_solve_overhead": us_it,
                "floor_us_per_iteration": a2a + xch, "floor_all_to_all_us": a2a, "floor_exchange_us": xch,
                # The bound of this kernel is the latency of the synchronisations its algorithm needs, measured live with the kernel's own
                # primitives: per solve 3 all-to-alls + 2 exchanges of the start phase (entry residual, recycled projection, coarse
                # part of M^-1 r, w = A u and its record) and one of each per iteration, the one that detects convergence included.
                "sync_floor_us_per_solve": 3.0 * a2a + 2.0 * xch + (it_per_solve + 1.0) * (a2a + xch),
                "frac": (3.0 * a2a + 2.0 * xch + (it_per_solve + 1.0) * (a2a + xch)) / solve_us if solve_us > 0 else None,
                # (round 2's definition: floor per iteration / (solve time / iterations) -- it punishes FEWER iterations)
                "frac_round2_definition": (a2a + xch) / us_it if us_it > 0 else None,
                "plan": pst, "pmc_bytes_per_iteration": pmc_traffic(args.workload, "pcg_bytes_per_iteration"),
            }
        if not args.no_roofline:
            # The HBM-bound kernel the north-star names: the per-tet prox kernel (local step) -- second by time behind the
            # persistent PCG launch (`roofline_global`).  ALGORITHMIC bytes per tet per ADMM iteration: 16 idx +
            # 72 Binv + 72 u read + 72 u write + 72 z write + 24 nv/nt.
            launches = max(lt_pairs, 1)
            # (with N ranks, rank 0 times its own element block: nt / N elements per launch)
            bytes_per_launch = ((188.0 if w["kinds"] == "cloth" else 304.0) + 24.0 * nv / nt) * nt / world
            # Duration of one launch, measured live on the context's own stream, four ways that bracket each other:
            # (1) `avg_launch_us`, used for `achieved` / `frac`: HIP events ATTACHED TO THE KERNEL'S DISPATCH in the timed region
            # (hipExtLaunchKernelGGL start / stop events: the kernel's own begin and end time stamps -- what "the kernel's launch
            # duration" means and what rocprofv3 reports; rounds 1-3 and the first session of round 4 used (2) here);
            # (2) `avg_launch_us_statistics_frames`: the interval between two hipEventRecords AROUND the launch in the statistics
            # frames (kernel + the two dispatch gaps: 1.5-3 us longer); (3) rocprofv3 --kernel-trace of the same command
            # (profiles/): within ~1 us of (1); (4) `kernel_us_device_clock` (only with ADMM_HIP_KERNEL_CLOCK=1: the stamps cost the
            # launch ~2 %): every wave stamps the device wall clock at entry and exit -- max exit - min entry is 2-3 us shorter than
            # rocprofv3 (it misses the dispatch ramp-up, the drain of the last stores and the end-of-kernel cache release).
            avg_s = 1e-3 * lt_ms / launches
            if not avg_s > 0.0:      # (ADMM_BENCH_LOCAL_EVENTS=0, an A/B run without the event pairs: the statistics frames' figure)
                avg_s = 1e-3 * local_ms / max(iters * args.steps, 1)
            achieved = bytes_per_launch / avg_s / 1e9
            out["roofline"] = {"role": "the HBM-bound kernel the north-star names (local step): %.0f %% of a statistics frame, second by time behind `roofline_global`"
                                       % (100.0 * local_ms / max(local_ms + global_ms, 1e-30)),
                               "measured_in": ("the TIMED region: %d hipEvent pairs, one attached to the dispatch of every local-step kernel" % lt_pairs) if lean else "the timed region (statistics frames)",
                               "kernel": "k_local_tris" if w["kinds"] == "cloth" else "k_local_tets (all constitutive models of one ADMM iteration)", "bound": "hbm",
                               "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                               "traffic": pmc_traffic(args.workload), "avg_launch_us": 1e6 * avg_s,
                               "timing": ("hipExtLaunchKernelGGL start / stop events of the kernel's dispatch, context stream (the pair of hipEventRecords around the launch: `avg_launch_us_statistics_frames`)"
                                          if lean else "hipEventRecord pair around the launch, context stream"),
                               "kernel_us_device_clock": (1e3 * lk_ms / (iters * args.steps)) if lk_ms > 0 else None,
                               "avg_launch_us_statistics_frames": 1e3 * local_ms / (iters * args.steps) if lean else None,
                               # both definitions every round (round-4 review): `frac` = events attached to the kernel's dispatch (round 4's
                               # final definition), `frac_events_around_launch` = the pair of hipEventRecords around it (rounds 1-3)
                               "frac_events_around_launch": (bytes_per_launch / (1e-3 * local_ms / (iters * args.steps)) / 1e9 / 8000.0) if (lean and local_ms > 0) else None,
                               "algorithmic_bytes_per_launch": bytes_per_launch}
        if not args.no_cpu_baseline and world == 1:
            sample = cpu_baseline(w)
            out["cpu_baseline"] = sample
            if nt >= 500000 and w["kinds"] != "cloth" and not args.n:
                # the extrapolation-free figure, and the PRIMARY one: the same CPU code on the SAME mesh, GS as the global step (the fair
                # 1 M baseline: the reference's LDLT needs a 31-minute factorisation at this size); the reduced-size
                # SuperLU sample of rounds 1-3 rides along as `sample_reduced_size`
                full = cpu_baseline_full_size(w, sample["cores"])
                out["cpu_baseline"] = {"value": full["admm_iters_per_s"], "unit": "ADMM it/s", "cores": full["cores"], "kind": "port",
                                       "sample": "the benchmarked mesh itself (%d elements): %d whole ADMM iterations in %.1f s on %d OpenMP threads; %s" %
                                                 (full["elements"], full["admm_iterations_timed"], full["seconds"], full["cores"], full["what"]),
                                       "full_size": full, "gpu_over_cpu_at_full_size": value / full["admm_iters_per_s"],
                                       "sample_reduced_size": sample}
            try:    # the port against the real reference pieces, measured in the build container (bench.py --calibrate-cpu-baseline)
                cal = json.load(open(CALIBRATION_FILE))
                out["cpu_baseline"]["calibration"] = dict(cal["summary"], file=os.path.relpath(CALIBRATION_FILE, ROOT), host=cal.get("host"),
                                                          omp_threads=cal.get("omp_threads"))
                # x-the-port read as x-the-reference: the reference's time = ratio x the port's, so the factor shrinks (ratio < 1) or grows by it.
                # Two ratios exist (triangle local step, prefactored solve); the tet prox and the GS sweeps of the reference cannot be timed here
                # (mcloptlib / mclscene absent), so the calibrated factor is quoted as the RANGE the two measured ratios span.
                rr = [cal["summary"]["local_step_reference_over_port"], cal["summary"]["solve_reference_over_port"]]
                f0 = out["cpu_baseline"].get("gpu_over_cpu_at_full_size") or (value / out["cpu_baseline"]["value"] if out["cpu_baseline"].get("unit") == "ADMM it/s" else None)
                if f0:
                    out["cpu_baseline"]["gpu_over_cpu_port"] = f0
                    out["cpu_baseline"]["gpu_over_cpu_reference_calibrated"] = [f0 * min(rr), f0 * max(rr)]
            except Exception:
                out["cpu_baseline"]["calibration"] = None
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
