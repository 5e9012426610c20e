"""What the two-level preconditioner of the tangent solves costs and saves on the 100k-tet cube (profiles/tangent_precond.txt),
at the state of experiments/newton_cost.py -- the run to put under rocprofv3 --kernel-trace.  In this order:
  phase J            1 call of tangent_solve(tol=0, max_iters=23), Jacobi           k_nw_cg_step, k_nw_cg_dir, the frozen pass: 23 dispatches
  phase G, G = 32    23 calls of tangent_solve(max_iters=1), two-level              the setup kernels: 23 solves (ceil(12 G / 16) passes each)
                     1 call of tangent_solve(tol=0, max_iters=23)                   k_nw_cg_step, k_tc_restrict, k_tc_coarse, k_tc_cg_dir
  phase G, G = 64    the same
then, timed on the host (three times each, kind by kind): tangent_solve(tol=1e-8) with Jacobi, G = 32 and G = 64; tangent_precond_apply
(the setup and one application); and, in a context each after one step of 5 ADMM iterations, newton_polish(max_iters=1) each way.
    python experiments/tangent_precond_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints, per phase, the medians of 20 dispatches after 3 warm ones
(per-pass kernels: the median over 20 solves of the sum over a solve's passes).
    python experiments/tangent_precond_cost.py parse out_kernel_trace.csv"""
import csv
import os
import sys
import time

import numpy as np

WARM, CALLS = 3, 20
N = WARM + CALLS
GS = (32, 64)

if len(sys.argv) > 2 and sys.argv[1] == "parse":
    rows = {}
    with open(sys.argv[2]) as fh:
        for r in csv.DictReader(fh):
            full = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1]
            name = full if full.startswith("k_newton_gather") else full.split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    dur = {k: np.array([e - s for s, e in sorted(v)]) / 1e3 for k, v in rows.items()}

    def line(label, d):
        return "   %-44s %3d: median %9.2f us, min %9.2f, max %9.2f" % (label, len(d), np.median(d), d.min(), d.max()) if len(d) else "   %-44s none" % label
    print("all dispatches of the run, per kernel:")
    for k in sorted(dur):
        if k.startswith(("k_tc_", "k_nw_cg", "k_tangent_frozen", "k_newton_gather", "k_tangent_diag", "k_tangent_setup")):
            print(line(k, dur[k]))
    # phase J: one solve of N iterations -- N + 1 frozen passes (the true residual), N of step / dir
    print("phase J (Jacobi, one %d-iteration solve): the last %d dispatches" % (N, CALLS))
    for k, per in (("k_tangent_frozen", N + 1), ("k_newton_gather<false>", N + 1), ("k_nw_cg_step", N), ("k_nw_cg_dir", N)):
        if k in dur and len(dur[k]) >= per:
            print(line(k, dur[k][:per][WARM:N]))
    off = {k: 0 for k in dur}
    off.update({"k_tangent_frozen": N + 1, "k_newton_gather<false>": N + 1, "k_nw_cg_step": N})      # (phase J's)
    for G in GS:
        passes = -(-12 * G // 16)
        solves = N + 1
        print("phase G = %d (%d passes a setup): setup kernels over solves %d .. %d, iteration kernels over the last %d of the %d-iteration solve" % (G, passes, WARM, N - 1, CALLS, N))
        for k in ("k_tc_basis", "k_tc_sym", "k_tc_invert"):
            if k in dur:
                print(line(k, dur[k][off[k]:off[k] + solves][WARM:N])); off[k] += solves
        for k in ("k_tc_fill", "k_tangent_frozen_block", "k_newton_gather_block", "k_tc_restrict_block"):
            if k in dur:
                d = dur[k][off[k]:off[k] + solves * passes]
                if len(d) == solves * passes:
                    print(line(k + ", sum of a setup's passes", d.reshape(solves, passes).sum(axis=1)[WARM:N]))
                    print(line(k + ", one pass", d.reshape(solves, passes)[WARM:N].ravel()))
                off[k] += solves * passes
        for k, per_small, per_big in (("k_tc_cg_init", 1, 1), ("k_tc_cg_init2", 1, 1), ("k_tc_restrict", 2, N + 1), ("k_tc_coarse", 2, N + 1),
                                      ("k_nw_cg_step", 1, N), ("k_tc_cg_dir", 1, N), ("k_tangent_frozen", 2, N + 1), ("k_newton_gather<false>", 2, N + 1)):
            if k in dur:
                tot = N * per_small + per_big
                d = dur[k][off[k]:off[k] + tot]
                print(line(k, d[-CALLS:] if per_big > 1 else d[WARM:N])); off[k] += tot
    sys.exit(0)

import torch  # noqa: F401,E402  (first, as in bench.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else None
sc, nt, nv = bench.build_scene(bench.WORKLOADS["cube100k_gs"], n)
sc.settings["admm_iters"] = 5
s = sc.make_solver()
rng = np.random.default_rng(0)
edge = 1.0 / round((nt / 6.0) ** (1.0 / 3.0))
x = sc.x * np.array([1.3, 0.8, 1.1]) + 0.06 * edge * rng.uniform(-1.0, 1.0, sc.x.shape)
d = rng.standard_normal(sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
KINDS = [("jacobi", None)] + [("two_level", G) for G in GS]

y, info = s.tangent_solve(d, x, tol=0.0, max_iters=N)
assert info["iterations"] == N, info
for G in GS:
    s.set_tangent_precond("two_level", G)
    for _ in range(N):
        s.tangent_solve(d, x, max_iters=1)
    y, info = s.tangent_solve(d, x, tol=0.0, max_iters=N)
    assert np.isfinite(y).all() and info["iterations"] == N, info
    print("G = %d: %s, residual after %d iterations %.3e" % (G, s.tangent_precond(), N, info["residual"]), flush=True)
for kind, G in KINDS:      # (kind by kind: a change of G plans and allocates again)
    s.set_tangent_precond(kind, G)
    for rep in range(3):
        t0 = time.perf_counter()
        y, info = s.tangent_solve(d, x, tol=1e-8, max_iters=4000)
        t1 = time.perf_counter()
        print("tangent_solve(tol=1e-8) %-9s G %-4s: %4d iterations, converged %s, %8.3f ms wall (copies included)"
              % (kind, G, info["iterations"], info["converged"], 1e3 * (t1 - t0)), flush=True)
    if kind == "two_level":
        for rep in range(3):
            t0 = time.perf_counter()
            s.tangent_precond_apply(d, x)
            t1 = time.perf_counter()
            print("tangent_precond_apply G %d (pin mask, frames, diagonal, coarse setup, one application, copies): %8.3f ms wall" % (G, 1e3 * (t1 - t0)), flush=True)
s.close()
for kind, G in KINDS:      # a context each: the polish runs on the state its own step left
    s = sc.make_solver()
    s.set_tangent_precond(kind, G)
    s.tangent_solve(d, x, max_iters=1)      # (the buffers of the solve)
    try:
        s.step()
        t0 = time.perf_counter()
        rec = s.newton_polish(max_iters=1, grad_tol=0.0, cg_tol=1e-8, cg_max=4000)
        t1 = time.perf_counter()
        print("newton_polish(max_iters=1) %-9s G %-4s: |g| %.3e -> %.3e, %4d CG iterations, step %g, %8.3f ms wall"
              % (kind, G, rec[0]["grad_norm"], rec[-1]["grad_norm"], rec[0]["cg_iterations"], rec[0]["step"], 1e3 * (t1 - t0)), flush=True)
    except Exception as e:      # (a workload the polish refuses)
        print("newton_polish: %s" % e)
    s.close()
