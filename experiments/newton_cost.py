"""What the frozen tangent, a PCG iteration on it and a Newton polish cost on the 100k-tet cube (profiles/newton_cost.txt), at
the state of experiments/tangent_cost.py -- the run to put under rocprofv3 --kernel-trace.  In this order, and nothing else:
  23 calls of stiffness_apply(d, x)              k_tangent, k_gather_tangent: the parent's figures in the same session
  23 calls of stiffness_apply_ex(d, x, psd=True)    k_tangent_setup, k_tangent_frozen, k_newton_gather<false>
  23 calls of tangent_solve(max_iters=1)         k_tangent_diag, k_newton_gather<true>
   1 call  of tangent_solve(tol=0, max_iters=23) k_nw_cg_step, k_nw_cg_dir: 23 more dispatches each
then, timed on the host: tangent_solve(tol=1e-8) and, after one step of 5 ADMM iterations, newton_polish(max_iters=1).
    python experiments/newton_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints the medians of 20 dispatches after 3 warm ones.
    python experiments/newton_cost.py parse out_kernel_trace.csv"""
import csv
import os
import sys
import time

import numpy as np

WARM, CALLS = 3, 20
N = WARM + CALLS

if len(sys.argv) > 2 and sys.argv[1] == "parse":
    rows = {}
    with open(sys.argv[2]) as fh:
        for r in csv.DictReader(fh):
            full = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1]
            name = full if full.startswith("k_newton_gather") else full.split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))

    def med(name, first):
        t = sorted(rows[name])[first + WARM:first + N]
        d = np.array([e - s for s, e in t]) / 1e3
        return "%-24s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (name, len(d), np.median(d), d.min(), d.max())
    for name, first in (("k_tangent", 0), ("k_gather_tangent", 0), ("k_tangent_setup", 0), ("k_tangent_frozen", 0), ("k_newton_gather<false>", 0),
                        ("k_tangent_diag", 0), ("k_newton_gather<true>", 0), ("k_nw_cg_step", N), ("k_nw_cg_dir", N)):
        if name in rows:
            print(med(name, first))
    sys.exit(0)

import torch  # noqa: F401,E402  (first, as in bench.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else None
sc, nt, nv = bench.build_scene(bench.WORKLOADS["cube100k_gs"], n)
sc.settings["admm_iters"] = 5
s = sc.make_solver()
rng = np.random.default_rng(0)
edge = 1.0 / round((nt / 6.0) ** (1.0 / 3.0))
x = sc.x * np.array([1.3, 0.8, 1.1]) + 0.06 * edge * rng.uniform(-1.0, 1.0, sc.x.shape)
d = rng.standard_normal(sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
for _ in range(N):
    k0 = s.stiffness_apply(d, x)
for _ in range(N):
    k1 = s.stiffness_apply_ex(d, x, psd=True)
for _ in range(N):
    s.tangent_solve(d, x, max_iters=1)
y, info = s.tangent_solve(d, x, tol=0.0, max_iters=N)
assert np.isfinite(k1).all() and np.isfinite(y).all() and info["iterations"] == N, info
print("|K d| %.6e  |K_psd d| %.6e  residual after %d iterations %.3e" % (np.linalg.norm(k0), np.linalg.norm(k1), N, info["residual"]))
for _ in range(3):
    t0 = time.perf_counter()
    y, info = s.tangent_solve(d, x, tol=1e-8, max_iters=2000)
    t1 = time.perf_counter()
    print("tangent_solve(tol=1e-8): %d iterations, converged %s, %.3f ms wall (%.1f us per iteration, copies included)"
          % (info["iterations"], info["converged"], 1e3 * (t1 - t0), 1e6 * (t1 - t0) / max(1, info["iterations"])))
try:
    s.step()
    for _ in range(3):
        t0 = time.perf_counter()
        rec = s.newton_polish(max_iters=1, grad_tol=0.0, cg_tol=1e-8, cg_max=2000)
        t1 = time.perf_counter()
        print("newton_polish(max_iters=1): |g| %.3e -> %.3e, %d CG iterations, step %g, %.3f ms wall"
              % (rec[0]["grad_norm"], rec[-1]["grad_norm"], rec[0]["cg_iterations"], rec[0]["step"], 1e3 * (t1 - t0)))
except Exception as e:      # (a workload the polish refuses)
    print("newton_polish: %s" % e)
s.close()
