"""What the parameter-sensitivity pass and an adjoint solve cost on the 100k-tet cube (profiles/adjoint_cost.txt), at the state of
experiments/tangent_cost.py -- the run to put under rocprofv3 --kernel-trace (no counters in the same run).  In this order, and nothing else:
  23 calls of forces(x)                           k_forces: the parent's figure in the same session
  23 calls of param_sensitivity(a, x), k = 1      k_param_sens
  23 calls of param_sensitivity(A, x), k = 8      k_param_sens: 23 more dispatches
then, timed on the host after one step of 5 ADMM iterations and a polish: step_adjoint(tol=1e-8) next to tangent_solve(tol=1e-8, the
exact tangent) at the same state; their vector kernels k_adj_rhs and k_adj_out are in the trace once per step_adjoint.
    python experiments/adjoint_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints the medians of 20 dispatches after 3 warm ones.
    python experiments/adjoint_cost.py parse out_kernel_trace.csv"""
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
            name = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1].split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))

    def med(name, first, label=None, count=CALLS):
        t = sorted(rows[name])[first + WARM:first + WARM + count]
        d = np.array([e - s for s, e in t]) / 1e3
        return "%-28s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (label or name, len(d), np.median(d), d.min(), d.max())
    print(med("k_forces", 0))
    print(med("k_param_sens", 0, "k_param_sens, k = 1"))
    print(med("k_param_sens", N, "k_param_sens, k = 8"))
    for name in ("k_adj_rhs", "k_adj_out"):
        if name in rows:
            t = sorted(rows[name])
            d = np.array([e - s for s, e in t]) / 1e3
            print("%-28s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (name, len(d), np.median(d), d.min(), d.max()))
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
A = rng.standard_normal((8,) + sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
for _ in range(N):
    f = s.forces(x)
for _ in range(N):
    p1 = s.param_sensitivity(A[0], x)
for _ in range(N):
    p8 = s.param_sensitivity(A, x)
assert p8["tets"][0].tobytes() == p1["tets"].tobytes()
print("a . f %.12e  sum d_scale %.12e" % (float(np.sum(A[0] * f)), float(p1["tets"][:, 3].sum())))
try:
    s.step()
    rec = s.newton_polish(max_iters=5, grad_tol=0.0, cg_tol=1e-8, cg_max=2000)
    print("polish: |g| %s" % " ".join("%.3e" % r["grad_norm"] for r in rec))
    for _ in range(3):
        t0 = time.perf_counter()
        out = s.step_adjoint(A[1], A[2], tol=1e-8, max_iters=2000)
        t1 = time.perf_counter()
        y, info = s.tangent_solve(A[1] + A[2] / s._settings.timestep_s, psd=False, tol=1e-8, max_iters=2000)
        t2 = time.perf_counter()
        print("step_adjoint(tol=1e-8): %d iterations, converged %s, %.3f ms wall; tangent_solve(tol=1e-8, psd=False): %d iterations, converged %s, "
              "%.3f ms wall" % (out["info"]["iterations"], out["info"]["converged"], 1e3 * (t1 - t0), info["iterations"], info["converged"], 1e3 * (t2 - t1)))
except Exception as e:      # (a workload the adjoint refuses)
    print("step_adjoint: %s" % e)
s.close()
