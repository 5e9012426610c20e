"""What the rest-shape sensitivity pass costs next to the tangent pass on the 100k-tet cube (profiles/rest_sens_cost.txt), at the
state of experiments/tangent_cost.py -- the run to put under rocprofv3 --kernel-trace (no counters in the same run).  In this order, and
nothing else:
  23 calls of stiffness_apply(d, x), 1 direction      k_tangent
  23 calls of stiffness_apply(D, x), 8 directions     k_tangent: 23 more dispatches
  23 calls of rest_sensitivity(a, x), k = 1           k_rest_sens
  23 calls of rest_sensitivity(A, x), k = 8           k_rest_sens: 23 more dispatches
    python experiments/rest_sens_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints the medians of 20 dispatches after 3 warm ones.
    python experiments/rest_sens_cost.py parse out_kernel_trace.csv"""
import csv
import os
import sys

import numpy as np

WARM, CALLS = 3, 20
N = WARM + CALLS

if len(sys.argv) > 2 and sys.argv[1] == "parse":
    rows = {}
    with open(sys.argv[2]) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1].split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))

    def med(name, first, label):
        t = sorted(rows[name])[first + WARM:first + WARM + CALLS]
        d = np.array([e - s for s, e in t]) / 1e3
        return "%-28s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (label, len(d), np.median(d), d.min(), d.max())
    print(med("k_tangent", 0, "k_tangent, 1 direction"))
    print(med("k_tangent", N, "k_tangent, 8 directions"))
    print(med("k_rest_sens", 0, "k_rest_sens, k = 1"))
    print(med("k_rest_sens", N, "k_rest_sens, k = 8"))
    g = sorted(rows["k_gather_tangent"])
    for first, label in ((0, "1 direction"), (N, "8 directions"), (2 * N, "k = 1 (rest)"), (3 * N, "k = 8 (rest)")):
        d = np.array([e - s for s, e in g[first + WARM:first + WARM + CALLS]]) / 1e3
        print("%-28s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % ("k_gather_tangent, " + label, len(d), np.median(d), d.min(), d.max()))
    sys.exit(0)

import torch  # noqa: F401,E402  (first, as in bench.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else None
sc, nt, nv = bench.build_scene(bench.WORKLOADS["cube100k_gs"], n)
s = sc.make_solver()
rng = np.random.default_rng(0)
edge = 1.0 / round((nt / 6.0) ** (1.0 / 3.0))
x = sc.x * np.array([1.3, 0.8, 1.1]) + 0.06 * edge * rng.uniform(-1.0, 1.0, sc.x.shape)
A = rng.standard_normal((8,) + sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
for _ in range(N):
    k1 = s.stiffness_apply(A[0], x)
for _ in range(N):
    k8 = s.stiffness_apply(A, x)
for _ in range(N):
    r1 = s.rest_sensitivity(A[0], x)
for _ in range(N):
    r8 = s.rest_sensitivity(A, x)
assert k8[0].tobytes() == k1.tobytes() and r8[0].tobytes() == r1.tobytes()
print("|K a| %.12e  |d(a . f)/dX| %.12e  |sum_v| %.3e" % (np.linalg.norm(k1), np.linalg.norm(r1), np.abs(r1.sum(axis=0)).max()))
s.close()
