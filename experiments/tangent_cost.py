"""What the tangent pass costs next to the force pass on the 100k-tet cube (profiles/tangent_cost.txt): after three untimed
calls each, 20 calls of forces(x), 20 of stiffness_apply(d, x) with one direction and 20 with eight, at a stretched and perturbed state,
and nothing else -- the run to put under rocprofv3 --kernel-trace --stats.  k_tangent's dispatches come in that order: the first 23
have n_vec = 1, the last 23 n_vec = 8.
    python experiments/tangent_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints the medians of the timed dispatches.
    python experiments/tangent_cost.py parse out_kernel_trace.csv"""
import csv
import os
import sys

import numpy as np

WARM, CALLS = 3, 20

if len(sys.argv) > 2 and sys.argv[1] == "parse":
    rows = {}
    with open(sys.argv[2]) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].split("(")[0].split("<")[0].split()[-1]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))

    def med(name, a, b):
        t = sorted(rows[name])[a:b]
        d = np.array([e - s for s, e in t]) / 1e3
        return "%-20s %3d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (name.split("::")[-1], len(d), np.median(d), d.min(), d.max())
    for name in rows:
        short = name.split("::")[-1]
        if short in ("k_forces", "k_gather_forces"):
            print("forces        " + med(name, WARM, WARM + CALLS))
        elif short in ("k_tangent", "k_gather_tangent"):
            print("n_vec = 1     " + med(name, WARM, WARM + CALLS))
            print("n_vec = 8     " + med(name, 2 * WARM + CALLS, 2 * WARM + 2 * CALLS))
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
D = rng.standard_normal((8,) + sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
for _ in range(WARM + CALLS):
    f = s.forces(x)
for _ in range(WARM + CALLS):
    k1 = s.stiffness_apply(D[0], x)
for _ in range(WARM + CALLS):
    k8 = s.stiffness_apply(D, x)
assert np.isfinite(f).all() and np.isfinite(k8).all() and np.array_equal(k1, k8[0])
print("|f| %.6e  |K d_0| %.6e" % (np.linalg.norm(f), np.linalg.norm(k1)))
s.close()
