"""What the block frozen pass and an iteration of the block eigensolver cost on the 100k-tet cube (profiles/modes_cost.txt), at
the state of experiments/newton_cost.py -- the run to put under rocprofv3 --kernel-trace.  In this order, and nothing else:
  23 calls of stiffness_apply_ex(d, x, psd=True)                       k_tangent_frozen, k_newton_gather<false>: one direction
  23 calls of stiffness_apply_ex(D [12], x, psd=True, block=True)      k_tangent_frozen_block, k_newton_gather_block: 12 directions
   1 call  of modes(k=8, guard=4, tol=0, max_iters=23)                 k_modal_resid, k_modal_gram, k_modal_rr, k_modal_update: 23 iterations
                                                                       (the first dispatch of gram / rr / update is the start's Rayleigh-Ritz)
then, timed on the host: modes(k=8, guard=4, tol=1e-8, max_iters=2000), three calls.
    python experiments/modes_cost.py [n]
With `parse FILE` it reads the kernel trace (csv) of such a run and prints the medians of 20 dispatches after 3 warm ones.
    python experiments/modes_cost.py parse out_kernel_trace.csv"""
import csv
import os
import sys
import time

import numpy as np

WARM, CALLS = 3, 20
N = WARM + CALLS
K, GUARD = 8, 4

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
    # k_tangent_frozen_block: the 23 blocked calls come first, the eigensolver's dispatches (12 directions as well) after them
    for name, first in (("k_tangent_frozen", 0), ("k_newton_gather<false>", 0), ("k_tangent_frozen_block", 0), ("k_newton_gather_block", 0),
                        ("k_modal_resid", 0), ("k_modal_gram", 1), ("k_modal_rr", 1), ("k_modal_update", 1)):
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
D = rng.standard_normal((K + GUARD,) + sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)
for _ in range(N):
    k1 = s.stiffness_apply_ex(D[0], x, psd=True)
for _ in range(N):
    kb = s.stiffness_apply_ex(D, x, psd=True, block=True)
assert np.array_equal(kb[0], k1) and np.isfinite(kb).all()
lam, phi, info = s.modes(K, x, tol=0.0, max_iters=N, guard=GUARD)
assert info["iterations"] == N and np.isfinite(phi).all(), info
print("after %d iterations: lambda %s, residuals %s" % (N, np.array2string(lam, precision=4), np.array2string(info["residual"], precision=2)), flush=True)
for _ in range(3):
    t0 = time.perf_counter()
    lam, phi, info = s.modes(K, x, tol=1e-8, max_iters=2000, guard=GUARD)
    t1 = time.perf_counter()
    print("modes(k=%d, guard=%d, tol=1e-8): %d iterations, ended by %s, %d restarts, %.3f ms wall (%.1f us per iteration, copies included); "
          "lambda %s; residuals %s" % (K, GUARD, info["iterations"], info["ended_by"], info["restarts"], 1e3 * (t1 - t0),
                                      1e6 * (t1 - t0) / max(1, info["iterations"]), np.array2string(lam, precision=4),
                                      np.array2string(info["residual"], precision=2)), flush=True)
s.close()
