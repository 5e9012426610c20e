"""What the coarse inverse of the two-level tangent preconditioner costs one-block and blocked (Solver.set_tangent_coarse) on the
100k-tet cube (profiles/tangent_coarse_blocked.txt), at the state of experiments/tangent_precond_cost.py and by its method.
    python experiments/tangent_coarse_cost.py trace [n]     the run to put under rocprofv3 --kernel-trace: for G = 8, 16, 32, 64 and
                                                            each inverse, 3 warm + 10 calls of tangent_solve(max_iters=1) (a setup each)
    python experiments/tangent_coarse_cost.py parse FILE    reads the kernel trace (csv) of such a run: per G the median, min and max over
                                                            the 10 solves of k_tc_invert and of the SUM of a solve's k_tcb_ chain, the
                                                            ratio, and the chain's kernels one by one
    python experiments/tangent_coarse_cost.py wall [n]      no profiler: tangent_solve(tol=1e-8) with Jacobi, two-level one-block and
                                                            two-level blocked at G = 8, 16, 32, 64, ALTERNATED (5 rounds of the three
                                                            after a warm round), host clock around the Python call, copies included"""
import csv
import os
import sys
import time

import numpy as np

WARM, CALLS = 3, 10
N = WARM + CALLS
GS = (8, 16, 32, 64)
T = 64
CHAIN = ("k_tcb_scan", "k_tcb_scale", "k_tcb_potrf", "k_tcb_panel", "k_tcb_update", "k_tcb_winv", "k_tcb_wtw", "k_tcb_unscale", "k_tcb_final")


def per_solve(nc):
    """launches of one chain, per kernel"""
    nt = -(-nc // T)
    return dict(k_tcb_scan=1, k_tcb_scale=1, k_tcb_potrf=nt, k_tcb_panel=nt - 1, k_tcb_update=nt - 1, k_tcb_winv=1, k_tcb_wtw=1, k_tcb_unscale=1, k_tcb_final=1)


mode = sys.argv[1] if len(sys.argv) > 1 else "wall"
if mode == "parse":
    rows = {}
    with open(sys.argv[2]) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1].split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    dur = {k: np.array([e - s for s, e in sorted(v)]) / 1e3 for k, v in rows.items()}
    off = {k: 0 for k in CHAIN}
    one = dur.get("k_tc_invert", np.zeros(0))
    for gi, G in enumerate(GS):
        nc, cnt = 12 * G, per_solve(12 * G)
        o = one[gi * N:(gi + 1) * N][WARM:]
        parts = {}
        for k in CHAIN:
            d = dur[k][off[k]:off[k] + N * cnt[k]]
            off[k] += N * cnt[k]
            parts[k] = d.reshape(N, cnt[k])[WARM:] if cnt[k] else np.zeros((CALLS, 0))
        tot = sum(p.sum(axis=1) for p in parts.values())
        print("G = %d, nc = %d, %d launches a chain:" % (G, nc, sum(cnt.values())))
        print("   k_tc_invert (one block)        %2d: median %10.2f us, min %10.2f, max %10.2f, spread %.2f %%" % (len(o), np.median(o), o.min(), o.max(), 100 * (o.max() - o.min()) / np.median(o)))
        print("   sum of the k_tcb_ chain        %2d: median %10.2f us, min %10.2f, max %10.2f   ratio of the medians %.1f" % (len(tot), np.median(tot), tot.min(), tot.max(), np.median(o) / np.median(tot)))
        for k in CHAIN:
            if cnt[k]:
                print("      %-14s x %2d: per chain median %8.2f us; one dispatch median %7.2f, min %7.2f, max %7.2f"
                      % (k, cnt[k], np.median(parts[k].sum(axis=1)), np.median(parts[k]), parts[k].min(), parts[k].max()))
    sys.exit(0)

import torch  # noqa: F401,E402  (first, as in bench.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

n = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else None
sc, nt, nv = bench.build_scene(bench.WORKLOADS["cube100k_gs"], n)
sc.settings["admm_iters"] = 5
s = sc.make_solver()
rng = np.random.default_rng(0)
edge = 1.0 / round((nt / 6.0) ** (1.0 / 3.0))
x = sc.x * np.array([1.3, 0.8, 1.1]) + 0.06 * edge * rng.uniform(-1.0, 1.0, sc.x.shape)
d = rng.standard_normal(sc.x.shape)
print("tets %d verts %d" % (nt, nv), flush=True)

if mode == "trace":
    for G in GS:
        s.set_tangent_precond("two_level", G)
        for solver in ("one_block", "blocked"):
            s.set_tangent_coarse(solver)
            for _ in range(N):
                s.tangent_solve(d, x, max_iters=1)
            print("G = %d %s: %s %s" % (G, solver, s.tangent_precond(), s.tangent_coarse()), flush=True)
    s.close()
    sys.exit(0)

ROUNDS = 5
for G in GS:
    cases = (("jacobi", "one_block"), ("two_level", "one_block"), ("two_level", "blocked"))
    times = {c: [] for c in cases}
    its = {}
    for rnd in range(ROUNDS + 1):      # (round 0 warms: the plan and the buffers of this G)
        for c in cases:
            s.set_tangent_precond(c[0], G)
            s.set_tangent_coarse(c[1])
            t0 = time.perf_counter()
            y, info = s.tangent_solve(d, x, tol=1e-8, max_iters=4000)
            t1 = time.perf_counter()
            assert info["converged"], info
            its[c] = info["iterations"]
            if rnd:
                times[c].append(1e3 * (t1 - t0))
    for c in cases:
        t = np.array(times[c])
        print("G %2d tangent_solve(tol=1e-8) %-9s %-9s: %4d iterations, wall ms median %8.3f, min %8.3f, max %8.3f  (%s)"
              % (G, c[0], c[1] if c[0] == "two_level" else "-", its[c], np.median(t), t.min(), t.max(), " ".join("%.3f" % v for v in t)), flush=True)
s.close()
