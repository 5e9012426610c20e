"""What the force pass costs on the bench body (profiles/forces_cost.txt):
  1. ms per step with the monitor off / in mode 2 / in mode 3 (mode 2 + the stationarity residual: one force pass, its gather and two
     small reductions more per ADMM iteration), alternated in ONE process, three rounds, 6 steps per entry after one untimed step in
     the mode;
  2. the wall time of one forces(x), stress(x) and energy(x) call from Python, copies included.
With `trace` as the first argument: five warm-up steps, then four steps in mode 3 and nothing else -- the run to put under
rocprofv3 --kernel-trace --stats.
    python experiments/forces_cost.py [trace] [n]"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (first, as in bench.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

args = sys.argv[1:]
trace = bool(args) and args[0] == "trace"
if trace:
    args = args[1:]
n = int(args[0]) if args else None
w = bench.WORKLOADS["blob1m_mix"]
sc, nt, nv = bench.build_scene(w, n)
tol, soft = bench.workload_settings("blob1m_mix")
s = sc.make_solver(pcg_tol=tol, pcg_max_iters=600, soft_modes=soft)
s.upload()
iters = w["admm_iters"]
print("tets %d verts %d admm_iters %d pcg_tol %g soft_modes %d" % (nt, nv, iters, tol, soft), flush=True)


def sync():
    torch.cuda.synchronize(0)


if trace:
    for _ in range(5):
        s.step_device(stats=True)
    s.set_monitor(3)
    for _ in range(4):
        s.step_device()
    sync()
    st = s.admm_history()["stationarity"]
    print("last history (mode 3): stationarity %.6g .. %.6g" % (st[0], st[-1]))
    sys.exit(0)

for _ in range(5):
    s.step_device(stats=True)
sync()
ms = {0: [], 2: [], 3: []}
for rnd in range(3):
    for mode in (0, 2, 3):
        s.set_monitor(mode)
        s.step_device()
        sync()
        t0 = time.perf_counter()
        for _ in range(6):
            s.step_device()
        sync()
        ms[mode].append(1e3 * (time.perf_counter() - t0) / 6)
        print("round %d mode %d: %.3f ms per step" % (rnd, mode, ms[mode][-1]), flush=True)
med = {m: float(np.median(v)) for m, v in ms.items()}
print("median ms per step: off %.3f  mode 2 %.3f  mode 3 %.3f" % (med[0], med[2], med[3]))
print("per ADMM iteration: mode 2 %+.2f us, mode 3 %+.2f us, mode 3 - mode 2 %+.2f us" % (1e3 * (med[2] - med[0]) / iters, 1e3 * (med[3] - med[0]) / iters,
                                                                                    1e3 * (med[3] - med[2]) / iters))
h = s.admm_history()
print("last history (mode 3): stationarity %.6g .. %.6g, primal %.6g .. %.6g" % (h["stationarity"][0], h["stationarity"][-1], h["primal"][0], h["primal"][-1]))
print("solve totals (solves, converged, iterations):", s.solve_totals())
s.set_monitor(0)
s.download()
x = s.m_x.copy()
for name, fn in (("forces", s.forces), ("stress", s.stress), ("energy", s.energy)):
    fn(x)      # (the first call allocates)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn(x)
        t.append(1e3 * (time.perf_counter() - t0))
    print("%s(x) from Python, copies included: %.3f ms (median of 5; %s)" % (name, float(np.median(t)), " ".join("%.3f" % v for v in t)))
t = []
for _ in range(5):
    t0 = time.perf_counter()
    s.forces()
    t.append(1e3 * (time.perf_counter() - t0))
print("forces() of the device-resident state: %.3f ms (median of 5)" % float(np.median(t)))
s.close()
