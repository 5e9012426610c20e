"""What Anderson acceleration of the ADMM loop costs and what it buys at scale (profiles/anderson_cost.txt).  The scenes are
bench.py's own (bench.build_scene, imported): the 100k-tet Neo-Hookean cube of DESIGN 4i / 4j and the 1M-tet bench body, both with
linsolver 0 (the acceleration refuses the other two).

    python experiments/anderson_cost.py kernels WORKLOAD WINDOW [n]
        the run to put under rocprofv3 --kernel-trace --stats: 4 steps of 20 iterations with the window (0: the plain loop, for the other
        kernels' totals); nothing else
    python experiments/anderson_cost.py parse WORKLOAD WINDOW out_kernel_trace.csv [n]
        medians of the three phases' dispatches from that trace, the bytes they move by count and the share of the HBM rate
    python experiments/anderson_cost.py plain WORKLOAD [n]
        one process: ms per plain step (window 0) by device events, 3 warm steps, then 8 timed ones -- run once per library
        (ADMM_HIP_LIB selects the parent's), alternating, by the caller
    python experiments/anderson_cost.py target WORKLOAD [n]
        time to a stationarity target: the level the plain run reaches after 60 iterations (monitor mode 3); for the plain run and windows
        3 and 5 the first accepted iteration at or below it, then the time of a step of that many iterations (monitor off) from the same
        state by the step's device events, 5 alternating repeats

WORKLOAD: cube100k (bench's cube100k_gs scene, linsolver 0) or body1m (bench's default workload's scene, linsolver 0).
"""
import csv
import os
import re
import sys

import numpy as np

HBM_PEAK = 8.0e12      # bytes/s, MI355X specification


def build(name, n=None):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    key = {"cube100k": "cube100k_gs", "body1m": "blob1m_mix"}[name]
    w = dict(bench.WORKLOADS[key], linsolver=0)
    sc, nt, nv = bench.build_scene(w, n)
    tol, soft = bench.workload_settings(key)
    return sc, nt, nv, dict(pcg_tol=tol, pcg_max_iters=600, soft_modes=soft if name == "body1m" else 0)


def state_doubles(sc, nt, nv):
    """meaningful entries of the state (x, u): 3 nv + 9 nt + 6 ntri + 3 nbend + 3 per pin term (the rows 3..5 of a pin are never populated)"""
    ntri = sum(len(t[1]) for t in sc.tris)
    return 3 * nv + 9 * nt + 6 * ntri + 3 * len(sc.pins)


def main():
    mode, name = sys.argv[1], sys.argv[2]
    if mode == "parse":
        window, path = int(sys.argv[3]), sys.argv[4]
        n = int(sys.argv[5]) if len(sys.argv) > 5 else None
        sc, nt, nv, _ = build(name, n)
        vec = 8.0 * state_doubles(sc, nt, nv)
        rows = {}
        with open(path) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"(\w+)\s*(?:<[^()]*>)?\s*(?:\(|$)", r["Kernel_Name"].replace("void ", ""))      # the name without namespace and template arguments
                k = m.group(1) if m else r["Kernel_Name"]
                rows.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        print("%s, window %d: %d tets, %d verts, a state vector %.1f MB" % (name, window, nt, nv, vec / 1e6))
        # steady state: the ring full -- record reads g, s and `window` old F (window + 2) and writes g, F; apply reads window + 1 g and writes s twice
        counts = {"k_aa_record": (window + 2 + 2) * vec, "k_aa_apply": (window + 1 + 2) * vec, "k_aa_solve": 0.0, "k_aa_init": 2 * vec}
        for k in ("k_aa_init", "k_aa_record", "k_aa_solve", "k_aa_apply"):
            if k not in rows:
                continue
            d = np.array(rows[k])
            big = d[d >= 0.5 * np.median(d)] if k == "k_aa_apply" else d      # (an apply behind a plain or the last evaluation returns at once)
            med = float(np.median(big))
            line = "%-12s %4d dispatches: median %9.2f us, min %9.2f, max %9.2f" % (k, len(d), med, d.min(), d.max())
            if counts[k] > 0:
                rate = counts[k] / (med * 1e-6)
                line += "   %.1f MB by count -> %.2f TB/s = %.0f %% of %.1f TB/s" % (counts[k] / 1e6, rate / 1e12, 100.0 * rate / HBM_PEAK, HBM_PEAK / 1e12)
            print(line)
        for k in sorted(rows):
            if not k.startswith("k_aa_"):
                print("    %-28s %5d dispatches, total %10.1f us" % (k, len(rows[k]), sum(rows[k])))
        return
    import torch  # noqa: F401  (first, as in bench.py)
    if mode == "kernels":
        window = int(sys.argv[3]); n = int(sys.argv[4]) if len(sys.argv) > 4 else None
        sc, nt, nv, kw = build(name, n)
        sc.settings["admm_iters"] = 20
        s = sc.make_solver(anderson=window, **kw)
        s.upload()
        for _ in range(4):
            s.step_device()
        s.download()
        h = s.anderson_history()
        if window:
            print("%s window %d: tets %d verts %d; last step: %d accepted, %d rejected, |F| %.3e -> %.3e" %
                  (name, window, nt, nv, int(h["accepted"].sum()), int((h["accepted"] == 0).sum()), h["resid"][0], h["resid"][-1]), flush=True)
        assert np.isfinite(s.m_x).all()
        s.close()
        return
    n = int(sys.argv[3]) if len(sys.argv) > 3 else None
    sc, nt, nv, kw = build(name, n)
    if mode == "plain":
        sc.settings["admm_iters"] = 20
        s = sc.make_solver(**kw)
        s.upload()
        ms = []
        for i in range(11):
            s.step_device(stats=True)
            if i >= 3:
                ms.append(s.runtime_data().step_ms)
        s.close()
        print("plain %s lib %s: ms per step of 20 iterations (8 steps after 3 warm): median %.3f min %.3f max %.3f" %
              (name, os.environ.get("ADMM_HIP_LIB", "in-tree"), np.median(ms), min(ms), max(ms)), flush=True)
        return
    assert mode == "target"
    sc.settings["admm_iters"] = 60
    s = sc.make_solver(monitor=3, **kw)
    x0, v0 = s.m_x.copy(), s.m_v.copy()

    def from_rest(iters, stats=False):
        s.m_x, s.m_v = x0.copy(), v0.copy()
        s.upload()
        s.step_device(stats=stats, admm_iters=iters)

    from_rest(60)      # (warm: code objects, the plan's first frames)
    reach = {}
    target = None
    for window in (0, 3, 5):
        s.set_anderson(window)
        from_rest(60)
        st = s.admm_history()["stationarity"]
        if window == 0:
            target = st[59]
            ok = st <= target
        else:
            ok = (st <= target) & (s.anderson_history()["accepted"] == 1)
        hit = np.nonzero(ok)[0]
        reach[window] = int(hit[0]) + 1 if hit.size else None
        print("%s window %d: stationarity it 1 %.3e, it 20 %.3e, it 60 %.3e; target %.3e first met at iteration %s; rejections %d" %
              (name, window, st[0], st[19], st[59], target, reach[window], 0 if window == 0 else int((s.anderson_history()["accepted"] == 0).sum())), flush=True)
    s.set_monitor(0)
    times = {w: [] for w in reach if reach[w]}
    for rep in range(6):
        for window in times:
            s.set_anderson(window)
            from_rest(reach[window], stats=True)
            if rep:      # (the first round warms every variant)
                times[window].append(s.runtime_data().step_ms)
    for window, t in times.items():
        print("%s window %d: %d iterations to the target, step %.3f ms median of 5 (min %.3f, max %.3f), %.1f us per iteration" %
              (name, window, reach[window], np.median(t), min(t), max(t), 1e3 * np.median(t) / reach[window]), flush=True)
    for window in times:
        if window:
            print("%s window %d against plain: %.2f x the time" % (name, window, np.median(times[window]) / np.median(times[0])), flush=True)
    s.close()


if __name__ == "__main__":
    main()
