"""What the block PCG costs against single solves on the 100k-tet cube (profiles/tangent_solve_block.txt), at the state of
experiments/newton_cost.py, tol = 1e-8, k in {1, 2, 4, 8, 16} random right-hand sides.

    python experiments/tangent_block_cost.py [--out FILE] [--n N]
is the driver: it starts one child process per k (`measure K`) and one under rocprofv3 --kernel-trace (`trace`), each under a time limit
of its own, stops at the first that fails, and writes the report.  A child does, and nothing else:
  measure K   2 warm rounds, then ROUNDS alternated rounds of {one tangent_solve_block of K columns; K tangent_solve calls}, wall time of
              each on the host (copies included, the stream idle before and after: both entry points synchronise); checks the bits
  trace       k = 8: three block solves and three single solves of column 0 -- the run whose kernel trace gives the per-kernel medians
`parse FILE` prints the medians of a kernel trace (csv) of the `trace` run."""
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 4, 8, 16)
WARM, ROUNDS = 2, 7
TOL, MAX_ITERS = 1e-8, 4000
BLOCK_KERNELS = ("k_tangent_frozen_block", "k_newton_gather_block<true>", "k_nw_cg_step_block", "k_nw_cg_dir_block")
SINGLE_KERNELS = ("k_tangent_frozen", "k_newton_gather<false>", "k_nw_cg_step", "k_nw_cg_dir")


def parse(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            full = r["Kernel_Name"].split("(")[0].split()[-1].split("::")[-1]
            name = full if full.startswith("k_newton_gather") else full.split("<")[0]
            rows.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for name in BLOCK_KERNELS + SINGLE_KERNELS:
        if name in rows:
            d = np.array(rows[name])
            out.append("%-30s %6d dispatches: median %8.2f us, min %8.2f, max %8.2f" % (name, len(d), np.median(d), d.min(), d.max()))
    return out


def scene(n):
    import torch  # noqa: F401  (first, as in bench.py)
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bench
    sc, nt, nv = bench.build_scene(bench.WORKLOADS["cube100k_gs"], n)
    sc.settings["admm_iters"] = 5
    s = sc.make_solver()
    rng = np.random.default_rng(0)
    edge = 1.0 / round((nt / 6.0) ** (1.0 / 3.0))
    x = sc.x * np.array([1.3, 0.8, 1.1]) + 0.06 * edge * rng.uniform(-1.0, 1.0, sc.x.shape)
    return s, x, rng, nt, nv


def measure(k, n):
    s, x, rng, nt, nv = scene(n)
    R = rng.standard_normal((k,) + x.shape)
    tb, ts = [], []
    for rnd in range(WARM + ROUNDS):
        for what in (("block", "singles") if rnd % 2 == 0 else ("singles", "block")):      # alternated: neither always runs behind the other
            t0 = time.perf_counter()
            if what == "block":
                Y, info = s.tangent_solve_block(R, x, tol=TOL, max_iters=MAX_ITERS)
            else:
                single = [s.tangent_solve(R[j], x, tol=TOL, max_iters=MAX_ITERS) for j in range(k)]
            if rnd >= WARM:
                (tb if what == "block" else ts).append(1e3 * (time.perf_counter() - t0))
    for j, (y, i) in enumerate(single):
        assert Y[j].tobytes() == y.tobytes() and info["columns"][j] == i, j
    s.close()
    print(json.dumps(dict(k=k, tets=nt, verts=nv, block_ms=tb, singles_ms=ts, iterations=[i["iterations"] for i in info["columns"]],
                          block_iterations=info["block_iterations"], column_passes=info["column_passes"], blocked=info["blocked"])))


def trace(n):
    s, x, rng, nt, nv = scene(n)
    R = rng.standard_normal((8,) + x.shape)
    for _ in range(3):
        s.tangent_solve_block(R, x, tol=TOL, max_iters=MAX_ITERS)
    for _ in range(3):
        s.tangent_solve(R[0], x, tol=TOL, max_iters=MAX_ITERS)
    s.close()


def driver(out, n):
    me = [sys.executable, os.path.abspath(__file__)]
    extra = ["--n", str(n)] if n else []
    lines = ["block PCG against single solves, tol = %g, %d alternated rounds after %d warm ones; wall ms per call, host clock, copies included" % (TOL, ROUNDS, WARM)]
    for k in KS:
        p = subprocess.run(me + ["measure", str(k)] + extra, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:
            lines.append("k = %d: the child ended with status %d; nothing after it was run\n%s" % (k, p.returncode, p.stderr[-2000:]))
            break
        r = json.loads(p.stdout.strip().splitlines()[-1])
        b, sg = np.array(r["block_ms"]), np.array(r["singles_ms"])
        lines.append("k = %2d (%d tets): block %8.2f ms median [%8.2f .. %8.2f] = %7.2f ms per solve; %2d singles %8.2f ms median [%8.2f .. %8.2f]; "
                     "block / singles per round %s; block wins %d of %d rounds; iterations %d .. %d, block_iterations %d, column_passes %d, "
                     "%.1f us per block iteration" % (k, r["tets"], np.median(b), b.min(), b.max(), np.median(b) / k, k, np.median(sg), sg.min(), sg.max(),
                                                     " ".join("%.2f" % q for q in b / sg), int((b < sg).sum()), len(b), min(r["iterations"]),
                                                     max(r["iterations"]), r["block_iterations"], r["column_passes"],
                                                     1e3 * np.median(b) / max(1, r["block_iterations"])))
    else:
        tdir = os.path.join(os.path.dirname(os.path.abspath(out)), "tangent_block_trace")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tdir, "-o", "p", "--"] + me + ["trace"] + extra,
                           capture_output=True, text=True, timeout=300)
        found = [os.path.join(d, f) for d, _, fs in os.walk(tdir) for f in fs if f.endswith("kernel_trace.csv")]
        if p.returncode != 0 or not found:
            lines.append("rocprofv3 --kernel-trace: status %d, no trace\n%s" % (p.returncode, p.stderr[-2000:]))
        else:
            lines.append("rocprofv3 --kernel-trace, k = 8: three block solves, then three single solves (every dispatch of the run)")
            lines += parse(found[0])
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    a = sys.argv[1:]
    n = int(a[a.index("--n") + 1]) if "--n" in a else None
    if a and a[0] == "parse":
        print("\n".join(parse(a[1])))
    elif a and a[0] == "measure":
        measure(int(a[1]), n)
    elif a and a[0] == "trace":
        trace(n)
    else:
        driver(a[a.index("--out") + 1] if "--out" in a else os.path.join(HERE, "..", "profiles", "tangent_solve_block.txt"), n)
