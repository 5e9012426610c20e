"""Writes tests/golden/pcg2_entry_halo_parent_bits.json: what the on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2) computed BEFORE the first
residual of a launch stopped exchanging the entry x between the blocks (it now reads the halo of x0 from global memory through the plan's
halo_vert).  SHA-256 digests of m_x and m_v after the last frame, the solve totals and the instance counts; for the stand-alone solves the
digest of the solution and the iteration count.  tests/test_pcg2_entry_halo.py holds every later library to these bits.  Same method as
make_solve_entry_parent_bits.py (whose helpers are used), on the cases the earlier fixtures do not pin and that change can break:
  * blob_scene(30) at the plan's own block shape -- T = 128 with a longest halo of 287 > 2 T entries, the only small scene that walks the
    third halo entry of a thread from the list -- and at one wave per block (the largest halo / T, generic instance only);
  * stand-alone solves (generic instance, no recycled start) from a random x0 that holds -0.0, denormals and 1e-100 at halo vertices; the
    same with entries of 1e100 among them; and the first with b = 0;
  * pcg_tol 1e-13 on mixed_cube_scene(12), the stand-alone solves included: verifications and further passes, so the first residual of a
    launch takes the new path and the later ones the exchange, within one launch;
  * a cap of three iterations: solves that end unconverged, from a cold first frame on.
No plan of these scenes has a block with more than 64 neighbour blocks (at most 22, tests/test_halo_vert_plan.py prints them), so none
reaches the kernel's path without hand-off lists by itself; tests/test_pcg2_no_handoff.py runs these cases on it with ADMM_HIP_OC_HANDOFF=0.

Run ONCE, on the GPU, with the library of the commit the fixture is named after, in a checkout of that commit (this file copied into its
tests/golden; the generators it imports are there):

    python tests/golden/make_pcg2_entry_halo_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it, and imports the case list and the runner from this file."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "pcg2_entry_halo_parent_bits.json")
PARENT = "0a7e9fe"

_spec = importlib.util.spec_from_file_location("make_solve_entry_parent_bits", os.path.join(HERE, "make_solve_entry_parent_bits.py"))
entry = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(entry)
base = entry.base

FRAMES, ADMM_ITERS = entry.FRAMES, entry.ADMM_ITERS
SCENES = ("blob", "mixed_cube")
ENV_KEYS = entry.ENV_KEYS
CAP = 3      # pcg_max_iters of the capped case
make_scene = entry.make_scene


def _cfg(tol=1e-8, spb=None, max_iters=600, solves=False):
    return dict(tol=tol, spb=spb, max_iters=max_iters, solves=solves)


# name -> (scene, configuration).  Wherever the hot instance serves a case, the test and the generator repeat it with ADMM_HIP_OC_GENERIC=1.
CASES = {
    "blob-uzawa-spb_plan": ("blob", _cfg()),
    "blob-uzawa-spb_1": ("blob", _cfg(spb=1)),
    "blob-uzawa-solves": ("blob", _cfg(solves=True)),
    "mixed_cube-uzawa-cold_paths": ("mixed_cube", _cfg(tol=1e-13, solves=True)),
    "blob-uzawa-capped": ("blob", _cfg(max_iters=CAP)),
}


def entry_vectors(sc, s):
    """The stand-alone solves' inputs: b, and x0 = standard normal with special values at vertices that are halo entries of the plan
    admm_hip_create makes at its own block shape (vertices with a matrix neighbour in another block); the same with 1e100 among them."""
    import numpy as np
    nv = len(sc.x)
    ns = (nv + 63) // 64
    G = min(256, ns); spb = (ns + G - 1) // G
    while spb < 16 and (ns + spb - 1) // spb > 32 * spb:
        spb += 1
    G = (ns + spb - 1) // spb
    rv = s.host_oc_plan(G, spb, settings=sc.product_settings, coarse=False)["row_vertex"]
    blk = np.empty(nv, np.int64); live = rv >= 0
    blk[rv[live]] = np.nonzero(live)[0] // (64 * spb)
    rp, ci, _ = s.host_matrix(sc.product_settings)
    rows = np.repeat(np.arange(nv), np.diff(rp))
    halo = np.unique(ci[blk[ci] != blk[rows]])
    assert len(halo) > 100, len(halo)
    rng = np.random.default_rng(20)
    b = rng.standard_normal((nv, 3))
    x0 = rng.standard_normal((nv, 3))
    small = np.array([-0.0, 5e-324, -2.2e-310, 1e-100, -1e-100, 0.0])
    pick = halo[::3]
    x0[pick] = small[(np.arange(len(pick))[:, None] + np.arange(3)[None, :]) % len(small)]
    x1 = x0.copy()
    x1[halo[1::9]] = np.array([1e100, -1e100, 1e100])
    return b, x0, x1


def run(sc, cfg, generic):
    """FRAMES frames of `sc` under `cfg`; returns (record for the fixture, m_x, m_v).  The switches are read once, when the context is created."""
    import numpy as np
    env = {}
    if cfg["spb"] is not None:
        env["ADMM_HIP_OC_SPB"] = str(cfg["spb"])
    if generic:
        env["ADMM_HIP_OC_GENERIC"] = "1"
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        s = sc.make_solver(pcg_tol=cfg["tol"], pcg_max_iters=cfg["max_iters"], linsolver=2)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    verifications = []      # of the last solve of every frame: two and more = a failed verification, i.e. a further pass
    for _ in range(FRAMES):
        s.step()
        verifications.append(int(s.pcg_instances()["last_verifications"]))
    x, v = s.m_x.copy(), s.m_v.copy()
    rec = dict(m_x=base.digest(x), m_v=base.digest(v), last_verifications=verifications)
    if cfg["solves"]:
        b, x0, x1 = entry_vectors(sc, s)
        for key, bb, xx in (("small", b, x0), ("huge", b, x1), ("zero_rhs", np.zeros_like(b), x0)):
            y, it = s.global_solve(bb, xx)
            rec["solve_" + key + "_x"] = base.digest(y); rec["solve_" + key + "_iters"] = int(it)
            rec["solve_" + key + "_finite"] = bool(np.isfinite(y).all())
            rec["solve_" + key + "_verifications"] = int(s.pcg_instances()["last_verifications"])
    inst = s.pcg_instances()
    rec.update(solve_totals=list(s.solve_totals()), hot=int(inst["hot"]), generic=int(inst["generic"]),
               lane_hot=int(inst["lane_hot"]), lane_generic=int(inst["lane_generic"]))
    s.close()
    return rec, x, v


def main(out):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    sys.path.insert(0, os.path.join(HERE, ".."))
    scs = {name: make_scene(name) for name in SCENES}
    fx = dict(parent=PARENT, frames=FRAMES, admm_iters=ADMM_ITERS, scenes={n: base.scene_digest(s) for n, s in scs.items()}, cases={})
    for cid, (name, cfg) in CASES.items():
        d, _, _ = run(scs[name], cfg, False)
        g = None
        if d["hot"] > 0:
            g, _, _ = run(scs[name], cfg, True)
            assert g["hot"] == 0, (cid, g)
        fx["cases"][cid] = dict(default=d, forced_generic=g)
        print(cid, d["solve_totals"], "hot %d generic %d" % (d["hot"], d["generic"]), "verifications", d["last_verifications"],
              {k: v for k, v in d.items() if k.startswith("solve_") and not k.endswith("_x")}, "| forced generic:", g and g["m_x"] == d["m_x"], flush=True)
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)
    # what the cases are about must have happened on the parent, or they test nothing
    c = fx["cases"]
    bad = []
    for cid in ("blob-uzawa-spb_plan", "mixed_cube-uzawa-cold_paths", "blob-uzawa-capped", "blob-uzawa-solves"):
        if not c[cid]["default"]["hot"] >= FRAMES * ADMM_ITERS:
            bad.append(cid + ": the hot instance did not serve the ADMM loop")
    if c["blob-uzawa-spb_1"]["default"]["hot"] != 0:
        bad.append("blob-uzawa-spb_1: one wave per block ran the hot instance")
    d = c["mixed_cube-uzawa-cold_paths"]["default"]
    # (a pass is trusted for nine orders of magnitude: a solve from a random x0 to 1e-13 cannot end in one)
    if not (d["solve_small_verifications"] >= 2 and d["solve_small_finite"]):
        bad.append("mixed_cube-uzawa-cold_paths: no solve with more than one pass: " + repr(d))
    d = c["blob-uzawa-capped"]["default"]
    if not d["solve_totals"][0] > d["solve_totals"][1]:
        bad.append("blob-uzawa-capped: no solve ended unconverged")
    d = c["blob-uzawa-solves"]["default"]
    if not (d["solve_small_iters"] > 0 and d["solve_small_finite"]):
        bad.append("blob-uzawa-solves: " + repr(d))
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
