"""Writes tests/golden/pcg2_parent_bits.json: what the on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2) computed BEFORE the block-local
reductions of its iteration were shortened -- SHA-256 digests of m_x and m_v after the last frame, the solve totals and the instance counts,
per scene, solver setting, forced block shape (ADMM_HIP_OC_SPB) and instance (ADMM_HIP_OC_GENERIC=1).  tests/test_pcg2_block_sums.py holds
every later library to these bits.

Run ONCE, on the GPU, with the library of the commit the fixture is named after (commit 1563b43, "k_pcg2: single-exit iteration loop, hot
instance for the ADMM loop"): either in a checkout of that commit or with ADMM_HIP_LIB pointing at a library built from it.

    python tests/golden/make_pcg2_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it.  The case list and the runner live here so that the fixture and the
test cannot drift apart; the test imports them from this file."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "pcg2_parent_bits.json")
PARENT = "1563b43"

FRAMES, ADMM_ITERS = 3, 5
SCENES = ("blob", "mixed_cube")
# (pcg_tol, soft_modes): the trusted short first pass; the same with the end projection on the soft modes; a tolerance below what a pass is
# trusted for -- verification, restart from the true residual, further passes and the classic form
SETTINGS = {"short_pass": (1e-8, 0), "modes8": (1e-8, 8), "cold_paths": (1e-13, 0)}
# waves per block: the plan's own choice; 1 (no two-level preconditioner: 4 G coarse unknowns > 2 T, generic instance only); an odd count; the
# full 768-thread block of the bench body; the 1024-thread instance
SPBS = (None, 1, 3, 12, 16)
CASES = [(sc, st, spb) for sc in SCENES for st in SETTINGS for spb in SPBS]


def case_id(case):
    sc, st, spb = case
    return "%s-%s-spb_%s" % (sc, st, "plan" if spb is None else spb)


def make_scene(name):
    import scenes
    if name == "blob":
        return scenes.blob_scene(30, admm_iters=ADMM_ITERS, linsolver=0)      # 16 k tets, unstructured: several blocks with halos
    return scenes.mixed_cube_scene(12, admm_iters=ADMM_ITERS, linsolver=0)


def digest(arr):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def scene_digest(sc):
    """The mesh the solver is given: positions and tets.  Says when the mesh generator, not the kernel, has moved."""
    import numpy as np
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(sc.x, dtype=np.float64).tobytes())
    for verts, tets, lame, kind, off in sc.tets:
        h.update(np.ascontiguousarray(tets, dtype=np.int64).tobytes())
        h.update(("|%d|%d|" % (int(kind), int(off))).encode())
    return h.hexdigest()


def run(sc, setting, spb, generic):
    """Three frames of `sc`; returns (record for the fixture, m_x, m_v).  The switches are read once, when the context is created."""
    tol, soft = SETTINGS[setting]
    env = {}
    if spb is not None:
        env["ADMM_HIP_OC_SPB"] = str(spb)
    if generic:
        env["ADMM_HIP_OC_GENERIC"] = "1"
    old = {k: os.environ.get(k) for k in ("ADMM_HIP_OC_SPB", "ADMM_HIP_OC_GENERIC")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        s = sc.make_solver(pcg_tol=tol, pcg_max_iters=600, soft_modes=soft)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for _ in range(FRAMES):
        s.step()
    x, v = s.m_x.copy(), s.m_v.copy()
    inst = s.pcg_instances()
    rec = dict(m_x=digest(x), m_v=digest(v), solve_totals=list(s.solve_totals()), hot=int(inst["hot"]), generic=int(inst["generic"]))
    s.close()
    return rec, x, v


def main(out):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    sys.path.insert(0, os.path.join(HERE, ".."))
    scs = {name: make_scene(name) for name in SCENES}
    fx = dict(parent=PARENT, frames=FRAMES, admm_iters=ADMM_ITERS, scenes={n: scene_digest(s) for n, s in scs.items()}, cases={})
    for case in CASES:
        name, setting, spb = case
        d, _, _ = run(scs[name], setting, spb, False)
        g = None
        if d["hot"] > 0:      # the hot instance is eligible: the same configuration on the forced generic instance
            g, _, _ = run(scs[name], setting, spb, True)
            assert g["hot"] == 0, (case, g)
        fx["cases"][case_id(case)] = dict(default=d, forced_generic=g)
        print(case_id(case), d["solve_totals"], "hot %d generic %d" % (d["hot"], d["generic"]), "| forced generic:", g and g["m_x"] == d["m_x"], flush=True)
    # a forced block shape the plan refused would silently repeat the plan's own: the shapes must differ in their iteration counts
    for name in SCENES:
        tot = {spb: tuple(fx["cases"][case_id((name, "short_pass", spb))]["default"]["solve_totals"]) for spb in SPBS}
        assert len(set(tot.values())) >= 4, (name, tot)
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
