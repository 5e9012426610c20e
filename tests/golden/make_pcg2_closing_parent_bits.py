"""Writes tests/golden/pcg2_closing_parent_bits.json: what whole steps computed BEFORE the closing phase of the on-chip PCG kernel
(csrc/pcg_onchip2.hpp: k_pcg2 -- the end projection on the soft modes and the stores of a solve's results) was rescheduled: the stores of the
recycled pair under the closing grid barrier.  SHA-256 digests of m_x and m_v after the last frame, the solve totals and the instance
counts.  tests/test_pcg2_closing_bits.py holds every later library to these bits.  Same method as make_solve_entry_parent_bits.py (whose
helpers are used), on the shapes at which a schedule of the closing phase can go wrong and which the earlier fixtures lack (they run soft
modes only as 8 modes at the plan's own block shape): 8, 24 and 32 modes (32 = kOc2DeflMax; counts that are no multiple of the wave count;
K^2 above the thread count) under every forced block shape and instance, the PCG solver, a tolerance that forces verification, restarts and
the classic form, a cap of three iterations (solves that end unconverged: no projection although modes are set), a stand-alone solve with
b = 0, and a cube dropped on a floor (UzawaCG's column lanes, which run without the projection).

Run ONCE, on the GPU, with the library of the commit the fixture is named after: in a checkout of that commit or with ADMM_HIP_LIB pointing
at a library built from it.

    python tests/golden/make_pcg2_closing_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it, and imports the case list and the runner from this file."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "pcg2_closing_parent_bits.json")
PARENT = "5dae79b"

_spec = importlib.util.spec_from_file_location("make_solve_entry_parent_bits", os.path.join(HERE, "make_solve_entry_parent_bits.py"))
entry = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(entry)
base = entry.base

FRAMES, ADMM_ITERS = entry.FRAMES, entry.ADMM_ITERS
SCENES = ("blob", "mixed_cube", "cube_on_floor")
ENV_KEYS = entry.ENV_KEYS
MODES = (8, 24, 32)
SPBS = (None, 1, 3, 12, 16)
CAP = 3      # pcg_max_iters of the capped cases


def _cfg(soft, linsolver=2, tol=1e-8, spb=None, max_iters=600, zero_solve=False):
    return dict(soft=soft, linsolver=linsolver, tol=tol, spb=spb, max_iters=max_iters, zero_solve=zero_solve)


# name -> (scene, configuration).  Wherever the hot instance serves a case, the test and the generator repeat it with ADMM_HIP_OC_GENERIC=1.
CASES = {}
for _sc in ("blob", "mixed_cube"):
    for _k in MODES:
        for _spb in SPBS:
            CASES["%s-uzawa-modes%d-spb_%s" % (_sc, _k, "plan" if _spb is None else _spb)] = (_sc, _cfg(_k, spb=_spb))
    CASES[_sc + "-pcg-modes24"] = (_sc, _cfg(24, linsolver=0))
    CASES[_sc + "-uzawa-modes24-cold_paths"] = (_sc, _cfg(24, tol=1e-13))
    CASES[_sc + "-uzawa-modes24-capped"] = (_sc, _cfg(24, max_iters=CAP))
    CASES[_sc + "-uzawa-modes24-zero_rhs"] = (_sc, _cfg(24, zero_solve=True))
CASES["cube_on_floor-uzawa-modes24"] = ("cube_on_floor", _cfg(24))

make_scene = entry.make_scene


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
        s = sc.make_solver(pcg_tol=cfg["tol"], pcg_max_iters=cfg["max_iters"], soft_modes=cfg["soft"], linsolver=cfg["linsolver"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for _ in range(FRAMES):
        s.step()
    x, v = s.m_x.copy(), s.m_v.copy()
    rec = dict(m_x=base.digest(x), m_v=base.digest(v))
    if cfg["zero_solve"]:      # one stand-alone solve with b = 0 from the state's positions, modes set
        y, it = s.global_solve(np.zeros_like(x), x)
        rec["zero_solve_x"] = base.digest(y); rec["zero_solve_iters"] = int(it)
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
    plain = {}      # the same run without modes (not part of the fixture): (scene, configuration less the modes) -> digest of m_x
    same_as_plain = []
    for cid, (name, cfg) in CASES.items():
        d, _, _ = run(scs[name], cfg, False)
        g = None
        if d["hot"] > 0:
            g, _, _ = run(scs[name], cfg, True)
            assert g["hot"] == 0, (cid, g)
        fx["cases"][cid] = dict(default=d, forced_generic=g)
        key = (name,) + tuple(sorted((k, v) for k, v in cfg.items() if k != "soft"))
        if key not in plain:
            plain[key] = run(scs[name], dict(cfg, soft=0), False)[0]["m_x"]
        if plain[key] == d["m_x"]:
            same_as_plain.append(cid)
        print(cid, d["solve_totals"], "hot %d generic %d lanes %d" % (d["hot"], d["generic"], d["lane_hot"] + d["lane_generic"]),
              "| forced generic:", g and g["m_x"] == d["m_x"], "| moved by the modes:", plain[key] != d["m_x"], flush=True)
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)
    # what the cases are about must have happened on the parent, or they test nothing
    c = fx["cases"]
    bad = []
    for cid, (name, cfg) in CASES.items():
        d = c[cid]["default"]
        if cfg["max_iters"] == CAP:      # (solves that end unconverged run WITHOUT the projection: these need not differ from the run without modes)
            if not d["solve_totals"][0] > d["solve_totals"][1]:
                bad.append(cid + ": no solve ended unconverged")
        elif cid in same_as_plain:
            bad.append(cid + ": the modes did not move the result")
        if cfg["spb"] != 1 and not d["hot"] >= FRAMES * ADMM_ITERS:      # (one wave per block: no two-level preconditioner, generic only)
            bad.append(cid + ": the hot instance did not serve the ADMM loop")
    d = c["cube_on_floor-uzawa-modes24"]["default"]
    if not d["lane_hot"] + d["lane_generic"] > 0:
        bad.append("cube_on_floor-uzawa-modes24: no column-lane launch")
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
