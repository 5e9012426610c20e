"""Writes tests/golden/solve_entry_parent_bits.json: what whole steps computed BEFORE the gather of the right-hand side (csrc/kernels.hpp:
k_gather_rhs) got its record lists in flight, the state any later change to the load schedule of the solve entry of the on-chip PCG kernel
(csrc/pcg_onchip2.hpp: k_pcg2) has to keep as well -- SHA-256 digests of m_x and m_v after the last frame, the solve totals and the instance
counts.  tests/test_solve_entry_bits.py holds every later library to these bits.  Same method
as make_pcg2_parent_bits.py (whose helpers are used), on the configurations that fixture lacks: UzawaCG without obstacles (the bench's
path) under every forced block shape and instance, less LDS (the streamed tail of the slab, short on-chip parts), soft modes, a tolerance
that forces verification and restarts, the early exit of the ADMM loop on the device (skip word), a stand-alone solve with b = 0, and a
cube dropped on a floor (UzawaCG's column lanes).

Run ONCE, on the GPU, with the library of the commit the fixture is named after: in a checkout of that commit or with ADMM_HIP_LIB pointing
at a library built from it.

    python tests/golden/make_solve_entry_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it, and imports the case list and the runner from this file."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "solve_entry_parent_bits.json")
PARENT = "8584119"

_spec = importlib.util.spec_from_file_location("make_pcg2_parent_bits", os.path.join(HERE, "make_pcg2_parent_bits.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

FRAMES, ADMM_ITERS = 3, 5
SCENES = ("blob", "mixed_cube", "cube_on_floor")
ENV_KEYS = ("ADMM_HIP_OC_SPB", "ADMM_HIP_OC_GENERIC", "ADMM_HIP_OC_LDS_KB")


def _cfg(linsolver=2, tol=1e-8, soft=0, spb=None, lds_kb=None, stop=0.0, zero_solve=False):
    return dict(linsolver=linsolver, tol=tol, soft=soft, spb=spb, lds_kb=lds_kb, stop=stop, zero_solve=zero_solve)


# name -> (scene, configuration).  Wherever the hot instance serves a case, the test and the generator repeat it with ADMM_HIP_OC_GENERIC=1.
CASES = {}
for _sc in ("blob", "mixed_cube"):
    CASES[_sc + "-uzawa"] = (_sc, _cfg())
    for _kb in (32, 48):
        CASES["%s-uzawa-lds_%d" % (_sc, _kb)] = (_sc, _cfg(lds_kb=_kb))
        CASES["%s-pcg-lds_%d" % (_sc, _kb)] = (_sc, _cfg(linsolver=0, lds_kb=_kb))
    for _spb in (1, 3, 12, 16):
        CASES["%s-uzawa-spb_%d" % (_sc, _spb)] = (_sc, _cfg(spb=_spb))
    CASES[_sc + "-uzawa-modes8"] = (_sc, _cfg(soft=8))
    CASES[_sc + "-uzawa-cold_paths"] = (_sc, _cfg(tol=1e-13))
    CASES[_sc + "-uzawa-lds_32-cold_paths"] = (_sc, _cfg(tol=1e-13, lds_kb=32))
    CASES[_sc + "-pcg-admm_stop"] = (_sc, _cfg(linsolver=0, stop=1e-2))
    CASES[_sc + "-uzawa-zero_rhs"] = (_sc, _cfg(zero_solve=True))
CASES["cube_on_floor-uzawa"] = ("cube_on_floor", _cfg())
CASES["cube_on_floor-uzawa-lds_32"] = ("cube_on_floor", _cfg(lds_kb=32))


def make_scene(name):
    import numpy as np
    import scenes
    import admm_elastic_amd as pkg
    if name == "cube_on_floor":      # a free cube whose lowest layer is under the floor from the first frame on: obstacle rows, column lanes
        sc = scenes.cube_scene(6, pkg.TET_NEOHOOKEAN, pin_face=False, admm_iters=ADMM_ITERS)
        sc.obstacles.append((0, [0.05, 0.0, 0.0, 0.0]))
        return sc
    sc = base.make_scene(name)
    assert sc.settings["admm_iters"] == ADMM_ITERS and np.isfinite(sc.x).all()
    return sc


def run(sc, cfg, generic):
    """FRAMES frames of `sc` under `cfg`; returns (record for the fixture, m_x, m_v).  The switches are read once, when the context is created."""
    import numpy as np
    env = {}
    if cfg["spb"] is not None:
        env["ADMM_HIP_OC_SPB"] = str(cfg["spb"])
    if cfg["lds_kb"] is not None:
        env["ADMM_HIP_OC_LDS_KB"] = str(cfg["lds_kb"])
    if generic:
        env["ADMM_HIP_OC_GENERIC"] = "1"
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        s = sc.make_solver(pcg_tol=cfg["tol"], pcg_max_iters=600, soft_modes=cfg["soft"], linsolver=cfg["linsolver"], admm_tol=cfg["stop"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    executed = []
    for _ in range(FRAMES):
        s.step()
        executed.append(int(s.admm_stop()["last_iters"]) if cfg["stop"] else ADMM_ITERS)
    x, v = s.m_x.copy(), s.m_v.copy()
    rec = dict(m_x=base.digest(x), m_v=base.digest(v), admm_iters=executed)
    if cfg["stop"]:
        rec["stop_on_device"] = int(s.admm_stop()["on_device"])
    if cfg["zero_solve"]:      # one stand-alone solve with b = 0 from the state's positions: the entry residual is the whole work
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
    for cid, (name, cfg) in CASES.items():
        d, _, _ = run(scs[name], cfg, False)
        g = None
        if d["hot"] > 0:
            g, _, _ = run(scs[name], cfg, True)
            assert g["hot"] == 0, (cid, g)
        fx["cases"][cid] = dict(default=d, forced_generic=g)
        print(cid, d["solve_totals"], "hot %d generic %d lanes %d" % (d["hot"], d["generic"], d["lane_hot"] + d["lane_generic"]), "iters", d["admm_iters"],
              "| forced generic:", g and g["m_x"] == d["m_x"], flush=True)
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)
    # what the cases are about must have happened on the parent, or they test nothing
    c = fx["cases"]
    assert c["cube_on_floor-uzawa"]["default"]["lane_hot"] + c["cube_on_floor-uzawa"]["default"]["lane_generic"] > 0, "no column-lane launch"
    for sc in ("blob", "mixed_cube"):
        assert c[sc + "-uzawa"]["default"]["hot"] >= FRAMES * ADMM_ITERS, "UzawaCG without obstacles did not take the hot instance"
        assert c[sc + "-pcg-admm_stop"]["default"]["stop_on_device"] == 1 and min(c[sc + "-pcg-admm_stop"]["default"]["admm_iters"]) < ADMM_ITERS, \
            "the ADMM loop never stopped early on the device: " + repr(c[sc + "-pcg-admm_stop"]["default"])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
