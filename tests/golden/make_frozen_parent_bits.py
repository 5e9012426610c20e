"""Writes tests/golden/frozen_parent_bits.json: what the frozen tangent (csrc/newton.hpp: stiffness_apply_ex, tangent_solve, newton_polish)
computed BEFORE its way out of the kernels -- the chunk epilogue, the hinge scatter, the head of the vertex gather, the pin rule -- moved
into csrc/elements.hpp beside that of forces.hpp and tangent.hpp: SHA-256 digests of every output, per scene, Binv mode and state.
tests/test_frozen_tangent_bits.py holds every later library to these bits; element_parent_bits.json, the sibling this is modelled on,
predates newton.hpp.

Run ONCE, on the GPU, with the library of the commit the fixture is named after (commit 5fe8266, "Anderson acceleration of the ADMM loop on
the device (off by default)"): either in a checkout of that commit or with ADMM_HIP_LIB pointing at a library built from it.

    python tests/golden/make_frozen_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it and imports the case list and the runners from this file.  The
scenes, the states and the digests are those of make_element_parent_bits.py."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "frozen_parent_bits.json")
PARENT = "5fe8266"

_spec = importlib.util.spec_from_file_location("make_element_parent_bits", os.path.join(HERE, "make_element_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# the smallest shapes at which these kernels can go wrong: one tet (255 lanes redo it); 6 tets (a partial wave); 162 (records cut after 8
# corners); 750 of three kinds (several chunks, model boundaries); the TABLE instance of k_tangent_setup; triangles and hinges without tets
SCENES = ("one_tet", "nh1", "nh3", "mixed5", "kind6", "cloth6")
# default Binv mode everywhere, and nh3 streamed (ADMM_HIP_TET_REST=0)
CASES = [(sc, None, pushed) for sc in SCENES for pushed in (False, True)] + [("nh3", "0", pushed) for pushed in (False, True)]
SOLVE = dict(psd=True, hold_pins=True, tol=1e-10, max_iters=40)      # 40 > one chunk of 8 iterations: the chunk-ahead stop runs
# whole steps: one frame, then the polish.  The step scenes of the sibling: no collider, no strain limit, no slide pin (run_polish asserts it)
STEP_SCENES = gen.STEP_SCENES
POLISH = dict(max_iters=3, grad_tol=0.0, cg_tol=1e-8, cg_max=60)

case_id = gen.case_id


def make_solver(name, rest):
    """gen.make_solver; a scene without a pin gets one on vertex 0 before its context is created, so that hold_pins does something"""
    s, verts, n = gen.make_solver(name, rest)
    if not s._pins:
        s.close()
        s.initialized = False      # (set_pins then only records the pin; initialize creates the context with it)
        s.set_pins([0], [verts[0]])
        assert gen._with_rest_env(rest, lambda: s.initialize(s.settings()))
    return s, verts, n


def run(case):
    """stiffness_apply_ex and tangent_solve of one scene, Binv mode and state -> (record of digests, scene digest)"""
    import numpy as np
    name, rest, pushed = case
    s, verts, n = make_solver(name, rest)
    if name != "cloth6":
        assert (s.tet_rest_mode() != 0) == (rest is None), (case, s.tet_rest_mode())
    assert s._pins
    x = gen.state(name, verts, n, pushed)
    rng = np.random.default_rng(23)
    D = rng.standard_normal((2,) + x.shape)
    rhs = rng.standard_normal(x.shape)
    idt2 = 1.0 / s.settings().timestep_s ** 2
    rec = {}
    for psd in (False, True):
        for hold in (False, True):
            for tag, shift in (("0", 0.0), ("idt2", idt2)):
                key = "apply_psd%d_hold%d_shift_%s_" % (psd, hold, tag)
                rec[key + "1"] = gen.digest(s.stiffness_apply_ex(D[0], x, shift=shift, psd=psd, hold_pins=hold))
                rec[key + "2"] = gen.digest(s.stiffness_apply_ex(D, x, shift=shift, psd=psd, hold_pins=hold))
    y, info = s.tangent_solve(rhs, x, **SOLVE)
    rec["solve_y"] = gen.digest(y)
    rec["solve_info"] = gen.digest([info["iterations"], info["converged"], info["residual"], info["rhs_norm"]])
    sd = gen.scene_digest(s, verts)
    s.close()
    return rec, sd


def run_polish(name):
    """one frame of gen.STEP_ITERS iterations, then newton_polish -> the digests of its records, m_x, m_v"""
    sc = gen.step_scene(name)
    assert not sc.obstacles and not sc.dynamic and not sc.slides and all(t[2].limit_min <= 0.0 and t[2].limit_max >= 100.0 for t in sc.tris)
    s = sc.make_solver(**gen.PCG)
    s.step()
    recs = s.newton_polish(**POLISH)
    assert len(recs) >= 2, "the polish took no Newton step"
    keys = ("objective", "grad_norm", "cg_iterations", "step", "energy")
    out = dict(records=gen.digest([[r[k] for k in keys] for r in recs]), n=len(recs), m_x=gen.digest(s.m_x), m_v=gen.digest(s.m_v))
    s.close()
    return out


def main(out):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    sys.path.insert(0, os.path.join(HERE, ".."))
    fx = dict(parent=PARENT, scenes={}, cases={}, polish={})
    for case in CASES:
        rec, sd = run(case)
        assert fx["scenes"].setdefault(case[0], sd) == sd, case
        fx["cases"][case_id(case)] = rec
        print(case_id(case), rec["apply_psd1_hold1_shift_idt2_2"][:12], rec["solve_y"][:12], flush=True)
    # held rows and the projection must change something somewhere, or a flag is dead
    c0 = fx["cases"][case_id(("mixed5", None, True))]
    assert c0["apply_psd0_hold0_shift_0_1"] != c0["apply_psd0_hold1_shift_0_1"] and c0["apply_psd0_hold0_shift_0_1"] != c0["apply_psd1_hold0_shift_0_1"]
    for name in STEP_SCENES:
        fx["polish"][name] = run_polish(name)
        print("polish", name, fx["polish"][name]["n"], fx["polish"][name]["m_x"][:12], flush=True)
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
