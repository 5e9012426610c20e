"""Writes tests/golden/element_parent_bits.json: what the three device passes over all energy terms -- csrc/monitor.hpp (energy, residuals,
the stop decision), csrc/forces.hpp (forces, stress, stationarity) and csrc/tangent.hpp (K(x) d) -- computed BEFORE their per-element code
moved into csrc/elements.hpp: SHA-256 digests of every output, per scene, Binv mode and state.  tests/test_element_layer_bits.py holds every
later library to these bits.

Run ONCE, on the GPU, with the library of the commit the fixture is named after (commit 9537517, "Add stiffness_apply(): the exact tangent
stiffness K(x) d on the device"): either in a checkout of that commit or with ADMM_HIP_LIB pointing at a library built from it.

    python tests/golden/make_element_parent_bits.py [OUT.json]

The code under test never writes the fixture: the test only reads it.  The case list and the runners live here so that the fixture and the
test cannot drift apart; the test imports them from this file."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "element_parent_bits.json")
PARENT = "9537517"

# the project's smallest shapes: one tet (255 lanes redo it); 6 tets (a partial wave); 162 (records cut after 8 corner forces); 750 of three
# kinds (model boundaries, several chunks); the 162-tet cube of every dense-Hessian kind; triangles with hinges
TET_SCENES = ("one_tet", "nh1", "nh3", "mixed5", "kind3", "kind4", "kind5", "kind6", "kind7")
SCENES = TET_SCENES + ("cloth6",)
# ADMM_HIP_TET_REST when the context is created: unset = Binv recomputed from the rest positions, "0" = streamed
CASES = [(sc, rest, pushed) for sc in TET_SCENES for rest in (None, "0") for pushed in (False, True)] + [("cloth6", None, p) for p in (False, True)]
# whole steps: two frames with monitor = 3 (RES + ENERGY, stationarity), and one scene whose ADMM loop stops early on the device (the STOP
# instances and k_mon_decide)
STEP_SCENES = ("mixed4", "cloth6_nolimits")
STEP_FRAMES, STEP_ITERS = 2, 12
STOP_TOLS = (1e-3, 1e-4, 1e-5, 1e-6, 1e-7)      # the generator keeps the first that ends frame 0 after 2 .. 11 of the 12 iterations
PCG = dict(pcg_tol=1e-12, pcg_max_iters=500)


def case_id(case):
    sc, rest, pushed = case
    return "%s-%s-%s" % (sc, "rest" if rest is None else "streamed", "pushed" if pushed else "plain")


def _kind(name):
    import admm_elastic_amd as pkg
    return {"kind3": pkg.TET_SPLINE_NH, "kind4": pkg.TET_SPLINE_STVK, "kind5": pkg.TET_SPLINE_COROTATED, "kind6": pkg.TET_SPLINE_TABLE,
            "kind7": pkg.TET_STABLE_NH}[name]


def _with_rest_env(rest, make):
    old = os.environ.pop("ADMM_HIP_TET_REST", None)
    if rest is not None:
        os.environ["ADMM_HIP_TET_REST"] = rest
    try:
        return make()
    finally:
        os.environ.pop("ADMM_HIP_TET_REST", None)
        if old is not None:
            os.environ["ADMM_HIP_TET_REST"] = old


def make_solver(name, rest):
    """-> (solver, rest positions, n of plain_state / pushed_state).  The switch is read once, when the context is created."""
    from test_energy_monitor import cloth_with_hinges, kind_solver
    from test_forces import SPLINE_KINDS, _tet_scene
    if name.startswith("kind"):
        assert _kind(name) in SPLINE_KINDS
        s, verts = _with_rest_env(rest, lambda: kind_solver(3, _kind(name)))
        return s, verts, 3
    if name == "cloth6":
        sc = cloth_with_hinges(6)
        return sc.make_solver(), sc.x, 6
    sc, n = _tet_scene(name)
    return _with_rest_env(rest, sc.make_solver), sc.x, n


def state(name, verts, n, pushed):
    from test_energy_monitor import plain_state, pushed_state
    from test_forces import _one_tet_state
    return _one_tet_state(verts, pushed) if name == "one_tet" else (pushed_state if pushed else plain_state)(verts, n)


def digest(*arrs):
    import numpy as np
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def scene_digest(s, verts):
    """What the solver was given, flattened: rest positions and the connectivity of every family."""
    import numpy as np
    f = s.flatten()
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(verts, dtype=np.float64).tobytes())
    for key in ("tet_idx", "tri_idx", "bend_idx"):
        h.update(np.ascontiguousarray(f[key], dtype=np.int64).tobytes())
    return h.hexdigest()


def run(case):
    """Every element-level output of one scene, Binv mode and state -> (record of digests, scene digest)"""
    import numpy as np
    name, rest, pushed = case
    s, verts, n = make_solver(name, rest)
    if name != "cloth6":
        assert (s.tet_rest_mode() != 0) == (rest is None), (case, s.tet_rest_mode())      # both Binv branches really run
    x = state(name, verts, n, pushed)
    rng = np.random.default_rng(23)
    D = rng.standard_normal((3,) + x.shape)
    R = s.num_rows()
    z, zp = rng.standard_normal(R), rng.standard_normal(R)
    idt2 = 1.0 / s.settings().timestep_s ** 2
    e = s.energy(x, per_term=True)
    st = s.stress(x)
    rec = dict(energy_totals=digest([e["tets"], e["tris"], e["hinges"], e["total"]]), energy_terms=digest(e["terms"]),
               forces=digest(s.forces(x)), stress=digest(st["P"], st["stretches"], st["von_mises"]),
               residuals=digest(s.residuals(x, z, zp)))
    for tag, shift in (("0", 0.0), ("idt2", idt2)):
        rec["stiffness_1_shift_" + tag] = digest(s.stiffness_apply(D[0], x, shift=shift))
        rec["stiffness_3_shift_" + tag] = digest(s.stiffness_apply(D, x, shift=shift))
    sd = scene_digest(s, verts)
    s.close()
    return rec, sd


def step_scene(name):
    import scenes
    if name == "mixed4":
        return scenes.mixed_cube_scene(4, admm_iters=STEP_ITERS)
    return scenes.cloth_scene(6, limits=None, admm_iters=STEP_ITERS)


def _history_digests(s):
    h = s.admm_history()
    return {k: digest(h[k]) for k in sorted(h)}, len(h["primal"])


def run_step(name):
    """STEP_FRAMES frames with monitor = 3 -> per frame the digests of admm_history(), m_x, m_v"""
    s = step_scene(name).make_solver(monitor=3, **PCG)
    out = []
    for _ in range(STEP_FRAMES):
        s.step()
        hist, n = _history_digests(s)
        assert n == STEP_ITERS
        out.append(dict(history=hist, m_x=digest(s.m_x), m_v=digest(s.m_v)))
    s.close()
    return out


def run_stop(tol):
    """STEP_FRAMES stream-ordered frames of mixed4 whose ADMM loop ends on its residuals at `tol`, the rest skipped on the device"""
    s = step_scene("mixed4").make_solver(admm_tol=tol, **PCG)
    s.upload()
    out = []
    for _ in range(STEP_FRAMES):
        s.step_device(stats=True)
        st = s.admm_stop()
        hist, n = _history_digests(s)
        assert n == st["last_iters"]
        out.append(dict(history=hist, last_iters=int(st["last_iters"]), on_device=int(st["on_device"])))
    s.download()
    out.append(dict(m_x=digest(s.m_x), m_v=digest(s.m_v)))
    s.close()
    return out


def main(out):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    sys.path.insert(0, os.path.join(HERE, ".."))
    fx = dict(parent=PARENT, scenes={}, cases={}, steps={}, stop=None)
    for case in CASES:
        rec, sd = run(case)
        assert fx["scenes"].setdefault(case[0], sd) == sd, case
        fx["cases"][case_id(case)] = rec
        print(case_id(case), rec["forces"][:12], rec["stiffness_3_shift_idt2"][:12], flush=True)
    # the two Binv modes must differ somewhere (fast_rcp of the recomputed determinant against the host's division), or the switch is dead
    assert any(fx["cases"][case_id((sc, None, False))]["forces"] != fx["cases"][case_id((sc, "0", False))]["forces"] for sc in TET_SCENES)
    for name in STEP_SCENES:
        fx["steps"][name] = run_step(name)
        print("step", name, fx["steps"][name][-1]["m_x"][:12], flush=True)
    for tol in STOP_TOLS:
        frames = run_stop(tol)
        print("stop tol %g: executed %s on_device %s" % (tol, [f["last_iters"] for f in frames[:-1]], [f["on_device"] for f in frames[:-1]]), flush=True)
        if 2 <= frames[0]["last_iters"] < STEP_ITERS and frames[0]["on_device"] == 1:
            fx["stop"] = dict(tol=tol, frames=frames)
            break
    assert fx["stop"] is not None, "no tolerance of STOP_TOLS ends frame 0 early on the device"
    with open(out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
