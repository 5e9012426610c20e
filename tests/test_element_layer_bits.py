"""The per-element code under the three device passes over all energy terms -- energy and residuals (csrc/monitor.hpp), forces and stress
(csrc/forces.hpp), K(x) d (csrc/tangent.hpp) -- moved into one layer (csrc/elements.hpp, device_math.hpp: tet_energy_grad) WITHOUT touching
the arithmetic or its order.  So every bit these passes compute is what the commit before computed: tests/golden/element_parent_bits.json
holds that commit's digests (written once by tests/golden/make_element_parent_bits.py with that commit's library; nothing here writes it),
and each case below must reproduce them.

The cases are the project's smallest shapes -- one tet (255 lanes redo it), 6 tets (a partial wave), 162 (records cut after 8 corner
forces), 750 of three kinds (model boundaries, several chunks), the 162-tet cube of the five dense-Hessian kinds, a cloth with hinges -- each
at a plain and a pushed (inverted) state, the tet scenes with Binv recomputed from the rest positions and streamed (ADMM_HIP_TET_REST=0);
two frames with monitor = 3; and a step whose ADMM loop ends early on the device (the STOP instances and k_mon_decide).

A digest that differs says that some helper changed the shape of an expression (an fma contracted across a statement the old text kept
apart, a sum in another order): restore the shape.  The fixture is never regenerated from the code under test."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_element_parent_bits", os.path.join(_GOLDEN, "make_element_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT
    assert sorted(fx["cases"]) == sorted(gen.case_id(c) for c in gen.CASES)
    assert sorted(fx["scenes"]) == sorted(gen.SCENES) and sorted(fx["steps"]) == sorted(gen.STEP_SCENES)
    return fx


def _same(got, want, what):
    bad = [k for k in want if got.get(k) != want[k]]
    assert sorted(got) == sorted(want) and not bad, "%s: %s differ(s) from the parent commit's bits" % (what, ", ".join(bad) or "the keys")


@pytest.mark.parametrize("case", gen.CASES, ids=gen.case_id)
def test_same_bits_as_the_parent_commit(case, parent_bits):
    """energy (totals and per term), forces, stress, stiffness_apply (1 and 3 directions, shift 0 and 1 / dt^2) and residuals (seeded rows,
    the 6-row pin layout) of one scene, Binv mode and state; gen.run asserts tet_rest_mode() so that both Binv branches really run"""
    rec, sd = gen.run(case)
    assert sd == parent_bits["scenes"][case[0]], "the mesh of %r is not the one the fixture was recorded on" % case[0]
    _same(rec, parent_bits["cases"][gen.case_id(case)], gen.case_id(case))


@pytest.mark.parametrize("name", gen.STEP_SCENES)
def test_steps_with_monitor_3_have_the_parent_commits_bits(name, parent_bits):
    """two frames with monitor = 3 (k_monitor<RES, ENERGY>, k_mon_final, k_forces behind the stationarity): admm_history(), m_x, m_v"""
    got, want = gen.run_step(name), parent_bits["steps"][name]
    assert len(got) == len(want) == gen.STEP_FRAMES
    for f, (g, w) in enumerate(zip(got, want)):
        _same(g["history"], w["history"], "%s frame %d history" % (name, f))
        assert (g["m_x"], g["m_v"]) == (w["m_x"], w["m_v"]), "%s frame %d: the state differs from the parent commit's bits" % (name, f)


def test_early_exit_on_the_device_has_the_parent_commits_bits(parent_bits):
    """mixed4 with set_admm_stop at the fixture's tolerance: the loop ends before admm_iters, the rest skipped on the device (the STOP
    instances of k_monitor, k_mon_decide): the executed counts, the history and the final state"""
    want = parent_bits["stop"]
    assert want["tol"] in gen.STOP_TOLS and 2 <= want["frames"][0]["last_iters"] < gen.STEP_ITERS and want["frames"][0]["on_device"] == 1
    got = gen.run_stop(want["tol"])
    assert len(got) == len(want["frames"]) == gen.STEP_FRAMES + 1
    for f, (g, w) in enumerate(zip(got[:-1], want["frames"][:-1])):
        assert (g["last_iters"], g["on_device"]) == (w["last_iters"], w["on_device"]), (f, g, w)
        _same(g["history"], w["history"], "early exit frame %d history" % f)
    assert got[-1] == want["frames"][-1], "the state after the early-exit frames differs from the parent commit's bits"
