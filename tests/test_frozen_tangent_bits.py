"""The way out of the kernels of the frozen tangent (csrc/newton.hpp) -- the chunk epilogue, the edge matrix of a direction, the hinge
scatter, the head of the vertex gather, the pin rule -- moved into the one layer forces.hpp and tangent.hpp use (csrc/elements.hpp) WITHOUT
touching the arithmetic or its order.  So every bit stiffness_apply_ex, tangent_solve and newton_polish compute is what the commit before
computed: tests/golden/frozen_parent_bits.json holds that commit's digests (written once by tests/golden/make_frozen_parent_bits.py with
that commit's library; nothing here writes it), and each case below must reproduce them.  tests/test_element_layer_bits.py does the same
for energy, forces, stress and stiffness_apply.

A digest that differs says that some helper changed the shape of an expression: restore the shape.  The fixture is never regenerated from
the code under test."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_frozen_parent_bits", os.path.join(_GOLDEN, "make_frozen_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT
    assert sorted(fx["cases"]) == sorted(gen.case_id(c) for c in gen.CASES)
    assert sorted(fx["scenes"]) == sorted(gen.SCENES) and sorted(fx["polish"]) == sorted(gen.STEP_SCENES)
    return fx


@pytest.mark.parametrize("case", gen.CASES, ids=gen.case_id)
def test_frozen_tangent_has_the_parent_commits_bits(case, parent_bits):
    """stiffness_apply_ex for the four combinations of psd / hold_pins, shift 0 and 1 / dt^2, one and two directions, and a tangent_solve of
    up to 40 iterations (y and the four info values) of one scene, Binv mode and state"""
    rec, sd = gen.run(case)
    assert sd == parent_bits["scenes"][case[0]], "the mesh of %r is not the one the fixture was recorded on" % case[0]
    want = parent_bits["cases"][gen.case_id(case)]
    bad = [k for k in want if rec.get(k) != want[k]]
    assert sorted(rec) == sorted(want) and not bad, "%s: %s differ(s) from the parent commit's bits" % (gen.case_id(case), ", ".join(bad) or "the keys")


@pytest.mark.parametrize("name", gen.STEP_SCENES)
def test_newton_polish_has_the_parent_commits_bits(name, parent_bits):
    """one frame of 12 iterations, then newton_polish(max_iters=3, grad_tol=0, cg_tol=1e-8, cg_max=60): the records, m_x, m_v"""
    assert gen.run_polish(name) == parent_bits["polish"][name], "%s: the polish differs from the parent commit's bits" % name
