"""The schedule of the closing phase of the on-chip PCG kernel changed (csrc/pcg_onchip2.hpp: k_pcg2 -- after a converged solve with soft
modes the stores of the recycled pair are issued under the closing grid barrier of the end projection), and no sum, order of sums or
decision moved with it.  So every bit a step computes is what the commit before computed: tests/golden/pcg2_closing_parent_bits.json holds
that commit's digests (written once by tests/golden/make_pcg2_closing_parent_bits.py with that commit's library; nothing here writes it) on
the shapes at which such a schedule can go wrong and which the earlier fixtures do not run: 8, 24 and 32 soft modes under every forced block
shape and instance (one wave per block, where the polling wave also stores; mode counts that are no multiple of the wave count; K^2 above
the thread count), the PCG solver, a tolerance that forces verification and restarts, solves capped at three iterations (unconverged: no
projection although modes are set), a stand-alone solve with b = 0, and a cube on a floor (column lanes, which run without the projection)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pcg2_closing_parent_bits", os.path.join(_GOLDEN, "make_pcg2_closing_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

KEYS = ("m_x", "m_v", "zero_solve_x", "zero_solve_iters", "solve_totals", "hot", "generic", "lane_hot", "lane_generic")


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT and fx["frames"] == gen.FRAMES and fx["admm_iters"] == gen.ADMM_ITERS
    assert sorted(fx["cases"]) == sorted(gen.CASES)
    return fx


@pytest.fixture(scope="module")
def scene_of(parent_bits):
    scs = {}
    for name in gen.SCENES:
        scs[name] = gen.make_scene(name)
        assert gen.base.scene_digest(scs[name]) == parent_bits["scenes"][name], "the mesh of %r is not the one the fixture was recorded on" % name
    return scs


def _check(rec, want, what):
    print(what, "totals", rec["solve_totals"], "fixture", want["solve_totals"], "hot %d generic %d lanes %d" % (rec["hot"], rec["generic"], rec["lane_hot"] + rec["lane_generic"]))
    assert sorted(rec) == sorted(want), (what, sorted(rec), sorted(want))
    for k in KEYS:
        if k in want:
            assert rec[k] == want[k], "%s: %s differs from the parent commit's: %r, fixture %r" % (what, k, rec[k], want[k])


@pytest.mark.parametrize("cid", list(gen.CASES))
def test_same_bits_as_the_parent_commit(cid, parent_bits, scene_of):
    name, cfg = gen.CASES[cid]
    want = parent_bits["cases"][cid]
    d, x, v = gen.run(scene_of[name], cfg, False)
    assert d["solve_totals"][0] > 0 and d["solve_totals"][2] > 0 and np.isfinite(x).all()
    _check(d, want["default"], cid)
    if want["forced_generic"] is not None:      # the hot instance is eligible (and ran: its count was compared above)
        g, xg, vg = gen.run(scene_of[name], cfg, True)
        assert g["hot"] == 0
        _check(g, want["forced_generic"], cid + " forced generic")
        assert np.array_equal(x, xg) and np.array_equal(v, vg)
