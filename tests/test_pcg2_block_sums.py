"""The block-local reductions of the on-chip PCG kernel (csrc/pcg_onchip2.hpp: cross_wave_total, block_sums_gen, reduce_and_coarse) were
shortened -- the cross-wave totals read their wave partials in one go, the record sums and the coarse rows share a block barrier, the totals
stay in registers -- WITHOUT touching the arithmetic or its order.  So every bit the kernel computes is what the commit before computed:
tests/golden/pcg2_parent_bits.json holds that commit's digests (written once by tests/golden/make_pcg2_parent_bits.py with that commit's
library; nothing here writes it), and each case below must reproduce them.

The changed code depends on the waves per block and on which instance runs, so the cases force both: ADMM_HIP_OC_SPB (1: no two-level
preconditioner, generic instance only; 3: an odd count; 12: the 768-thread block of the bench body; 16: the 1024-thread instance; unset: the
plan's own choice) and, wherever the hot instance is eligible, ADMM_HIP_OC_GENERIC=1 next to it.  No forced shape is refused by the plan
on these two scenes (the generator checks that the shapes differ in their iteration counts), so the list is the full product."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pcg2_parent_bits", os.path.join(_GOLDEN, "make_pcg2_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT and fx["frames"] == gen.FRAMES and fx["admm_iters"] == gen.ADMM_ITERS
    assert sorted(fx["cases"]) == sorted(gen.case_id(c) for c in gen.CASES)
    return fx


@pytest.fixture(scope="module")
def scene_of(parent_bits):
    """The two scenes, built once; their digest says clearly when the mesh generator, not the kernel, has moved."""
    scs = {}
    for name in gen.SCENES:
        scs[name] = gen.make_scene(name)
        assert gen.scene_digest(scs[name]) == parent_bits["scenes"][name], "the mesh of %r is not the one the fixture was recorded on" % name
    return scs


def _check(rec, want, what):
    print(what, "totals", rec["solve_totals"], "fixture", want["solve_totals"], "hot %d generic %d" % (rec["hot"], rec["generic"]))
    assert (rec["hot"], rec["generic"]) == (want["hot"], want["generic"]), (what, rec, want)      # the same instance served the same launches
    assert rec["solve_totals"] == want["solve_totals"], (what, rec["solve_totals"], want["solve_totals"])
    assert rec["m_x"] == want["m_x"], what + ": m_x differs from the parent commit's bits"
    assert rec["m_v"] == want["m_v"], what + ": m_v differs from the parent commit's bits"


@pytest.mark.parametrize("case", gen.CASES, ids=gen.case_id)
def test_same_bits_as_the_parent_commit(case, parent_bits, scene_of):
    name, setting, spb = case
    want = parent_bits["cases"][gen.case_id(case)]
    d, x, v = gen.run(scene_of[name], setting, spb, False)
    assert d["solve_totals"][0] >= gen.FRAMES * gen.ADMM_ITERS and d["solve_totals"][2] > 0 and np.isfinite(x).all()
    _check(d, want["default"], gen.case_id(case))
    if spb == 1:
        assert d["hot"] == 0      # 4 G coarse unknowns > 2 T: no two-level preconditioner, so never the hot instance
    if want["forced_generic"] is not None:      # the hot instance is eligible (and ran: its count was compared above)
        assert d["hot"] >= gen.FRAMES * gen.ADMM_ITERS
        g, xg, vg = gen.run(scene_of[name], setting, spb, True)
        assert g["hot"] == 0
        _check(g, want["forced_generic"], gen.case_id(case) + " forced generic")
        assert np.array_equal(x, xg) and np.array_equal(v, vg)
