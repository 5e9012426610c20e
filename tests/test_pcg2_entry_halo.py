"""The first residual of a launch of the on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2) no longer exchanges the entry x between the
blocks: x0 lies complete in global memory, so the halo of r0 = b - A x0 is read from it through the plan's halo_vert.  A change of schedule
-- the halo entries are the very doubles the neighbours published, the product runs in the same order -- so every bit a step or a solve
computes is what the commit before computed: tests/golden/pcg2_entry_halo_parent_bits.json holds that commit's digests (written once by
tests/golden/make_pcg2_entry_halo_parent_bits.py with that commit's library; nothing here writes it), on the cases the earlier bit tests
(test_pcg2_block_sums.py, test_solve_entry_bits.py, test_pcg2_closing_bits.py) do not pin and this change can break: a halo longer than two
entries per thread (blob_scene(30): T = 128, longest halo 287, the third entry comes from the list), one wave per block, stand-alone solves
from an x0 with -0.0, denormals, 1e-100 and 1e100 at halo vertices and with b = 0, a tolerance that forces verifications and further passes
(the later residuals of the launch keep the exchange), and capped solves that end unconverged from a cold first frame on.  Wherever the hot
instance serves a case it is repeated on the forced generic instance; both must agree with each other and with the fixture.

No plan of a small scene reaches the kernel's path without hand-off lists (a block with more than 64 neighbour blocks): blob_scene(30) at
one wave per block has at most 22, mixed_cube_scene(12) at most 19 (tests/test_halo_vert_plan.py prints them).  That path is run by
tests/test_pcg2_no_handoff.py: on these cases with ADMM_HIP_OC_HANDOFF=0, held to this fixture as well, and on scenes.hub_scene(), whose plan has it."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pcg2_entry_halo_parent_bits", os.path.join(_GOLDEN, "make_pcg2_entry_halo_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT and fx["frames"] == gen.FRAMES and fx["admm_iters"] == gen.ADMM_ITERS
    assert sorted(fx["cases"]) == sorted(gen.CASES)
    # what the cases are about happened when the fixture was recorded
    c = fx["cases"]
    assert c["mixed_cube-uzawa-cold_paths"]["default"]["solve_small_verifications"] >= 2, "no solve of the parent's run had more than one pass"
    assert c["blob-uzawa-capped"]["default"]["solve_totals"][0] > c["blob-uzawa-capped"]["default"]["solve_totals"][1], "no capped solve ended unconverged"
    assert c["blob-uzawa-spb_1"]["forced_generic"] is None and c["blob-uzawa-spb_plan"]["forced_generic"] is not None
    return fx


@pytest.fixture(scope="module")
def scene_of(parent_bits):
    scs = {}
    for name in gen.SCENES:
        scs[name] = gen.make_scene(name)
        assert gen.base.scene_digest(scs[name]) == parent_bits["scenes"][name], "the mesh of %r is not the one the fixture was recorded on" % name
    return scs


def _check(rec, want, what):
    print(what, "totals", rec["solve_totals"], "fixture", want["solve_totals"], "hot %d generic %d" % (rec["hot"], rec["generic"]),
          {k: v for k, v in rec.items() if k.startswith("solve_") and not k.endswith("_x")})
    assert sorted(rec) == sorted(want), (what, sorted(rec), sorted(want))
    for k in sorted(want):
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
        for k in d:
            if k.startswith("solve_") or k in ("m_x", "m_v", "solve_totals"):
                assert d[k] == g[k], (cid, k)
