"""The on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2) reads the halo of a solve's ENTRY x from global memory through halo_vert, the
vertex of every halo entry, instead of exchanging it between the blocks.  The list is host logic (csrc/oc_plan.cpp), so it is checked here
without a GPU, on the plans the GPU bit tests run: blob_scene(30) and mixed_cube_scene(12) at the block shape admm_hip_create chooses and at
every forced ADMM_HIP_OC_SPB of {1, 3, 12, 16} it accepts -- halo_vert has the length of halo_src, equals orig[halo_src] & 0x0fffffff entry
by entry, every source row is live and every vertex is below the vertex count.  (The nbr_max these plans report is printed: the path of the
kernel without hand-off lists needs a block with more than 64 neighbour blocks, stats["max_neighbour_blocks"] == -1 -- the plan of
scenes.hub_scene() at one wave per block, checked by the last test here; tests/test_pcg2_no_handoff.py runs that path on the GPU.)"""
import numpy as np
import pytest

import scenes

CUS = 256      # compute units of the device the plans are made for


def _shapes(nv):
    """(label, G, spb) as plan_pcg_onchip (csrc/admm_hip.hip) chooses them: its own choice, then every forced shape it accepts"""
    ns = (nv + 63) // 64
    G = min(CUS, ns)
    spb = (ns + G - 1) // G
    assert spb <= 16
    while spb < 16 and (ns + spb - 1) // spb > 32 * spb:
        spb += 1
    out = [("plan", (ns + spb - 1) // spb, spb)]
    for se in (1, 3, 12, 16):
        if (ns + se - 1) // se <= CUS:
            out.append(("spb_%d" % se, (ns + se - 1) // se, se))
    return out


@pytest.mark.parametrize("name", ["blob", "mixed_cube"])
def test_halo_vert_is_the_vertex_of_every_halo_entry(name):
    sc = scenes.blob_scene(30, admm_iters=5, linsolver=0) if name == "blob" else scenes.mixed_cube_scene(12, admm_iters=5, linsolver=0)
    s = sc.make_solver(init=False)
    nv = len(sc.x)
    shapes = _shapes(nv)
    assert len(shapes) >= 4, shapes
    for label, G, spb in shapes:
        plan = s.host_oc_plan(G, spb, settings=sc.product_settings, coarse=False)
        halo = s.host_oc_plan_halo(G, spb, settings=sc.product_settings)
        orig, hp, hs, hv = plan["row_vertex"], halo["halo_ptr"], halo["halo_src"], halo["halo_vert"]
        T = 64 * spb
        nh = np.diff(hp)
        print(name, label, "G %d T %d entries %d longest halo %d (%.2f T) max neighbour blocks %d" %
              (G, T, hp[-1], nh.max(), nh.max() / T, plan["stats"]["max_neighbour_blocks"]))
        assert hp[0] == 0 and (nh >= 0).all() and nh.max() == plan["stats"]["max_halo"]
        assert len(hv) == len(hs) == hp[-1] and hp[-1] > 0
        assert (hs >= 0).all() and (hs < len(orig)).all()
        assert (orig[hs] >= 0).all(), "a halo entry points at a dummy row"
        assert np.array_equal(hv, orig[hs] & 0x0fffffff)
        assert (hv >= 0).all() and (hv < nv).all()
        # the lists themselves: per block sorted, without repeats, rows of OTHER blocks
        for b in range(G):
            h = hs[hp[b]:hp[b + 1]]
            assert (np.diff(h) > 0).all() and (h // T != b).all()


def test_hub_scene_plan_has_no_hand_off_lists():
    """scenes.hub_scene() at one wave per block is the one small scene whose plan leaves k_pcg2 without hand-off lists, so that grid barriers
    order the kernel's vector exchanges (tests/test_pcg2_no_handoff.py runs that path on the GPU): 4301 vertices make 68 slices, at one
    slice per block 68 blocks, and the hub's block has a halo entry from each of the 67 others -- more than the 64 a list holds.  If the
    partitioner or that cap changes, this test says that those GPU tests no longer reach the path.  The halo lists of the plan are held to
    the same properties as above; the longest halo is more than 60 entries per thread of the entry residual's list."""
    sc = scenes.hub_scene(admm_iters=5, linsolver=0)
    s = sc.make_solver(init=False)
    nv = len(sc.x)
    assert nv == 4301 and len(sc.tets[0][1]) == 8596 and len(sc.pins) == 8
    G, spb = 68, 1
    T = 64 * spb
    assert (nv + 63) // 64 == G and G <= CUS      # what plan_pcg_onchip makes of ADMM_HIP_OC_SPB=1
    plan = s.host_oc_plan(G, spb, settings=sc.product_settings, coarse=False)
    halo = s.host_oc_plan_halo(G, spb, settings=sc.product_settings)
    st = plan["stats"]
    orig, hp, hs, hv = plan["row_vertex"], halo["halo_ptr"], halo["halo_src"], halo["halo_vert"]
    nh = np.diff(hp)
    print("hub G %d T %d entries %d longest halo %d (%.2f T) lds_cols %d max neighbour blocks %d" %
          (G, T, hp[-1], nh.max(), nh.max() / T, st["lds_cols"], st["max_neighbour_blocks"]))
    assert st["max_neighbour_blocks"] == -1
    assert st["max_halo"] >= 4000 and st["lds_cols"] >= 4
    assert hp[0] == 0 and (nh >= 0).all() and nh.max() == st["max_halo"]
    assert len(hv) == len(hs) == hp[-1] and hp[-1] > 0
    assert (hs >= 0).all() and (hs < len(orig)).all()
    assert (orig[hs] >= 0).all(), "a halo entry points at a dummy row"
    assert np.array_equal(hv, orig[hs] & 0x0fffffff)
    assert (hv >= 0).all() and (hv < nv).all()
    for b in range(G):
        h = hs[hp[b]:hp[b + 1]]
        assert (np.diff(h) > 0).all() and (h // T != b).all()
    # the hub (vertex 0) is a matrix neighbour of every rim vertex, and its block gathers from every other block
    rp, ci, _ = s.host_matrix(sc.product_settings)
    row = ci[rp[0]:rp[1]]
    assert len(row[row != 0]) == 4300 and len(np.unique(row[row != 0])) == 4300
    hub_row = int(np.nonzero(((orig & 0x0fffffff) == 0) & (orig >= 0))[0][0])
    hb = hub_row // T
    assert len(np.unique(hs[hp[hb]:hp[hb + 1]] // T)) == G - 1 > 64
