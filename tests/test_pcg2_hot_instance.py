"""The two instances of the on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2<MAXT, HOT>).  The hot instance has the configuration of the
ADMM loop's solves fixed at compile time; the generic one serves every other launch (csrc/admm_hip.hip: pcg2_hot_ok).  Both run the same
arithmetic in the same order, so a scene stepped with the hot instance and with the generic one forced (ADMM_HIP_OC_GENERIC=1) must give the
same bits -- also where a solve leaves the pipelined pass for the verification, the restart and the classic continuation, which the hot
instance keeps behind its iteration loop.  Which instance a launch took is asked through admm_hip_pcg_instances."""
import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes

pytestmark = pytest.mark.gpu

FRAMES, ADMM_ITERS = 3, 5


def _scene(name):
    if name == "blob":
        return scenes.blob_scene(30, admm_iters=ADMM_ITERS, linsolver=0)      # 16 k tets, unstructured: several blocks with halos
    return scenes.mixed_cube_scene(12, admm_iters=ADMM_ITERS, linsolver=0)


def _forced_generic(monkeypatch, sc, **kw):
    monkeypatch.setenv("ADMM_HIP_OC_GENERIC", "1")      # (read once, when the context is created)
    try:
        return sc.make_solver(**kw)
    finally:
        monkeypatch.delenv("ADMM_HIP_OC_GENERIC")


@pytest.mark.parametrize("tol", [1e-8, 1e-13], ids=["short_pass", "cold_paths"])
@pytest.mark.parametrize("soft", [0, 8], ids=["no_modes", "modes8"])
@pytest.mark.parametrize("name", ["blob", "mixed_cube"])
def test_hot_and_generic_instance_give_the_same_bits(name, soft, tol, monkeypatch):
    """pcg_tol 1e-8: the trusted short first pass.  1e-13: below what a pass is trusted for -- every solve that iterates leaves the iteration loop
    to verify its true residual (asserted through the solve's own report) and, where one pass does not get there, goes on to further passes and
    the classic form: the paths both instances keep behind the iteration loop."""
    sc = _scene(name)
    kw = dict(pcg_tol=tol, pcg_max_iters=600, soft_modes=soft)
    hot = sc.make_solver(**kw)
    gen = _forced_generic(monkeypatch, sc, **kw)
    if soft:      # the modes were computed at initialize: solves without the recycled start, the generic instance's on both contexts
        assert hot.pcg_instances()["hot"] == 0 and hot.pcg_instances()["generic"] > 0
        assert np.array_equal(hot.get_soft_modes(), gen.get_soft_modes())
    for f in range(FRAMES):
        hot.step(); gen.step()
        assert np.array_equal(hot.m_x, gen.m_x), (f, np.abs(hot.m_x - gen.m_x).max())
        assert np.array_equal(hot.m_v, gen.m_v), (f, np.abs(hot.m_v - gen.m_v).max())
        vh, vg = hot.pcg_instances()["last_verifications"], gen.pcg_instances()["last_verifications"]
        print(name, soft, tol, "frame", f, "verifications of the frame's last solve: hot %d generic %d" % (vh, vg))
        assert vh == vg
        if tol < 1e-10:      # below the trust rule's tolerance (kOc2TrustTol2 = 1e-20 squared): no pass may end without a verification, so the
            assert vh >= 1   # solve DID leave the iteration loop for the path behind it (a solve converged at entry would report 0)
    ih, ig = hot.pcg_instances(), gen.pcg_instances()
    assert ih["last"] == "hot" and ih["hot"] == FRAMES * ADMM_ITERS, ih
    assert ig["last"] == "generic" and ig["hot"] == 0 and ig["generic"] == ih["generic"] + ih["hot"], (ih, ig)
    th, tg = hot.solve_totals(), gen.solve_totals()
    assert th == tg and th[0] >= FRAMES * ADMM_ITERS and th[2] > 0, (th, tg)
    assert np.isfinite(hot.m_x).all() and np.abs(hot.m_x - sc.x.ravel()).max() > 1e-4      # the scene moved
    hot.close(); gen.close()


@pytest.fixture(scope="module")
def cube_oracle():
    """Five frames of the pinned Neo-Hookean cube on the CPU oracle (exact global solve): the reference of the step-parity tests."""
    sc = scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, admm_iters=10, linsolver=0)
    o = sc.make_oracle(mode=1)
    for _ in range(5):
        o.step()
    x = o.x.copy(); x.setflags(write=False)
    return sc, x


@pytest.mark.parametrize("env, instance", [(None, "hot"), ("ADMM_HIP_OC_COARSE=0", "generic"), ("ADMM_HIP_OC_GENERIC=1", "generic")])
def test_dispatch_in_the_admm_loop(env, instance, cube_oracle, monkeypatch):
    """The ADMM loop launches the hot instance; without the coarse space, or under the force switch, the generic one -- and each agrees with the
    oracle as the step-parity tests ask (test_gpu_parity.test_step_parity_cube_ldlt: 1e-7 of the bounding box at pcg_tol 1e-11)."""
    sc, x_ref = cube_oracle
    if env:
        monkeypatch.setenv(*env.split("="))
    s = sc.make_solver(pcg_tol=1e-11, pcg_max_iters=300)
    if env:
        monkeypatch.delenv(env.split("=")[0])
    assert s.pcg_instances()["last"] == "none"
    for _ in range(5):
        s.step()
    i = s.pcg_instances()
    assert i["last"] == instance, i
    assert (i["hot"] == 50 and i["generic"] == 0) if instance == "hot" else (i["hot"] == 0 and i["generic"] == 50), i
    assert i["lane_hot"] == 0 and i["lane_generic"] == 0, i
    err = scenes.rel_err(s.m_x, x_ref)
    assert err < 1e-7, err
    assert s.runtime_data().last_solve_converged == 1
    s.close()


def test_stand_alone_solve_takes_the_generic_instance():
    """admm_hip_global_solve is not one of the loop's solves: generic, between hot ones, and as exact as test_global_solve_pcg_matches_exact asks."""
    sc = scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, admm_iters=4)
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=400)
    o = sc.make_oracle()
    s.step()
    assert s.pcg_instances()["last"] == "hot"
    b = o.A @ np.random.default_rng(31).standard_normal(o.dof)
    x, it = s.global_solve(b, np.zeros(o.dof))
    i = s.pcg_instances()
    assert i["last"] == "generic" and i["generic"] == 1 and i["hot"] == 4, i
    xo = o.solve_ldlt(b)
    assert 0 < it < 400 and np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    s.step()
    assert s.pcg_instances()["last"] == "hot"
    s.close()


def test_uzawa_column_lanes_take_the_generic_instance(monkeypatch):
    """UzawaCG on a floor: the loop's own solves (recycled start) are the hot instance's, the K^-1 columns of the contact rows are solved on side
    streams by the generic one.  Frozen active set, so that the steps agree with the oracle as tightly as
    test_gpu_parity.test_step_uzawa_frozen_active_set_is_tight asks (1e-7)."""
    sc = scenes.cube_scene(6, pkg.TET_NEOHOOKEAN, pin_face=False, admm_iters=8, linsolver=2, size=0.5)
    sc.pins.clear()
    sc.obstacles.append((0, [-0.0217, 0.0, 0.0, 0.0]))
    monkeypatch.setenv("ADMM_HIP_UZ_FREEZE", "1")
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=600)
    monkeypatch.delenv("ADMM_HIP_UZ_FREEZE")
    o = sc.make_oracle(mode=1)
    o.freeze_active = True
    hit_frames = 0
    for _ in range(8):
        s.step(); o.step()
        hit_frames += 1 if len(o._hits) else 0
    assert hit_frames >= 3, "scene meant to collide"
    i, st = s.pcg_instances(), s.uzawa_cache_stats()
    assert st["lanes"] >= 2 and st["lane_batches"] >= 1 and st["columns"] >= 49, st      # the bottom face: 7 x 7 vertices
    assert i["lane_generic"] > 0 and i["lane_hot"] == 0 and i["hot"] > 0, i
    err = scenes.rel_err(s.m_x, o.x)
    assert err < 1e-7, err
    s.close()
