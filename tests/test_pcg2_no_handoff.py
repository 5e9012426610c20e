"""The on-chip PCG kernel (csrc/pcg_onchip2.hpp: k_pcg2) orders its vector exchanges between the blocks in one of two ways: by the plan's
neighbour hand-off lists (a.nbr, a.flags), or -- when a block of the plan has more than 64 neighbour blocks and the plan therefore has no
lists -- by a grid barrier per exchange (`++be; oc_barrier(...)` in true_residual, at the start of a pass and in the pipelined loop), with
its own bookkeeping: one more barrier epoch per exchange, so the record parity `be & 1` runs differently.  This file runs that second path.

A.  ADMM_HIP_OC_HANDOFF=0 (read at create) leaves the lists out of any plan.  The two paths differ in how a block WAITS, in nothing it
    computes, so on the same scene and build every bit must agree with the hand-off path on the forced generic instance, and with what
    tests/golden/pcg2_entry_halo_parent_bits.json recorded of that instance: every case of make_pcg2_entry_halo_parent_bits.CASES through
    that module's run() (the plan's own shape, one wave per block, stand-alone solves from an x0 with -0.0, denormals, 1e+-100 and with
    b = 0, a tolerance that forces verifications and further passes, capped solves that end unconverged), and three more configurations
    through make_solve_entry_parent_bits.run(): the 1024-thread instance, soft modes with the fused end projection, and 32 KB of LDS
    (the slab's streamed tail; the smaller of the two sizes tests/test_solve_entry_bits.py runs).  This is also the only way to the
    two-level flavour of the path: no small natural scene has it.
B.  scenes.hub_scene() at one wave per block reaches the path by itself (tests/test_halo_vert_plan.py pins its plan): stand-alone solves
    against float64 references, whole frames against the launch path and the oracle, capped solves, and the kernel's abort exits.

Every run asserts through Solver.pcg_plan() which path it took and that the context did not give the on-chip solver up: a barrier that
times out makes the context fall back quietly, and every comparison here would pass without the path."""
import contextlib
import importlib.util
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import scenes

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pcg2_entry_halo_parent_bits", os.path.join(_GOLDEN, "make_pcg2_entry_halo_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
entry = gen.entry      # make_solve_entry_parent_bits: a runner with soft modes and the LDS size

SWITCHES = ("ADMM_HIP_OC_HANDOFF", "ADMM_HIP_OC_SPB", "ADMM_HIP_PCG_LAUNCHES", "ADMM_HIP_TEST_ABORT_SOLVE", "ADMM_HIP_UZ_FREEZE")


@contextlib.contextmanager
def _env(**kv):
    """The switches a context reads when it is created, set for that long and put back."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- A. the switched path against the hand-off path ----

class _Spy:
    """A scene whose solvers say, just before a runner closes them, what the runner's record lacks: the plan, the launch counts, the modes."""
    def __init__(self, sc):
        self._sc = sc
        self.seen = None

    def __getattr__(self, k):
        return getattr(self._sc, k)

    def make_solver(self, **kw):
        s = self._sc.make_solver(**kw)
        close = s.close

        def closing():
            if not getattr(s, "_ctx", None):      # (closed already: Solver.__del__ closes again)
                return
            plan = s.pcg_plan()
            self.seen = dict(plan=plan, pcg=s.persistent_launches()["pcg"], hot=s.pcg_instances()["hot"], modes=len(s.get_soft_modes()),
                             unconverged=s.runtime_data().unconverged_solves)
            if not plan["handoff"]:      # (without the lists the probe launches nothing: the plan's statistics only)
                self.seen["stats"] = s.probe_sync(1)[2]
            close()
        s.close = closing
        return s


def _both_paths(run, sc, cfg):
    """`cfg` twice: hand-off lists on the forced generic instance, then without the lists.  Asserts the path each took; returns the records."""
    spy = _Spy(sc)
    with _env():
        g, xg, vg = run(spy, cfg, True)
    on = spy.seen
    with _env(ADMM_HIP_OC_HANDOFF=0):
        n, xn, vn = run(spy, cfg, False)
    off = spy.seen
    print("hand-off", on, "\nbarriers", off, "\ntotals", g["solve_totals"], n["solve_totals"])
    assert on["plan"]["enabled"] and on["plan"]["handoff"] and not on["plan"]["gave_up"] and on["plan"]["nbr_max"] > 0 and g["hot"] == 0
    assert off["plan"] == dict(on["plan"], handoff=False), "the switched run is not the same plan without the lists"
    assert off["hot"] == 0 and n["hot"] == 0
    assert off["pcg"] == on["pcg"] > 0, "a solve of the switched run left the on-chip kernel"
    assert off["modes"] == on["modes"]
    return g, xg, vg, n, xn, vn, on, off


def _same_bits(what, g, xg, vg, n, xn, vn):
    assert np.isfinite(xn).all() and n["solve_totals"][0] > 0 and n["solve_totals"][2] > 0
    assert sorted(n) == sorted(g)
    for k in sorted(g):      # digests of m_x and m_v, the solves' digests, iteration and verification counts, the totals, the instance counts
        assert n[k] == g[k], "%s: %s without hand-off lists %r, with them %r" % (what, k, n[k], g[k])
    assert np.array_equal(xn, xg) and np.array_equal(vn, vg), what


@pytest.fixture(scope="module")
def parent_bits():
    with open(gen.FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["parent"] == gen.PARENT and sorted(fx["cases"]) == sorted(gen.CASES)
    return fx


@pytest.fixture(scope="module")
def scene_of(parent_bits):
    scs = {}
    for name in gen.SCENES:
        scs[name] = gen.make_scene(name)
        assert gen.base.scene_digest(scs[name]) == parent_bits["scenes"][name], "the mesh of %r is not the one the fixture was recorded on" % name
    return scs


@pytest.mark.parametrize("cid", list(gen.CASES))
def test_barrier_path_has_the_bits_of_the_hand_off_path(cid, parent_bits, scene_of):
    name, cfg = gen.CASES[cid]
    g, xg, vg, n, xn, vn, on, off = _both_paths(gen.run, scene_of[name], cfg)
    _same_bits(cid, g, xg, vg, n, xn, vn)
    if cfg["max_iters"] == gen.CAP:
        assert n["solve_totals"][0] > n["solve_totals"][1], "no capped solve ended unconverged"
    if cfg["tol"] < 1e-12:
        assert n["solve_small_verifications"] >= 2, "no solve with more than one pass"
    assert on["plan"]["two_level"] == (cfg["spb"] != 1)      # (one wave per block: 4 G coarse unknowns > 2 T, the block smoother alone)
    # ... and of the parent commit: its generic instance's record (where the hot instance is not eligible, the default record is that one's)
    want = parent_bits["cases"][cid]
    ref = want["forced_generic"] if want["forced_generic"] is not None else want["default"]
    assert ref["hot"] == 0
    for k in sorted(ref):
        if k.startswith("solve_") or k in ("m_x", "m_v"):
            assert n[k] == ref[k], "%s: %s differs from the parent commit's: %r, fixture %r" % (cid, k, n[k], ref[k])


MORE = {
    "blob-uzawa-spb_16": entry._cfg(spb=16),            # T = 1024: the other block-size instance
    "blob-uzawa-modes16": entry._cfg(soft=16),          # the fused end projection on the soft modes (a.defl_k > 0)
    "blob-uzawa-lds_32": entry._cfg(lds_kb=32),         # the slab does not hold the block's matrix: its tail is streamed
}


@pytest.mark.parametrize("cid", list(MORE))
def test_barrier_path_has_the_bits_of_the_hand_off_path_in_more_configurations(cid, scene_of):
    cfg = MORE[cid]
    g, xg, vg, n, xn, vn, on, off = _both_paths(entry.run, scene_of["blob"], cfg)
    _same_bits(cid, g, xg, vg, n, xn, vn)
    assert on["plan"]["two_level"]
    assert on["plan"]["T"] == (1024 if cfg["spb"] == 16 else 128)
    assert on["modes"] == cfg["soft"]
    if cfg["lds_kb"]:
        assert off["stats"]["on_chip"] < off["stats"]["stored"], "the slab holds the whole matrix: no streamed tail"


# ---- B. the natural path: a hub of valence 4300 at one wave per block ----

HUB_PLAN = dict(enabled=True, G=68, spb=1, T=64, two_level=False, handoff=False, nbr_max=-1, gave_up=False)
TIGHT = dict(pcg_tol=1e-12, pcg_max_iters=4000)
FRAMES, ADMM_ITERS = 3, 5
JACOBI_ITERS = 274      # float64 Jacobi-PCG (numpy) on the hub system to r . D^-1 r <= 1e-24 b . D^-1 b, the kernel's stop rule


def _hub(ls=0):
    if ls == 0:
        return scenes.hub_scene(admm_iters=ADMM_ITERS, linsolver=0)
    # UzawaCG: a floor 1.2 mm under the body, which sags into it under a tenth of the gravity -- the inertial prediction of the first frame
    # lies 1.7 mm lower, so the lowest rim vertices (spaced 0.23 mm in height) are rows of C from the first frame on (2, then 11, then 19
    # in the oracle): K^-1 columns on the lanes in every frame, and few enough of them for a quick test
    sc = scenes.hub_scene(admm_iters=ADMM_ITERS, linsolver=2, gravity=-1.0)
    sc.obstacles.append((0, [-0.5012, 0.0, 0.0, 0.0]))
    return sc


def _hub_solver(sc, launches=False, abort=None, freeze=False, **kw):
    with _env(ADMM_HIP_OC_SPB=1, ADMM_HIP_PCG_LAUNCHES=1 if launches else None, ADMM_HIP_TEST_ABORT_SOLVE=abort, ADMM_HIP_UZ_FREEZE=1 if freeze else None):
        return sc.make_solver(**kw)


def _frames(s, n=FRAMES, converged=True):
    out = []
    for _ in range(n):
        s.step()
        if converged:
            assert s.runtime_data().unconverged_solves == 0
        out.append(s.m_x.copy())
    return out


@pytest.fixture(scope="module")
def launch_frames():
    """The hub scene on the launch path at 1e-12 (linsolver 0): the frames two tests compare with.  Not modified."""
    s = _hub_solver(_hub(), launches=True, **TIGHT)
    xs = _frames(s)
    assert s.persistent_launches()["pcg"] == 0 and not s.pcg_plan()["enabled"]
    s.close()
    return xs


def test_hub_solves_against_float64():
    """Stand-alone solves on the path a hub mesh takes by itself, to 1e-12: the error against the known solution and against a sparse
    direct solve below 1e-8 max|xs| (the bar of tests/test_big_pcg.py for the same kind of solve; float64 Jacobi-PCG gets 6e-11 here).
    Iterations: float64 Jacobi-PCG needs 274 to the same stop rule and the device's block smoother is at least Jacobi, so 274 is the
    bound; the MI355X needs 206 (208 from the x0 with special values)."""
    sc = _hub()
    s = _hub_solver(sc, **TIGHT)
    assert s.pcg_plan() == HUB_PLAN, s.pcg_plan()
    rp, ci, va = s.system_matrix()
    nv = len(sc.x)
    K = (sp.csr_matrix((va, ci, rp), shape=(nv, nv)) + sp.diags(sc.m)).tocsc()
    assert K[:, 0].nnz >= 4300      # the hub's column
    xs = np.random.default_rng(1).standard_normal((nv, 3))
    b = (K @ xs).ravel()
    lu = spla.splu(K)
    bar = 1e-8 * np.abs(xs).max()
    x, it = s.global_solve(b, np.zeros(3 * nv))
    err, err_lu = np.abs(x - xs.ravel()).max(), np.abs(x.reshape(-1, 3) - lu.solve(b.reshape(-1, 3))).max()
    print("hub solve: %d iterations (float64 Jacobi-PCG: %d), error %.3e, against the direct solve %.3e, bar %.3e" % (it, JACOBI_ITERS, err, err_lu, bar))
    assert err < bar and err_lu < bar
    assert 0 < it <= JACOBI_ITERS
    x2, it2 = s.global_solve(b, x)      # warm start from the solution
    assert it2 <= 1 and np.abs(x2 - x).max() < 1e-9 * np.abs(xs).max(), it2
    # special values at halo vertices of the entry x: from them with a right-hand side, and with b = 0 (the entry residual is the whole work)
    hv = np.unique(s.host_oc_plan_halo(68, 1, settings=sc.product_settings)["halo_vert"])
    assert len(hv) > 4000 and hv[0] == 0
    rng = np.random.default_rng(20)
    x0 = rng.standard_normal((nv, 3))
    small = np.array([-0.0, 5e-324, -2.2e-310, 1e-100, -1e-100, 0.0])      # (the values of make_pcg2_entry_halo_parent_bits.entry_vectors)
    pick = hv[::3]
    x0[pick] = small[(np.arange(len(pick))[:, None] + np.arange(3)[None, :]) % len(small)]
    y, it3 = s.global_solve(b, x0.ravel())
    print("from the special x0: %d iterations, error against the direct solve %.3e" % (it3, np.abs(y.reshape(-1, 3) - lu.solve(b.reshape(-1, 3))).max()))
    assert np.abs(y.reshape(-1, 3) - lu.solve(b.reshape(-1, 3))).max() < bar
    z, it4 = s.global_solve(np.zeros(3 * nv), x0.ravel())
    print("b = 0 from the special x0: %d iterations, max|x| %.3e" % (it4, np.abs(z).max()))
    assert np.isfinite(z).all()
    p = s.pcg_plan()
    assert p == HUB_PLAN, p
    print("on-chip launches of the four solves:", s.persistent_launches()["pcg"])
    assert s.persistent_launches()["pcg"] >= 3 and s.pcg_instances()["hot"] == 0      # (b = 0 may be answered without a launch)
    s.close()


@pytest.mark.parametrize("ls", [0, 2])
def test_hub_frames_match_the_launch_path_and_the_oracle(ls, launch_frames):
    """Three frames with PCG (linsolver 0) and with UzawaCG on a floor (linsolver 2: its K^-1 columns run on lanes whose a.flags are null
    here), both at 1e-12, against the same scene on the launch path (bars of tests/test_big_pcg.py) and the oracle (1e-7).  With contact the
    active set is detected once per step on every side (ADMM_HIP_UZ_FREEZE=1, the oracle's freeze_active; as in
    test_gpu_parity.py::test_step_uzawa_frozen_active_set_is_tight): detected in every ADMM iteration, a vertex the last solve put ON the
    floor is a row or not by the sign of its round-off, and no two solvers, the oracle included, stay within 1e-3 of each other on this
    scene -- that comparison says nothing about the exchange path."""
    sc = _hub(ls)
    s = _hub_solver(sc, freeze=ls == 2, **TIGHT)
    assert s.pcg_plan() == HUB_PLAN, s.pcg_plan()
    o = sc.make_oracle(mode=1)
    if ls == 0:
        ref = launch_frames
    else:
        o.freeze_active = True
        r = _hub_solver(sc, launches=True, freeze=True, **TIGHT)
        ref = _frames(r)
        assert r.persistent_launches()["pcg"] == 0
        r.close()
    xs, rows = [], []
    for f in range(FRAMES):
        s.step()
        assert s.runtime_data().unconverged_solves == 0
        xs.append(s.m_x.copy()); rows.append(s.contact_totals())
    for f in range(FRAMES):
        e = scenes.rel_err(xs[f], ref[f])
        print("linsolver %d frame %d: against the launch path %.3e, contact rows so far %d" % (ls, f, e, rows[f]))
        assert e < (1e-8 if ls == 0 else 1e-5), (f, e)
        o.step()
        eo = scenes.rel_err(xs[f], o.x)
        print("  against the oracle %.3e (its contact rows: %d)" % (eo, len(o._hits)))
        assert eo < 1e-7, (f, eo)
    p, inst = s.pcg_plan(), s.pcg_instances()
    print(p, inst, s.persistent_launches(), s.solve_totals(), s.uzawa_cache_stats() if ls == 2 else "", "inner iterations of the last frame", s.runtime_data().inner_iters)
    assert p == HUB_PLAN, p
    assert s.persistent_launches()["pcg"] > 0 and inst["hot"] == 0 and inst["generic"] >= FRAMES * ADMM_ITERS
    if ls == 2:
        assert rows[0] > 0 and rows[0] < rows[1] < rows[2] and inst["lane_generic"] > 0, "no K^-1 column ran on a lane"
    tot = s.solve_totals()
    assert tot[0] > 0 and tot[0] == tot[1]
    s.close()


def test_hub_capped_solves():
    """pcg_max_iters = 3: every solve ends unconverged in the pipelined loop, frames stay finite and the context keeps the on-chip solver.
    The frames are NOT compared with the launch path capped the same way: three iterations of two different preconditioners -- here
    the block-local Chebyshev smoother (no coarse space at one wave per block), there the two-level preconditioner of csrc/pcg_big.hpp --
    are different iterates (measured on the MI355X: the frames of the two are 5.0e-3, 1.8e-2 and 4.7e-2 apart; with both preconditioners cut
    down to Jacobi still 5e-6, 1.3e-3, 2.8e-3: the recurrences and the warm starts differ too).  What three iterations of ANY preconditioned CG do, whatever the preconditioner: the error in the K-norm
    falls monotonically (CG minimises it over a growing subspace).  That is asserted on a stand-alone capped solve, in float64."""
    sc = _hub()
    s = _hub_solver(sc, pcg_tol=1e-12, pcg_max_iters=3)
    assert s.pcg_plan() == HUB_PLAN, s.pcg_plan()
    xs = _frames(s, converged=False)
    tot = s.solve_totals()
    print("capped: totals", tot, "unconverged in the last frame", s.runtime_data().unconverged_solves)
    assert all(np.isfinite(x).all() for x in xs) and np.isfinite(s.m_v).all()
    assert tot[0] == FRAMES * ADMM_ITERS and tot[0] > tot[1] and tot[2] <= 3 * tot[0]
    assert s.runtime_data().unconverged_solves > 0
    rp, ci, va = s.system_matrix()
    nv = len(sc.x)
    K = (sp.csr_matrix((va, ci, rp), shape=(nv, nv)) + sp.diags(sc.m)).tocsr()
    sol = np.random.default_rng(1).standard_normal((nv, 3))
    b = K @ sol
    x3, it = s.global_solve(b.ravel(), np.zeros(3 * nv))
    e0 = np.sqrt((sol * (K @ sol)).sum(axis=0))
    d = x3.reshape(-1, 3) - sol
    e3 = np.sqrt((d * (K @ d)).sum(axis=0))
    print("capped solve: %d iterations, K-norm of the error per axis %s -> %s" % (it, e0, e3))
    assert 0 < it <= 3 and np.isfinite(x3).all() and (e3 < e0).all()
    p = s.pcg_plan()
    assert p == HUB_PLAN, p
    assert s.persistent_launches()["pcg"] == FRAMES * ADMM_ITERS + 1
    s.close()


def test_hub_abort_leaves_through_the_barrier_paths_exits(launch_frames):
    """The test hook ADMM_HIP_TEST_ABORT_SOLVE raises the abort word of one solve's barrier set: the kernel leaves through the
    `!oc_barrier(...)` exits of the path without hand-off lists (a cooperative early return of every block), the context sees it at the
    step's synchronisation, gives the on-chip solver up and replays the frame on the launch path."""
    k = ADMM_ITERS + 3      # a solve inside the second frame
    s = _hub_solver(_hub(), abort=k, **TIGHT)
    assert s.pcg_plan() == HUB_PLAN, s.pcg_plan()
    s.step()
    assert s.pcg_plan() == HUB_PLAN and s.persistent_launches()["pcg"] == ADMM_ITERS
    assert scenes.rel_err(s.m_x, launch_frames[0]) < 1e-8
    for f in (1, 2):
        s.step()
        assert s.runtime_data().unconverged_solves == 0
        p = s.pcg_plan()
        assert p == dict(HUB_PLAN, enabled=False, gave_up=True), p
        e = scenes.rel_err(s.m_x, launch_frames[f])
        print("after the abort, frame %d: against the launch path %.3e, on-chip launches %d" % (f, e, s.persistent_launches()["pcg"]))
        assert e < 1e-8, (f, e)
    assert k <= s.persistent_launches()["pcg"] <= 2 * ADMM_ITERS      # (launches behind the abort leave at once; none after it was seen)
    s.close()
