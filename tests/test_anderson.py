"""Anderson acceleration of the ADMM loop on the device (csrc/anderson.hpp; admm_hip_set_anderson, Solver.set_anderson,
Solver.anderson_history).

Scenes (linsolver 0, pcg_tol 1e-12, so that the PCG's noise sits below everything compared):
  cantilever162   scenes.cube_scene(3, NH)            162 tets: less than one chunk, one kind
  mixed750        scenes.mixed_cube_scene(5)          750 tets: three chunks, a wavefront across a model boundary, pin terms
  cloth           cloth_with_hinges(12)               288 triangles, 408 hinges, pin terms: all four u buffers and their padding

test_device_runs_the_stated_algorithm restates the algorithm in numpy (reference_run) and drives it over the DEVICE's own map
(Solver.local_step / Solver.global_solve), 12 iterations, windows 1, 3, 8.  MEASURED on the MI355X (largest deviation over the nine
scene/window pairs; no pair met a tie of the safeguard, every flag of every iteration equal): |F_k| 3.4e-7 relative, theta 1.8e-5 of the
iteration's largest entry, the step's x 6.0e-11 of the bounding box -- the two sides share G up to the PCG's noise (pcg_tol 1e-12, a
different start and recycled subspace per side), which the extrapolation amplifies by the conditioning of its small system.  Asserted at
10 x: BOUND_* below.
"""
import functools

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from test_energy_monitor import cloth_with_hinges

NH = pkg.TET_NEOHOOKEAN
SCENES = ("cantilever162", "mixed750", "cloth")
GPU_KW = dict(pcg_tol=1e-12, pcg_max_iters=500)

# measured on the MI355X by this test (printed before the assertion), asserted at 10 x
MEASURED_RESID = 3.4e-7      # |F_k| relative (cloth, window 8; cantilever162 window 1: 1.0e-8)
MEASURED_THETA = 1.8e-5      # theta, of the iteration's largest |theta_j| (mixed750, window 8; windows 1 and 3: <= 3.2e-6)
MEASURED_X = 6.0e-11         # the step's x, of the bounding box (cantilever162, window 8)
BOUND_RESID, BOUND_THETA, BOUND_X = 10 * MEASURED_RESID, 10 * MEASURED_THETA, 10 * MEASURED_X
assert BOUND_X <= 1e-5       # the project's whole-step bar


def make_scene(name, **settings):
    settings = dict(dict(linsolver=0), **settings)
    if name == "cantilever162":
        return scenes.cube_scene(3, NH, **settings)
    if name == "mixed750":
        return scenes.mixed_cube_scene(5, **settings)
    return cloth_with_hinges(12, **settings)


def run_steps(name, n_steps=1, settings=None, **gpu_kw):
    """a fresh solver, n_steps from rest -> (x, v, solver); the caller closes the solver"""
    sc = make_scene(name, **(settings or {}))
    s = sc.make_solver(**dict(GPU_KW, **gpu_kw))
    for _ in range(n_steps):
        s.step()
    return s.m_x.copy(), s.m_v.copy(), s


def bbox_err(a, b):
    return scenes.rel_err(a, b)


@functools.lru_cache(None)
def x_star(name):
    """the device's own plain run, 600 iterations"""
    x, _, s = run_steps(name, settings=dict(admm_iters=600))
    s.close()
    return x


@functools.lru_cache(None)
def plain_history(name, iters):
    x, _, s = run_steps(name, settings=dict(admm_iters=iters), monitor=1)
    h = s.admm_history()
    s.close()
    return x, h


# ---------------------------------------------------------------- the algorithm, in numpy ------------------------------------
def reference_run(name, iters, window):
    """The stated algorithm over the device's own G: one step from rest.  -> dict(accepted, accelerated, entries, resid, theta, x,
    tie): tie = the first iteration whose safeguard comparison is closer than 1e-6 relative (None: none)."""
    sc = make_scene(name, admm_iters=iters)
    s = sc.make_solver(**GPU_KW)
    o = sc.make_oracle(mode=1)
    dt = sc.settings["timestep_s"]; dt2 = dt * dt
    m = sc.masses3(); W2 = o.W * o.W
    v = np.zeros_like(s.m_x); v[1::3] += dt * sc.settings["gravity"]
    x = s.m_x + dt * v
    Mxbar = m * x
    u = np.zeros(s.num_rows())
    assert W2.size == u.size

    def dot(ax, au, bx, bu):
        return float(np.dot(m / dt2 * ax, bx) + np.dot(W2 * au, bu))

    ring = []      # (gx, gu, Fx, Fu), oldest first
    r_acc = np.inf; accel = False; tie = None
    rec = dict(accepted=[], accelerated=[], entries=[], resid=[], theta=[])
    x_out = None
    for k in range(iters):
        _, gu, b = s.local_step(x, u, Mxbar)
        gx, _ = s.global_solve(b, x)
        Fx, Fu = gx - x, gu - u
        FF = dot(Fx, Fu, Fx, Fu)
        theta = np.zeros(8)
        rec["accelerated"].append(int(accel)); rec["resid"].append(np.sqrt(FF))
        if accel and tie is None and abs(FF - r_acc) <= 1e-6 * max(FF, r_acc):
            tie = k
        if accel and FF > r_acc:      # rejected
            x, u = ring[-1][0].copy(), ring[-1][1].copy()
            x_out = x
            ring = []; accel = False
            rec["accepted"].append(0); rec["entries"].append(0); rec["theta"].append(theta)
            continue
        r_acc = FF
        ring.append((gx, gu, Fx, Fu)); ring = ring[-(window + 1):]
        p = len(ring)
        x, u, accel = gx, gu, False
        x_out = gx
        if p >= 2:
            dF = [(ring[j + 1][2] - ring[j][2], ring[j + 1][3] - ring[j][3]) for j in range(p - 1)]
            H = np.array([[dot(a[0], a[1], c[0], c[1]) for c in dF] for a in dF])
            rhs = np.array([dot(a[0], a[1], Fx, Fu) for a in dF])
            A = H + 1e-10 * (np.trace(H) / (p - 1)) * np.eye(p - 1)
            ok = np.all(np.isfinite(A)) and np.all(np.isfinite(rhs))
            if ok:
                try:
                    Lc = np.linalg.cholesky(A)
                    th = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
                    ok = bool(np.all(np.isfinite(th)))
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                theta[:p - 1] = th
                if k + 1 < iters:      # nothing is extrapolated behind the last iteration
                    x = gx - sum(th[j] * (ring[j + 1][0] - ring[j][0]) for j in range(p - 1))
                    u = gu - sum(th[j] * (ring[j + 1][1] - ring[j][1]) for j in range(p - 1))
                accel = True
            else:
                ring = []; p = 0
        rec["accepted"].append(1); rec["entries"].append(p); rec["theta"].append(theta)
    s.close()
    out = {k2: np.array(v2) for k2, v2 in rec.items()}
    out["x"] = x_out; out["tie"] = tie
    return out


# ---------------------------------------------------------------- 1. off is off -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_off_is_off(name):
    """Settings(anderson=0) explicit against the setting untouched: three steps, identical bytes.  anderson=3 with admm_iters=2: two
    evaluations give one ring difference only after the second solve, and nothing is extrapolated behind the last iteration --
    identical bytes again."""
    x0, v0, s0 = run_steps(name, 3)
    x1, v1, s1 = run_steps(name, 3, anderson=0)
    assert s0.anderson_history()["accepted"].size == 0 and s1.anderson_history()["resid"].size == 0
    assert x0.tobytes() == x1.tobytes() and v0.tobytes() == v1.tobytes()
    s0.close(); s1.close()
    xp, vp, sp = run_steps(name, 3, settings=dict(admm_iters=2))
    xa, va, sa = run_steps(name, 3, settings=dict(admm_iters=2), anderson=3)
    h = sa.anderson_history()
    assert list(h["accepted"]) == [1, 1] and list(h["accelerated"]) == [0, 0] and list(h["entries"]) == [1, 2]
    assert xp.tobytes() == xa.tobytes() and vp.tobytes() == va.tobytes()
    sp.close(); sa.close()


# ---------------------------------------------------------------- 2. the stated algorithm -------------------------------------
@functools.lru_cache(None)
def algorithm_deviations():
    """every scene/window pair once: (name, window, cut, d_resid, d_theta, d_x, flags_equal)"""
    rows = []
    for name in SCENES:
        for window in (1, 3, 8):
            ref = reference_run(name, 12, window)
            x, _, s = run_steps(name, settings=dict(admm_iters=12), anderson=window)
            h = s.anderson_history()
            s.close()
            n = 12 if ref["tie"] is None else ref["tie"]
            flags = all(np.array_equal(h[k][:n], ref[k][:n]) for k in ("accepted", "accelerated", "entries"))
            d_resid = float(np.max(np.abs(h["resid"][:n] - ref["resid"][:n]) / ref["resid"][:n])) if n else 0.0
            scale = np.maximum(np.abs(ref["theta"][:n]).max(axis=1), 1e-300)
            d_theta = float(np.max(np.abs(h["theta"][:n] - ref["theta"][:n]).max(axis=1) / scale)) if n else 0.0
            d_x = bbox_err(x, ref["x"]) if ref["tie"] is None else 0.0
            rows.append((name, window, ref["tie"], d_resid, d_theta, d_x, flags, int(np.sum(ref["accepted"] == 0))))
    return rows


@pytest.mark.gpu
def test_device_runs_the_stated_algorithm():
    """12 iterations, windows 1, 3, 8, three scenes: per iteration the flags (accepted, accelerated, entries) equal the numpy run's,
    |F_k|, theta and the step's x within 10 x the deviation measured on the MI355X.  From the first iteration whose safeguard
    comparison is a tie (|F_k|^2 and r_acc closer than 1e-6 relative in the numpy run) a pair is no longer compared; at most one
    pair may be cut short that way."""
    rows = algorithm_deviations()
    for r in rows:
        print("anderson vs numpy  %-14s window %d  tie %-4s  |F| %.3e  theta %.3e  x %.3e  flags %s  rejections %d" % r)
    print("anderson vs numpy  largest: |F| %.3e  theta %.3e  x %.3e" % (max(r[3] for r in rows), max(r[4] for r in rows), max(r[5] for r in rows)))
    assert sum(r[2] is not None for r in rows) <= 1
    for r in rows:
        assert r[6], r
        assert r[3] <= BOUND_RESID and r[4] <= BOUND_THETA and r[5] <= BOUND_X, r


# ---------------------------------------------------------------- 3. it converges faster --------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_converges_faster(name):
    """One step of 20 iterations against x* (the device's plain run, 600 iterations): the accelerated run's max |x - x*| is at most
    1/10 of the plain run's, windows 3 and 5.  MEASURED factors on the MI355X: window 3 100 / 33 / 388, window 5 117 / 35 / 113 (cantilever162 /
    mixed750 / cloth)."""
    xs = x_star(name)
    xp, _, sp = run_steps(name, settings=dict(admm_iters=20)); sp.close()
    ep = bbox_err(xp, xs)
    for window in (3, 5):
        xa, _, sa = run_steps(name, settings=dict(admm_iters=20), anderson=window)
        h = sa.anderson_history(); sa.close()
        ea = bbox_err(xa, xs)
        print("anderson convergence  %-14s window %d: plain %.3e  accelerated %.3e  factor %.1f  rejections %d" %
              (name, window, ep, ea, ep / ea, int(np.sum(h["accepted"] == 0))))
        assert ea <= ep / 10.0, (name, window, ep, ea)


# ---------------------------------------------------------------- 4. a residual level sooner ----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_meets_a_residual_level_sooner(name):
    """The plain run's primal and dz of iteration 60 are met together by an accepted iteration <= 40 of the accelerated run (window 3).
    MEASURED on the MI355X: iteration 22 / 25 / 25."""
    _, hp = plain_history(name, 80)
    primal, dz = hp["primal"][59], hp["dz"][59]
    _, _, s = run_steps(name, settings=dict(admm_iters=40), anderson=3, monitor=1)
    hm, ha = s.admm_history(), s.anderson_history()
    s.close()
    assert len(hm["primal"]) == len(ha["accepted"]) == 40
    hit = np.nonzero((ha["accepted"] == 1) & (hm["primal"] <= primal) & (hm["dz"] <= dz))[0]
    best = np.min(np.maximum(hm["primal"] / primal, hm["dz"] / dz)[ha["accepted"] == 1])
    print("anderson residual level  %-14s plain it 60: primal %.3e dz %.3e; accelerated first at iteration %s, best ratio %.3e" %
          (name, primal, dz, hit[0] + 1 if hit.size else None, best))
    assert hit.size > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_admm_tol_stops_sooner(name):
    """admm_tol set so that the plain run stops at iteration 60 (between 40 and 80): the accelerated run (window 3) stops after at
    most 2/3 of the plain run's iterations, on an accepted evaluation, with admm_history() and anderson_history() of one length.
    MEASURED on the MI355X: plain 60, accelerated 22 / 25 / 25, decided on the device."""
    _, hp = plain_history(name, 80)
    need = np.maximum(hp["primal"] / np.maximum(hp["wz"], hp["wdx"]), hp["dz"] / hp["wz"])
    tol = float(need[59]) * (1.0 + 1e-9)
    _, _, sp = run_steps(name, settings=dict(admm_iters=100), admm_tol=tol)
    n_plain = sp.admm_stop()["last_iters"]; sp.close()
    assert 40 <= n_plain <= 80, n_plain
    _, _, sa = run_steps(name, settings=dict(admm_iters=100), admm_tol=tol, anderson=3)
    st = sa.admm_stop(); hm, ha = sa.admm_history(), sa.anderson_history()
    sa.close()
    print("anderson admm_tol  %-14s tol %.3e: plain %d iterations, accelerated %d (on device %d)" % (name, tol, n_plain, st["last_iters"], st["on_device"]))
    assert len(hm["primal"]) == len(ha["accepted"]) == st["last_iters"]
    assert ha["accepted"][-1] == 1
    assert st["last_iters"] <= (2 * n_plain) // 3, (st["last_iters"], n_plain)


# ---------------------------------------------------------------- 5. the safeguard --------------------------------------------
@pytest.mark.gpu
def test_safeguard():
    """Cloth, 60 iterations, window 3: at least one rejection; an accepted accelerated evaluation never has a larger |F| than the
    accepted evaluation before it; the evaluation after a rejection starts from a plain state with an empty ring; and a step cut to
    end ON a rejected evaluation returns the solve output of the last accepted one -- the bytes of the step that ends one iteration
    earlier.  MEASURED on the MI355X: 5 rejections, at evaluations 38, 42, 47, 50, 56."""
    _, _, s = run_steps("cloth", settings=dict(admm_iters=60), anderson=3)
    h = s.anderson_history(); s.close()
    acc, accel, ent, res, th = h["accepted"], h["accelerated"], h["entries"], h["resid"], h["theta"]
    rej = np.nonzero(acc == 0)[0]
    print("anderson safeguard  cloth, 60 iterations, window 3: %d rejections at %s" % (rej.size, list(rej)))
    assert rej.size >= 1
    last = None
    for k in range(60):
        if acc[k]:
            if accel[k] and last is not None:
                assert res[k] <= last, (k, res[k], last)
            last = res[k]
        else:
            assert accel[k] == 1 and ent[k] == 0 and np.all(th[k] == 0.0)
            if k + 1 < 60:
                assert acc[k + 1] == 1 and accel[k + 1] == 0 and ent[k + 1] == 1 and np.all(th[k + 1] == 0.0)
    r = int(rej[0])
    assert r >= 2 and acc[r - 1] == 1
    xa, va, sa = run_steps("cloth", settings=dict(admm_iters=r + 1), anderson=3)
    ha = sa.anderson_history(); sa.close()
    assert ha["accepted"][-1] == 0      # (the shorter step does end on the rejected evaluation)
    xb, vb, sb = run_steps("cloth", settings=dict(admm_iters=r), anderson=3); sb.close()
    assert xa.tobytes() == xb.tobytes() and va.tobytes() == vb.tobytes()


# ---------------------------------------------------------------- 6. refusals --------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    """Every refused case raises AdmmHipError with code -1 and leaves the setting as it was; a step after set_anderson(0) on an
    accelerated context runs as a plain one."""
    def refused(s, window, word):
        with pytest.raises(pkg.AdmmHipError) as e:
            s.set_anderson(window)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
        assert s._settings.anderson == 0

    s = scenes.cube_scene(3, NH, linsolver=0).make_solver(world_size=2, rank=0)
    refused(s, 3, "single-GPU"); s.set_anderson(0); s.close()
    s = scenes.cloth_scene(6, floor=-0.3, linsolver=2).make_solver()
    refused(s, 3, "colliders"); s.close()
    s = scenes.two_blocks_scene().make_solver()
    refused(s, 3, "colliders"); s.close()
    for ls in (1, 2):
        s = scenes.cube_scene(3, NH, linsolver=ls).make_solver()
        refused(s, 3, "linsolver"); s.set_anderson(0); s.close()
    with pytest.raises(pkg.AdmmHipError):
        scenes.cube_scene(3, NH, linsolver=1).make_solver(anderson=3)
    xp, vp, sp = run_steps("cantilever162")
    s = make_scene("cantilever162").make_solver(**GPU_KW)
    x_rest = s.m_x.copy()
    for w in (-1, 9):
        refused(s, w, "window")
    s.step()
    assert s.anderson_history()["accepted"].size == 0
    assert s.m_x.tobytes() == xp.tobytes() and s.m_v.tobytes() == vp.tobytes()      # (the refusals left a plain context)
    # accelerated, then off again: the same state stepped by both contexts
    s.set_anderson(3); s.m_x = x_rest.copy(); s.m_v = np.zeros_like(x_rest); s.step()
    assert s.anderson_history()["accepted"].size == 10 and bbox_err(s.m_x, xp) > 0.0
    s.set_anderson(0)
    for q in (s, sp):
        q.m_x = x_rest.copy(); q.m_v = np.zeros_like(x_rest); q.step()
    assert s.anderson_history()["accepted"].size == 0
    d = bbox_err(s.m_x, sp.m_x)
    print("anderson off again: against the plain context %.3e of the bounding box" % d)
    assert d <= 1e-9      # (the two contexts' PCGs start from different recycled subspaces: pcg_tol 1e-12, not bits)
    s.close(); sp.close()


# ---------------------------------------------------------------- 7. reproducible ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_bit_reproducible(name):
    """The same accelerated run twice (three steps of 20 iterations, window 3): identical bytes of the state and of anderson_history()."""
    runs = []
    for _ in range(2):
        x, v, s = run_steps(name, 3, settings=dict(admm_iters=20), anderson=3)
        h = s.anderson_history(); s.close()
        runs.append((x, v, h))
    (xa, va, ha), (xb, vb, hb) = runs
    assert xa.tobytes() == xb.tobytes() and va.tobytes() == vb.tobytes()
    for k in ha:
        assert ha[k].tobytes() == hb[k].tobytes(), k
    assert np.any(ha["accelerated"] == 1)
