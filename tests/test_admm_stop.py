"""Early exit of a step's ADMM loop on the monitor's residuals (admm_hip_set_admm_stop; csrc/monitor.hpp: admm_stop_test, k_mon_decide),
skipped on the device: the criterion against a numpy restatement, the stop against the CPU oracle's trace, the bits against a step of
the same fixed count, the host-decided variant (ADMM_HIP_STOP_HOST=1) against the device-skipped one."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi
from admm_elastic_amd.solver import RuntimeData, Settings, Solver
from test_cpp_api import _build_exe

NH = pkg.TET_NEOHOOKEAN
PCG = dict(pcg_tol=1e-12, pcg_max_iters=500)
GAP = 1.02      # the tolerance sits at least 2 % away from the criterion of the iterations on either side of it


# ---------------------------------------------------------------- the criterion in numpy -----------------------------------
def crit_of(primal, dz, wz, wdx):
    """crit[s] = max(primal / max(wz, wdx), dz / wz)"""
    return np.maximum(primal / np.maximum(wz, wdx), dz / wz)


def stop_np(rec, tol):
    """the stop test on one record (primal, dz, wz, wdx, ...): product form, <=; a NaN or tol = 0 never stops"""
    primal, dz, wz, wdx = (float(v) for v in rec[:4])
    if not tol > 0.0 or any(np.isnan(v) for v in (primal, dz, wz, wdx)):
        return False
    return bool(primal <= tol * max(wz, wdx) and dz <= tol * wz)


def geometric_tol(crit, k):
    """t between crit[k - 1] and crit[k]; asserts (a condition on the INPUT) that iteration k is the first to meet it, with GAP to spare"""
    t = float(np.sqrt(crit[k - 1] * crit[k]))
    assert (crit[:k] >= GAP * t).all() and crit[k] <= t / GAP, (k, t, crit)
    return t


def first_stop(crit, tol, min_iters=1):
    """iterations a step with this criterion trace executes"""
    for s, c in enumerate(crit):
        if s + 1 >= min_iters and c <= tol:
            return s + 1
    return len(crit)


def _host_test(rec, tol):
    r = np.zeros(8); r[:len(rec)] = rec
    return capi.lib().admm_host_admm_stop_test(capi.dptr(r), float(tol))


# ---------------------------------------------------------------- CPU ------------------------------------------------------
def test_admm_stop_symbols_and_settings():
    """The entry points exist in libadmm_hip.so with the documented signatures and declarations; the feature is off by default."""
    L = capi.lib()
    sig = {name: (res, args) for name, res, args in capi.SYMBOLS}
    dp, ip = capi.c_double_p, capi.c_int_p
    assert sig["admm_hip_set_admm_stop"] == (C.c_int, [C.c_void_p, C.c_double, C.c_int32])
    assert sig["admm_hip_get_admm_stop"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double), ip, ip, ip])
    assert sig["admm_host_admm_stop_test"] == (C.c_int, [dp, C.c_double])
    for name in ("admm_hip_set_admm_stop", "admm_hip_get_admm_stop", "admm_host_admm_stop_test"):
        assert getattr(L, name) is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    for decl in ("int admm_hip_set_admm_stop(admm_hip_ctx *ctx, double tol, int32_t min_iters);",
                 "int admm_hip_get_admm_stop(admm_hip_ctx *ctx, double *tol, int32_t *min_iters, int32_t *last_iters, int32_t *on_device);",
                 "int admm_host_admm_stop_test(const double *rec8, double tol);"):
        assert decl in hdr, decl
    assert "ADMM_HIP_STOP_HOST" in hdr      # the header says which paths synchronise
    # NULL contexts are refused, not dereferenced
    assert L.admm_hip_set_admm_stop(None, 1e-6, 1) == -1
    assert L.admm_hip_get_admm_stop(None, None, None, None, None) == -1
    st = Settings()
    assert st.admm_tol == 0.0 and st.admm_min_iters == 1
    assert Settings(admm_tol=1e-6, admm_min_iters=3).admm_min_iters == 3
    assert RuntimeData().admm_iters == 0
    assert list(inspect.signature(Solver.set_admm_stop).parameters) == ["self", "tol", "min_iters"]
    assert inspect.signature(Solver.set_admm_stop).parameters["min_iters"].default == 1
    assert callable(Solver.admm_stop)
    with open(os.path.join(os.path.dirname(capi.__file__), "host", "include", "Solver.hpp")) as fh:
        hpp = fh.read()
    for word in ("double admm_tol;", "int admm_min_iters;", "int admm_iters;", "void set_admm_stop(double tol, int min_iters = 1);"):
        assert word in hpp, word


def test_admm_stop_test_matches_numpy():
    """admm_host_admm_stop_test (the inline the device decision calls) against the numpy restatement: records strictly inside the bound,
    exactly on it and just outside it, on either of the two conditions and with either of wz, wdx the larger; all-zero records stop;
    a NaN in any of the four slots never stops; tol = 0 never stops."""
    tol = 2.0 ** -20      # (a power of two: tol * wz is exact, so "exactly on the bound" is exact)
    up = lambda v: float(np.nextafter(v, np.inf))
    cases = []
    for wz, wdx in ((4.0, 3.0), (3.0, 4.0), (4.0, 4.0)):
        big = max(wz, wdx)
        inside = (0.5 * tol * big, 0.5 * tol * wz)
        on = (tol * big, tol * wz)
        cases += [(inside[0], inside[1], wz, wdx, True), (on[0], on[1], wz, wdx, True),
                  (up(on[0]), inside[1], wz, wdx, False), (inside[0], up(on[1]), wz, wdx, False),
                  (on[0], inside[1], wz, wdx, True), (inside[0], on[1], wz, wdx, True)]
    # dz is held against wz alone: a dz that only max(wz, wdx) would admit does not stop
    cases.append((0.0, tol * 3.5, 3.0, 4.0, False))
    for primal, dz, wz, wdx, expect in cases:
        rec = (primal, dz, wz, wdx)
        assert stop_np(rec, tol) == expect, rec
        assert _host_test(rec, tol) == int(expect), rec
        assert _host_test(rec, 0.0) == 0, rec
    assert _host_test((0.0, 0.0, 0.0, 0.0), tol) == 1 and stop_np((0.0, 0.0, 0.0, 0.0), tol)
    assert _host_test((0.0, 0.0, 0.0, 0.0), 0.0) == 0
    for slot in range(4):
        for base in ((0.0, 0.0, 0.0, 0.0), (1e-9, 1e-9, 4.0, 3.0)):
            rec = list(base); rec[slot] = float("nan")
            assert _host_test(rec, tol) == 0 and not stop_np(rec, tol), rec
            assert _host_test(rec, 1e300) == 0, rec
    # slots 4..7 (energies) are not read
    assert _host_test((1e-9, 1e-9, 4.0, 3.0, float("nan"), float("nan"), float("nan"), float("nan")), tol) == 1
    assert capi.lib().admm_host_admm_stop_test(None, tol) == 0


# ---------------------------------------------------------------- GPU: helpers ---------------------------------------------
def _crit_of_history(h):
    return crit_of(h["primal"], h["dz"], h["wz"], h["wdx"])


def _oracle_crit(o):
    """one frame of the oracle with its trace (the recipe of test_energy_monitor._oracle_history) -> crit per ADMM iteration"""
    x0 = o.x.copy()
    tr = []
    o.step(trace=tr)
    zprev = o.D @ x0
    primal, dz, wz, wdx = [], [], [], []
    for z, u, b, x in tr:
        primal.append(np.linalg.norm(o.W * (o.D @ x - z)))
        dz.append(np.linalg.norm(o.W * (z - zprev)))
        wz.append(np.linalg.norm(o.W * z))
        wdx.append(np.linalg.norm(o.W * (o.D @ x)))
        zprev = z
    return crit_of(np.array(primal), np.array(dz), np.array(wz), np.array(wdx))


def _frame(s, admm_iters=None):
    """one ordinary stream-ordered step on the device-resident state, with statistics"""
    s.step_device(stats=True, admm_iters=admm_iters)
    return s.runtime_data()


def _records(s):
    h = s.admm_history()
    return np.stack([h[k] for k in ("primal", "dz", "wz", "wdx")], axis=1)


def _scene4(name):
    if name == "gs5":
        return scenes.cube_scene(5, NH, linsolver=1), {}
    if name == "mixed12":
        return scenes.mixed_cube_scene(12, admm_iters=20), PCG
    return scenes.blob_scene(30, admm_iters=20), PCG


FRAMES4 = 4
UZ_FRAMES = 6
_cache = {}


def _plain_crit(name):
    """crit per frame of a plain monitor = 1 run (computed once per scene, shared, never changed)"""
    if ("plain", name) not in _cache:
        sc, kw = _scene4(name)
        s = sc.make_solver(monitor=1, **kw)
        s.upload()
        out = []
        for _ in range(FRAMES4):
            _frame(s)
            out.append(_crit_of_history(s.admm_history()))
        s.close()
        _cache[("plain", name)] = out
    return _cache[("plain", name)]


def _candidate_tols(crits):
    """Tolerances by the geometric-mean rule from the plain run's own history for which the PLAIN frames would stop both below and above
    five iterations, each at least GAP away from every criterion value of that history; the roomiest first."""
    allc = np.concatenate(crits)
    allc = allc[allc > 0.0]
    out = []
    for c in crits:
        for k in range(1, len(c)):
            if not (c[k] > 0.0 and c[k - 1] > c[k]):
                continue
            t = float(np.sqrt(c[k - 1] * c[k]))
            counts = [first_stop(cc, t) for cc in crits]
            room = float(np.min(np.abs(np.log(allc / t))))
            if min(counts) < 5 < max(counts) and room >= np.log(GAP):
                out.append((room, t))
    assert out, "no tolerance lets the plain frames stop below and above five iterations: %s" % (crits,)
    return [t for _, t in sorted(out, reverse=True)]


def _early_frames(name, tol, host):
    sc, kw = _scene4(name)
    old = os.environ.get("ADMM_HIP_STOP_HOST")
    if host:
        os.environ["ADMM_HIP_STOP_HOST"] = "1"
    try:
        s = sc.make_solver(admm_tol=tol, **kw)
    finally:
        if host:
            if old is None: del os.environ["ADMM_HIP_STOP_HOST"]
            else: os.environ["ADMM_HIP_STOP_HOST"] = old
    s.upload()
    t0 = s.solve_totals()
    counts, recs, on_dev, rts = [], [], [], []
    for _ in range(FRAMES4):
        rt = _frame(s)
        st = s.admm_stop()
        assert st["last_iters"] == rt.admm_iters
        counts.append(st["last_iters"]); on_dev.append(st["on_device"]); recs.append(_records(s)); rts.append(rt)
    s.download()
    out = dict(tol=tol, counts=counts, x=s.m_x.copy(), v=s.m_v.copy(), recs=recs, on_dev=on_dev, rts=rts,
               totals=(t0, s.solve_totals()), admm_iters=sc.settings["admm_iters"])
    s.close()
    return out


def _early_run(name, host=False):
    """FRAMES4 frames with early exit -> counts, states, records, on_device per frame (computed once per scene and variant).  Early exit
    changes the trajectory from the second frame on, so the plain history only PROPOSES tolerances: the first candidate (at most six are
    tried) whose early-exit frames really stop both below and above five iterations is the scene's tolerance, for both variants."""
    key = ("early", name, host)
    if key not in _cache:
        if ("tol", name) not in _cache:
            crits = _plain_crit(name)
            for f, c in enumerate(crits):
                print("%s plain frame %d crit %s" % (name, f, np.array2string(c, precision=3)))
            tried = []
            for tol in _candidate_tols(crits)[:6]:
                run = _early_frames(name, tol, False)
                tried.append((tol, run["counts"]))
                if min(run["counts"]) < 5 < max(run["counts"]):
                    _cache[("tol", name)] = tol
                    _cache[("early", name, False)] = run
                    break
            print("%s: tolerances tried %s" % (name, tried))
            assert ("tol", name) in _cache, "no candidate tolerance made the early-exit frames stop below and above five iterations: %s" % (tried,)
        if key not in _cache:
            _cache[key] = _early_frames(name, _cache[("tol", name)], host)
    return _cache[key]


def _fixed_run(name, counts):
    """the same frames without the feature, monitor = 1, step_device(admm_iters = n_f)"""
    sc, kw = _scene4(name)
    s = sc.make_solver(monitor=1, **kw)
    s.upload()
    recs, rts = [], []
    for n in counts:
        rts.append(_frame(s, admm_iters=n))
        recs.append(_records(s))
    s.download()
    out = dict(x=s.m_x.copy(), v=s.m_v.copy(), recs=recs, rts=rts)
    s.close()
    return out


def _fixed_pair(name, counts):
    key = ("fixed", name, tuple(counts))
    if key not in _cache:
        _cache[key] = (_fixed_run(name, counts), _fixed_run(name, counts)) if name != "gs5" else (_fixed_run(name, counts),) * 2
    return _cache[key]


def _dist(a, b):
    return max(np.abs(a["x"] - b["x"]).max(), np.abs(a["v"] - b["v"]).max())


def _assert_same_state(name, run, fa, fb, what):
    if name == "gs5":
        assert np.array_equal(run["x"], fa["x"]) and np.array_equal(run["v"], fa["v"]), what
        return
    plain, mine = _dist(fa, fb), _dist(run, fa)
    print("%s %s: fixed-count runs differ by %.3e, the early-exit run by %.3e" % (name, what, plain, mine))
    if plain == 0.0:
        assert mine == 0.0, what
    else:
        assert mine <= 4.0 * plain, what


# ---------------------------------------------------------------- GPU ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed4", "nh5", "cloth6"])
def test_stops_where_the_oracle_says(name):
    """Three frames.  From the oracle's 12-iteration trace of the frame: k = 5, t = sqrt(crit[4] crit[5]), asserted on the input:
    crit[s] >= 1.02 t for s < 5 and crit[5] <= t / 1.02.  With tol = t the step executes k + 1 = 6 iterations (admm_stop(), the history
    and RuntimeData agree), and m_x matches the oracle stepped again from the frame's start with admm_iters = 6 to 1e-7 of the
    bounding box -- the bar the monitor test's scenes meet for whole steps."""
    sc = (scenes.mixed_cube_scene(4, admm_iters=12) if name == "mixed4" else
          scenes.cube_scene(5, NH, admm_iters=12) if name == "nh5" else scenes.cloth_scene(6, admm_iters=12))
    s = sc.make_solver(**PCG)
    o = sc.make_oracle(mode=1)
    k = 5
    for frame in range(3):
        x0, v0 = o.x.copy(), o.v.copy()
        crit = _oracle_crit(o)
        assert len(crit) == 12
        t = geometric_tol(crit, k)
        o.x, o.v = x0.copy(), v0.copy()      # rewind, and step again with the count the trace predicts
        o.admm_iters = k + 1
        o.step()
        o.admm_iters = 12
        s.set_admm_stop(t)
        s.step()
        st = s.admm_stop()
        h = s.admm_history()
        print("%s frame %d: tol %.4e, oracle crit %s, executed %d, device crit %s" % (name, frame, t, crit[:7], st["last_iters"], _crit_of_history(h)))
        assert st["last_iters"] == k + 1 and st["tol"] == t and st["min_iters"] == 1
        assert all(len(h[key]) == k + 1 for key in h)
        assert s.runtime_data().admm_iters == k + 1
        err = scenes.rel_err(s.m_x, o.x, sc.x)
        print("%s frame %d: m_x against the oracle at %d iterations: %.3e of the bounding box" % (name, frame, k + 1, err))
        assert err <= 1e-7, err
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gs5", "mixed12", "blob30"])
def test_same_bits_as_a_fixed_count(name):
    """Four frames with early exit against a context without the feature (monitor = 1) that runs step_device(admm_iters = n_f) with
    the counts the first reported.  tol: the geometric-mean rule on a plain monitor = 1 run's own history, chosen so that one frame
    stops below five iterations and one above (the recycled history slots).  GS: m_x, m_v bit-identical.  PCG: bit-identical if two
    fixed-count runs are, else within 4 x their distance.  The records are bit-identical to the fixed-count run's."""
    run = _early_run(name)
    counts = run["counts"]
    print("%s: tol %.4e, executed %s of %d, on_device %s" % (name, run["tol"], counts, run["admm_iters"], run["on_dev"]))
    assert min(counts) < 5 < max(counts), counts
    assert all(d == 1 for d in run["on_dev"]), run["on_dev"]
    fa, fb = _fixed_pair(name, counts)
    _assert_same_state(name, run, fa, fb, "device")
    for f in range(FRAMES4):
        assert run["recs"][f].shape == (counts[f], 4)
        assert np.array_equal(run["recs"][f], fa["recs"][f]), (f, np.abs(run["recs"][f] - fa["recs"][f]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gs5", "mixed12", "blob30"])
def test_host_and_device_variants_agree(name):
    """The same early-exit frames under ADMM_HIP_STOP_HOST=1: equal counts, states as in the fixed-count test, on_device 1 in one run
    and 0 in the other."""
    dev, host = _early_run(name), _early_run(name, host=True)
    print("%s: device %s, host %s" % (name, dev["counts"], host["counts"]))
    assert host["counts"] == dev["counts"]
    assert all(d == 1 for d in dev["on_dev"]) and all(d == 0 for d in host["on_dev"])
    fa, fb = _fixed_pair(name, dev["counts"])
    _assert_same_state(name, host, fa, fb, "host")
    for f in range(FRAMES4):
        assert np.array_equal(host["recs"][f], fa["recs"][f]), f


@pytest.mark.gpu
def test_body_at_rest_stops_after_one_iteration():
    """cube_scene(3, NH, gravity = 0, admm_iters = 12), tol 1e-12: one iteration; with min_iters = 3: three.  The state stays the start
    state to 1e-13."""
    sc = scenes.cube_scene(3, NH, gravity=0.0, admm_iters=12)
    s = sc.make_solver(admm_tol=1e-12, **PCG)
    s.step()
    st = s.admm_stop()
    h = s.admm_history()
    print("at rest: executed %d, crit %s" % (st["last_iters"], _crit_of_history(h)))
    assert st["last_iters"] == 1 and len(h["primal"]) == 1 and s.runtime_data().admm_iters == 1
    s.set_admm_stop(1e-12, min_iters=3)
    s.step()
    st = s.admm_stop()
    assert st["last_iters"] == 3 and st["min_iters"] == 3 and len(s.admm_history()["primal"]) == 3
    assert np.abs(s.m_x - sc.x.ravel()).max() <= 1e-13 and np.abs(s.m_v).max() <= 1e-13
    s.close()


@pytest.mark.gpu
def test_off_is_off():
    """tol = 0 after tol > 0 on a live context: the next step runs all iterations on the hot instance of k_pcg2 again; contexts that
    never set the feature match each other as before (GS: bit for bit)."""
    sc = scenes.cube_scene(5, NH, admm_iters=12)      # (crit ~ 2e-2, 1.2e-5, 4.2e-6, ...: 1e-5 ends the frame after three iterations)
    s = sc.make_solver(admm_tol=1e-5, **PCG)
    s.upload()
    _frame(s)
    st = s.admm_stop()
    assert st["last_iters"] < 12 and st["on_device"] == 1
    assert s.pcg_instances()["last"] == "generic"      # (the instance that reads the stop word)
    assert s.pcg_instances()["generic"] == st["last_iters"] and s.persistent_launches()["pcg"] == st["last_iters"]      # executed solves, not launches
    before_i, before_p = s.pcg_instances(), s.persistent_launches()
    s.set_admm_stop(0.0)
    rt = _frame(s)
    st = s.admm_stop()
    assert st["tol"] == 0.0 and st["last_iters"] == 12 and st["on_device"] == 0 and rt.admm_iters == 12
    after_i, after_p = s.pcg_instances(), s.persistent_launches()
    assert after_i["last"] == "hot" and after_i["hot"] - before_i["hot"] == 12 and after_i["generic"] == before_i["generic"]
    assert after_p["pcg"] - before_p["pcg"] == 12
    assert all(len(v) == 0 for v in s.admm_history().values())      # (the monitor was only on for the early exit)
    s.close()
    sg = scenes.cube_scene(5, NH, linsolver=1)
    outs = []
    for _ in range(2):
        g = sg.make_solver()
        for _ in range(3):
            g.step()
        assert g.admm_stop()["last_iters"] == sg.settings["admm_iters"] and g.admm_stop()["on_device"] == 0
        outs.append((g.m_x.copy(), g.m_v.copy()))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_skipped_work_is_skipped():
    """After the early-exited PCG frames solve_totals() grew by the executed solves only, no solve was left unconverged, and
    pcg_iters_per_solve has the executed length and the fixed-count run's values."""
    name = "mixed12"
    run = _early_run(name)
    counts = run["counts"]
    (s0, c0, i0), (s1, c1, i1) = run["totals"]
    assert s1 - s0 == sum(counts) and c1 - c0 == sum(counts), (run["totals"], counts)
    fa, _ = _fixed_pair(name, counts)
    iters = 0
    for f in range(FRAMES4):
        rt, rf = run["rts"][f], fa["rts"][f]
        assert rt.unconverged_solves == 0 and rt.admm_iters == counts[f]
        assert len(rt.pcg_iters_per_solve) == counts[f]
        assert list(rt.pcg_iters_per_solve) == list(rf.pcg_iters_per_solve), (f, rt.pcg_iters_per_solve, rf.pcg_iters_per_solve)
        assert rt.inner_iters == rf.inner_iters == sum(rt.pcg_iters_per_solve)
        iters += rt.inner_iters
    assert i1 - i0 == iters


@pytest.mark.gpu
def test_uzawa_over_a_floor_decides_on_the_host():
    """cube_scene(6, NH, pin_face = False, linsolver = 2, size = 0.5) over a Floor: the host variant (on_device 0) stops, and the state
    matches the run of the same fixed counts to 1e-10."""
    def make(**kw):
        sc = scenes.cube_scene(6, NH, pin_face=False, linsolver=2, size=0.5, admm_iters=12)
        sc.pins.clear()
        sc.obstacles.append((0, [-0.0217, 0.0, 0.0, 0.0]))      # (touched from the fourth frame on)
        return sc.make_solver(**dict(PCG, **kw))
    p = make(monitor=1)
    p.upload()
    crits = []
    for _ in range(UZ_FRAMES):
        _frame(p)
        crits.append(_crit_of_history(p.admm_history()))
    p.close()
    # the tolerance: between two consecutive criterion values of a plain frame, GAP away from EVERY criterion value of the plain run (in
    # free fall the criterion sits at round-off, ~2e-16: only the frames in contact offer such a pair); the roomiest pair
    allc = np.concatenate(crits)
    cands = []
    for c in crits:
        for k in range(2, len(c)):
            if c[k - 1] > c[k] > 1e-14:
                t = float(np.sqrt(c[k - 1] * c[k]))
                cands.append((float(np.min(np.abs(np.log(allc / t)))), t))
    assert cands, crits
    room, tol = max(cands)
    assert room >= np.log(GAP), (room, tol)
    s = make(admm_tol=tol)
    s.upload()
    counts = []
    for _ in range(UZ_FRAMES):
        _frame(s)
        st = s.admm_stop()
        assert st["on_device"] == 0
        counts.append(st["last_iters"])
    s.download()
    assert s.m_x[1::3].min() < -0.01, "scene meant to reach the floor"
    print("uzawa + floor: tol %.4e, executed %s of 12; plain crit %s" % (tol, counts, [c[[1, 5, 11]] for c in crits]))
    assert min(counts) < 12 and max(counts) > 1      # (stops, and not only in free fall)
    f = make(monitor=1)
    f.upload()
    for n in counts:
        _frame(f, admm_iters=n)
    f.download()
    d = max(np.abs(s.m_x - f.m_x).max(), np.abs(s.m_v - f.m_v).max())
    print("uzawa + floor: early exit against the fixed counts: %.3e" % d)
    assert d <= 1e-10, d
    s.close(); f.close()


@pytest.mark.gpu
def test_admm_stop_refuses_multi_rank_contexts():
    sc = scenes.cube_scene(3, NH)
    s = sc.make_solver(world_size=2, rank=0)
    with pytest.raises(pkg.AdmmHipError):
        s.set_admm_stop(1e-6)
    with pytest.raises(pkg.AdmmHipError):
        s.set_monitor(1)
    s.set_admm_stop(0.0)      # (off is always accepted)
    with pytest.raises(pkg.AdmmHipError):
        s.set_admm_stop(-1.0)
    with pytest.raises(pkg.AdmmHipError):
        s.set_admm_stop(float("nan"))
    with pytest.raises(pkg.AdmmHipError):
        s.set_admm_stop(1e-6, min_iters=0)
    s.close()


@pytest.mark.gpu
def test_cpp_admm_stop():
    """tests/cpp/test_admm_stop.cpp: -tol parsed by Settings::parse_args; on a pinned cube at rest runtime_data().admm_iters and
    admm_history() stay below Settings::admm_iters."""
    exe = _build_exe("test_admm_stop")
    r = subprocess.run([exe, "-tol", "1e-12", "-it", "12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
