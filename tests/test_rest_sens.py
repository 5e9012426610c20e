"""Gradients in the rest shape and in the held vertices (csrc/adjoint.hpp: k_rest_sens, k_adj_held): rest_sensitivity() and
step_adjoint(rest=True, held=True), against numpy.

THE REFERENCE of rest_sensitivity is per element, on the one-element descriptions as test_adjoint.element_reference builds them: P from
test_forces.tet_forces, T = H[A] from test_stiffness.numpy_stiffness on a's corners (its result is vol T Binv^T corner by corner, so
T = G Dm^T / vol), then
    Gs = -vol [ (P : A) I - F^T T - A^T P ],   rest corner m + 1 gets column m of Gs Binv^T, corner 0 minus their sum.
It is itself held against central differences in `rest` of numpy's a . tet_forces(flat, rest +- h e, x) on the 6-tet cube (CPU).
  bar     |device - reference|_v <= 1e-9 scale_v,  scale_v = sum_{e at v} vol_e |Binv_e|_F^2 (|P_e| + c_e |F_e|) sum_c |a_c|,  c_e the largest
          tangent coefficient of the element: the magnitudes of the summed terms, never the result (the convention of test_stiffness.py).
  held    the dense numpy value g_held - (K lam)_held with test_adjoint.numpy_K and numpy's own lam; bar 1e-6 kappa of its norm, as
          test_adjoint.test_step_adjoint_against_the_dense_numpy_adjoint.
  the derivative   central differences of the whole device pipeline, |dev - q| <= 2 |numpy - q| + 4.73e-12 |q| (test_adjoint.py).

Meshes and states: those of test_newton.py and test_adjoint.py, and kuhn_cube(4) (384 tets: one full chunk and one half chunk)."""
import ctypes as C
import functools

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Lame, Solver, Settings
from test_adjoint import NH, R_ASSERT, TIGHT, _check_derivative, _loss_vectors, _quotients, _start, numpy_K, numpy_adjoint, polished
from test_adjoint_cpp import _cube48
from test_energy_monitor import cloth_with_hinges
from test_forces import SPLINE_KINDS, table_fgh, tet_F, tet_forces
from test_newton import _empty, compressed_state, open_case
from test_stiffness import numpy_stiffness

gpu = pytest.mark.gpu
BAR = 1e-9


# ---------------------------------------------------------------- the numpy reference ----------------------------------------------
def numpy_rest_sens(flat, rest, x, a, tab=None):
    """-> d(a . f)/dX [nv, 3] and scale [nv], element by element from tet_forces (P) and numpy_stiffness (T) on one-element descriptions"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    dfgh = table_fgh(tab)[1] if tab is not None else None
    e = _empty(flat)
    out = np.zeros(x.shape); scale = np.zeros(len(x))
    for i, t in enumerate(flat["tet_idx"]):
        sub = dict(e, tet_idx=np.array([[0, 1, 2, 3]], np.int32))
        for key in ("tet_kind", "tet_mu", "tet_lambda", "tet_k", "tet_kappa"):
            sub[key] = flat[key][i:i + 1]
        X, xe, ae = rest[t], x[t], a[t]
        P = tet_forces(sub, X, xe, dfgh)[2]["P"][0]
        Dm = np.stack([X[1] - X[0], X[2] - X[0], X[3] - X[0]], axis=1)
        B = np.linalg.inv(Dm)
        vol = np.linalg.det(Dm) / 6.0
        F = np.stack([xe[1] - xe[0], xe[2] - xe[0], xe[3] - xe[0]], axis=1) @ B
        A = np.stack([ae[1] - ae[0], ae[2] - ae[0], ae[3] - ae[0]], axis=1) @ B
        Kd, sc = numpy_stiffness(sub, X, xe, ae[None], tab=tab)
        T = np.stack([Kd[0, 1], Kd[0, 2], Kd[0, 3]], axis=1) @ Dm.T / vol
        an = np.linalg.norm(ae, axis=1)
        ce = sc[0, 0] / (vol * np.sum(B * B) * an.max()) if an.max() > 0.0 else 0.0
        H = -vol * (np.sum(P * A) * np.eye(3) - F.T @ T - A.T @ P) @ B.T
        out[t[1]] += H[:, 0]; out[t[2]] += H[:, 1]; out[t[3]] += H[:, 2]; out[t[0]] -= H.sum(axis=1)
        scale[t] += vol * np.sum(B * B) * (np.linalg.norm(P) + ce * np.linalg.norm(F)) * an.sum()
    return out, scale


def test_reference_is_the_derivative_of_the_numpy_forces():
    """CPU: on the 6-tet Neo-Hookean cube at its compressed state, numpy_rest_sens against central differences in every rest coordinate
    of a . tet_forces(flat, rest +- h e, x); steps 2e-3 2^-i: the largest h (i >= 1) at which the quotient changes less from h to h / 2
    than from 2h to h; |reference - q(h / 2)| <= 4 |q(h) - q(h / 2)| + 1e-9 scale_v.  Measured: 5.5e-2 of the bar (the quotient's own
    error, (q(h) - q(h / 2)) / 3, is 8.3e-2 of it)."""
    verts, tets = meshes.kuhn_cube(1)
    lame = Lame.soft_rubber()
    s = Solver()
    s.add_nodes(verts, np.repeat(meshes.lumped_masses_tets(verts, tets), 3))
    s.add_tets(verts, tets, lame, NH)
    s.make_desc(Settings())
    flat = s.flatten()
    x = verts * np.array([0.75, 0.6, 0.8]); x[7] = x[7] + np.array([-0.9, -0.1, 0.0])      # (test_newton.case("tet6"): inverts tets)
    a = np.random.default_rng(97).standard_normal(x.shape)
    ref, scale = numpy_rest_sens(flat, verts, x, a)
    fn = lambda X: float(np.sum(a * tet_forces(flat, X, x)[0]))
    hs = [2e-3 * 0.5 ** i for i in range(4)]
    worst = 0.0
    for v in range(len(verts)):
        for j in range(3):
            q = []
            for h in hs:
                Xp, Xm = verts.copy(), verts.copy()
                Xp[v, j] += h; Xm[v, j] -= h
                q.append((fn(Xp) - fn(Xm)) / (2.0 * h))
            i = next(i for i in (1, 2) if abs(q[i] - q[i + 1]) < abs(q[i - 1] - q[i]))
            bar = 4.0 * abs(q[i] - q[i + 1]) + 1e-9 * scale[v]
            worst = max(worst, abs(ref[v, j] - q[i + 1]) / bar)
    print("numpy_rest_sens against central differences in rest: worst |reference - q| / bar = %.3e" % worst)
    assert worst <= 1.0, worst


def ratio(dev, ref, scale):
    return (np.linalg.norm(dev - ref, axis=1) / (BAR * scale)).max()


@functools.lru_cache(None)
def cube384(split):
    """kuhn_cube(4): 384 Neo-Hookean tets in one add_tets call, or two calls of 192 (StVK first, Neo-Hookean second: the device sorts the
    Neo-Hookean group in front) -> the description, the rest positions, the compressed state"""
    verts, tets = meshes.kuhn_cube(4)
    return verts, tets, compressed_state(verts, 4)


def make384(split):
    verts, tets, x = cube384(split)
    lame = Lame.soft_rubber()
    s = Solver()
    s.add_nodes(verts, np.repeat(meshes.lumped_masses_tets(verts, tets), 3))
    if split:
        s.add_tets(verts, tets[:192], lame, pkg.TET_STVK)
        s.add_tets(verts, tets[192:], lame, NH)
    else:
        s.add_tets(verts, tets, lame, NH)
    assert s.initialize(Settings())
    return s, s.flatten(), verts, x


# ---------------------------------------------------------------- 1: the device against the numpy reference -------------------------
CASES = ["tet1", "tet6", "cube384", "cube384split", "mixed162", "mixed750"] + ["kind%d" % k for k in SPLINE_KINDS] + ["mixed162rest"]


@gpu
@pytest.mark.parametrize("name", CASES)
def test_rest_sensitivity_against_numpy(name):
    """One random a at the case's state (compressed, with inverted tets; mixed162rest: exactly at rest): every vertex within 1e-9 scale_v
    of the reference; the sum over the vertices within 1e-12 sum_v scale_v of 0 (a translation of the rest shape changes nothing); a
    second call has the bits of the first.

    Measured on an MI355X, the worst |device - numpy|_v / (1e-9 scale_v) and |sum_v| / (1e-12 sum_v scale_v): tet1 1.2e-7 / 2.8e-7,
    tet6 1.3e-8 / 2.4e-8, cube384 3.3e-8 / 6.0e-8, cube384split 6.4e-8 / 2.8e-7, mixed162 9.5e-8 / 2.1e-7, mixed750 4.9e-8 / 1.6e-7, the
    kappa splines 9.1e-8, 7.7e-8, 1.1e-7 / <= 3.8e-7, the tabulated spline 1.1e-4 / 7.8e-8 (its second derivative comes out of node
    differences, as in test_stiffness.py), stable Neo-Hookean 7.4e-8 / 1.8e-7, mixed162 at rest 9.1e-8 / 4.2e-7."""
    tab = None
    if name.startswith("cube384"):
        s, flat, rest, x = make384(name.endswith("split"))
        if name.endswith("split"):
            assert list(flat["tet_kind"][:192]) == [pkg.TET_STVK] * 192 and list(flat["tet_kind"][192:]) == [NH] * 192
    else:
        s, flat, c, tab = open_case(name[:8] if name == "mixed162rest" else name)
        rest = c["rest"]; x = rest.copy() if name == "mixed162rest" else c["x"]
    a = np.random.default_rng(101).standard_normal(x.shape)
    dev = s.rest_sensitivity(a, x)
    again = s.rest_sensitivity(a, x)
    s.close()
    ref, scale = numpy_rest_sens(flat, rest, x, a, tab)
    assert dev.shape == x.shape and np.isfinite(dev).all()
    worst = ratio(dev, ref, scale)
    tr = np.abs(dev.sum(axis=0)).max() / (1e-12 * scale.sum())
    print("%s: worst |device - numpy|_v / (1e-9 scale_v) = %.3e; |sum_v out_v| / (1e-12 sum_v scale_v) = %.3e; |out| max %.3e, scale max %.3e"
          % (name, worst, tr, np.abs(dev).max(), scale.max()))
    assert worst <= 1.0, worst
    assert tr <= 1.0, tr
    assert again.tobytes() == dev.tobytes()
    assert np.abs(dev).max() > 1e-3 * scale.max()      # the input condition: the result is not lost in the bar


@gpu
def test_rest_sensitivity_returns_the_callers_order():
    """the split 384-tet cube with its halves' kinds exchanged in the REFERENCE misses the bar by orders of magnitude: the kinds matter,
    and the device reads each tet with the kind its add_tets call gave it"""
    s, flat, rest, x = make384(True)
    a = np.random.default_rng(101).standard_normal(x.shape)
    dev = s.rest_sensitivity(a, x)
    s.close()
    swapped = dict(flat, tet_kind=np.concatenate([flat["tet_kind"][192:], flat["tet_kind"][:192]]))
    ref, scale = numpy_rest_sens(swapped, rest, x, a)
    assert ratio(dev, ref, scale) > 1e3


@gpu
def test_stacks_have_the_bits_of_their_columns():
    """k = 1, 3, 16 and 17 (the second pass of 16 columns) on the 6-tet cube: every column is bit-identical to the same vector alone"""
    s, flat, c, tab = open_case("tet6")
    A = np.random.default_rng(103).standard_normal((17,) + c["x"].shape)
    alone = [s.rest_sensitivity(A[j], c["x"]) for j in range(17)]
    for k in (1, 3, 16, 17):
        st = s.rest_sensitivity(A[:k], c["x"])
        assert st.shape == (k,) + c["x"].shape
        for j in range(k):
            assert st[j].tobytes() == alone[j].tobytes(), (k, j)
    s.close()


@gpu
@pytest.mark.parametrize("name", ["tet6", "mixed162", "kind%d" % pkg.TET_STABLE_NH])
def test_at_the_rest_state_it_is_the_stiffness(name):
    """at x = X, P = 0 and F = I: d(a . f)/dX = K(X) a; rest_sensitivity(a, x=rest) against stiffness_apply(a, x=rest) at the device
    bar 1e-9 scale_v.  Measured on an MI355X, of the bar: tet6 exactly 0, mixed162 2.4e-8, stable Neo-Hookean 2.0e-8."""
    s, flat, c, tab = open_case(name)
    rest = c["rest"]
    a = np.random.default_rng(107).standard_normal(rest.shape)
    dev = s.rest_sensitivity(a, rest)
    Ka = s.stiffness_apply(a, rest)
    s.close()
    scale = numpy_rest_sens(flat, rest, rest, a, tab)[1]
    worst = ratio(dev, Ka, scale)
    print("%s at rest: worst |rest_sensitivity - stiffness_apply|_v / (1e-9 scale_v) = %.3e" % (name, worst))
    assert worst <= 1.0, worst


# ---------------------------------------------------------------- 2: held against the dense numpy value -----------------------------
@gpu
@pytest.mark.parametrize("name", ["cantilever162", "mixed750", "cloth"])
def test_held_against_the_dense_numpy_adjoint(name):
    """test_adjoint.polished(name), step_adjoint(held=True) with random dL/dx and dL/dv: held = g_held - (K lam)_held with numpy's K and
    numpy's lam, |held - ref| <= 1e-6 kappa |ref| over the held rows; the free rows are exactly 0; every other output has the bits of
    the call without held.  Measured on an MI355X, relative error / bar: cantilever162 4.1e-13 / 5.1e-4, mixed750 3.1e-13 / 1.1e-3, cloth
    5.6e-13 / 4.0e-4."""
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished(name)
    dt = s._settings.timestep_s
    flat = s.flatten()
    x = s.m_x.reshape(-1, 3).copy()
    rng = np.random.default_rng(61)
    Lx = rng.standard_normal(x.shape); Lv = rng.standard_normal(x.shape)
    plain = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000)
    out = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000, held=True)
    s.close()
    assert "held" not in plain and "rest" not in plain and "rest" not in out
    for k in ("lam", "xbar", "x_prev", "v_prev", "masses", "tets", "tris", "hinges"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    ref = numpy_adjoint(flat, sc.x, x, xbar, m3, dt, fm, Lx.copy(), Lv.copy(), tri_k)
    K = numpy_K(flat, sc.x, x, tri_k)
    want = (Lx + Lv / dt) - (K @ ref["lam"].ravel()).reshape(-1, 3)
    want[fm] = 0.0
    err = np.linalg.norm(out["held"] - want) / np.linalg.norm(want)
    bar = 1e-6 * ref["kappa"]
    print("%s: held against numpy: relative error %.3e, bar %.3e (kappa %.3e); |held| %.3e over %d held vertices"
          % (name, err, bar, ref["kappa"], np.linalg.norm(want), int((~fm).sum())))
    assert (out["held"][fm] == 0.0).all()
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------- 3: the adjoint is the derivative ----------------------------------
H_REST = 4e-3      # of a cube of edge 1 with cells of 1 / 3, along a standard normal direction on every rest vertex
H_HELD = 1.6e-2    # test_adjoint.STEP["x_prev"]: a position of the same body


class RestPipeline:
    """test_adjoint.Pipeline with the rest positions behind add_tets moved: masses, initial state and pins are the same arrays"""

    def __init__(self, dX=None):
        self.sc = scenes.cube_scene(3, NH, admm_iters=5)
        if dX is not None:
            verts, tets, lame, kind, off = self.sc.tets[0]
            self.sc.tets[0] = (verts + dX, tets, lame, kind, off)
        self.s = self.sc.make_solver()
        self.fm = np.ones(len(self.sc.x), bool); self.fm[sorted(self.sc.pins)] = False
        self.m3 = np.asarray(self.s.m_masses, dtype=np.float64)
        self.dt = self.s._settings.timestep_s
        self.grad_tol = TIGHT * np.linalg.norm((self.m3.reshape(-1, 3) * 9.8)[self.fm])

    def frame(self, x_prev, v_prev):
        s = self.s
        s.m_x = np.ascontiguousarray(x_prev, dtype=np.float64).ravel().copy()
        s.m_v = np.ascontiguousarray(v_prev, dtype=np.float64).ravel().copy()
        s.upload()
        s.step()
        s.newton_polish(max_iters=20, grad_tol=self.grad_tol, cg_tol=1e-12, cg_max=4000)
        return s.m_x.reshape(-1, 3).copy(), s.m_v.reshape(-1, 3).copy()


@gpu
@pytest.mark.parametrize("which", [0, 1])
def test_rest_is_the_derivative(which):
    """L = c . x + d . v after one frame of the device pipeline on the 162-tet cantilever rebuilt with verts +- h delta in add_tets
    (masses, initial state and pins the same arrays), for two random directions delta over all rest vertices; against rest . delta of
    step_adjoint(rest=True) and of numpy (numpy_rest_sens at numpy's own lam).  Asserted as test_adjoint._check_derivative does:
    |dev - q(h / 2)| <= 2 |numpy - q(h / 2)| + 4.73e-12 |q(h / 2)|, and of the input that the quotient still converges.

    Measured on an MI355X: |dev - numpy| / |q| = 3.7e-13 and 1.6e-14; the deviation from q(h / 2) common to both, 5.4e-4 and 3.3e-5, is
    the quotient's own h^2 term (it falls by 4 per halving; extrapolated, 2.2e-5 and 5.7e-5 remain: the yardstick's error of
    test_adjoint.py, the spring pins of the pipeline)."""
    p = RestPipeline()
    x0, v0 = _start(p)
    c, d = _loss_vectors(x0.shape)
    x, v = p.frame(x0, v0)
    out = p.s.step_adjoint(c, d, tol=1e-13, max_iters=4000, rest=True)
    flat = p.s.flatten()
    xbar = x0 + p.dt * v0; xbar[:, 1] += p.dt ** 2 * p.s._settings.gravity
    p.s.close()
    ref = numpy_adjoint(flat, p.sc.x, x, xbar, p.m3, p.dt, p.fm, c.copy(), d.copy())
    delta = np.random.default_rng(109 + which).standard_normal(x0.shape)

    def fn(q):
        pp = RestPipeline(q * delta)
        xx, vv = pp.frame(x0, v0); pp.s.close()
        return float(np.sum(c * xx) + np.sum(d * vv))
    dev = float(np.sum(out["rest"] * delta))
    npy = float(np.sum(numpy_rest_sens(flat, p.sc.x, x, ref["lam"])[0] * delta))
    _check_derivative("rest%d" % which, dev, npy, _quotients(fn, H_REST))


def _gs_cube(target_shift=None, vertex=None):
    """the scene of test_adjoint_cpp.py: the 48-tet Neo-Hookean cube, the face x = 0 held exactly by the pins of the sweeps (linsolver 1);
    one pin target moved"""
    verts, tets = _cube48()
    n3 = 3 * len(verts)
    s = Solver()
    s.add_nodes(verts, np.full(n3, 0.05))
    s.add_tets(verts, tets, Lame(1.0e5, 0.35), NH)
    pins = [int(v) for v in np.nonzero(verts[:, 0] < 1e-9)[0]]
    targets = [verts[v].copy() for v in pins]
    if target_shift is not None:
        targets[pins.index(vertex)] = targets[pins.index(vertex)] + target_shift
    s.set_pins(pins, targets)
    st = Settings(); st.admm_iters = 5; st.linsolver = 1
    assert s.initialize(st)
    fm = np.ones(len(verts), bool); fm[pins] = False
    return s, verts, pins, fm, st


def _gs_frame(s, fm, st):
    s.step()
    mg = np.linalg.norm(np.full(int(fm.sum()), 0.05 * st.gravity))
    s.newton_polish(max_iters=20, grad_tol=TIGHT * mg, cg_tol=1e-12, cg_max=4000)
    return s.m_x.reshape(-1, 3).copy(), s.m_v.reshape(-1, 3).copy()


@gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_held_is_the_derivative(axis):
    """The pins of the sweeps hold their vertices exactly at the targets: one pin target moved by +- h e before the step, L = c . x + d . v
    after step and polish, against held[v] . e of step_adjoint(held=True) and of numpy (g_held - (K lam)_held, numpy's K and lam).
    Asserted as test_rest_is_the_derivative.  Measured on an MI355X: |dev - numpy| / |q| = 2.0e-14 and 1.4e-14; the common deviation from
    q(h / 2), 1.3e-4 and 1.4e-5, is the quotient's h^2 term -- extrapolated, 1.3e-7 and 2.7e-10 remain: these pins hold exactly."""
    s, verts, pins, fm, st = _gs_cube()
    vtx = pins[len(pins) // 2]
    e = np.zeros(3); e[axis] = 1.0
    c, d = _loss_vectors(verts.shape)
    x, v = _gs_frame(s, fm, st)
    assert np.abs(x[pins] - verts[pins]).max() <= 1e-14      # the input condition: the pins hold their vertices at the targets
    out = s.step_adjoint(c, d, tol=1e-13, max_iters=4000, held=True)
    flat = s.flatten()
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    dt = st.timestep_s
    s.close()
    xbar = verts.copy(); xbar[:, 1] += dt ** 2 * st.gravity
    ref = numpy_adjoint(flat, verts, x, xbar, m3, dt, fm, c.copy(), d.copy())
    want = (c + d / dt) - (numpy_K(flat, verts, x) @ ref["lam"].ravel()).reshape(-1, 3)

    def fn(q):
        ss = _gs_cube(q * e, vtx)[0]
        xx, vv = _gs_frame(ss, fm, st); ss.close()
        return float(np.sum(c * xx) + np.sum(d * vv))
    _check_derivative("held%d" % axis, float(out["held"][vtx] @ e), float(want[vtx] @ e), _quotients(fn, H_HELD))


# ---------------------------------------------------------------- 4: refusals and housekeeping ---------------------------------------
@gpu
def test_refusals_carry_their_message():
    """rest_sensitivity and step_adjoint(rest=True) on a cloth and on a tets + triangles context; held where step_adjoint is refused
    (colliders, slide pins, before the first step): ADMM_HIP_ERR_ARG with a message that names the reason; the state is left alone."""
    def refused(call, word):
        with pytest.raises(capi.AdmmHipError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), e.value
    sc = cloth_with_hinges(6, limits=None, admm_iters=4)
    s = sc.make_solver(); s.step()
    x0 = s.m_x.copy()
    one = np.ones_like(sc.x)
    refused(lambda: s.rest_sensitivity(one), "triangles or hinges")
    refused(lambda: s.step_adjoint(one, rest=True), "triangles or hinges")
    assert "held" in s.step_adjoint(one, held=True)      # held is not refused on a cloth
    s.download(); assert s.m_x.tobytes() == x0.tobytes()
    s.close()
    mixed = scenes.cube_scene(2, NH, admm_iters=4)      # tets and a cloth in one context
    verts, tris = meshes.cloth_grid(4, size=1.0, y=1.5)
    mixed.add_tri_mesh(verts, tris, Lame(100.0, 0.1))
    s = mixed.make_solver(); s.step()
    refused(lambda: s.rest_sensitivity(np.ones_like(mixed.x)), "triangles or hinges")
    refused(lambda: s.step_adjoint(np.ones_like(mixed.x), rest=True), "triangles or hinges")
    s.close()
    L = capi.lib()

    def held_refused(s, word):
        n3 = s.m_x.size
        v = np.ones(n3); o = np.zeros(n3)
        assert L.admm_hip_adjoint_held(s._ctx, capi.dptr(v), capi.dptr(v), None, capi.dptr(o)) == -1
        assert word in L.admm_hip_last_error().decode(), L.admm_hip_last_error()
        refused(lambda: s.step_adjoint(v.reshape(-1, 3), held=True), "step_adjoint")
        s.close()
    s = scenes.cloth_scene(6, limits=None, floor=-1.0, linsolver=1).make_solver(); s.step(); held_refused(s, "colliders")
    sc = scenes.cloth_scene(6, limits=None); sc.slides[3] = (sc.x[3].copy(), np.array([0.0, 1.0, 0.0]))
    s = sc.make_solver(); s.step(); held_refused(s, "slide pins")
    s = scenes.cube_scene(2, NH).make_solver(); s.upload(); held_refused(s, "no step has run")
    s = scenes.cube_scene(2, NH).make_solver(); s.step()
    n = s.m_x.size // 3
    for bad in (np.ones((n + 1, 3)), np.ones((2, n, 2)), np.ones(3 * n)):
        with pytest.raises(ValueError):
            s.rest_sensitivity(bad)
    one = np.ones(3 * n)
    assert L.admm_hip_rest_sensitivity(s._ctx, None, 0, capi.dptr(one), capi.dptr(one)) == -1      # k < 1
    assert L.admm_hip_rest_sensitivity(s._ctx, None, 1, capi.dptr(one), None) == -1                # no output
    s.close()


@gpu
@pytest.mark.parametrize("linsolver", [0, 1])
def test_the_new_calls_do_not_disturb_a_run(linsolver):
    """3 frames (linsolver 0: the on-chip PCG, k_pcg2; 1: the GS sweeps) with rest_sensitivity and step_adjoint(rest, held) between the
    frames: m_x and m_v bit-identical to the same run without those calls."""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=linsolver)
        s = sc.make_solver()
        xs = []
        for _ in range(3):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                o = s.step_adjoint(np.ones_like(sc.x), 0.5 * np.ones_like(sc.x), tol=1e-8, rest=True, held=True)
                assert np.isfinite(o["rest"]).all() and np.isfinite(o["held"]).all()
                s.rest_sensitivity(np.ones((2,) + sc.x.shape), compressed_state(sc.x, 3))
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


@gpu
def test_step_adjoint_without_the_new_outputs_keeps_its_bits():
    """step_adjoint(rest=False, held=False) after the new entry points have run returns the bits of the call made before any of them
    had, and no new key"""
    sc = scenes.mixed_cube_scene(3, admm_iters=5)
    s = sc.make_solver()
    s.step()
    rng = np.random.default_rng(113)
    Lx, Lv = rng.standard_normal(sc.x.shape), rng.standard_normal(sc.x.shape)
    before = s.step_adjoint(Lx, Lv, tol=1e-10)
    full = s.step_adjoint(Lx, Lv, tol=1e-10, rest=True, held=True)
    s.rest_sensitivity(np.ones((17,) + sc.x.shape))
    after = s.step_adjoint(Lx, Lv, tol=1e-10)
    s.close()
    assert sorted(after) == sorted(before) == sorted(k for k in full if k not in ("rest", "held"))
    for k in before:
        if k == "info":
            assert before[k] == after[k] == full[k]
        elif before[k] is not None:
            assert before[k].tobytes() == after[k].tobytes() == full[k].tobytes(), k


@gpu
def test_rest_output_is_rest_sensitivity_of_lam_and_buffers_are_freed():
    """step_adjoint(rest=True)["rest"] has the bits of rest_sensitivity(lam) at the device state; a closed context leaves no device
    buffer behind; the next create and step report no error"""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = scenes.mixed_cube_scene(3, admm_iters=4)
    s = sc.make_solver()
    s.step()
    o = s.step_adjoint(np.ones_like(sc.x), rest=True, held=True)
    assert o["rest"].tobytes() == s.rest_sensitivity(o["lam"]).tobytes()
    s.rest_sensitivity(np.ones((17,) + sc.x.shape))      # two passes: 16 columns and 1
    s.close()
    sc2 = cloth_with_hinges(6, limits=None, admm_iters=4)
    s = sc2.make_solver(); s.step(); s.step_adjoint(np.ones_like(sc2.x), held=True); s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)
    s = sc.make_solver()
    s.step()
    assert np.isfinite(s.m_x).all()
    s.close()
