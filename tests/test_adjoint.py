"""The adjoint of an implicit-Euler step on the device (csrc/adjoint.hpp): param_sensitivity() and step_adjoint(), against numpy.

THE REFERENCES are the numpy yardsticks of test_forces.py, test_stiffness.py and test_newton.py:
  parameter sensitivities   per element, the dot of a with tet_forces of the ONE-element description whose (mu, lambda, kappa) are a
                            unit vector of theta (the density's gradient is linear in them); tri_forces and hinge_forces for the cloth.
                            Bar: that of test_forces.py carried to this quantity, 1e-9 vol_e |Binv_e|_F sum_c |a_c| max_i |d g_i / d theta|
                            (w^2 |rest| and stiffness |c|^2 |x| in the place of the first two factors for triangles and hinges).
  the adjoint               A = K + M / dt^2 on the free rows with K assembled element by element from test_stiffness.numpy_stiffness,
                            numpy.linalg.solve, the formulas of adjoint.hpp in numpy.  Bar: test_newton.py's for tangent_solve, 1e-6 kappa.
  the derivative            central differences of the whole device pipeline (set state, step, polish).

Meshes and states: those of test_newton.py (1, 6, 162 and 750 tets, the five dense-Hessian kinds on 162 tets, the 12 x 12 cloth with hinges;
compressed, with inverted tets)."""
import ctypes as C
import functools

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Lame, Solver, Settings
from test_energy_monitor import cloth_with_hinges
from test_forces import SPLINE_KINDS, hinge_forces, stretch_gradient, table_fgh, tet_forces, tri_forces
from test_newton import _empty, compressed_state, open_case
from test_stiffness import numpy_stiffness

gpu = pytest.mark.gpu
WITH_KAPPA = (pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED)
PARAMETERLESS = (pkg.TET_LINEAR, pkg.TET_SPLINE_TABLE)
NH = pkg.TET_NEOHOOKEAN


# ---------------------------------------------------------------- the numpy references --------------------------------------------
def element_reference(flat, rest, x, tri_k=None, tab=None):
    """Per term, from the one-element descriptions: tets C [nt, 4, 4, 3] = the corner forces at theta = e_mu, e_la, e_kappa and at the
    element's own constants (d_scale), unit [nt, 4] = vol |Binv|_F max_i |d g_i / d theta_p|; triangles [ntri, 3, 3] and w^2 |rest|;
    hinges [nb, 4, 3] and stiffness |c|^2 |x|."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    dfgh = table_fgh(tab)[1] if tab is not None else None
    e = _empty(flat)
    tets = flat["tet_idx"]
    Ct = np.zeros((len(tets), 4, 4, 3)); ut = np.zeros((len(tets), 4))
    for i, t in enumerate(tets):
        kd = int(flat["tet_kind"][i]); k = float(flat["tet_k"][i])
        sub = dict(e, tet_idx=np.array([[0, 1, 2, 3]], np.int32), tet_kind=flat["tet_kind"][i:i + 1], tet_k=flat["tet_k"][i:i + 1])
        own = (float(flat["tet_mu"][i]), float(flat["tet_lambda"][i]), float(flat["tet_kappa"][i]))
        for p, th in enumerate([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), own]):
            if p < 3 and (kd in PARAMETERLESS or (p == 2 and kd not in WITH_KAPPA)):
                continue      # the kind reads no such constant: the column is exactly 0
            sub.update(tet_mu=np.array([th[0]]), tet_lambda=np.array([th[1]]), tet_kappa=np.array([th[2]]))
            f, sc, st = tet_forces(sub, rest[t], x[t], dfgh)
            Ct[i, p] = f
            ut[i, p] = sc[0] / k * np.abs(stretch_gradient(st["stretches"][0], kd, th[0], th[1], k, th[2], dfgh)).max()
    tris = flat["tri_idx"]
    Cr = np.zeros((len(tris), 3, 3)); ur = np.zeros(len(tris))
    for i, t in enumerate(tris):
        sub = dict(e, tri_idx=np.array([[0, 1, 2]], np.int32), tri_weight=flat["tri_weight"][i:i + 1], tri_rest=flat["tri_rest"][i:i + 1])
        Cr[i], sc = tri_forces(sub, rest[t], x[t], tri_k)
        ur[i] = sc[0]
    idx = flat["bend_idx"]
    Ch = np.zeros((len(idx), 4, 3)); uh = np.zeros(len(idx))
    for i, t in enumerate(idx):
        sub = dict(e, bend_idx=np.array([[0, 1, 2, 3]], np.int32), bend_coef=flat["bend_coef"][i:i + 1], bend_stiffness=flat["bend_stiffness"][i:i + 1])
        Ch[i], sc = hinge_forces(sub, rest[t], x[t])
        uh[i] = sc[0]
    return dict(Ct=Ct, ut=ut, Cr=Cr, ur=ur, Ch=Ch, uh=uh)


def contract(ref, flat, a):
    """a [nv, 3] -> (tets [nt, 4], tris, hinges) of the reference and the sums sum_c |a_c| per term"""
    at, ar, ah = a[flat["tet_idx"]], a[flat["tri_idx"]], a[flat["bend_idx"]]
    n = lambda q: np.linalg.norm(q, axis=2).sum(axis=1)
    return (np.einsum("tpcj,tcj->tp", ref["Ct"], at), np.einsum("tcj,tcj->t", ref["Cr"], ar), np.einsum("tcj,tcj->t", ref["Ch"], ah),
            n(at), n(ar), n(ah))


@functools.lru_cache(None)
def case_reference(name):
    """the element reference of a case of test_newton.py at its state: computed once, shared, left unchanged"""
    s, flat, c, tab = open_case(name)
    s.close()
    ref = element_reference(flat, c["rest"], c["x"], c["tri_k"], tab)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def worst_ratio(dev, flat, ref, a):
    """the largest |device - reference| / (1e-9 unit) over the terms and parameters; columns of unit 0 must be exactly 0"""
    rt, rr, rh, nt, nr, nh = contract(ref, flat, a)
    worst = 0.0
    bt = 1e-9 * ref["ut"] * nt[:, None]
    zero = bt == 0.0
    assert (dev["tets"][zero] == 0.0).all() and (rt[zero] == 0.0).all()
    if (~zero).any():
        worst = max(worst, (np.abs(dev["tets"] - rt)[~zero] / bt[~zero]).max())
    if len(rr):
        worst = max(worst, (np.abs(dev["tris"] - rr) / (1e-9 * ref["ur"] * nr)).max())
    if len(rh):
        worst = max(worst, (np.abs(dev["hinges"] - rh) / (1e-9 * ref["uh"] * nh)).max())
    return worst


# ---------------------------------------------------------------- 1: param_sensitivity against numpy ------------------------------
@gpu
@pytest.mark.parametrize("name", ["tet1", "tet6", "mixed162", "mixed750", "cloth"] + ["kind%d" % k for k in SPLINE_KINDS])
def test_param_sensitivity_against_numpy(name):
    """k = 1 and a stack of 3 random a at the compressed state: every term and parameter within the bar of the module docstring; the
    parameter columns of the linear tet and of the tabulated spline, and the kappa column of a kind without kappa, exactly 0;
    sum_e d_scale over all terms = a . forces(x) to 1e-12 sum_v |a_v| |f_v|; a stack's column has the bits of the column alone; a second
    call has the bits of the first.

    Measured on an MI355X, the worst |device - numpy| / bar: DESIGN.md 4m."""
    s, flat, c, tab = open_case(name)
    ref = case_reference(name)
    A = np.random.default_rng(53).standard_normal((3,) + c["x"].shape)
    one = s.param_sensitivity(A[0], c["x"])
    stack = s.param_sensitivity(A, c["x"])
    again = s.param_sensitivity(A, c["x"])
    f = s.forces(c["x"])
    s.close()
    assert one["tets"].shape == (len(flat["tet_idx"]), 4) and stack["tets"].shape == (3, len(flat["tet_idx"]), 4)
    assert stack["tris"].shape == (3, len(flat["tri_idx"])) and stack["hinges"].shape == (3, len(flat["bend_idx"]))
    worst = 0.0
    for j in range(3):
        worst = max(worst, worst_ratio({k: stack[k][j] for k in stack}, flat, ref, A[j]))
    total = [stack["tets"][j, :, 3].sum() + stack["tris"][j].sum() + stack["hinges"][j].sum() for j in range(3)]
    af = [float(np.sum(A[j] * f)) for j in range(3)]
    unit = [float(np.sum(np.linalg.norm(A[j], axis=1) * np.linalg.norm(f, axis=1))) for j in range(3)]
    sum_err = max(abs(total[j] - af[j]) / unit[j] for j in range(3))
    print("%s: worst |device - numpy| / bar = %.3e (bar: 1e-9 of the element's unit); |sum d_scale - a . f| / sum |a_v| |f_v| = %.3e (bar 1e-12)"
          % (name, worst, sum_err))
    assert worst <= 1.0, worst
    assert sum_err <= 1e-12, sum_err
    for k in stack:
        assert stack[k][0].tobytes() == one[k].tobytes(), k
        assert again[k].tobytes() == stack[k].tobytes(), k


@gpu
def test_param_sensitivity_returns_the_callers_order():
    """48 tets added by two add_tets calls, StVK first and Neo-Hookean second: the device sorts the Neo-Hookean group in front; the result
    is in the order the terms were added (held against the per-element reference, whose kinds differ between the halves)."""
    verts, tets = meshes.kuhn_cube(2)
    lame = Lame.soft_rubber()
    s = Solver()
    s.add_nodes(verts, np.repeat(meshes.lumped_masses_tets(verts, tets), 3))
    s.add_tets(verts, tets[:24], lame, pkg.TET_STVK)
    s.add_tets(verts, tets[24:], lame, NH)
    assert s.initialize(Settings())
    flat = s.flatten()
    assert list(flat["tet_kind"][:24]) == [pkg.TET_STVK] * 24 and list(flat["tet_kind"][24:]) == [NH] * 24
    x = compressed_state(verts, 2)
    ref = element_reference(flat, verts, x)
    a = np.random.default_rng(59).standard_normal(x.shape)
    dev = s.param_sensitivity(a, x)
    s.close()
    worst = worst_ratio(dev, flat, ref, a)
    swapped = dict(dev, tets=np.concatenate([dev["tets"][24:], dev["tets"][:24]]))
    print("two add_tets calls, kinds in descending group order: worst |device - numpy| / bar = %.3e; with the halves swapped %.3e"
          % (worst, worst_ratio(swapped, flat, ref, a)))
    assert worst <= 1.0, worst
    assert worst_ratio(swapped, flat, ref, a) > 1e3      # the input condition: the order matters


# ---------------------------------------------------------------- 2: the device adjoint against the dense numpy adjoint -------------
def numpy_K(flat, rest, x, tri_k=None):
    """K(x) [3 nv, 3 nv] from test_stiffness.numpy_stiffness, element by element on the one-element descriptions (the unit directions of
    the element's own corners: what numpy_stiffness of the whole mesh on the 3 nv unit vectors sums, without the zero blocks)"""
    nv = len(rest)
    K = np.zeros((3 * nv, 3 * nv))
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    e = _empty(flat)

    def add(verts, sub, k=None):
        n = len(verts)
        Ke = numpy_stiffness(sub, rest[verts], x[verts], np.eye(3 * n).reshape(3 * n, n, 3), k)[0].reshape(3 * n, 3 * n)
        dof = (3 * np.asarray(verts)[:, None] + np.arange(3)[None]).ravel()
        K[np.ix_(dof, dof)] += 0.5 * (Ke + Ke.T)
    for i, t in enumerate(flat["tet_idx"]):
        sub = dict(e, tet_idx=np.array([[0, 1, 2, 3]], np.int32))
        for key in ("tet_kind", "tet_mu", "tet_lambda", "tet_k", "tet_kappa"):
            sub[key] = flat[key][i:i + 1]
        add(t, sub)
    for i, t in enumerate(flat["tri_idx"]):
        add(t, dict(e, tri_idx=np.array([[0, 1, 2]], np.int32), tri_weight=flat["tri_weight"][i:i + 1], tri_rest=flat["tri_rest"][i:i + 1]), tri_k)
    for i, t in enumerate(flat["bend_idx"]):
        add(t, dict(e, bend_idx=np.array([[0, 1, 2, 3]], np.int32), bend_coef=flat["bend_coef"][i:i + 1], bend_stiffness=flat["bend_stiffness"][i:i + 1]))
    return K


def numpy_adjoint(flat, rest, x, xbar, m3, dt, fm, Lx, Lv, tri_k=None):
    """the formulas of adjoint.hpp, dense: dict(lam, xbar, x_prev, v_prev, masses, tets, tris, hinges, kappa = cond(A), ref = the
    element reference at x)"""
    f3 = np.repeat(fm, 3)
    A = (numpy_K(flat, rest, x, tri_k) + np.diag(m3) / dt ** 2)[np.ix_(f3, f3)]
    g = Lx + Lv / dt
    g[~fm] = 0.0
    lam = np.zeros(x.size); lam[f3] = np.linalg.solve(A, g.ravel()[f3]); lam = lam.reshape(-1, 3)
    M = m3.reshape(-1, 3)
    xb = M * lam / dt ** 2
    xp = xb - Lv / dt; xp[~fm] = 0.0
    ref = element_reference(flat, rest, x, tri_k)
    rt, rr, rh = contract(ref, flat, lam)[:3]
    return dict(lam=lam, xbar=xb, x_prev=xp, v_prev=M * lam / dt, masses=-lam * (x - xbar) / dt ** 2, tets=rt, tris=rr, hinges=rh,
                kappa=np.linalg.cond(A), ref=ref, g=g)


def polished(name, grad_rel=1e-8, **kw):
    """-> (scene, solver after one step of 5 ADMM iterations and the polish, the polish's records, x_prev, x_bar, free mask, masses, tri_k)"""
    if name == "cantilever162":
        sc = scenes.cube_scene(3, NH, admm_iters=5, **kw)
    elif name == "mixed750":
        sc = scenes.mixed_cube_scene(5, admm_iters=5, **kw)
    else:
        sc = cloth_with_hinges(12, limits=None, admm_iters=5, **kw)
    s = sc.make_solver()
    dt = s._settings.timestep_s
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    fm = np.ones(len(sc.x), bool); fm[sorted(sc.pins)] = False
    x_prev = s.m_x.reshape(-1, 3).copy()
    xbar = x_prev.copy(); xbar[:, 1] += dt * dt * s._settings.gravity
    s.step()
    grad_tol = grad_rel * np.linalg.norm((m3.reshape(-1, 3) * 9.8)[fm])
    rec = s.newton_polish(max_iters=20, grad_tol=grad_tol, cg_tol=1e-10, cg_max=2000)
    tri_k = sc.tris[0][2].bulk_modulus() if sc.tris else None
    return sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol


@gpu
@pytest.mark.parametrize("name", ["cantilever162", "mixed750", "cloth"])
def test_step_adjoint_against_the_dense_numpy_adjoint(name):
    """One step of 5 ADMM iterations, the polish to 1e-8 |m g| as in test_newton.py, then step_adjoint with random dL/dx and dL/dv
    against numpy at the same state.  lam: |lam - ref| <= 1e-6 kappa |ref| (test_newton.py's bar for tangent_solve: the bar is the
    reference's, kappa numpy's condition number of A); xbar, x_prev, v_prev and masses: the same bar times their own norm -- each is
    lam times a factor, x_prev less the exact Lv / dt; tets, tris and hinges per term: the bar of test 1 at a = lam plus what an error of
    1e-6 kappa |lam| in lam moves the term by, unit_e (1e-9 sum_c |lam_c| + 2e-6 kappa |lam|) (sum_c |d lam_c| <= 2 |d lam| over four
    corners).  info: the reported residual is the one recomputed through stiffness_apply_ex(hold_pins) to 2 eps |g_x| and <= 2 tol;
    rhs_norm is |g_x|; stationarity has the bits of the polish's last grad_norm; held rows of every vector are 0.

    Measured on an MI355X: DESIGN.md 4m."""
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished(name)
    assert rec[-1]["grad_norm"] <= grad_tol, rec
    dt = s._settings.timestep_s
    flat = s.flatten()
    x = s.m_x.reshape(-1, 3).copy()
    rng = np.random.default_rng(61)
    Lx = rng.standard_normal(x.shape); Lv = rng.standard_normal(x.shape)
    tol = 1e-12
    out = s.step_adjoint(Lx, Lv, tol=tol, max_iters=4000)
    info = out["info"]
    shift = 1.0 / dt ** 2
    g = Lx + Lv / dt; g[~fm] = 0.0
    r = (g - s.stiffness_apply_ex(out["lam"], shift=shift, hold_pins=True))[fm]
    rel = np.linalg.norm(r) / np.linalg.norm(g[fm])
    x_after = s.m_x.copy(); s.download()
    assert s.m_x.tobytes() == x_after.tobytes()      # the state is not changed
    s.close()
    ref = numpy_adjoint(flat, sc.x, x, xbar, m3, dt, fm, Lx, Lv, tri_k)
    bar = 1e-6 * ref["kappa"]
    errs = {k: np.linalg.norm(out[k] - ref[k]) / np.linalg.norm(ref[k]) for k in ("lam", "xbar", "x_prev", "v_prev", "masses")}
    lam_n = np.linalg.norm(ref["lam"])
    nt, nr, nh = contract(ref["ref"], flat, ref["lam"])[3:]
    worst_p = 0.0
    for key, unit, nc in (("tets", ref["ref"]["ut"], nt[:, None] if len(nt) else nt), ("tris", ref["ref"]["ur"], nr), ("hinges", ref["ref"]["uh"], nh)):
        if not len(unit):
            continue
        b = unit * (1e-9 * nc + 2.0 * bar * lam_n)
        d = np.abs(out[key] - ref[key])
        assert (d[b == 0.0] == 0.0).all(), key
        worst_p = max(worst_p, (d[b > 0.0] / b[b > 0.0]).max())
    print("%s: kappa %.3e, bar %.3e; relative errors %s; parameters: worst error / bar %.3e; %d iterations, residual reported %.3e recomputed %.3e; "
          "stationarity %.3e (polish %.3e)" % (name, ref["kappa"], bar, " ".join("%s %.2e" % kv for kv in errs.items()), worst_p, info["iterations"],
                                                info["residual"], rel, info["stationarity"], rec[-1]["grad_norm"]))
    assert info["converged"] and info["residual"] <= 2 * tol
    # (numpy forms g_x = Lx + Lv / dt with two roundings, the device with one fma on Lv * (1 / dt): the two right-hand sides differ by up
    # to eps |g_x| entry by entry, and so do the two residual norms -- 2 eps in the unit |g_x| the residual is reported in)
    assert rel <= 2 * tol and abs(info["residual"] - rel) <= 2.0 * np.finfo(np.float64).eps, (info["residual"], rel)
    assert abs(info["rhs_norm"] - np.linalg.norm(g[fm])) <= 1e-12 * info["rhs_norm"]
    assert info["stationarity"] == rec[-1]["grad_norm"]
    assert info["shift"] == shift
    for k, e in errs.items():
        assert e <= bar, (k, e, bar)
        assert (out[k][~fm] == 0.0).all(), k
    assert worst_p <= 1.0, worst_p


# ---------------------------------------------------------------- 3, 4: the adjoint is the derivative --------------------------------
# THE YARDSTICK'S OWN ERROR.  The pipeline pins the face x = 0 with the step's spring pins (linsolver 0): the ADMM iterations leave those
# vertices where the springs balance the load (1e-6 off their targets here) and the polish holds them THERE, so in the pipeline they move
# with whatever changes the load they carry -- a change of x_bar is passed on to them almost whole, the body being stiff -- while the
# adjoint, the device's and numpy's alike, differentiates the problem the polish solves, with those vertices held.  Measured on an MI355X,
# (adjoint - quotient) / quotient, numpy and device alike: x_prev -8.4e-5 and -6.0e-5, v_prev 9.0e-3 and 1.15e-2, mu 3e-5, lambda -3.3e-3,
# masses -5.5e-5, dL/dx_0 through two frames 1.65e-2.  The polish itself ends at |g| = 7e-4 = 2e-7 |m g| (its line search finds no further decrease).
# R: the worst |device - numpy| / |quotient(h / 2)| of tests 3 and 4 as measured on an MI355X -- the device's own share of the difference;
# the assertion adds 10 x that to twice the numpy adjoint's discrepancy to the same quotient.
R_MEASURED = 4.73e-13
R_ASSERT = 10.0 * R_MEASURED
TIGHT = 1e-11      # the polish of the pipeline: |g| <= TIGHT |m g| asked for
# the steps h (quotients at 2h, h, h / 2), from a ladder of steps measured on an MI355X: the largest at which the quotient still changes by
# less from h to h / 2 than from 2h to h with a factor of 2.5 or more to spare; below them the polish's error over h takes over
STEP = {"x_prev": 1.6e-2, "v_prev": 0.64, "mu": 0.025, "la": 0.025, "masses": 0.025}


class Pipeline:
    """the 162-tet cantilever: set state, step, polish -- for any factor on mu, lambda and the masses"""

    def __init__(self, mu_f=1.0, la_f=1.0, m_f=1.0):
        base = Lame.soft_rubber()
        self.sc = scenes.cube_scene(3, NH, lame=Lame(mu=base.mu * mu_f, lambda_=base.lambda_ * la_f), admm_iters=5)
        self.sc.m = self.sc.m * m_f
        self.s = self.sc.make_solver()
        self.fm = np.ones(len(self.sc.x), bool); self.fm[sorted(self.sc.pins)] = False
        self.m3 = np.asarray(self.s.m_masses, dtype=np.float64)
        self.dt = self.s._settings.timestep_s
        self.grad_tol = TIGHT * np.linalg.norm((self.m3.reshape(-1, 3) * 9.8)[self.fm])

    def frame(self, x_prev=None, v_prev=None):
        s = self.s
        if x_prev is not None:
            s.m_x = np.ascontiguousarray(x_prev, dtype=np.float64).ravel().copy()
            s.m_v = np.ascontiguousarray(v_prev, dtype=np.float64).ravel().copy()
            s.upload()
        s.step()
        s.newton_polish(max_iters=20, grad_tol=self.grad_tol, cg_tol=1e-12, cg_max=4000)
        return s.m_x.reshape(-1, 3).copy(), s.m_v.reshape(-1, 3).copy()


def _loss_vectors(shape):
    rng = np.random.default_rng(67)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def _start(p):
    """a start state off the rest pose with a velocity"""
    rng = np.random.default_rng(71)
    x0 = p.sc.x + 0.01 * rng.standard_normal(p.sc.x.shape) * p.fm[:, None]
    v0 = 0.2 * rng.standard_normal(p.sc.x.shape) * p.fm[:, None]
    return x0, v0


def _quotients(fn, h):
    """central differences of fn at 2h, h, h / 2"""
    return [(fn(q) - fn(-q)) / (2.0 * q) for q in (2.0 * h, h, 0.5 * h)]


def _check_derivative(what, dev, npy, q):
    """the assertion of tests 3 and 4 on one quantity"""
    d_dev, d_np = abs(dev - q[2]), abs(npy - q[2])
    print("%-8s device %.12e numpy %.12e quotients(2h, h, h/2) %.12e %.12e %.12e; |dev - q| / |q| = %.3e, |numpy - q| / |q| = %.3e, "
          "|dev - numpy| / |q| = %.3e" % (what, dev, npy, q[0], q[1], q[2], d_dev / abs(q[2]), d_np / abs(q[2]), abs(dev - npy) / abs(q[2])))
    assert abs(q[2] - q[1]) < abs(q[1] - q[0]), (what, q)      # the input condition: the quotient still converges, it is above the rounding floor
    assert d_dev <= 2.0 * d_np + R_ASSERT * abs(q[2]), (what, d_dev, d_np)


@gpu
@pytest.mark.parametrize("what", ["x_prev0", "x_prev1", "v_prev0", "v_prev1", "mu", "la", "masses"])
def test_the_adjoint_is_the_derivative(what):
    """L = c . x + d . v after one frame of the device pipeline on the 162-tet cantilever; central differences at 2h, h and h / 2 along two
    random directions of x_prev and of v_prev (free rows) and in a global factor on mu, on lambda (the solver is rebuilt with
    Lame(mu, lambda_): the ADMM weights change with it, the polished minimiser does not) and on the masses, against the adjoint's
    prediction x_prev . delta, v_prev . delta, sum mu d_mu, sum la d_la, sum m dL/dm.  Asserted: |dev - q(h / 2)| <= 2 |numpy - q(h / 2)|
    + R_ASSERT |q(h / 2)| with the dense numpy adjoint at the device's state, and of the input that the quotient changes by less from h
    to h / 2 than from 2h to h.

    Measured on an MI355X: DESIGN.md 4m."""
    p = Pipeline()
    x0, v0 = _start(p)
    c, d = _loss_vectors(x0.shape)
    x, v = p.frame(x0, v0)
    out = p.s.step_adjoint(c, d, tol=1e-13, max_iters=4000)
    flat = p.s.flatten()
    g_acc = p.s._settings.gravity
    xbar = x0 + p.dt * v0; xbar[:, 1] += p.dt ** 2 * g_acc
    ref = numpy_adjoint(flat, p.sc.x, x, xbar, p.m3, p.dt, p.fm, c.copy(), d.copy())
    loss = lambda xv: float(np.sum(c * xv[0]) + np.sum(d * xv[1]))
    if what in ("mu", "la", "masses"):
        def fn(q):
            pp = Pipeline(**{{"mu": "mu_f", "la": "la_f", "masses": "m_f"}[what]: 1.0 + q})
            r = loss(pp.frame(x0, v0)); pp.s.close()
            return r
        h = STEP[what]
        if what == "masses":
            dev = float(np.sum(p.m3.reshape(-1, 3) * out["masses"])); npy = float(np.sum(p.m3.reshape(-1, 3) * ref["masses"]))
            # (a factor on the masses leaves x_bar as it is: gravity is an acceleration)
        else:
            col = 0 if what == "mu" else 1
            th = flat["tet_mu"] if what == "mu" else flat["tet_lambda"]
            dev = float(np.sum(th * out["tets"][:, col])); npy = float(np.sum(th * ref["tets"][:, col]))
    else:
        delta = np.random.default_rng(73 + int(what[-1])).standard_normal(x0.shape) * p.fm[:, None]
        key = what[:-1]
        h = STEP[key]
        fn = (lambda q: loss(p.frame(x0 + q * delta, v0))) if key == "x_prev" else (lambda q: loss(p.frame(x0, v0 + q * delta)))
        dev = float(np.sum(out[key] * delta)); npy = float(np.sum(ref[key] * delta))
    q = _quotients(fn, h)
    p.s.close()
    _check_derivative(what, dev, npy, q)


@gpu
def test_two_steps_chain():
    """Two frames on the 162-tet cantilever, L = c . x_2 + d . v_2: frame 2's adjoint gives x_prev and v_prev, which are dL/dx_1 and
    dL/dv_1; fed into frame 1's adjoint (a second solver that stopped after frame 1: the device holds the last step only) they give
    dL/dx_0.  Held along one direction against the central difference of the two-frame device pipeline, with the bar of test 3; numpy
    chains its own dense adjoints the same way."""
    pa, pb = Pipeline(), Pipeline()
    x0, v0 = _start(pa)
    c, d = _loss_vectors(x0.shape)
    x1, v1 = pa.frame(x0, v0)
    xb1, vb1 = pb.frame(x0, v0)
    assert xb1.tobytes() == x1.tobytes() and vb1.tobytes() == v1.tobytes()
    x2, v2 = pb.frame()
    o2 = pb.s.step_adjoint(c, d, tol=1e-13, max_iters=4000)
    o1 = pa.s.step_adjoint(o2["x_prev"], o2["v_prev"], tol=1e-13, max_iters=4000)
    flat = pa.s.flatten()
    g_acc = pa.s._settings.gravity
    dt = pa.dt
    xbar2 = x1 + dt * v1; xbar2[:, 1] += dt ** 2 * g_acc
    xbar1 = x0 + dt * v0; xbar1[:, 1] += dt ** 2 * g_acc
    r2 = numpy_adjoint(flat, pa.sc.x, x2, xbar2, pa.m3, dt, pa.fm, c.copy(), d.copy())
    r1 = numpy_adjoint(flat, pa.sc.x, x1, xbar1, pa.m3, dt, pa.fm, r2["x_prev"].copy(), r2["v_prev"].copy())
    delta = np.random.default_rng(79).standard_normal(x0.shape) * pa.fm[:, None]

    def fn(q):
        pb.frame(x0 + q * delta, v0)
        xx, vv = pb.frame()
        return float(np.sum(c * xx) + np.sum(d * vv))
    q = _quotients(fn, STEP["x_prev"])
    pa.s.close(); pb.s.close()
    _check_derivative("dL/dx_0", float(np.sum(o1["x_prev"] * delta)), float(np.sum(r1["x_prev"] * delta)), q)


# ---------------------------------------------------------------- 5: refusals and housekeeping ---------------------------------------
@gpu
def test_adjoint_refusals():
    """step_adjoint is refused where newton_polish is, with its error code, and leaves the state alone; wrong shapes are refused by both."""
    def refused(s):
        x0, v0 = s.m_x.copy(), s.m_v.copy()
        n = s.m_x.size // 3
        with pytest.raises(capi.AdmmHipError) as e:
            s.step_adjoint(np.ones((n, 3)))
        assert e.value.code == -1, e.value      # ADMM_HIP_ERR_ARG, as newton_polish
        with pytest.raises(capi.AdmmHipError) as e2:
            s.newton_polish()
        assert e2.value.code == e.value.code
        s.download()
        assert s.m_x.tobytes() == x0.tobytes() and s.m_v.tobytes() == v0.tobytes()
        s.close()
    s = scenes.cloth_scene(6, limits=None, floor=-1.0, linsolver=1).make_solver(); s.step(); refused(s)      # a floor
    s = scenes.cloth_scene(6).make_solver(); s.step(); refused(s)                              # strain-limited triangles
    sc = scenes.cloth_scene(6, limits=None); sc.slides[3] = (sc.x[3].copy(), np.array([0.0, 1.0, 0.0]))
    s = sc.make_solver(); s.step(); refused(s)                                                 # slide pins
    s = scenes.cube_scene(2, NH).make_solver(); s.upload(); refused(s)                         # before its first step
    s = scenes.cube_scene(2, NH).make_solver(); s.step()
    n = s.m_x.size // 3
    x0 = s.m_x.copy()
    for bad in (np.ones(n * 3 - 1), np.ones((n + 1, 3))):
        with pytest.raises(ValueError):
            s.step_adjoint(bad)
        with pytest.raises(ValueError):
            s.step_adjoint(np.ones((n, 3)), bad)
    for bad in (np.ones((n + 1, 3)), np.ones((2, n, 2)), np.ones(3 * n)):
        with pytest.raises(ValueError):
            s.param_sensitivity(bad)
    L = capi.lib()
    one = np.ones(3 * n); info = np.zeros(6)
    assert L.admm_hip_param_sensitivity(s._ctx, None, 0, capi.dptr(one), None, None, None) == -1      # k < 1
    assert L.admm_hip_step_adjoint(s._ctx, capi.dptr(one), None, 4, 1e-10, 100, *([None] * 8), capi.dptr(info)) == -1      # unknown flag
    assert L.admm_hip_step_adjoint(s._ctx, capi.dptr(one), None, 0, -1.0, 100, *([None] * 8), capi.dptr(info)) == -1       # tol < 0
    s.download()
    assert s.m_x.tobytes() == x0.tobytes()
    s.close()


@gpu
@pytest.mark.parametrize("linsolver", [0, 1])
def test_adjoint_calls_do_not_disturb_a_run(linsolver):
    """3 frames (linsolver 0: the on-chip PCG, k_pcg2; 1: the GS sweeps) with step_adjoint and param_sensitivity between the frames:
    m_x and m_v bit-identical to the same run without those calls."""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=linsolver)
        s = sc.make_solver()
        xs = []
        for _ in range(3):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                o = s.step_adjoint(np.ones_like(sc.x), 0.5 * np.ones_like(sc.x), tol=1e-8)
                assert np.isfinite(o["lam"]).all() and np.isfinite(o["tets"]).all()
                s.param_sensitivity(np.ones_like(sc.x))
                s.param_sensitivity(np.ones((2,) + sc.x.shape), compressed_state(sc.x, 3))
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


@gpu
def test_adjoint_buffers_are_freed_with_the_context():
    """a closed context leaves no device buffer behind; the next create and step report no error"""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = cloth_with_hinges(6, limits=None, admm_iters=4)
    s = sc.make_solver()
    s.step()
    s.step_adjoint(np.ones_like(sc.x))
    s.param_sensitivity(np.ones((17,) + sc.x.shape))      # two passes: 16 columns and 1
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)
    s = sc.make_solver()
    s.step()
    assert np.isfinite(s.m_x).all()
    s.close()
