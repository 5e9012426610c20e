"""The blocked dense inverse behind the two-level tangent preconditioner (csrc/tangent_coarse.hpp; Solver.set_tangent_coarse("blocked"))
on the GPU: the inverse itself through Solver.tangent_coarse_invert against numpy, against the host build of the same text and against
the one-block inverse; then everything that sits on it -- the application, tangent_solve, the polish, the adjoint -- against the
references of test_tangent_precond.py, with the one-block inverse on the same context as the second witness.

THE MATRICES, sizes and bars of the inverse are test_tangent_coarse_host.py's (matrix(), dropped_case(), bad_cases(): built once,
shared).  THE SCENES are test_tangent_precond.py's small ones: mixed162 with 4 aggregates, mixed750 and cloth with 8, and mixed750 with
16 -- nc = 192 is three tiles of 64, the default nc = 96 one and a half, nc = 48 less than one."""
import ctypes as C

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi
from admm_elastic_amd.solver import Solver
from test_adjoint import numpy_adjoint, polished
from test_newton import _rhs, compressed_state, free_mask, open_case
from test_tangent_coarse_host import BAD_SIZES, CONDS, SIZES, T, bad_cases, dropped_case, invert, libs, matrix      # noqa: F401 (libs: the host builds, a fixture)
from test_tangent_precond import AGG, _check_solve, dense_setup

gpu = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NH = pkg.TET_NEOHOOKEAN
SCENES = [("mixed162", 4), ("mixed750", 8), ("cloth", 8), ("mixed750", 16)]


def launches(n):
    """of the blocked chain: scan, scale; per tile step potrf, panel, update (the last step: potrf alone); winv, wtw, unscale, final"""
    nt = -(-n // T)
    return 2 + 3 * nt - 2 + 4


@pytest.fixture(scope="module")
def ctx():
    """a small context that only carries the inverse"""
    s = scenes.cube_scene(1, NH).make_solver()
    yield s
    s.close()


def both(s, A):
    """(blocked twice, one-block) on the device"""
    s.set_tangent_coarse("blocked")
    b1 = s.tangent_coarse_invert(A)
    nl = s.tangent_coarse()
    b2 = s.tangent_coarse_invert(A)
    s.set_tangent_coarse("one_block")
    o = s.tangent_coarse_invert(A)
    assert s.tangent_coarse() == dict(solver="one_block", tile=T, launches=1)
    assert nl == dict(solver="blocked", tile=T, launches=launches(len(A)))
    assert b1[0].tobytes() == b2[0].tobytes() and b1[1:] == b2[1:]      # run to run: the bits
    return b1, o


# ---------------------------------------------------------------- 1: the inverse ---------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cond", CONDS)
def test_invert_against_numpy_host_and_one_block(ctx, libs, n, cond):
    """|X A - I|_max <= 64 n eps cond and X symmetric to the bit; two runs return equal bits; |X - X_host|_max and |X - X_one_block|_max
    <= 64 n eps cond |X|_max (each is within that forward error of the inverse; not bits: the compilers contract a * b + c differently).

    Measured on an MI355X: DESIGN.md 4o."""
    A = matrix(n, cond)
    (X, ok, dropped), (Xo, oko, droppedo) = both(ctx, A)
    okh, droppedh, Xh = invert(libs[0].hm_tcb_invert, A)
    bar = 64 * n * EPS * cond
    res = np.abs(X @ A - np.eye(n)).max()
    dh = np.abs(X - Xh).max() / np.abs(Xh).max()
    do = np.abs(X - Xo).max() / np.abs(Xo).max()
    print("n = %d, cond = %.0e: |X A - I|_max = %.3e = %.2e of the bar; against the host build %.3e = %.2e of the bar; against one-block %.3e = %.2e of the bar"
          % (n, cond, res, res / bar, dh, dh / bar, do, do / bar))
    assert (ok, dropped) == (True, 0) == (oko, droppedo) and (okh, droppedh) == (1, 0)
    assert res <= bar, (res, bar)
    assert X.tobytes() == X.T.copy().tobytes()
    assert dh <= bar, (dh, bar)
    assert do <= bar, (do, bar)


@gpu
@pytest.mark.parametrize("n", [12, T + 1, 2 * T + 1, 384])
def test_invert_dropped_columns(ctx, n):
    """test_tangent_coarse_host.test_dropped_columns on the device; the one-block inverse drops the same."""
    A, z = dropped_case(n)
    (X, ok, dropped), (Xo, oko, droppedo) = both(ctx, A)
    rest = np.setdiff1d(np.arange(n), z)
    assert (ok, dropped) == (True, 3) == (oko, droppedo)
    assert (X[z, :] == 0.0).all() and (X[:, z] == 0.0).all()
    sub = A[np.ix_(rest, rest)]
    res = np.abs(X[np.ix_(rest, rest)] @ sub - np.eye(len(rest))).max()
    bar = 64 * n * EPS * np.linalg.cond(sub)
    print("n = %d, zeroed %s: |X A - I|_max on the rest = %.3e (bar %.3e)" % (n, z, res, bar))
    assert res <= bar, (res, bar)
    assert X.tobytes() == X.T.copy().tobytes()
    (X, ok, dropped), _ = both(ctx, np.zeros((n, n)))
    assert ok and dropped == n and (X == 0.0).all()


@gpu
@pytest.mark.parametrize("n", BAD_SIZES)
def test_invert_not_positive_definite(ctx, n):
    """test_tangent_coarse_host.test_not_positive_definite on the device: verdict 0 and X = 0 exactly, the defect in the first tile, in
    the last tile of a multi-tile matrix and in the tile (last, first); the one-block inverse's verdict.  These are data the verdict
    rule handles, not faults."""
    for name, (A, _) in bad_cases(n).items():
        (X, ok, dropped), (Xo, oko, _) = both(ctx, A)
        assert not ok and not oko, name
        assert (X == 0.0).all() and (Xo == 0.0).all(), name


# ---------------------------------------------------------------- 2: the application ----------------------------------------------
def _apply_both(s, r, x, hold):
    """z and tangent_precond() with the blocked and with the one-block inverse"""
    out = []
    for solver in ("blocked", "one_block"):
        s.set_tangent_coarse(solver)
        z = s.tangent_precond_apply(r, x, hold_pins=hold)
        out.append((z, s.tangent_precond(), s.tangent_coarse()))
    return out


@gpu
@pytest.mark.parametrize("name,G,hold", [(n, g, True) for n, g in SCENES] + [("mixed750", 16, False), ("cloth", 8, False)])
def test_application_against_numpy(name, G, hold):
    """z = M^-1 r with the blocked inverse against numpy's dense D^-1 r + P (P^T A P)^-1 P^T r: |z - z_ref| <= 1e-10 cond(A_c) |z_ref|
    (test_tangent_precond.test_application_against_numpy's bar); coarse_ok and coarse_dropped those of the one-block run.

    Measured on an MI355X: DESIGN.md 4o."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("jacobi", G)
    A, f3, M, shift, fm = dense_setup(name, s, c, hold, G=G)
    r = _rhs(c, 43)
    (z, info, co), (zo, infoo, coo) = _apply_both(s, r, c["x"], hold)
    s.close()
    ref = M(r.ravel())
    err = np.linalg.norm(z.ravel() - ref) / np.linalg.norm(ref)
    erro = np.linalg.norm(zo.ravel() - ref) / np.linalg.norm(ref)
    print("%s, G = %d, pins %s: |z - z_ref| / |z_ref| = %.3e blocked, %.3e one-block, cond(A_c) = %.3e, ratio to the bar 1e-10 cond = %.3e; %s %s"
          % (name, G, "held" if hold else "free", err, erro, M.cond, err / (1e-10 * M.cond), info, co))
    assert info == infoo and info["coarse_ok"] and info["coarse_dim"] == 12 * G and info["coarse_dropped"] == M.dropped == 0
    assert co == dict(solver="blocked", tile=T, launches=launches(12 * G)) and coo["launches"] == 1
    assert err <= 1e-10 * M.cond, (err, M.cond)


@gpu
def test_application_flat_cloth_and_held_aggregate():
    """The flat cloth's 24 dropped columns and a wholly held aggregate's 12 with the blocked inverse: coarse_dropped and coarse_ok of
    the one-block run, and a solve on top of each meets the bars of test_two_level_solve_residual."""
    s, flat, c, tab = open_case("cloth")
    x = np.array(c["rest"], dtype=np.float64)
    assert (np.ptp(x, axis=0) == 0.0).sum() == 1      # the input condition: exactly flat
    s.set_tangent_precond("two_level", 8)
    (z, info, _), (zo, infoo, _) = _apply_both(s, _rhs(c, 43), x, True)
    s.set_tangent_coarse("blocked")
    _check_solve(s, c, x, _rhs(c))
    s.close()
    assert info == infoo and info["coarse_ok"] and info["coarse_dropped"] == 24, (info, infoo)
    assert np.isfinite(z).all()
    sc = scenes.cube_scene(3, NH, pin_face=False)
    ptr, vert = Solver.tangent_plan(sc.x, 4)
    for v in vert[ptr[0]:ptr[1]]:
        sc.pins[int(v)] = sc.x[v].copy()
    s = sc.make_solver()
    s.set_tangent_precond("two_level", 4)
    xs = compressed_state(sc.x, 3)
    rhs = np.random.default_rng(41).standard_normal(sc.x.shape)
    (z, info, _), (zo, infoo, _) = _apply_both(s, rhs, xs, True)
    s.set_tangent_coarse("blocked")
    _check_solve(s, dict(rest=sc.x, pins=sorted(sc.pins)), xs, rhs)
    s.close()
    assert info == infoo and info["coarse_ok"] and info["coarse_dropped"] == 12 and info["coarse_dim"] == 48, (info, infoo)


@gpu
@pytest.mark.parametrize("name,G", [("mixed750", 16), ("cloth", 8)])
def test_application_is_symmetric(name, G):
    """r1 . M^-1 r2 = r2 . M^-1 r1 to 1e-12 |r1| |M^-1 r2| with the blocked inverse, r . M^-1 r > 0 (test_symmetric_and_positive)."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("two_level", G)
    s.set_tangent_coarse("blocked")
    R = np.random.default_rng(47).standard_normal((8,) + c["x"].shape)
    Z = np.stack([s.tangent_precond_apply(r, c["x"]) for r in R])
    assert s.tangent_precond()["coarse_ok"]
    s.close()
    fm = free_mask(c)
    Rm = R.copy(); Rm[:, ~fm] = 0.0
    worst = 0.0
    for i in range(8):
        assert np.sum(Rm[i] * Z[i]) > 0.0, i
        for j in range(i):
            worst = max(worst, abs(np.sum(Rm[i] * Z[j]) - np.sum(Rm[j] * Z[i])) / (np.linalg.norm(Rm[i]) * np.linalg.norm(Z[j])))
    print("%s, G = %d: asymmetry %.3e (bar 1e-12)" % (name, G, worst))
    assert worst <= 1e-12, worst


# ---------------------------------------------------------------- 3: the solve ----------------------------------------------------
@gpu
@pytest.mark.parametrize("name,G", SCENES)
def test_solve_with_blocked(name, G):
    """tol = 1e-12 and 1e-8 with the blocked inverse: converged, the reported residual <= 2 tol and equal to the recomputed one
    (_check_solve of test_tangent_precond.py); the iteration count within 2 of the one-block run's on the same context (the two
    inverses differ by rounding; 2 keeps a residual that sits on the threshold from flaking); |y - numpy.linalg.solve| <= 1e-6 kappa
    |y_ref| at tol 1e-12.

    Measured on an MI355X: DESIGN.md 4o."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("two_level", G)
    A, f3, M, shift, fm = dense_setup(name, s, c, True, G=G)
    rhs = _rhs(c)
    res = {}
    for tol in (1e-12, 1e-8):
        for solver in ("blocked", "one_block"):
            s.set_tangent_coarse(solver)
            res[tol, solver] = _check_solve(s, c, c["x"], rhs, tol=tol)
            assert s.tangent_precond()["coarse_ok"]
    s.close()
    Af = A[np.ix_(f3, f3)]
    ref = np.linalg.solve(Af, rhs.ravel()[f3])
    kappa = np.linalg.cond(Af)
    err = np.linalg.norm(res[1e-12, "blocked"][0].ravel()[f3] - ref) / np.linalg.norm(ref)
    its = {k: v[1]["iterations"] for k, v in res.items()}
    print("%s, G = %d: iterations %s; |y - y_ref| / |y_ref| = %.3e (bar 1e-6 kappa = %.3e)" % (name, G, its, err, 1e-6 * kappa))
    for tol in (1e-12, 1e-8):
        assert abs(its[tol, "blocked"] - its[tol, "one_block"]) <= 2, its
    assert err <= 1e-6 * kappa, (err, kappa)


@gpu
def test_indefinite_coarse_matrix_falls_back_to_jacobi():
    """psd=False at the compressed state of mixed162 with the blocked inverse: coarse_ok False, the iteration count, the verdict and the
    iterate of the Jacobi run to 1e-12 relative (test_tangent_precond's rule), and the BITS of the one-block run: both leave
    A_c^-1 = 0 and the iteration kernels are the same."""
    s, flat, c, tab = open_case("mixed162")
    rhs = _rhs(c)
    yj, ij = s.tangent_solve(rhs, c["x"], psd=False, tol=1e-10, max_iters=400)
    s.set_tangent_precond("two_level", 4)
    yo, io = s.tangent_solve(rhs, c["x"], psd=False, tol=1e-10, max_iters=400)
    infoo = s.tangent_precond()
    s.set_tangent_coarse("blocked")
    yb, ib = s.tangent_solve(rhs, c["x"], psd=False, tol=1e-10, max_iters=400)
    info = s.tangent_precond()
    s.close()
    print("psd=False at the compressed state: Jacobi %s; one-block %s; blocked %s; %s" % (ij, io, ib, info))
    assert not info["coarse_ok"] and info == infoo and info["coarse_dim"] == 48
    assert ib["iterations"] == ij["iterations"] and ib["converged"] == ij["converged"]
    assert np.linalg.norm(yb - yj) <= 1e-12 * max(np.linalg.norm(yj), 1e-300)
    assert yb.tobytes() == yo.tobytes() and ib == io


# ---------------------------------------------------------------- 4: nothing else moves -------------------------------------------
@gpu
def test_settings_and_bits_of_everything_else():
    """A fresh context: tangent_precond() is its exact dict and tangent_coarse() one_block, tile 64, no launches.  After blocked and
    back to one_block a two-level solve returns the bits it returned before; a Jacobi solve returns its bits before, between and
    after; tangent_coarse_invert in between changes neither; two blocked solves return equal bits."""
    s, flat, c, tab = open_case("mixed750")
    rhs = _rhs(c)
    assert s.tangent_precond() == dict(kind="jacobi", aggregates=0, coarse_dim=0, coarse_dropped=0, coarse_ok=False, setup_passes=0)
    assert s.tangent_coarse() == dict(solver="one_block", tile=T, launches=0)
    yj0, ij0 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.set_tangent_precond("two_level", 8)
    yo0, io0 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.set_tangent_coarse("blocked")
    yb0, ib0 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.tangent_coarse_invert(matrix(T + 1, 1e6))
    yb1, ib1 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    pre = s.tangent_precond()
    s.set_tangent_precond("jacobi")
    yj1, ij1 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.set_tangent_precond("two_level", 8)
    s.set_tangent_coarse("one_block")
    s.tangent_coarse_invert(matrix(T + 1, 1e6))
    yo1, io1 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.set_tangent_precond("jacobi")
    yj2, ij2 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.close()
    assert pre == dict(kind="two_level", aggregates=8, coarse_dim=96, coarse_dropped=0, coarse_ok=True, setup_passes=6)
    assert yj1.tobytes() == yj0.tobytes() == yj2.tobytes() and ij1 == ij0 == ij2
    assert yo1.tobytes() == yo0.tobytes() and io1 == io0
    assert yb1.tobytes() == yb0.tobytes() and ib1 == ib0
    assert abs(ib0["iterations"] - io0["iterations"]) <= 2


@gpu
@pytest.mark.parametrize("linsolver", [0, 1])
def test_blocked_solves_do_not_disturb_a_run(linsolver):
    """2 steps with blocked two-level solves, applications and inverses between them: bit-identical to the same frames without."""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=linsolver)
        s = sc.make_solver()
        xs = []
        for _ in range(2):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                xp = compressed_state(sc.x, 3)
                s.set_tangent_precond("two_level", 4)
                s.set_tangent_coarse("blocked")
                _, info = s.tangent_solve(np.ones_like(xp), xp, tol=1e-8)
                assert info["converged"] and s.tangent_precond()["coarse_ok"] and s.tangent_coarse()["launches"] == launches(48)
                s.tangent_precond_apply(np.ones_like(xp), xp)
                s.tangent_coarse_invert(matrix(12, 1e2))
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


@gpu
def test_blocked_buffers_are_freed_with_the_context():
    """a closed context leaves no device buffer behind: the blocked inverse selected before the first solve, after it, and with the
    aggregates planned again"""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = scenes.mixed_cube_scene(3)
    s = sc.make_solver()
    s.set_tangent_precond("two_level", 4)
    s.tangent_solve(np.ones_like(sc.x), sc.x, tol=1e-8)
    s.set_tangent_coarse("blocked")
    for G in (4, 2):
        s.set_tangent_precond("two_level", G)
        _, info = s.tangent_solve(np.ones_like(sc.x), sc.x, tol=1e-8)
        assert info["converged"] and s.tangent_coarse()["launches"] == launches(12 * G)
    s.tangent_coarse_invert(matrix(T + 1, 1e2))
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)


# ---------------------------------------------------------------- 5: the users of the loop ----------------------------------------
# The polish accepts a step by Armijo's test on two values of the objective Phi.  Phi ~ 1e2 here is a sum of ~1e3 terms of both signs
# (the inertia term against the elastic energy): it carries a rounding of some 1e2 ulp ~ 1e-12, and a Newton step from a gradient g lowers
# it by g . A^-1 g / 2 only.  Two runs whose CG iterates differ in the last digits can be compared state for state only while every
# accepted decrement is far above that rounding; below it the line search halves steps at random (with |g| ~ 1e-8 |m g| as the target
# the cantilever's last decrement is 8e-12, and one of two runs that differ by rounding stalls at |g| ~ 1e-3: measured with both
# inverses' roundings).  So the target is 1e-5 |m g| -- the last decrement is then orders above the rounding (8.5e-6 on the cantilever) -- and
# the test asserts the input condition: every step of both runs was a full step.
POLISH_GRAD_REL = 1e-5


def _polish(name, G, coarse):
    sc = scenes.cube_scene(3, NH, admm_iters=5) if name == "cantilever162" else scenes.mixed_cube_scene(5, admm_iters=5)
    s = sc.make_solver()
    s.set_tangent_precond("two_level", G)
    s.set_tangent_coarse(coarse)
    s.step()
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    fm = np.ones(len(sc.x), bool); fm[sorted(sc.pins)] = False
    grad_tol = POLISH_GRAD_REL * np.linalg.norm((m3.reshape(-1, 3) * 9.8)[fm])
    rec = s.newton_polish(max_iters=20, grad_tol=grad_tol, cg_tol=1e-10, cg_max=2000)
    x = s.m_x.reshape(-1, 3).copy()
    co = s.tangent_coarse()
    s.close()
    return sc, rec, x, grad_tol, co


@gpu
@pytest.mark.parametrize("name,G", [("cantilever162", 4), ("mixed750", 16)])
def test_newton_polish_with_blocked(name, G):
    """The polish with the blocked inverse reaches the one-block polish's x to 1e-10 of the bounding box (the bar of
    test_newton_polish_with_two_level) and meets the gradient tolerance, in full Newton steps (POLISH_GRAD_REL above)."""
    sc, ro, xo, grad_tol, coo = _polish(name, G, "one_block")
    _, rb, xb, _, cob = _polish(name, G, "blocked")
    dist = np.abs(xb - xo).max() / np.ptp(sc.x, axis=0).max()
    co, cb = [r["cg_iterations"] for r in ro], [r["cg_iterations"] for r in rb]
    print("%s, G = %d: CG iterations one-block %s, blocked %s; gradients %s, %s; max |x - x_one_block| / box = %.3e (bar 1e-10)"
          % (name, G, co, cb, ["%.2e" % r["grad_norm"] for r in ro], ["%.2e" % r["grad_norm"] for r in rb], dist))
    assert ro[-1]["grad_norm"] <= grad_tol and rb[-1]["grad_norm"] <= grad_tol
    assert len(ro) == len(rb) >= 3 and all(r["step"] == 1.0 for r in ro[:-1] + rb[:-1])      # the input condition: full steps, at least two
    assert cob == dict(solver="blocked", tile=T, launches=launches(12 * G)) and coo["launches"] == 1
    assert dist <= 1e-10, dist


@gpu
@pytest.mark.parametrize("name,G", [("cantilever162", 4), ("mixed750", 16)])
def test_step_adjoint_with_blocked(name, G):
    """step_adjoint's lam with the blocked inverse against the dense numpy adjoint of test_adjoint.py: |lam - ref| <= 1e-6 kappa |ref|,
    and the iteration count within 2 of the one-block run's."""
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished(name)
    dt = s._settings.timestep_s
    flat = s.flatten()
    x = s.m_x.reshape(-1, 3).copy()
    rng = np.random.default_rng(61)
    Lx = rng.standard_normal(x.shape); Lv = rng.standard_normal(x.shape)
    s.set_tangent_precond("two_level", G)
    oo = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000, params=False)
    s.set_tangent_coarse("blocked")
    ob = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000, params=False)
    info, co = s.tangent_precond(), s.tangent_coarse()
    s.close()
    ref = numpy_adjoint(flat, sc.x, x, xbar, m3, dt, fm, Lx, Lv, tri_k)
    err = np.linalg.norm(ob["lam"] - ref["lam"]) / np.linalg.norm(ref["lam"])
    print("%s step_adjoint: %d iterations with one-block, %d with blocked; |lam - ref| / |ref| = %.3e (bar 1e-6 kappa = %.3e); %s %s"
          % (name, oo["info"]["iterations"], ob["info"]["iterations"], err, 1e-6 * ref["kappa"], info, co))
    assert info["coarse_ok"] and ob["info"]["converged"] and co["launches"] == launches(12 * G)
    assert abs(ob["info"]["iterations"] - oo["info"]["iterations"]) <= 2
    assert err <= 1e-6 * ref["kappa"], (err, ref["kappa"])


# ---------------------------------------------------------------- 6: argument checks ----------------------------------------------
@gpu
def test_refusals():
    """An unknown solver name and solver numbers outside 0 .. 1 are refused and leave the setting; tangent_coarse_invert refuses n = 0
    and n = 769, a matrix that is not square, NULL; a multi-GPU context refuses both."""
    sc = scenes.cube_scene(1, NH)
    s = sc.make_solver()
    s.set_tangent_coarse("blocked")
    with pytest.raises(ValueError):
        s.set_tangent_coarse("lu")
    for solver in (2, -1):
        with pytest.raises(capi.AdmmHipError) as e:
            capi.check(capi.lib().admm_hip_set_tangent_coarse(s._ctx, solver))
        assert e.value.code == -1, e.value
    assert s.tangent_coarse()["solver"] == "blocked"
    for bad in (np.zeros((0, 0)), np.eye(769), np.ones((3, 4))):
        with pytest.raises(ValueError):
            s.tangent_coarse_invert(bad)
    A = np.eye(4); X = np.zeros((4, 4)); ok = C.c_int32(0); dr = C.c_int32(0)
    dp = C.POINTER(C.c_double)
    for n, a in ((0, A), (769, A), (-3, A), (4, None)):
        with pytest.raises(capi.AdmmHipError) as e:
            capi.check(capi.lib().admm_hip_tangent_coarse_invert(s._ctx, n, a.ctypes.data_as(dp) if a is not None else None, X.ctypes.data_as(dp),
                                                                 C.byref(ok), C.byref(dr)))
        assert e.value.code == -1, e.value
    s.close()
    s = sc.make_solver(world_size=2, rank=0)
    with pytest.raises(capi.AdmmHipError) as e:
        s.set_tangent_coarse("blocked")
    assert e.value.code == -1, e.value
    with pytest.raises(capi.AdmmHipError):
        s.tangent_coarse_invert(np.eye(4))
    s.close()
