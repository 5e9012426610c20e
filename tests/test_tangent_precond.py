"""The two-level preconditioner of the tangent solves (csrc/tangent_precond.hpp; Solver.set_tangent_precond) on the GPU, against numpy.

THE REFERENCE is test_newton.py's: the scenes of `case`, the dense projected stiffness of `dense_K` (through `reference`, computed once and
shared with test_newton.py), `free_mask`, `compressed_state`, `_rhs`.  From it, the plan of Solver.tangent_plan (the aggregates the device
uses: the same host function, on the same rest positions) and the positions the tangent is frozen at, numpy builds P -- 12 columns per
aggregate, {1, (x - mean) / h} (x) {e_x, e_y, e_z}, zero on held vertices -- and M^-1 = D^-1 + P (P^T A P)^-1 P^T densely, with the
library's drop rule (diagonal <= 2^-40 of the largest).

aggregates = 4 on mixed162 and 8 on mixed750 and cloth: the default would be 1 there and leave the coupling between aggregates untested."""
import ctypes as C

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi
from admm_elastic_amd.solver import Solver
from test_adjoint import numpy_adjoint, polished
from test_newton import _rhs, case, compressed_state, free_mask, open_case, reference

gpu = pytest.mark.gpu
AGG = {"mixed162": 4, "mixed750": 8, "cloth": 8}
NH = pkg.TET_NEOHOOKEAN


# ---------------------------------------------------------------- the dense preconditioner ----------------------------------------
def basis(x, ptr, vert, fm):
    """P [3 nv, 12 G] at the positions x"""
    nv, G = len(x), len(ptr) - 1
    P = np.zeros((3 * nv, 12 * G))
    for g in range(G):
        a = vert[ptr[g]:ptr[g + 1]]
        h = np.ptp(x[a], axis=0).max()
        phi = np.concatenate([np.ones((len(a), 1)), (x[a] - x[a].mean(axis=0)) / (h if h > 0 else 1.0)], axis=1) * fm[a][:, None]
        for j in range(4):
            for c in range(3):
                P[3 * a + c, 12 * g + 3 * j + c] = phi[:, j]
    return P


def dense_operator(K, m3, shift, fm):
    """A = K + shift M with the rows and columns of held vertices zeroed"""
    f3 = np.repeat(fm, 3)
    A = (K + shift * np.diag(m3)) * f3[:, None] * f3[None, :]
    return A, f3


class DensePrecond:
    def __init__(self, A, f3, P):
        d = np.diag(A)
        self.dinv = np.where(f3, 1.0 / np.where(f3, d, 1.0), 0.0)
        self.f3, self.P = f3, P
        Ac = P.T @ A @ P
        Ac = 0.5 * (Ac + Ac.T)
        dc = np.diag(Ac)
        self.keep = dc > 2.0 ** -40 * dc.max()
        self.dropped = int((~self.keep).sum())
        sub = Ac[np.ix_(self.keep, self.keep)]
        self.cond = np.linalg.cond(sub)
        self.X = np.zeros_like(Ac)
        self.X[np.ix_(self.keep, self.keep)] = np.linalg.inv(sub)

    def __call__(self, r):
        r = np.where(self.f3, r, 0.0)
        return self.dinv * r + self.P @ (self.X @ (self.P.T @ r))

    def jacobi(self, r):
        return self.dinv * np.where(self.f3, r, 0.0)


def numpy_pcg(A, apply_M, b, tol, max_iters=5000):
    """the iteration of tangent_solve_device: stop at |r| <= tol |b| on the recursive residual; -> iterations"""
    y = np.zeros_like(b); r = b.copy(); z = apply_M(r); p = z.copy(); rz = r @ z; bb = b @ b
    for it in range(1, max_iters + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        y += alpha * p; r -= alpha * Ap
        if r @ r <= tol * tol * bb:
            return it
        z = apply_M(r); rz_new = r @ z
        p = z + (rz_new / rz) * p; rz = rz_new
    return max_iters


def dense_setup(name, s, c, hold, x=None, G=None):
    _, K, _ = reference(name)
    shift = 1.0 / s._settings.timestep_s ** 2
    fm = free_mask(c) if hold else np.ones(len(c["rest"]), bool)
    A, f3 = dense_operator(K, np.asarray(s.m_masses, dtype=np.float64), shift, fm)
    ptr, vert = Solver.tangent_plan(c["rest"], G or AGG[name])
    return A, f3, DensePrecond(A, f3, basis(c["x"] if x is None else x, ptr, vert, fm)), shift, fm


# ---------------------------------------------------------------- 1: the application against numpy --------------------------------
@gpu
@pytest.mark.parametrize("hold", [True, False])
@pytest.mark.parametrize("name", ["mixed162", "mixed750", "cloth"])
def test_application_against_numpy(name, hold):
    """z = M^-1 r from the device against D^-1 r + P (P^T A P)^-1 P^T r built densely: |z - z_ref| <= 1e-10 cond(A_c) |z_ref|, cond(A_c)
    numpy's condition number of the coarse matrix (the error of applying an inverse).  shift = 1 / dt^2, the pins held and not.

    Measured on an MI355X: DESIGN.md 4o."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("jacobi", AGG[name])      # (the aggregates; precond_apply applies the two-level operator whatever the kind)
    A, f3, M, shift, fm = dense_setup(name, s, c, hold)
    r = _rhs(c, 43)
    z = s.tangent_precond_apply(r, c["x"], shift=shift, hold_pins=hold)
    info = s.tangent_precond()
    s.close()
    ref = M(r.ravel())
    err = np.linalg.norm(z.ravel() - ref) / np.linalg.norm(ref)
    jac = np.linalg.norm(M.jacobi(r.ravel()) - ref) / np.linalg.norm(ref)
    print("%s, pins %s: |z - z_ref| / |z_ref| = %.3e, cond(A_c) = %.3e, ratio to the bar 1e-10 cond = %.3e; the coarse term is %.2e of |z_ref|; %s"
          % (name, "held" if hold else "free", err, M.cond, err / (1e-10 * M.cond), jac, info))
    assert info["coarse_ok"] and info["coarse_dim"] == 12 * AGG[name] and info["coarse_dropped"] == M.dropped == 0
    assert info["setup_passes"] == -(-12 * AGG[name] // 16)
    assert jac > 1e-3      # the input condition: the coarse term is not negligible
    assert err <= 1e-10 * M.cond, (err, M.cond)


# ---------------------------------------------------------------- 2: symmetric and positive ---------------------------------------
@gpu
@pytest.mark.parametrize("name", ["mixed750", "cloth"])
def test_symmetric_and_positive(name):
    """r1 . M^-1 r2 = r2 . M^-1 r1 to 1e-12 |r1| |M^-1 r2|, r . M^-1 r > 0 for 8 random r, z = 0 on held vertices."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("two_level", AGG[name])
    rng = np.random.default_rng(47)
    R = rng.standard_normal((8,) + c["x"].shape)
    Z = np.stack([s.tangent_precond_apply(r, c["x"]) for r in R])
    s.close()
    fm = free_mask(c)
    assert (Z[:, ~fm] == 0.0).all() and (~fm).any()
    Rm = R.copy(); Rm[:, ~fm] = 0.0
    worst = 0.0
    for i in range(8):
        assert np.sum(Rm[i] * Z[i]) > 0.0, i
        for j in range(i):
            a = abs(np.sum(Rm[i] * Z[j]) - np.sum(Rm[j] * Z[i])) / (np.linalg.norm(Rm[i]) * np.linalg.norm(Z[j]))
            worst = max(worst, a)
    print("%s: asymmetry %.3e (bar 1e-12), lowest r . M^-1 r / |r|^2 = %.3e" % (name, worst, min(np.sum(Rm[i] * Z[i]) / np.sum(Rm[i] ** 2) for i in range(8))))
    assert worst <= 1e-12, worst


# ---------------------------------------------------------------- 3: the solve is a solve ------------------------------------------
def _check_solve(s, c, x, rhs, tol=1e-12):
    fm = free_mask(c)
    shift = 1.0 / s._settings.timestep_s ** 2
    y, info = s.tangent_solve(rhs, x, tol=tol, max_iters=2000)
    r = (rhs - s.stiffness_apply_ex(y, x, shift=shift, psd=True, hold_pins=True))[fm]
    rel = np.linalg.norm(r) / np.linalg.norm(rhs[fm])
    print("two-level: %d iterations, converged %s, |r| / |rhs| reported %.3e recomputed %.3e (bar %.0e); %s"
          % (info["iterations"], info["converged"], info["residual"], rel, 2 * tol, s.tangent_precond()))
    assert info["converged"] and info["residual"] <= 2 * tol
    assert rel <= 2 * tol, rel
    assert abs(info["residual"] - rel) <= 1e-6 * rel, (info["residual"], rel)
    assert (y[~fm] == 0.0).all()
    return y, info


@gpu
@pytest.mark.parametrize("name", ["mixed162", "mixed750", "cloth"])
def test_two_level_solve_residual(name):
    """The bar of test_newton.test_tangent_solve_residual with the two-level preconditioner: tol = 1e-12, the reported true residual
    <= 2 tol |rhs| and equal to the recomputed one to 1e-6 relative; y = 0 on held vertices."""
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("two_level", AGG[name])
    _check_solve(s, c, c["x"], _rhs(c))
    assert s.tangent_precond()["coarse_ok"]
    s.close()


@gpu
def test_two_level_solve_against_dense_solve():
    """162 tets: |y - numpy.linalg.solve| <= 1e-6 kappa |y_ref| (test_newton.test_tangent_solve_against_dense_solve's rule)."""
    name = "mixed162"
    s, flat, c, tab = open_case(name)
    s.set_tangent_precond("two_level", AGG[name])
    A, f3, M, shift, fm = dense_setup(name, s, c, True)
    rhs = _rhs(c)
    y, info = s.tangent_solve(rhs, c["x"], tol=1e-12, max_iters=2000)
    s.close()
    Af = A[np.ix_(f3, f3)]
    ref = np.linalg.solve(Af, rhs.ravel()[f3])
    kappa = np.linalg.cond(Af)
    err = np.linalg.norm(y.ravel()[f3] - ref) / np.linalg.norm(ref)
    print("two-level tangent_solve against numpy.linalg.solve: |y - y_ref| / |y_ref| = %.3e, kappa = %.3e (bar %.3e), %d iterations"
          % (err, kappa, 1e-6 * kappa, info["iterations"]))
    assert info["converged"]
    assert err <= 1e-6 * kappa, (err, kappa)


# ---------------------------------------------------------------- 4: iterations ---------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["mixed750", "cloth"])
def test_iterations(name):
    """tol = 1e-8: iterations(two_level) <= 0.6 iterations(jacobi), both from the same run (the Jacobi path is the parent's); and the
    device's two-level count exceeds that of a numpy PCG with the same dense preconditioner by no more than the device's Jacobi count
    exceeds numpy's Jacobi count, plus 2.

    Measured on an MI355X: DESIGN.md 4o."""
    s, flat, c, tab = open_case(name)
    rhs = _rhs(c)
    _, ij = s.tangent_solve(rhs, c["x"], tol=1e-8, max_iters=4000)
    s.set_tangent_precond("two_level", AGG[name])
    _, it = s.tangent_solve(rhs, c["x"], tol=1e-8, max_iters=4000)
    ok = s.tangent_precond()["coarse_ok"]
    A, f3, M, shift, fm = dense_setup(name, s, c, True)
    s.close()
    b = np.where(f3, rhs.ravel(), 0.0)
    nj = numpy_pcg(A, M.jacobi, b, 1e-8)
    nt = numpy_pcg(A, M, b, 1e-8)
    print("%s: device Jacobi %d, two-level %d (ratio %.3f, bar 0.6); numpy Jacobi %d, two-level %d; device - numpy: Jacobi %+d, two-level %+d"
          % (name, ij["iterations"], it["iterations"], it["iterations"] / ij["iterations"], nj, nt, ij["iterations"] - nj, it["iterations"] - nt))
    assert ij["converged"] and it["converged"] and ok
    assert it["iterations"] <= 0.6 * ij["iterations"], (it["iterations"], ij["iterations"])
    assert it["iterations"] - nt <= ij["iterations"] - nj + 2


# ---------------------------------------------------------------- 5: fall-backs and drops -----------------------------------------
@gpu
def test_indefinite_coarse_matrix_falls_back_to_jacobi():
    """psd=False at the compressed state of mixed162: coarse_ok == 0, the iteration count and `converged` of the Jacobi run, y equal to
    1e-12 relative."""
    s, flat, c, tab = open_case("mixed162")
    rhs = _rhs(c)
    yj, ij = s.tangent_solve(rhs, c["x"], psd=False, tol=1e-10, max_iters=400)
    s.set_tangent_precond("two_level", 4)
    yt, it = s.tangent_solve(rhs, c["x"], psd=False, tol=1e-10, max_iters=400)
    info = s.tangent_precond()
    s.close()
    print("psd=False at the compressed state: Jacobi %s; two-level %s; %s" % (ij, it, info))
    assert not info["coarse_ok"] and info["coarse_dim"] == 48
    assert it["iterations"] == ij["iterations"] and it["converged"] == ij["converged"]
    assert np.linalg.norm(yt - yj) <= 1e-12 * max(np.linalg.norm(yj), 1e-300)


@gpu
def test_free_body_without_shift_falls_back_and_with_shift_does_not():
    """A cube nothing holds, hold_pins=False: with shift = 0 the translations are a null space of A inside the span of P -- coarse_ok == 0
    and the call ends as the Jacobi call does (the same verdict and count, a finite y); with shift = 1 / dt^2, coarse_ok == 1 and the
    solve converges in fewer iterations than Jacobi."""
    sc = scenes.cube_scene(3, NH, pin_face=False)
    s = sc.make_solver()
    x = compressed_state(sc.x, 3)
    rhs = np.random.default_rng(41).standard_normal(x.shape)
    yj0, ij0 = s.tangent_solve(rhs, x, shift=0.0, hold_pins=False, tol=1e-8, max_iters=300)
    yj1, ij1 = s.tangent_solve(rhs, x, hold_pins=False, tol=1e-8, max_iters=2000)
    s.set_tangent_precond("two_level", 4)
    yt0, it0 = s.tangent_solve(rhs, x, shift=0.0, hold_pins=False, tol=1e-8, max_iters=300)
    info0 = s.tangent_precond()
    yt1, it1 = s.tangent_solve(rhs, x, hold_pins=False, tol=1e-8, max_iters=2000)
    info1 = s.tangent_precond()
    s.close()
    print("shift 0: Jacobi %s, two-level %s, %s\nshift 1 / dt^2: Jacobi %s, two-level %s, %s" % (ij0, it0, info0, ij1, it1, info1))
    assert not info0["coarse_ok"]
    assert np.isfinite(yt0).all() and np.isfinite(it0["residual"])
    assert (it0["iterations"], it0["converged"]) == (ij0["iterations"], ij0["converged"])
    assert np.linalg.norm(yt0 - yj0) <= 1e-12 * max(np.linalg.norm(yj0), 1e-300)
    assert info1["coarse_ok"] and info1["coarse_dropped"] == 0
    assert ij1["converged"] and it1["converged"] and it1["iterations"] < ij1["iterations"]


@gpu
def test_flat_cloth_drops_three_columns_per_aggregate():
    """The cloth at its flat rest state: the affine function of the normal coordinate vanishes, its three columns per aggregate are
    dropped (coarse_dropped == 3 G) and the solve meets the bars of test_two_level_solve_residual."""
    s, flat, c, tab = open_case("cloth")
    x = np.array(c["rest"], dtype=np.float64)
    assert (np.ptp(x, axis=0) == 0.0).sum() == 1      # the input condition: exactly flat
    s.set_tangent_precond("two_level", 8)
    _check_solve(s, c, x, _rhs(c))
    info = s.tangent_precond()
    s.close()
    assert info["coarse_ok"] and info["coarse_dropped"] == 24, info


@gpu
def test_held_aggregate_drops_its_twelve_columns():
    """The 162-tet cube with every vertex of aggregate 0 of its 4-aggregate plan pinned: that aggregate's 12 columns are dropped."""
    sc = scenes.cube_scene(3, NH, pin_face=False)
    ptr, vert = Solver.tangent_plan(sc.x, 4)
    for v in vert[ptr[0]:ptr[1]]:
        sc.pins[int(v)] = sc.x[v].copy()
    s = sc.make_solver()
    s.set_tangent_precond("two_level", 4)
    c = dict(rest=sc.x, pins=sorted(sc.pins))
    _check_solve(s, c, compressed_state(sc.x, 3), np.random.default_rng(41).standard_normal(sc.x.shape))
    info = s.tangent_precond()
    s.close()
    assert info["coarse_ok"] and info["coarse_dropped"] == 12 and info["coarse_dim"] == 48, info


# ---------------------------------------------------------------- 6: the users of the loop -----------------------------------------
def _polish(name, G):
    sc = scenes.cube_scene(3, NH, admm_iters=5) if name == "cantilever162" else scenes.mixed_cube_scene(5, admm_iters=5)
    s = sc.make_solver()
    if G:
        s.set_tangent_precond("two_level", G)
    s.step()
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    fm = np.ones(len(sc.x), bool); fm[sorted(sc.pins)] = False
    grad_tol = 1e-8 * np.linalg.norm((m3.reshape(-1, 3) * 9.8)[fm])
    rec = s.newton_polish(max_iters=20, grad_tol=grad_tol, cg_tol=1e-10, cg_max=2000)
    x = s.m_x.reshape(-1, 3).copy()
    s.close()
    return sc, rec, x, grad_tol


@gpu
@pytest.mark.parametrize("name,G", [("cantilever162", 4), ("mixed750", 8)])
def test_newton_polish_with_two_level(name, G):
    """The polish of test_newton.test_newton_polish with the two-level preconditioner reaches the Jacobi polish's x to 1e-10 of the
    bounding box, with a smaller sum of cg_iterations."""
    sc, rj, xj, grad_tol = _polish(name, 0)
    _, rt, xt, _ = _polish(name, G)
    dist = np.abs(xt - xj).max() / np.ptp(sc.x, axis=0).max()
    cj, ct = [r["cg_iterations"] for r in rj], [r["cg_iterations"] for r in rt]
    print("%s: CG iterations Jacobi %s = %d, two-level %s = %d; max |x - x_jacobi| / box = %.3e (bar 1e-10)" % (name, cj, sum(cj), ct, sum(ct), dist))
    assert rj[-1]["grad_norm"] <= grad_tol and rt[-1]["grad_norm"] <= grad_tol
    assert dist <= 1e-10, dist
    assert sum(ct) < sum(cj)


@gpu
def test_step_adjoint_with_two_level():
    """step_adjoint's lam with the two-level preconditioner against the dense numpy adjoint of test_adjoint.py: |lam - ref| <= 1e-6
    kappa |ref|."""
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished("cantilever162")
    dt = s._settings.timestep_s
    flat = s.flatten()
    x = s.m_x.reshape(-1, 3).copy()
    rng = np.random.default_rng(61)
    Lx = rng.standard_normal(x.shape); Lv = rng.standard_normal(x.shape)
    oj = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000, params=False)
    s.set_tangent_precond("two_level", 4)
    ot = s.step_adjoint(Lx, Lv, tol=1e-12, max_iters=4000, params=False)
    info = s.tangent_precond()
    s.close()
    ref = numpy_adjoint(flat, sc.x, x, xbar, m3, dt, fm, Lx, Lv, tri_k)
    err = np.linalg.norm(ot["lam"] - ref["lam"]) / np.linalg.norm(ref["lam"])
    print("step_adjoint: %d iterations with Jacobi, %d with two-level; |lam - ref| / |ref| = %.3e (bar 1e-6 kappa = %.3e); %s"
          % (oj["info"]["iterations"], ot["info"]["iterations"], err, 1e-6 * ref["kappa"], info))
    assert info["coarse_ok"] and ot["info"]["converged"]
    assert ot["info"]["iterations"] < oj["info"]["iterations"]
    assert err <= 1e-6 * ref["kappa"], (err, ref["kappa"])


# ---------------------------------------------------------------- 7: nothing else moves -------------------------------------------
@gpu
def test_jacobi_bits_before_and_after_and_two_level_repeats():
    """A solve before the feature is ever switched on and one after two_level followed by jacobi return equal bits; two identical
    two-level solves return equal bits (of y, of the info and of the application)."""
    s, flat, c, tab = open_case("mixed750")
    rhs = _rhs(c)
    y0, i0 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    assert s.tangent_precond() == dict(kind="jacobi", aggregates=0, coarse_dim=0, coarse_dropped=0, coarse_ok=False, setup_passes=0)
    s.set_tangent_precond("two_level", 8)
    y1, i1 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    z1 = s.tangent_precond_apply(rhs, c["x"])
    y2, i2 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    z2 = s.tangent_precond_apply(rhs, c["x"])
    s.set_tangent_precond("jacobi")
    y3, i3 = s.tangent_solve(rhs, c["x"], tol=1e-10)
    s.close()
    assert y3.tobytes() == y0.tobytes() and i3 == i0
    assert y2.tobytes() == y1.tobytes() and i2 == i1 and z2.tobytes() == z1.tobytes()
    assert y1.tobytes() != y0.tobytes() and i1["iterations"] < i0["iterations"]


@gpu
def test_a_zero_solve_after_a_two_level_solve_that_ended_on_an_odd_iteration():
    """test_tangent_block's test of the same name with the two-level preconditioner: a right-hand side of zero ends at the set-up of the
    solve -- 0 iterations, y = 0, residual 0, rhs_norm 0 -- whatever parity the solve before it left its scalars at (solves of 1 .. 6
    iterations before it), as a single call and as the columns of a block call (which goes column by column here: blocked is False)."""
    s, flat, c, tab = open_case("mixed162")
    s.set_tangent_precond("two_level", aggregates=AGG["mixed162"])
    rhs = _rhs(c)
    zero = np.zeros_like(rhs)
    want = dict(iterations=0, converged=True, residual=0.0, rhs_norm=0.0)
    for n in range(1, 7):
        _, i0 = s.tangent_solve(rhs, c["x"], tol=1e-12, max_iters=n)
        assert i0["iterations"] == n
        y, i1 = s.tangent_solve(zero, c["x"])
        print("two-level, %d iterations, then zero: %s" % (n, i1))
        assert i1 == want and not y.any(), (n, i1)
        s.tangent_solve_block(np.stack([rhs, 0.5 * rhs]), c["x"], tol=1e-12, max_iters=n)
        Y, ib = s.tangent_solve_block(np.stack([zero, zero]), c["x"])
        print("two-level, block of two, %d iterations, then zeros: %s" % (n, ib))
        assert ib["columns"] == [want, want] and not Y.any(), (n, ib)
        assert not ib["blocked"] and ib["column_passes"] == 0 and ib["block_iterations"] == 0, (n, ib)
    s.close()


@gpu
@pytest.mark.parametrize("linsolver", [0, 1])
def test_two_level_solves_do_not_disturb_a_run(linsolver):
    """3 steps (linsolver 0: the on-chip PCG; 1: the GS sweeps) with two-level solves and applications at an explicit x between the steps:
    bit-identical to the same run without them (test_newton.test_solve_and_projected_apply_do_not_disturb_a_run)."""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=linsolver)
        s = sc.make_solver()
        xs = []
        for _ in range(3):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                xp = compressed_state(sc.x, 3)
                s.set_tangent_precond("two_level", 4)
                _, info = s.tangent_solve(np.ones_like(xp), xp, tol=1e-8)
                assert info["converged"] and s.tangent_precond()["coarse_ok"]
                s.tangent_precond_apply(np.ones_like(xp), xp)
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


@gpu
def test_two_level_buffers_are_freed_with_the_context():
    """a closed context leaves no device buffer behind, also after the aggregates were planned twice"""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = scenes.mixed_cube_scene(3)
    s = sc.make_solver()
    for G in (4, 2):
        s.set_tangent_precond("two_level", G)
        s.tangent_solve(np.ones_like(sc.x), sc.x, tol=1e-8)
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)


# ---------------------------------------------------------------- 8: refusals -----------------------------------------------------
@gpu
def test_refusals():
    """aggregates = 65, more aggregates than vertices, kind = 2 and a multi-GPU context are refused (ADMM_HIP_ERR_ARG) and leave the
    setting as it was."""
    sc = scenes.cube_scene(1, NH)
    s = sc.make_solver()
    s.set_tangent_precond("two_level", 2)
    for kind, G in ((1, 65), (1, -1), (2, 0), (-1, 0), (1, 9)):
        with pytest.raises(capi.AdmmHipError) as e:
            capi.check(capi.lib().admm_hip_set_tangent_precond(s._ctx, kind, G))
        assert e.value.code == -1, e.value
    with pytest.raises(ValueError):
        s.set_tangent_precond("ssor")
    assert s.tangent_precond()["kind"] == "two_level" and s.tangent_precond()["aggregates"] == 2
    s.close()
    s = sc.make_solver(world_size=2, rank=0)
    with pytest.raises(capi.AdmmHipError) as e:
        s.set_tangent_precond("two_level")
    assert e.value.code == -1, e.value
    s.close()
