"""Modal analysis on the device (csrc/modal.hpp, admm_hip_modes) and the block frozen pass under it (csrc/newton.hpp:
k_tangent_frozen_block, stiffness_apply_ex(block=True)).

THE REFERENCE is numpy on the CPU: numpy.linalg.eigh of M^-1/2 A M^-1/2 on the free rows, A the dense matrix assembled from
stiffness_apply_ex on the unit vectors (symmetrised), or test_newton.dense_K where a test says so.

THE CASES are chosen by a condition that needs no GPU (test_cases_are_well_posed, on test_newton.dense_K): a plain numpy model of the
device's iteration (numpy_lobpcg below: the same start block, Jacobi preconditioner, [X W P] Rayleigh-Ritz with the unit-diagonal
scaling, the Cholesky pivot rule and the restart rule, the same stop test) converges to tol within max_iters with zero restarts, and
lambda_k and lambda_{k+1} of the numpy spectrum are separated by a relative gap >= 1e-3.

Meshes (test_newton.case): 162 tets (one partial chunk), mixed750 (three chunks with a partial last one, three kinds), the 12 x 12 cloth
(triangles + hinges), a tabulated-spline cube; all at their compressed states.

MEASURED on an MI355X / ASSERTED at 10 x: BOUNDS below holds (measured, asserted) per figure; every test prints its figures before it
asserts.  Iterations at tol = 1e-8, k = 4 + 4 columns: 162 tets 65, mixed750 147, cloth (shift 1 / dt^2) 268, the free cube (k = 8 + 4) 74,
the indefinite 162-tet state 45; no restarts."""
import functools

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi
from test_newton import case, dense_K, free_mask, open_case

gpu = pytest.mark.gpu

TOL = 1e-8
K_MODES, GUARD = 4, 4      # (k = 6 with 4 guard columns fails the condition below on the 162- and 750-tet meshes: see test_cases_are_well_posed)
IDT2 = 576.0      # 1 / dt^2 of the scenes (dt = 1 / 24)
# The shifts the condition below selects.  cloth: at shift 0 the numpy model stalls above tol (2000 iterations; its Ritz values are
# right to 2e-13) -- the modes of the implicit-Euler Hessian K + M / dt^2 converge in 288.  The indefinite 162-tet state: at shift 0 the
# Jacobi diagonal has negative entries and the model does not converge; with shift = 1e6 > |lambda_min| = 4.1e5 it needs 45 iterations,
# and lambda = theta - shift is negative all the same.
SHIFT = {"mixed162": 0.0, "mixed750": 0.0, "cloth": IDT2, "rigid": IDT2, "mixed162-indefinite": 1.0e6}

# name -> (measured on an MI355X: the largest over the test's cases, asserted = 10 x measured)
BOUNDS = {
    "lam": (2.5e-13, 2.5e-12),             # |lambda_i - ref| / lambda_k          (mixed162 1.5e-14, mixed750 7.1e-14, cloth 2.5e-13)
    "orth": (4.5e-16, 4.5e-15),            # |Phi^T M Phi - I|_max                (2 eps on all three)
    "subspace": (3.7e-09, 3.7e-08),        # |(I - Phi_ref Phi_ref^T M) phi_i|_M  (6.4e-10, 7.8e-10, 3.7e-9: tol times theta / gap)
    "resid_agree": (1.42e-08, 1.42e-07),       # reported against recomputed residual, relative (residuals of 1e-9: eps / 1e-9 each)
    "neg_lam": (1.17e-08, 1.17e-07),       # against the difference-quotient dense_K (whose own error is 1e-6 per element)
    "rigid": (1.7e-15, 1.7e-14),           # |lambda_rigid| / lambda_7
    "rigid_lam": (9.5e-16, 9.5e-15),       # |lambda_{7,8} - ref| / lambda_8 (a degenerate pair)
    # Ritz values after 1 and 5 iterations lie 2 .. 20 times above numpy's eigenvalues: measured 0 below.  Asserted: the error of the
    # reference itself, eigh on 144 unknowns with cond 650: 144 eps cond = 2e-11 of lambda_k (not derived from the device's figures)
    "ritz_above": (0.0, 2e-11),
    # device 65, model 65 (mixed750: 147 / 148, cloth 268 / 268 on dense_K).  Asserted: ITER_SPREAD, what the CPU condition allows the
    # model itself to move under rounding-level noise -- 10 x the measured 0 would assert bit-equal trajectories of two summation orders
    "iters": (0, 3),
}


# ---------------------------------------------------------------- the start block and the numpy model ------------------------------
def start_block(nb, nv):
    """the library's default start block (device_math.hpp: modal_start), restated: [nb, nv, 3] in (-1, 1)"""
    c = np.arange(nb, dtype=np.uint64)[:, None, None]; v = np.arange(nv, dtype=np.uint64)[None, :, None]; j = np.arange(3, dtype=np.uint64)[None, None, :]
    M32 = np.uint64(0xFFFFFFFF)
    h = (c * np.uint64(0x9E3779B1) + v * np.uint64(0x85EBCA77) + j * np.uint64(0xC2B2AE3D)) & M32
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x7FEB352D)) & M32
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x846CA68B)) & M32
    h ^= h >> np.uint64(16)
    return (h.astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0


PIVOT = 64.0 * np.finfo(np.float64).eps


def _rayleigh_ritz(GA, GM, rng=None):
    """the Rayleigh-Ritz of device_math.hpp: modal_geneig, in numpy: None on a failed pivot.  rng: both matrices are perturbed by a
    symmetric relative noise of 1e-15 first (the size of another summation order)"""
    if rng is not None:
        E = 1e-15 * rng.standard_normal(GM.shape); E = 0.5 * (E + E.T)
        GA = GA * (1.0 + E); GM = GM * (1.0 + E)
    d = np.diag(GM)
    if not (np.all(np.isfinite(d)) and np.all(d > 0)):
        return None
    s = 1.0 / np.sqrt(d)
    Ms = GM * s[:, None] * s[None, :]; As = GA * s[:, None] * s[None, :]
    n = len(d)
    L = np.zeros((n, n)); W = Ms.copy()
    for j in range(n):
        p = W[j, j]
        if not (np.isfinite(p) and p >= PIVOT):
            return None
        L[j, j] = np.sqrt(p); L[j + 1:, j] = W[j + 1:, j] / L[j, j]
        W[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    Y = np.linalg.solve(L, As); H = np.linalg.solve(L, Y.T).T
    w, Q = np.linalg.eigh(0.5 * (H + H.T))
    return w, s[:, None] * np.linalg.solve(L.T, Q)


def numpy_lobpcg(A, m, X0, k, tol=TOL, max_iters=2000, rng=None):
    """The device's iteration on a dense symmetric A and the masses m (free rows only).  -> dict(theta, X, iterations, restarts, ended)"""
    def _rr(GA, GM):
        return _rayleigh_ritz(GA, GM, rng)
    nb = X0.shape[1]
    dg = np.diag(A); dinv = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 1.0)
    X = X0.copy(); AX = A @ X
    r = _rr(X.T @ AX, X.T @ (m[:, None] * X))
    if r is None:
        return dict(theta=None, X=X, iterations=0, restarts=0, ended=2)
    th, C = r[0][:nb], r[1][:, :nb]
    X, AX = X @ C, AX @ C
    P = AP = None
    it = restarts = 0; ended = 1
    while it < max_iters:
        MX = m[:, None] * X
        R = AX - MX * th[None, :]
        rn = np.linalg.norm(R, axis=0); mn = np.linalg.norm(MX, axis=0)
        if not np.all(np.isfinite(rn)):
            ended = 2; break
        if np.all(rn[:k] <= tol * np.abs(th[:k]) * mn[:k]):
            ended = 0; break
        W = dinv[:, None] * R; AW = A @ W
        S = np.concatenate([X, W] + ([P] if P is not None else []), axis=1)
        AS = np.concatenate([AX, AW] + ([AP] if P is not None else []), axis=1)
        GA = S.T @ AS; GM = S.T @ (m[:, None] * S)
        r = _rr(GA, GM)
        if r is None and P is not None:
            restarts += 1
            S, AS = S[:, :2 * nb], AS[:, :2 * nb]
            r = _rr(GA[:2 * nb, :2 * nb], GM[:2 * nb, :2 * nb])
        if r is None:
            ended = 2; break
        th, C = r[0][:nb], r[1][:, :nb]
        Cp = C.copy(); Cp[:nb] = 0.0
        X, AX, P, AP = S @ C, AS @ C, S @ Cp, AS @ Cp
        it += 1
    r = _rr(X.T @ AX, X.T @ (m[:, None] * X))
    if r is not None:
        th, C = r[0][:nb], r[1][:, :nb]
        X = X @ C
    return dict(theta=th, X=X, iterations=it, restarts=restarts, ended=ended)


def pencil(A, m):
    """numpy's eigenpairs of A phi = theta M phi: (theta ascending, Phi M-orthonormal)"""
    isq = 1.0 / np.sqrt(m)
    w, V = np.linalg.eigh(0.5 * (A + A.T) * isq[:, None] * isq[None, :])
    return w, isq[:, None] * V


def rel_gap(w, k):
    return (w[k] - w[k - 1]) / max(abs(w[k]), abs(w[k - 1]))


# ---------------------------------------------------------------- the cases: a condition on the CPU --------------------------------
def rigid_scene():
    return scenes.cube_scene(3, pkg.TET_NEOHOOKEAN, pin_face=False)


@functools.lru_cache(None)
def cpu_problem(name, psd=True):
    """(A = dense_K [+ shift M] on the free rows, m free, f3 mask, shift, k) of a case, from an uninitialised Solver: no GPU"""
    if name == "rigid":
        sc = rigid_scene()
        s = sc.make_solver(init=False)
        c = dict(rest=sc.x, x=sc.x, tri_k=None, pins=[])
        k = 8
    else:
        c = case(name)
        s = c["make"](init=False)
        k = K_MODES
    flat = s.flatten()
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    shift = SHIFT[name if psd else name + "-indefinite"]
    assert s._settings.timestep_s == 1.0 / 24.0
    f3 = np.repeat(free_mask(c), 3)
    K = dense_K(flat, c["rest"], c["x"], c["tri_k"], None, psd=psd)
    A = (K + shift * np.diag(m3))[np.ix_(f3, f3)]
    return A, m3[f3], f3, shift, k


CPU_CASES = ["mixed162", "mixed750", "cloth", "rigid", "mixed162-indefinite"]
ITER_SPREAD = 3      # iterations (== BOUNDS["iters"][1]): what the condition allows the model's count to move under rounding-level noise


@pytest.mark.parametrize("name", CPU_CASES)
def test_cases_are_well_posed(name):
    """The condition on the cases, on the CPU: the numpy model converges with zero restarts, and the k-th gap is >= 1e-3.  Also: the
    model does so under five perturbations of its Gram matrices by 1e-15 relative noise, with an iteration count within ITER_SPREAD of
    the unperturbed one -- a case whose count depends on the summation order cannot be compared between the device and numpy.  (The
    iteration without orthogonalisation of W and P reaches a relative residual of about eps cond(G_M), 1e-9 .. 1e-10 on these meshes;
    k = 6 + 4 columns on the 162-tet mesh sit at that edge at tol = 1e-8: 63 iterations, or a restart and 93 .. 97, depending on the noise.
    k = 4 + 4 moves by at most 2 iterations on every mesh here.)"""
    A, m, f3, shift, k = cpu_problem(name.split("-")[0], psd=not name.endswith("indefinite"))
    if name.endswith("indefinite"):
        k = 4
    nv = len(f3) // 3
    nb = k + min(4, 16 - k)
    X0 = start_block(nb, nv).reshape(nb, -1)[:, f3].T
    w, _ = pencil(A, m)
    out = numpy_lobpcg(A, m, X0, k)
    gap = rel_gap(w, k)
    err = np.abs(out["theta"][:k] - w[:k]).max() / abs(w[k - 1])
    print("%s: %d unknowns, k = %d, nb = %d: numpy model %d iterations, %d restarts, ended %d; gap(k) %.3e; |theta - eigh| / |theta_k| %.2e; theta %s"
          % (name, len(m), k, nb, out["iterations"], out["restarts"], out["ended"], gap, err, np.array2string(w[:k] - shift, precision=4)))
    assert out["ended"] == 0 and out["restarts"] == 0 and out["iterations"] < 2000
    assert gap >= 1e-3
    noisy = [numpy_lobpcg(A, m, X0, k, rng=np.random.default_rng(seed)) for seed in range(1, 6)]
    print("    under noise: %s" % [(o["iterations"], o["restarts"]) for o in noisy])
    for o in noisy:
        assert o["ended"] == 0 and o["restarts"] == 0 and abs(o["iterations"] - out["iterations"]) <= ITER_SPREAD
    assert 3 * nb <= len(m)
    if name.endswith("indefinite"):
        assert w[0] - shift < 0.0 < w[0]


# ---------------------------------------------------------------- GPU helpers -----------------------------------------------------
def assemble(s, x, shift, psd, hold_pins):
    """the dense operator of stiffness_apply_ex, column by column through the block pass; symmetrised"""
    nv = s.m_x.size // 3
    D = np.eye(3 * nv).reshape(3 * nv, nv, 3)
    A = s.stiffness_apply_ex(D, x, shift=shift, psd=psd, hold_pins=hold_pins, block=True).reshape(3 * nv, 3 * nv).T
    return 0.5 * (A + A.T)


def directions(shape, n, seed):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(shape))


# ---------------------------------------------------------------- 1: the block pass ------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["mixed162", "mixed750", "cloth", "kind%d" % pkg.TET_SPLINE_TABLE])
def test_block_pass_has_the_single_pass_bits(name):
    """stiffness_apply_ex(block=True) equals block=False byte for byte: n_vec = 1, 2, 7, 16, 17 (17: a second slab), psd on / off, pins
    held or not, shift 0 and 1 / dt^2; and column j of a 7-column block equals the same direction sent alone."""
    s, flat, c, tab = open_case(name)
    x = c["x"]
    idt2 = 1.0 / s._settings.timestep_s ** 2
    D = directions(x.shape, 17, 53)
    for n_vec in (1, 2, 7, 16, 17):
        for psd, hold, shift in ((False, False, 0.0), (True, True, idt2), (True, False, 0.0), (False, True, idt2)):
            a = s.stiffness_apply_ex(D[:n_vec], x, shift=shift, psd=psd, hold_pins=hold, block=True)
            b = s.stiffness_apply_ex(D[:n_vec], x, shift=shift, psd=psd, hold_pins=hold)
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, n_vec, psd, hold, shift)
            assert np.isfinite(a).all() and np.abs(a).max() > 0.0
    blk = s.stiffness_apply_ex(D[:7], x, shift=idt2, psd=True, hold_pins=True, block=True)
    for j in range(7):
        one = s.stiffness_apply_ex(D[j], x, shift=idt2, psd=True, hold_pins=True, block=True)
        assert np.array_equal(one.view(np.uint64), blk[j].view(np.uint64)), j
    s.close()


# ---------------------------------------------------------------- 2: eigenpairs against numpy --------------------------------------
@gpu
@pytest.mark.parametrize("name", ["mixed162", "mixed750", "cloth"])
def test_eigenpairs_against_numpy(name):
    """k = 4 (+ 4 guard columns), pinned vertices held, psd, the compressed state, shift 0 (cloth: 1 / dt^2, see SHIFT), tol 1e-8.  Against numpy's eigh of the
    assembled operator: |lambda_i - ref| / lambda_k; |Phi^T M Phi - I|_max; the M-norm of (I - Phi_ref Phi_ref^T M) phi_i against
    numpy's k lowest vectors; the reported residuals against residuals recomputed through stiffness_apply_ex (relative); phi = 0
    exactly on held vertices.  Input condition, asserted: the k-th gap of numpy's spectrum is >= 1e-3."""
    s, flat, c, tab = open_case(name)
    k = K_MODES
    fm = free_mask(c); f3 = np.repeat(fm, 3)
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    shift = SHIFT[name]
    A = assemble(s, c["x"], shift, True, True)[np.ix_(f3, f3)]
    w, V = pencil(A, m3[f3])
    assert rel_gap(w, k) >= 1e-3
    lam, phi, info = s.modes(k, c["x"], shift=shift, tol=TOL)
    w = w - shift
    P = phi.reshape(k, -1)
    lam_err = np.abs(lam - w[:k]).max() / w[k - 1]
    orth = np.abs((P * m3[None]) @ P.T - np.eye(k)).max()
    Pf = P[:, f3].T
    E = Pf - V[:, :k] @ (V[:, :k].T @ (m3[f3][:, None] * Pf))
    sub = np.sqrt(np.sum(m3[f3][:, None] * E * E, axis=0)).max()
    AP = s.stiffness_apply_ex(phi, c["x"], shift=shift, psd=True, hold_pins=True).reshape(k, -1)
    MP = P * m3[None]
    th = lam + shift
    rec = np.linalg.norm(AP - th[:, None] * MP, axis=1) / (np.abs(th) * np.linalg.norm(MP, axis=1))
    agree = (np.abs(info["residual"] - rec) / rec).max()
    print("%s: %d iterations, %d restarts, ended by %s; lambda %s; |lam - ref| / lam_k %.3e; orth %.3e; subspace %.3e; residuals %s recomputed %s (agree %.3e)"
          % (name, info["iterations"], info["restarts"], info["ended_by"], np.array2string(lam, precision=5), lam_err, orth, sub,
             np.array2string(info["residual"], precision=2), np.array2string(rec, precision=2), agree))
    s.close()
    assert info["converged"] and info["converged_modes"] == k and info["ended_by"] == "tol"
    assert (phi[:, ~fm] == 0.0).all() and np.isfinite(phi).all()
    assert np.allclose(info["frequency_hz"], np.sqrt(np.maximum(lam, 0.0)) / (2 * np.pi), rtol=0, atol=0)
    assert lam_err <= BOUNDS["lam"][1], lam_err
    assert orth <= BOUNDS["orth"][1], orth
    assert sub <= BOUNDS["subspace"][1], sub
    assert agree <= BOUNDS["resid_agree"][1], agree


# ---------------------------------------------------------------- 3: negative modes -------------------------------------------------
@gpu
def test_negative_modes_of_the_unprojected_tangent():
    """162 tets at the compressed, inverted state, psd=False, shift = 1e6 (see SHIFT): lambda_0 = theta_0 - shift < 0 and the k = 4 lowest match eigvalsh of the pencil of the
    unprojected dense_K (a difference-quotient reference: 1e-6 relative of its own); with psd=True lambda_0 >= 0 (the held face removes
    the rigid modes, so no rounding allowance is needed: asserted > 0)."""
    s, flat, c, tab = open_case("mixed162")
    f3 = np.repeat(free_mask(c), 3)
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    shift = SHIFT["mixed162-indefinite"]
    w = pencil(dense_K(flat, c["rest"], c["x"], psd=False)[np.ix_(f3, f3)], m3[f3])[0]
    lam, phi, info = s.modes(4, c["x"], shift=shift, psd=False, tol=TOL)
    err = np.abs(lam - w[:4]).max() / np.abs(w[:4]).max()
    lam_p, _, info_p = s.modes(4, c["x"], psd=True, tol=TOL)
    print("psd=False: lambda %s (numpy %s), |diff| / max |lambda| %.3e, %d iterations ended by %s; psd=True: lambda_0 %.6e"
          % (lam, w[:4], err, info["iterations"], info["ended_by"], lam_p[0]))
    s.close()
    assert w[0] < 0.0 and lam[0] < 0.0
    assert info["converged"] and info_p["converged"]
    assert err <= BOUNDS["neg_lam"][1], err
    assert lam_p[0] > 0.0


# ---------------------------------------------------------------- 4: rigid modes ----------------------------------------------------
@gpu
def test_rigid_modes_of_a_free_body():
    """A free 162-tet Neo-Hookean cube at rest, shift = 1 / dt^2, k = 8: six lambda within rounding of 0 relative to lambda_7 (counting
    from 1), lambda_7 and lambda_8 against numpy's eigh of the assembled operator."""
    sc = rigid_scene()
    s = sc.make_solver()
    shift = SHIFT["rigid"]
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    w = pencil(assemble(s, sc.x, shift, True, True), m3)[0] - shift
    assert rel_gap(w + shift, 8) >= 1e-3
    lam, phi, info = s.modes(8, sc.x, shift=shift, tol=TOL)
    rigid = np.abs(lam[:6]).max() / lam[6]
    el = np.abs(lam[6:] - w[6:8]).max() / w[7]
    print("free cube: lambda %s; numpy %s; rigid |lambda| / lambda_7 %.3e; elastic |diff| / lambda_8 %.3e; %d iterations"
          % (lam, w[:8], rigid, el, info["iterations"]))
    s.close()
    assert info["converged"]
    assert rigid <= BOUNDS["rigid"][1], rigid
    assert el <= BOUNDS["rigid_lam"][1], el


# ---------------------------------------------------------------- 5: Ritz values bound from above ----------------------------------
@gpu
@pytest.mark.parametrize("max_iters", [1, 5])
def test_ritz_values_bound_the_spectrum_from_above(max_iters):
    """Stopped early: converged = False, ended by max_iters, the counts exact, phi finite and M-orthonormal, and theta_i >= lambda_i of
    numpy minus rounding for every i (Cauchy interlacing: Ritz values of a subspace)."""
    s, flat, c, tab = open_case("mixed162")
    k = K_MODES
    f3 = np.repeat(free_mask(c), 3)
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    w = pencil(assemble(s, c["x"], 0.0, True, True)[np.ix_(f3, f3)], m3[f3])[0]
    lam, phi, info = s.modes(k, c["x"], tol=TOL, max_iters=max_iters)
    below = max(0.0, ((w[:k] - lam) / w[k - 1]).max())
    print("max_iters = %d: lambda %s above numpy's %s; lowest (ref - lambda) / lambda_k = %.3e; %s" % (max_iters, lam, w[:k], below, info))
    s.close()
    assert not info["converged"] and info["ended_by"] == "max_iters"
    assert info["iterations"] == max_iters and info["restarts"] == 0 and info["converged_modes"] == 0
    assert np.isfinite(phi).all() and np.isfinite(lam).all()
    assert below <= BOUNDS["ritz_above"][1], below


# ---------------------------------------------------------------- 6: reproducible ---------------------------------------------------
@gpu
def test_modes_are_bit_reproducible():
    """two calls on one context, a call on a fresh context, and a caller's init equal to the default start block: identical bytes"""
    name = "mixed750"
    s, flat, c, tab = open_case(name)
    k = K_MODES
    a = s.modes(k, c["x"], tol=TOL)
    b = s.modes(k, c["x"], tol=TOL)
    nv = len(c["x"])
    d = s.modes(k, c["x"], tol=TOL, init=start_block(k + GUARD, nv))
    s.close()
    s2 = open_case(name)[0]
    e = s2.modes(k, c["x"], tol=TOL)
    s2.close()
    for o in (b, d, e):
        assert o[0].tobytes() == a[0].tobytes() and o[1].tobytes() == a[1].tobytes()
        assert o[2]["residual"].tobytes() == a[2]["residual"].tobytes() and o[2]["iterations"] == a[2]["iterations"]


# ---------------------------------------------------------------- 7: no side effects ------------------------------------------------
@gpu
@pytest.mark.parametrize("linsolver", [0, 1])
def test_modes_do_not_disturb_a_run(linsolver):
    """3 steps with modes() and a block stiffness_apply_ex at an explicit x between the steps: bit-identical to the run without"""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=linsolver)
        s = sc.make_solver()
        xs = []
        for _ in range(3):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                xp = case("mixed162")["x"]      # (the compressed state of the same mesh)
                s.modes(3, xp, tol=1e-6)
                s.stiffness_apply_ex(directions(xp.shape, 3, 7), xp, psd=True, block=True)
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


# ---------------------------------------------------------------- 8: refusals -------------------------------------------------------
@gpu
def test_refusals_leave_the_context_usable():
    s, flat, c, tab = open_case("tet6")
    x = c["x"]
    bad = [dict(k=0), dict(k=2, guard=-1), dict(k=13, guard=4), dict(k=17, guard=0), dict(k=2, shift=np.inf), dict(k=2, shift=np.nan),
           dict(k=2, tol=-1.0), dict(k=2, tol=np.nan), dict(k=2, tol=np.inf), dict(k=2, max_iters=0),
           dict(k=2, guard=2)]      # 8 vertices, 4 held: 12 free unknowns < 3 * 4... = 12 is allowed; see below
    bad[-1] = dict(k=3, guard=2)    # 3 * 5 = 15 > 12 free unknowns
    for kw in bad:
        with pytest.raises(capi.AdmmHipError) as e:
            s.modes(x=x, **kw)
        assert e.value.code == -1, (kw, e.value)      # ADMM_HIP_ERR_ARG
    with pytest.raises(capi.AdmmHipError):
        s.stiffness_apply_ex(np.ones_like(x), x, block=True, shift=np.nan)
    lam, phi, info = s.modes(2, x, guard=2, tol=TOL)      # 3 * 4 = 12 = the free unknowns: allowed, and the context still works
    assert np.isfinite(lam).all() and info["ended_by"] in ("tol", "max_iters", "breakdown")
    s.close()


# ---------------------------------------------------------------- 9: the device's iterations = the model's --------------------------
@gpu
def test_iteration_count_matches_the_numpy_model():
    """162 tets: the device and the numpy model of its iteration (on the operator assembled from the device) stop after the same number
    of iterations, within BOUNDS['iters']: the stop test is a threshold on a residual that falls by a factor per iteration, so the two
    summation orders can cross it an iteration apart."""
    s, flat, c, tab = open_case("mixed162")
    k = K_MODES; nb = k + GUARD
    f3 = np.repeat(free_mask(c), 3)
    m3 = np.asarray(s.m_masses, dtype=np.float64)
    A = assemble(s, c["x"], 0.0, True, True)[np.ix_(f3, f3)]
    X0 = start_block(nb, len(c["x"])).reshape(nb, -1)[:, f3].T
    model = numpy_lobpcg(A, m3[f3], X0, k)
    lam, phi, info = s.modes(k, c["x"], tol=TOL)
    print("iterations: device %d, numpy model %d; restarts %d / %d" % (info["iterations"], model["iterations"], info["restarts"], model["restarts"]))
    s.close()
    assert model["ended"] == 0 and info["converged"]
    assert abs(info["iterations"] - model["iterations"]) <= BOUNDS["iters"][1]
    assert info["restarts"] == model["restarts"] == 0
