"""Internal forces, stress and the stationarity residual on the device: admm_hip_forces, admm_hip_stress, monitor mode 3
(csrc/forces.hpp), their Python and C++ faces.

The reference has no gradient (TetEnergyTerm::gradient and TriEnergyTerm::gradient throw), so the yardstick is built here: the forces
are restated in numpy (numpy.linalg.svd, the derivatives of the densities of test_energy_monitor.tet_energies, the tabulated spline
through admm_host_spline_table_eval), that restatement is shown to be the gradient of the numpy ENERGIES of test_energy_monitor.py by
central differences on the CPU, and the device is then held to it."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Lame, Settings, Solver
from test_cpp_api import _build_exe
from test_energy_monitor import (KEYS, QuadSpline, check_state, cloth_with_hinges, hinge_energies, kind_solver, plain_state, pushed_state,
                                 signed_stretches, tet_F, tet_energies, tri_energies)

ALL_KINDS = [pkg.TET_LINEAR, pkg.TET_NEOHOOKEAN, pkg.TET_STVK, pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED,
             pkg.TET_SPLINE_TABLE, pkg.TET_STABLE_NH]
SPLINE_KINDS = [pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED, pkg.TET_SPLINE_TABLE, pkg.TET_STABLE_NH]


# ---------------------------------------------------------------- numpy restatement of the forces -----------------------------
def _xu_d(kind, mu, la, kappa):
    """f', g', h' of the three shipped xu:: splines: the derivatives of test_energy_monitor._xu."""
    def dcomp(J):
        return -kappa * ((1.0 - J) / 6.0) ** 2 / 24.0
    if kind == pkg.TET_SPLINE_NH:
        return (lambda s: mu * s, lambda p: 0.0, lambda J: dcomp(J) + (la * np.log(J) - mu) / J)
    if kind == pkg.TET_SPLINE_STVK:
        return (lambda s: la * (s ** 3 - 3.0 * s) / 2.0 + mu * (s * s - 1.0) * s, lambda p: la * p / 2.0, dcomp)
    return (lambda s: la * (s - 3.0) + 2.0 * mu * (s - 1.0), lambda p: la, dcomp)


def table_fgh(tab):
    """f, g, h and their derivatives of a tabulated spline as the DEVICE evaluates them (admm_host_spline_table_eval)."""
    def ev(which, order):
        def fn(x):
            out = np.zeros(3)
            capi.lib().admm_host_spline_table_eval(capi.dptr(tab), which, float(x), capi.dptr(out))
            return out[order]
        return fn
    return (ev(0, 0), ev(1, 0), ev(2, 0)), (ev(0, 1), ev(1, 1), ev(2, 1))


def stretch_gradient(s, kd, mu, la, k, kappa, table_d=None):
    """s_i g_i, the diagonal of P = dpsi/dF in the frame of the signed SVD: g = dpsi/da at a = |sigma| for the kinds whose energy is
    evaluated there (times sign(sigma)), at a = sigma for StVK and stable Neo-Hookean."""
    a = np.abs(s); sgn = np.where(s < 0.0, -1.0, 1.0)
    if kd == pkg.TET_LINEAR:
        return sgn * k * (a - 1.0)
    if kd == pkg.TET_NEOHOOKEAN:
        lJ = np.log(np.prod(a))
        return sgn * (mu * (a - 1.0 / a) + la * lJ / a)
    if kd == pkg.TET_STVK:
        st = 0.5 * (s * s - 1.0)
        return (2.0 * mu * st + la * np.sum(st)) * s
    if kd == pkg.TET_STABLE_NH:
        mus = 4.0 / 3.0 * mu; las = la + 5.0 / 6.0 * mu; al = 1.0 + 0.75 * mus / las
        IC = np.sum(s * s); J = np.prod(s)
        dJ = np.array([s[1] * s[2], s[2] * s[0], s[0] * s[1]])
        return mus * s + las * (J - al) * dJ - mus * s / (IC + 1.0)
    df, dg, dh = table_d if kd == pkg.TET_SPLINE_TABLE else _xu_d(kd, mu, la, kappa)
    g = np.zeros(3)
    for i in range(3):
        j, l = (i + 1) % 3, (i + 2) % 3
        g[i] = df(a[i]) + dg(a[i] * a[j]) * a[j] + dg(a[l] * a[i]) * a[l] + dh(a[0] * a[1] * a[2]) * a[j] * a[l]
    return sgn * g


def tet_forces(flat, rest, x, table_d=None):
    """f [nv, 3] of the tets, the per-vertex scale sum_{i in v} k_i vol_i |Binv_i|_F, and the per-tet stress."""
    tets = flat["tet_idx"]; nv = len(rest)
    f = np.zeros((nv, 3)); scale = np.zeros(nv)
    F, vol = tet_F(rest, tets, x)
    X = rest[tets]
    Dm = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    Binv = np.linalg.inv(Dm)
    P = np.zeros((len(tets), 3, 3)); S = np.zeros((len(tets), 3)); vm = np.zeros(len(tets))
    for i in range(len(tets)):
        U, sv, Vt = np.linalg.svd(F[i])
        s = sv.copy()
        if np.linalg.det(F[i]) < 0.0:
            s[2] = -s[2]
        # F = U diag(sv) Vt with sv >= 0; with s[2] = -sv[2] flip the third column of U so that F = U diag(s) Vt still
        if s[2] < 0.0:
            U = U.copy(); U[:, 2] = -U[:, 2]
        sg = stretch_gradient(s, int(flat["tet_kind"][i]), flat["tet_mu"][i], flat["tet_lambda"][i], flat["tet_k"][i], flat["tet_kappa"][i], table_d)
        Pi = U @ np.diag(sg) @ Vt
        H = -vol[i] * Pi @ Binv[i].T
        f[tets[i, 1]] += H[:, 0]; f[tets[i, 2]] += H[:, 1]; f[tets[i, 3]] += H[:, 2]; f[tets[i, 0]] -= H.sum(axis=1)
        scale[tets[i]] += flat["tet_k"][i] * vol[i] * np.linalg.norm(Binv[i])
        tau = sg * s / np.prod(s)
        P[i] = Pi; S[i] = s
        vm[i] = np.sqrt(0.5 * ((tau[0] - tau[1]) ** 2 + (tau[1] - tau[2]) ** 2 + (tau[2] - tau[0]) ** 2))
    return f, scale, dict(P=P, stretches=S, von_mises=vm)


def tri_forces(flat, rest, x, k):
    """E = k area / 2 sum (sigma_i - 1)^2: P = k area (F - R), R the closest isometry of the 3x2 F (thin SVD); scale w^2 |rest|_F."""
    tris = flat["tri_idx"]; nv = len(rest)
    f = np.zeros((nv, 3)); scale = np.zeros(nv)
    X = rest[tris]; p = x.reshape(-1, 3)[tris]
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    n = np.cross(e1, e2); area = 0.5 * np.linalg.norm(n, axis=1)
    u = e1 / np.linalg.norm(e1, axis=1)[:, None]
    w = np.cross(n / (2.0 * area)[:, None], u)
    Dm = np.stack([np.stack([np.sum(e1 * u, 1), np.sum(e1 * w, 1)], 1), np.stack([np.sum(e2 * u, 1), np.sum(e2 * w, 1)], 1)], axis=2)
    Ds = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=2)
    Bi = np.linalg.inv(Dm)
    for i in range(len(tris)):
        F = Ds[i] @ Bi[i]
        U, sv, Vt = np.linalg.svd(F, full_matrices=False)
        H = -k * area[i] * (F - U @ Vt) @ Bi[i].T
        f[tris[i, 1]] += H[:, 0]; f[tris[i, 2]] += H[:, 1]; f[tris[i, 0]] -= H.sum(axis=1)
        scale[tris[i]] += flat["tri_weight"][i] ** 2 * np.linalg.norm(flat["tri_rest"][i])
    return f, scale


def hinge_forces(flat, rest, x):
    """f_{v_k} = -stiffness c_k (D x); scale stiffness |c|^2 |x| with |x| the largest |x_v| of the hinge's vertices."""
    nv = len(rest)
    f = np.zeros((nv, 3)); scale = np.zeros(nv)
    idx, c, st = flat["bend_idx"], flat["bend_coef"], flat["bend_stiffness"]
    p = x.reshape(-1, 3)[idx]
    Dx = np.einsum("hk,hkj->hj", c, p)
    for h in range(len(idx)):
        for k in range(4):
            f[idx[h, k]] -= st[h] * c[h, k] * Dx[h]
        scale[idx[h]] += st[h] * np.sum(c[h] ** 2) * np.linalg.norm(p[h], axis=1).max()
    return f, scale


def numpy_forces(flat, rest, x, tri_k=None, table_d=None):
    """-> f [nv, 3], per-vertex scale of the derived bar, the tets' stress (None without tets)."""
    nv = len(rest)
    f = np.zeros((nv, 3)); scale = np.zeros(nv); stress = None
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    if len(flat["tet_idx"]):
        ft, sc, stress = tet_forces(flat, rest, x, table_d)
        f += ft; scale += sc
    if len(flat["tri_idx"]):
        fr, sc = tri_forces(flat, rest, x, tri_k)
        f += fr; scale += sc
    if len(flat["bend_idx"]):
        fh, sc = hinge_forces(flat, rest, x)
        f += fh; scale += sc
    return f, scale, stress


def numpy_energy(flat, rest, x, tri_k=None, table_f=None):
    """the total of test_energy_monitor's numpy energies on a flat description"""
    E = 0.0
    x = np.asarray(x, dtype=np.float64)
    if len(flat["tet_idx"]):
        F, vol = tet_F(rest, flat["tet_idx"], x)
        E += tet_energies(F, vol, flat["tet_kind"], flat["tet_mu"], flat["tet_lambda"], flat["tet_k"], flat["tet_kappa"], table_f)[0].sum()
    if len(flat["tri_idx"]):
        E += tri_energies(rest, flat["tri_idx"], x, tri_k)[0].sum()
    if len(flat["bend_idx"]):
        E += hinge_energies(flat, x)[0].sum()
    return E


def kind_description(n, kind):
    """kind_solver of test_energy_monitor.py without a context: the flat description, the rest positions and, for the tabulated kind,
    its table (admm_host_tabulate_spline is host code)."""
    verts, tets = meshes.kuhn_cube(n)
    lame = Lame.soft_rubber()
    s = Solver()
    s.add_nodes(verts, np.repeat(meshes.lumped_masses_tets(verts, tets), 3))
    if kind == pkg.TET_SPLINE_TABLE:
        s.add_tets(verts, tets, lame, kind, spline=QuadSpline(lame.mu, 0.25 * lame.lambda_, 0.5 * lame.lambda_))
    elif pkg.TET_SPLINE_NH <= kind <= pkg.TET_SPLINE_COROTATED:
        s.add_tets(verts, tets, lame, kind, kappa=0.3 * lame.lambda_)
    else:
        s.add_tets(verts, tets, lame, kind)
    s.make_desc(Settings())
    tab = s._spline_tables[0] if kind == pkg.TET_SPLINE_TABLE else None
    return s.flatten(), verts, tab


def cloth_states(sc):
    return (scenes.perturb(sc.x, 0.02, 1) * np.array([1.1, 1.0, 0.9]), scenes.perturb(sc.x, 0.05, 2) * np.array([0.8, 1.0, 1.25]))


def rigid(x, shift=(0.1, -0.2, 0.3)):
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.4), -np.sin(0.4)], [0.0, np.sin(0.4), np.cos(0.4)]])
    return x @ R.T + np.asarray(shift)


# ---------------------------------------------------------------- CPU ---------------------------------------------------------
def test_forces_symbols_and_settings():
    """The two entry points exist in libadmm_hip.so with the documented signatures and are declared in the header; NULL contexts are
    refused; Settings(monitor=3) is accepted; Solver.forces / Solver.stress exist; admm_history() documents `stationarity`."""
    L = capi.lib()
    sig = {name: (res, args) for name, res, args in capi.SYMBOLS}
    dp = capi.c_double_p
    assert sig["admm_hip_forces"] == (C.c_int, [C.c_void_p, dp, dp])
    assert sig["admm_hip_stress"] == (C.c_int, [C.c_void_p, dp, dp])
    for name in ("admm_hip_forces", "admm_hip_stress"):
        assert getattr(L, name) is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    for decl in ("int admm_hip_forces(admm_hip_ctx *ctx, const double *x, double *f);",
                 "int admm_hip_stress(admm_hip_ctx *ctx, const double *x, double *out13);"):
        assert decl in hdr, decl
    out = np.zeros(13)
    assert L.admm_hip_forces(None, None, capi.dptr(out)) == -1
    assert L.admm_hip_stress(None, None, capi.dptr(out)) == -1
    assert L.admm_hip_set_monitor(None, 3) == -1
    assert Settings(monitor=3).monitor == 3
    assert list(inspect.signature(Solver.forces).parameters) == ["self", "x"]
    assert list(inspect.signature(Solver.stress).parameters) == ["self", "x"]
    assert "stationarity" in Solver.admm_history.__doc__


def _fd_case(name, flat, rest, states, tri_k=None, table=None):
    """central differences of the numpy energy along 8 random directions at h and h / 2 against -f . d"""
    fgh, dfgh = table_fgh(table) if table is not None else (None, None)
    rng = np.random.default_rng(17)
    edge = np.linalg.norm(rest[flat["tet_idx"][0, 1]] - rest[flat["tet_idx"][0, 0]]) if len(flat["tet_idx"]) else \
        np.linalg.norm(rest[flat["tri_idx"][0, 1]] - rest[flat["tri_idx"][0, 0]])
    h = 4e-4 * edge
    worst = 0.0
    for x in states:
        f, _, _ = numpy_forces(flat, rest, x, tri_k, dfgh)
        E = lambda y: numpy_energy(flat, rest, y, tri_k, fgh)
        for _ in range(8):
            d = rng.standard_normal(x.shape)
            d /= np.linalg.norm(d, axis=1).max()
            ana = -np.sum(f * d)
            e1 = abs((E(x + h * d) - E(x - h * d)) / (2.0 * h) - ana)
            e2 = abs((E(x + 0.5 * h * d) - E(x - 0.5 * h * d)) / h - ana)
            bar = np.linalg.norm(f) * np.linalg.norm(d)
            worst = max(worst, e2 / bar)
            assert 3.0 <= e1 / e2 <= 5.0, (name, e1, e2, e1 / e2)
            assert e2 <= 1e-6 * bar, (name, e2, bar)
    print("%s: largest discrepancy at h / 2 = %.3e |f| |d|" % (name, worst))


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_numpy_forces_are_the_gradient_of_the_numpy_energies_tets(kind):
    """The yardstick before any GPU sees it: on the 48-tet Kuhn cube of every kind, at a plain and a pushed (inverted, |sigma| >= 0.1)
    state, the discrepancy between the central difference of the numpy energy and -f . d falls by 4 +- 25 % from h to h / 2 (it is the
    truncation error, not a wrong derivative) and is <= 1e-6 |f| |d| at the smaller h."""
    flat, verts, tab = kind_description(2, kind)
    states = (plain_state(verts, 2), pushed_state(verts, 2))
    for x, pushed in zip(states, (False, True)):
        check_state(signed_stretches(tet_F(verts, flat["tet_idx"], x)[0]), pushed)
    _fd_case("kind %d" % kind, flat, verts, states, table=tab)


def test_numpy_forces_are_the_gradient_of_the_numpy_energies_cloth():
    """The same for triangles (strain limits ignored) and bending hinges."""
    sc = cloth_with_hinges(4, limits=None)
    s = sc.make_solver(init=False)
    _fd_case("cloth", s.flatten(), sc.x, cloth_states(sc), tri_k=sc.tris[0][2].bulk_modulus())


# ---------------------------------------------------------------- GPU: parity and invariants ---------------------------------
def _tet_scene(case):
    if case == "one_tet":
        sc = scenes.Scene()
        verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        sc.add_tet_mesh(verts, np.array([[0, 1, 2, 3]], np.int32), Lame.soft_rubber(), pkg.TET_NEOHOOKEAN)
        return sc, 1
    if case == "mixed5":
        return scenes.mixed_cube_scene(5), 5
    n = int(case[2])
    return scenes.cube_scene(n, pkg.TET_NEOHOOKEAN), n


def _one_tet_state(verts, pushed):
    x = verts * np.array([1.3, 0.8, 1.1]) + 0.03 * np.random.default_rng(4).standard_normal(verts.shape)
    if pushed:
        x[3] = x[3] * np.array([1.0, 1.0, -0.6])      # the apex through the base: an inverted tet
    return x


def _parity(name, s, rest, x, pushed, tri_k=None, table=None, want_stress=False):
    flat = s.flatten()
    dfgh = table_fgh(table)[1] if table is not None else None
    ref, scale, stress = numpy_forces(flat, rest, x, tri_k, dfgh)
    if stress is not None:
        check_state(stress["stretches"], pushed)
    f = s.forces(x)
    assert f.shape == ref.shape
    err = np.linalg.norm(f - ref, axis=1) / scale
    print("%s: force parity, %d vertices, max |f_v - ref_v| / scale_v = %.3e (bar 1e-9)" % (name, len(ref), err.max()))
    if err.max() > 1e-10:
        print("%s: WITHIN 10x OF THE BAR" % name)
    assert err.max() <= 1e-9, (int(err.argmax()), err.max())
    return f, ref, scale, stress


def _invariants(name, f, x):
    """sum f = 0, sum x cross f = 0: a corner force dropped or counted twice breaks them"""
    x = x.reshape(-1, 3)
    tol = 1e-12 * np.sum(np.linalg.norm(f, axis=1) * (1.0 + np.linalg.norm(x, axis=1)))
    lin = np.abs(f.sum(axis=0)).max(); ang = np.abs(np.cross(x, f).sum(axis=0)).max()
    print("%s: |sum f| = %.3e, |sum x cross f| = %.3e (allowed %.3e)" % (name, lin, ang, tol))
    assert lin <= tol and ang <= tol, (lin, ang, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("case", ["one_tet", "nh1", "nh3", "mixed5"])
def test_force_parity_block_shapes(case, pushed):
    """One tet; 6 tets (a partial wave); 162 (a partial block, the interior vertices of valence 24: records cut after 8 corner forces);
    750 tets of three kinds (model boundaries inside the numbering, vertices shared by several chunks).  Per vertex
    |f_v - ref_v| <= 1e-9 sum_{i in v} k_i vol_i |Binv_i|_F: the 1e-9 bar of the local step's z times |d2 psi| of a few k, through the
    corner-force product.  At the pushed state also sum f = 0 and sum x cross f = 0 to 1e-12 sum |f_v| (1 + |x_v|).

    Measured on an MI355X: the largest |f_v - ref_v| / scale_v over the eight cases is 2.5e-15 (mixed5, pushed), five decades under
    the bar; |sum f| and |sum x cross f| stay four decades under theirs."""
    sc, n = _tet_scene(case)
    s = sc.make_solver()
    x = _one_tet_state(sc.x, pushed) if case == "one_tet" else (pushed_state if pushed else plain_state)(sc.x, n)
    f = _parity(case, s, sc.x, x, pushed)[0]
    if pushed:
        _invariants(case, f, x)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("kind", SPLINE_KINDS)
def test_force_parity_spline_kinds(kind, pushed):
    """The xu:: splines with kappa != 0, the tabulated spline (numpy evaluates the table as the device does) and stable Neo-Hookean on
    the 162-tet cube; the bar and the invariants as above.  Measured on an MI355X: at most 2.7e-15 of the scale (the tabulated spline, pushed)."""
    s, verts = kind_solver(3, kind)
    x = (pushed_state if pushed else plain_state)(verts, 3)
    f = _parity("kind %d" % kind, s, verts, x, pushed, table=s._spline_tables[0] if kind == pkg.TET_SPLINE_TABLE else None)[0]
    if pushed:
        _invariants("kind %d" % kind, f, x)
    s.close()


@pytest.mark.gpu
def test_force_parity_cloth_and_hinges():
    """Triangles (scale w^2 |rest|_F) and hinges (scale stiffness |c|^2 |x|) at two perturbed states; the invariants at the second.
    Measured on an MI355X: at most 6.7e-17 of the scale."""
    sc = cloth_with_hinges(6)
    s = sc.make_solver()
    k = sc.tris[0][2].bulk_modulus()
    xs = cloth_states(sc)
    _parity("cloth a", s, sc.x, xs[0], False, tri_k=k)
    f = _parity("cloth b", s, sc.x, xs[1], False, tri_k=k)[0]
    _invariants("cloth", f, xs[1])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_forces_vanish_in_a_rigid_motion(kind):
    """f = 0 to 1e-12 of the per-vertex scale at rest and after a rotation and translation, all eight kinds -- stable Neo-Hookean too:
    its rest ENERGY is a constant, its rest force zero.  Measured on an MI355X: at most 4.7e-16 of the scale, except the tabulated
    spline's 1.9e-14 (the interpolant's f'(1) is zero to the table's accuracy, not to the last bit): 50x under the bar."""
    s, verts = kind_solver(3, kind)
    scale = numpy_forces(s.flatten(), verts, verts, None, table_fgh(s._spline_tables[0])[1] if kind == pkg.TET_SPLINE_TABLE else None)[1]
    for name, x in (("rest", verts), ("rigid", rigid(verts))):
        f = s.forces(x)
        r = np.linalg.norm(f, axis=1) / scale
        print("kind %d %s: max |f_v| / scale_v = %.3e (allowed 1e-12)" % (kind, name, r.max()))
        assert r.max() <= 1e-12, (name, r.max())
    s.close()


@pytest.mark.gpu
def test_cloth_forces_vanish_in_a_rigid_motion():
    sc = cloth_with_hinges(6)
    s = sc.make_solver()
    k = sc.tris[0][2].bulk_modulus()
    for name, x in (("rest", sc.x), ("rigid", rigid(sc.x))):
        scale = numpy_forces(s.flatten(), sc.x, x, k)[1]
        r = np.linalg.norm(s.forces(x), axis=1) / scale
        print("cloth %s: max |f_v| / scale_v = %.3e (allowed 1e-12)" % (name, r.max()))
        assert r.max() <= 1e-12, (name, r.max())
    s.close()


# ---------------------------------------------------------------- GPU: directional derivative on the device ------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed5", "cloth"])
def test_device_forces_are_the_gradient_of_the_device_energy(case):
    """(energy(x + h d) - energy(x - h d)) / 2h against -forces(x) . d, 4 directions, device against device.  The same quantity in numpy
    gives the truncation error delta_ref at that h; asserted: device discrepancy <= 2 delta_ref + 1e-9 scale, scale = sum_v scale_v |d_v|
    (the force bar summed along d).  No free constant."""
    if case == "mixed5":
        sc = scenes.mixed_cube_scene(5); x = plain_state(sc.x, 5); tri_k = None; edge = 0.2
    else:
        sc = cloth_with_hinges(6); x = cloth_states(sc)[0]; tri_k = sc.tris[0][2].bulk_modulus(); edge = 1.0 / 6.0
    s = sc.make_solver()
    flat = s.flatten()
    fn, scale_v, _ = numpy_forces(flat, sc.x, x, tri_k)
    fd = s.forces(x)
    rng = np.random.default_rng(23)
    h = 1e-4 * edge
    for k in range(4):
        d = rng.standard_normal(x.shape)
        d /= np.linalg.norm(d, axis=1).max()
        dev = (s.energy(x + h * d)["total"] - s.energy(x - h * d)["total"]) / (2.0 * h)
        ref = (numpy_energy(flat, sc.x, x + h * d, tri_k) - numpy_energy(flat, sc.x, x - h * d, tri_k)) / (2.0 * h)
        delta_ref = abs(ref + np.sum(fn * d))
        delta_dev = abs(dev + np.sum(fd * d))
        scale = np.sum(scale_v * np.linalg.norm(d, axis=1))
        print("%s direction %d: device %.6e, truncation in numpy %.6e, 1e-9 scale %.3e" % (case, k, delta_dev, delta_ref, 1e-9 * scale))
        assert delta_dev <= 2.0 * delta_ref + 1e-9 * scale, (delta_dev, delta_ref, scale)
    s.close()


# ---------------------------------------------------------------- GPU: stress ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
def test_stress_parity_in_the_callers_order(pushed):
    """P, the signed stretches and von Mises of the 750-tet scene of three kinds against numpy, per tet in the CALLER's order (the
    scene adds NH, StVK, linear; the library sorts linear first): |P - ref| <= 1e-9 k, |sigma - ref| <= 1e-9, |vm - ref| <= 1e-9 k / |J|
    (the force bar per tet, without the corner-force product; the Cauchy stress divides by J).
    Measured on an MI355X: P 2.9e-14 k, stretches 1.8e-15, von Mises 9.6e-14 k / |J| (the pushed state; the plain one is below)."""
    sc = scenes.mixed_cube_scene(5)
    s = sc.make_solver()
    x = (pushed_state if pushed else plain_state)(sc.x, 5)
    flat = s.flatten()
    ref = numpy_forces(flat, sc.x, x)[2]
    check_state(ref["stretches"], pushed)
    out = s.stress(x)
    assert out["P"].shape == (750, 3, 3) and out["stretches"].shape == (750, 3) and out["von_mises"].shape == (750,)
    k = flat["tet_k"]
    # stretches: the same magnitudes per tet in any order, and the same orientation (which stretch of an inverted tet carries the
    # sign is the signed SVD's choice: P and the Cauchy stress do not depend on it)
    sd = np.sort(np.abs(out["stretches"]), axis=1); sr = np.sort(np.abs(ref["stretches"]), axis=1)
    assert np.array_equal(np.sign(np.prod(out["stretches"], axis=1)), np.sign(np.prod(ref["stretches"], axis=1)))
    eP = np.abs(out["P"] - ref["P"]).max(axis=(1, 2)) / k
    eS = np.abs(sd - sr).max(axis=1)
    eV = np.abs(out["von_mises"] - ref["von_mises"]) * np.abs(np.prod(ref["stretches"], axis=1)) / k
    print("stress parity (pushed %d): P %.3e k, stretches %.3e, von Mises %.3e k / |J|  (bars 1e-9)" % (pushed, eP.max(), eS.max(), eV.max()))
    assert eP.max() <= 1e-9 and eS.max() <= 1e-9 and eV.max() <= 1e-9
    s.close()


@pytest.mark.gpu
def test_von_mises_vanishes_without_shear():
    """A rigid motion and a uniform dilation carry no deviatoric stress: von Mises <= 1e-12 k, all three kinds of the mixed scene."""
    sc = scenes.mixed_cube_scene(5)
    s = sc.make_solver()
    k = s.flatten()["tet_k"]
    for name, x in (("rigid", rigid(sc.x)), ("dilation", 1.2 * sc.x + 0.1)):
        vm = s.stress(x)["von_mises"]
        print("%s: max von Mises / k = %.3e (allowed 1e-12)" % (name, (vm / k).max()))
        assert (vm <= 1e-12 * k).all(), (name, (vm / k).max())
    s.close()


# ---------------------------------------------------------------- GPU: reproducible ------------------------------------------
@pytest.mark.gpu
def test_forces_and_stress_are_bit_reproducible():
    """No floating-point atomics: two calls return identical bits; forces() of the device-resident state after a step equals
    forces(m_x)."""
    for sc, n in ((scenes.mixed_cube_scene(5, admm_iters=3), 5), (cloth_with_hinges(6, admm_iters=3), 1)):
        s = sc.make_solver()
        x = plain_state(sc.x, n)
        assert np.array_equal(s.forces(x), s.forces(x))
        if sc.tets:
            a, b = s.stress(x), s.stress(x)
            for key in ("P", "stretches", "von_mises"):
                assert np.array_equal(a[key], b[key])
        s.step()
        a = s.forces(); b = s.forces(s.m_x)
        assert np.array_equal(a, b) and np.abs(a).max() > 0.0
        s.close()


# ---------------------------------------------------------------- GPU: stationarity -------------------------------------------
# R: the largest |a - b| / (b + max_s b) of the stationarity over the three scenes and two frames against numpy on the oracle's trace, as
# measured on the MI355X (see the docstring of test_stationarity_matches_oracle_trace); the assertion is 10 x that.
R_MEASURED = 1.140e-8
R_ASSERT = 10.0 * R_MEASURED


def _stat_scene(name):
    if name == "mixed4":
        return scenes.mixed_cube_scene(4, admm_iters=12)
    if name == "nh5":
        return scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, admm_iters=12)
    return scenes.cloth_scene(6, limits=None, admm_iters=12)


def _oracle_stationarity(sc, o, flat):
    """one frame of the oracle with its trace -> |(m (x_s - x_bar) / dt^2 - f_numpy(x_s))_free| per ADMM iteration"""
    dt = o.dt
    x0 = o.x.copy(); v = o.v.copy()
    if abs(o.gravity) > 0:
        v[1::3] += dt * o.gravity
    xbar = x0 + dt * v
    tr = []
    o.step(trace=tr)
    free = np.ones(len(sc.x), bool)
    free[list(sc.pins.keys())] = False
    tri_k = sc.tris[0][2].bulk_modulus() if sc.tris else None
    out = []
    for z, u, b, x in tr:
        f = numpy_forces(flat, sc.x, x, tri_k)[0]
        r = (o.m * (x - xbar) / (dt * dt)).reshape(-1, 3) - f
        out.append(np.linalg.norm(r[free]))
    return np.array(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed4", "nh5", "cloth6"])
def test_stationarity_matches_oracle_trace(name):
    """admm_history()["stationarity"] of two frames (pcg_tol 1e-12, monitor 3) against numpy on the oracle's trace, pinned vertices left
    out, compared as |a - b| / (b + max_s b); the other seven fields equal a mode-2 run of the same scene to the tolerance
    test_monitor_mode_1_leaves_the_objective_slots_zero uses.

    Measured on an MI355X (largest ratio per scene over both frames): mixed4 1.58e-9, nh5 5.14e-9, cloth6 1.14e-8, each in frame 0.
    R_MEASURED = 1.140e-8, asserted: R_ASSERT = 10 x R_MEASURED = 1.14e-7 -- the size of the monitor's own R (test_energy_monitor.py),
    as it must be: both compare a quantity of the device's trajectory with the oracle's."""
    sc = _stat_scene(name)
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=3)
    s2 = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=2)
    o = sc.make_oracle(mode=1)
    flat = s.flatten()
    worst = 0.0
    for frame in range(2):
        ref = _oracle_stationarity(sc, o, flat)
        s.step(); s2.step()
        h, h2 = s.admm_history(), s2.admm_history()
        assert all(len(h[k]) == 12 for k in KEYS + ("stationarity",))
        ratio = np.abs(h["stationarity"] - ref) / (ref + ref.max())
        worst = max(worst, ratio.max())
        print("%s frame %d: oracle %.6g .. %.6g, device %.6g .. %.6g, max ratio %.3e" % (name, frame, ref[0], ref[-1], h["stationarity"][0],
                                                                                      h["stationarity"][-1], ratio.max()))
        for key in KEYS:
            assert np.allclose(h[key], h2[key], rtol=1e-6, atol=1e-6 * np.abs(h2[key]).max()), key
        assert not h2["stationarity"].any()
    print("%s: measured R = %.3e" % (name, worst))
    assert worst <= R_ASSERT, (worst, R_ASSERT)
    s.close(); s2.close()


@pytest.mark.gpu
def test_modes_1_and_2_leave_stationarity_zero():
    sc = _stat_scene("mixed4")
    for mode in (1, 2):
        s = sc.make_solver(monitor=mode)
        s.step()
        h = s.admm_history()
        assert len(h["stationarity"]) == 12 and not h["stationarity"].any() and (h["primal"] > 0).all()
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [pkg.TET_NEOHOOKEAN, pkg.TET_LINEAR])
def test_stationarity_converges(kind):
    """200 ADMM iterations of one frame (pcg_tol 1e-12): stationarity[199] <= 1e-4 stationarity[0].  The CPU oracle reaches 3e-8 (NH)
    and 1e-9 (linear) of |m g| there, more than three decades under this bar.  Measured on an MI355X: Neo-Hookean 5.08e3 -> 2.5e2 (19)
    -> 7.1e-2 (99) -> 1.05e-5 (199), linear 4.53e3 -> 8.2e1 -> 9.7e-4 -> 1.86e-5: ratios 2.1e-9 and 4.1e-9."""
    sc = scenes.cube_scene(2, kind, admm_iters=200)
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=3)
    s.step()
    st = s.admm_history()["stationarity"]
    print("kind %d: stationarity %.6e (iteration 0) .. %.6e (19) .. %.6e (99) .. %.6e (199)" % (kind, st[0], st[19], st[99], st[199]))
    assert len(st) == 200 and np.isfinite(st).all() and st[0] > 0.0
    assert st[199] <= 1e-4 * st[0], (st[0], st[199])
    s.close()


# ---------------------------------------------------------------- GPU: mode 3 does not disturb the step -----------------------
def _run(sc, frames, **kw):
    s = sc.make_solver(**kw)
    for _ in range(frames):
        s.step()
    out = s.m_x.copy(), s.m_v.copy()
    s.close()
    return out


@pytest.mark.gpu
def test_mode_3_does_not_change_the_gs_path():
    """linsolver 1 (bit-reproducible): m_x, m_v with monitor 3 equal monitor 0 bit for bit."""
    sc = scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, linsolver=1)
    x0, v0 = _run(sc, 3)
    x3, v3 = _run(sc, 3, monitor=3)
    assert np.array_equal(x0, x3) and np.array_equal(v0, v3)


@pytest.mark.gpu
def test_mode_3_does_not_change_the_pcg_path():
    """linsolver 0: if two plain runs are bit-identical the monitored one must be as well; otherwise its distance stays within 4x theirs."""
    sc = scenes.mixed_cube_scene(4)
    xa, va = _run(sc, 3)
    xb, vb = _run(sc, 3)
    xm, vm = _run(sc, 3, monitor=3)
    plain = max(np.abs(xa - xb).max(), np.abs(va - vb).max())
    mon = max(np.abs(xa - xm).max(), np.abs(va - vm).max())
    print("plain runs differ by %.3e, the run with monitor 3 by %.3e" % (plain, mon))
    if plain == 0.0:
        assert mon == 0.0
    else:
        assert mon <= 4.0 * plain


# ---------------------------------------------------------------- GPU: housekeeping -------------------------------------------
@pytest.mark.gpu
def test_forces_housekeeping():
    """Multi-rank contexts raise for forces, stress and set_monitor(3); set_monitor(4) is refused; a closed context leaves no device
    buffer behind."""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = scenes.cube_scene(3, pkg.TET_NEOHOOKEAN)
    s = sc.make_solver(world_size=2, rank=0)
    for call in (lambda: s.forces(sc.x), lambda: s.stress(sc.x), lambda: s.set_monitor(3)):
        with pytest.raises(pkg.AdmmHipError):
            call()
    s.close()
    sc = cloth_with_hinges(6, admm_iters=4)
    s = sc.make_solver(monitor=3)
    with pytest.raises(pkg.AdmmHipError):
        s.set_monitor(4)
    s.step()
    assert len(s.admm_history()["stationarity"]) == 4 and (s.admm_history()["stationarity"] > 0).all()
    s.forces(); s.stress()
    s.close()
    s = scenes.mixed_cube_scene(3, admm_iters=2).make_solver(monitor=3)
    s.step(); s.forces(); s.stress(s.m_x)
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)


# ---------------------------------------------------------------- GPU: C++ ----------------------------------------------------
@pytest.mark.gpu
def test_cpp_forces_and_stationarity():
    """tests/cpp/test_forces.cpp: Solver::forces satisfies sum f = 0, sum x cross f = 0 and f = 0 in a rigid motion on a scene with all
    eight tet kinds and a cloth; with Settings::monitor = 3 the history has finite, positive stationarity that falls over 50 iterations."""
    exe = _build_exe("test_forces")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
