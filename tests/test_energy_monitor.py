"""Energy and ADMM residuals on the device: admm_hip_energy, admm_hip_residuals, the step monitor (csrc/monitor.hpp), their Python
and C++ faces.  The references are numpy restatements of the reference's formulas (src/TetEnergyTerm.cpp:94-100,138-149,220-226;
src/TriEnergyTerm.cpp:104-114; numpy.linalg.svd) and the CPU oracle's per-iteration trace."""
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

KEYS = ("primal", "dz", "wz", "wdx", "energy", "inertia", "objective")


# ---------------------------------------------------------------- numpy restatement of EnergyTerm::energy ----------------
def _xu(kind, mu, la, kappa):
    """f, g, h of the three shipped xu:: splines (src/XuSpline.hpp:48-96) with their compression term (:43-45)."""
    def comp(J):
        return kappa * ((1.0 - J) / 6.0) ** 3 / 12.0
    if kind == pkg.TET_SPLINE_NH:
        return (lambda s: mu * (s * s - 1.0) / 2.0, lambda p: 0.0,
                lambda J: comp(J) + np.log(J) * (la * np.log(J) / 2.0 - mu))
    if kind == pkg.TET_SPLINE_STVK:
        return (lambda s: la * (s ** 4 - 6.0 * s * s + 5.0) / 8.0 + mu * (s * s - 1.0) ** 2 / 4.0, lambda p: la * (p * p - 1.0) / 4.0, comp)
    return (lambda s: la * (s * s - 6.0 * s + 5.0) / 2.0 + mu * (s - 1.0) ** 2, lambda p: la * (p - 1.0), comp)


def tet_F(rest, tets, x):
    """F = [x1 - x0, x2 - x0, x3 - x0] inv([X1 - X0, X2 - X0, X3 - X0]) and the rest volumes (src/TetEnergyTerm.cpp:31-48)."""
    X = rest[tets]; p = x.reshape(-1, 3)[tets]
    Dm = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    Ds = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]], axis=2)
    return Ds @ np.linalg.inv(Dm), np.linalg.det(Dm) / 6.0


def signed_stretches(F):
    s = np.linalg.svd(F, compute_uv=False)
    s[:, 2] *= np.sign(np.linalg.det(F))
    return s


def tet_energies(F, vol, kind, mu, la, k, kappa, table_fgh=None):
    """EnergyTerm::energy per tet.  Signs as the reference: the linear tet takes |sigma|, Neo-Hookean and every SplineTet flip a negative
    smallest stretch, StVK is even, stable Neo-Hookean keeps the sign."""
    S = signed_stretches(F)
    out = np.zeros(len(F))
    for i in range(len(F)):
        s = S[i]; a = np.abs(s); kd = int(kind[i])
        if kd == pkg.TET_LINEAR:
            psi = 0.5 * k[i] * np.sum((a - 1.0) ** 2)
        elif kd == pkg.TET_NEOHOOKEAN:
            l = np.log(np.prod(a) ** 2)
            psi = 0.5 * mu[i] * (np.sum(a * a) - l - 3.0) + 0.125 * la[i] * l * l
        elif kd == pkg.TET_STVK:
            st = 0.5 * (s * s - 1.0)
            psi = mu[i] * np.sum(st * st) + 0.5 * la[i] * np.sum(st) ** 2
        elif kd == pkg.TET_STABLE_NH:
            mus = 4.0 / 3.0 * mu[i]; las = la[i] + 5.0 / 6.0 * mu[i]; al = 1.0 + 0.75 * mus / las
            IC = np.sum(s * s); J = np.prod(s)
            psi = 0.5 * mus * (IC - 3.0) + 0.5 * las * (J - al) ** 2 - 0.5 * mus * np.log(IC + 1.0)
        else:
            f, g, h = table_fgh if kd == pkg.TET_SPLINE_TABLE else _xu(kd, mu[i], la[i], kappa[i])
            psi = f(a[0]) + f(a[1]) + f(a[2]) + g(a[0] * a[1]) + g(a[1] * a[2]) + g(a[2] * a[0]) + h(a[0] * a[1] * a[2])
        out[i] = psi * vol[i]
    return out, S


def tri_energies(rest, tris, x, k):
    """src/TriEnergyTerm.cpp:104-114: k / 2 area sum (sigma_i - 1)^2 of the 3x2 F, in any orthonormal frame of the rest triangle."""
    X = rest[tris]; p = x.reshape(-1, 3)[tris]
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    n = np.cross(e1, e2); area = 0.5 * np.linalg.norm(n, axis=1)
    u = e1 / np.linalg.norm(e1, axis=1)[:, None]
    w = np.cross(n / (2.0 * area)[:, None], u)
    Dm = np.stack([np.stack([np.sum(e1 * u, 1), np.sum(e1 * w, 1)], 1), np.stack([np.sum(e2 * u, 1), np.sum(e2 * w, 1)], 1)], axis=2)   # columns e1, e2 in 2D
    Ds = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=2)
    F = Ds @ np.linalg.inv(Dm)
    s = np.linalg.svd(F, compute_uv=False)
    return 0.5 * k * area * np.sum((s - 1.0) ** 2, axis=1), k * area


def hinge_energies(flat, x):
    p = x.reshape(-1, 3)[flat["bend_idx"]]
    Dx = np.einsum("hk,hkj->hj", flat["bend_coef"], p)
    return 0.5 * flat["bend_stiffness"] * np.sum(Dx * Dx, axis=1), flat["bend_stiffness"] * 0.0 + flat["bend_weight"] ** 2


def reference_energies(s, rest, x, lame_tri=None, table_fgh=None):
    """Per-term energies of solver s at x in the caller's order (tets, tris, hinges) and the scale k_i vol_i of every term."""
    f = s.flatten()
    E, scale, S = [], [], None
    if len(f["tet_idx"]):
        F, vol = tet_F(rest, f["tet_idx"], x)
        e, S = tet_energies(F, vol, f["tet_kind"], f["tet_mu"], f["tet_lambda"], f["tet_k"], f["tet_kappa"], table_fgh)
        E.append(e); scale.append(f["tet_k"] * vol)
    if len(f["tri_idx"]):
        e, sc = tri_energies(rest, f["tri_idx"], x, lame_tri.bulk_modulus())
        E.append(e); scale.append(sc)
    if len(f["bend_idx"]):
        e, sc = hinge_energies(f, x)
        E.append(e); scale.append(sc)
    return np.concatenate(E), np.concatenate(scale), S


# ---------------------------------------------------------------- states ---------------------------------------------------
def plain_state(verts, n, seed=0):
    return scenes.perturb(verts, 0.06 / n, seed) * np.array([1.3, 0.8, 1.1])


def pushed_state(verts, n, seed=0):
    x = plain_state(verts, n, seed)
    c = int(np.argmin(np.linalg.norm(verts - verts.mean(axis=0), axis=1)))
    x[c] += np.array([0.0, 1.6 / n, 0.0])
    return x


def check_state(S, pushed):
    """the stretch range the tolerances are derived for"""
    if pushed:
        assert (S[:, 2] < 0).any(), "the pushed state must invert some tets"
        assert np.abs(S).min() >= 0.1, np.abs(S).min()
    else:
        assert S.min() >= 0.5 and S.max() <= 2.0, (S.min(), S.max())


class QuadSpline:
    """a user-defined xu::Spline: f = a (s - 1)^2, g = b (p - 1)^2, h = c (J - 1)^2"""

    def __init__(self, a, b, c):
        self.a, self.b, self.c = a, b, c

    def f(self, x): return self.a * (x - 1.0) ** 2
    def g(self, x): return self.b * (x - 1.0) ** 2
    def h(self, x): return self.c * (x - 1.0) ** 2
    def df(self, x): return 2.0 * self.a * (x - 1.0)
    def dg(self, x): return 2.0 * self.b * (x - 1.0)
    def dh(self, x): return 2.0 * self.c * (x - 1.0)


def table_functions(s):
    """f, g, h of the solver's first tabulated spline as the DEVICE evaluates them (admm_host_spline_table_eval): the kernel is
    tested, not the table."""
    tab = s._spline_tables[0]
    def ev(which):
        def fn(x):
            out = np.zeros(3)
            capi.lib().admm_host_spline_table_eval(capi.dptr(tab), which, float(x), capi.dptr(out))
            return out[0]
        return fn
    return ev(0), ev(1), ev(2)


def kind_solver(n, kind):
    """Kuhn cube of one constitutive model, built on the Solver directly (scenes.Scene passes neither kappa nor a spline)."""
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
    assert s.initialize(Settings())
    return s, verts


def cloth_with_hinges(m=6, **settings):
    sc = scenes.cloth_scene(m, **settings)
    verts, tris, lame, off = sc.tris[0]
    sc.bends.append((verts, tris, 0.02, off))
    return sc


# ---------------------------------------------------------------- CPU ------------------------------------------------------
def test_monitor_symbols_and_settings():
    """The four entry points exist in libadmm_hip.so with the documented signatures; the monitor is off by default."""
    L = capi.lib()
    sig = {name: (res, args) for name, res, args in capi.SYMBOLS}
    dp, ip = capi.c_double_p, capi.c_int_p
    assert sig["admm_hip_energy"] == (C.c_int, [C.c_void_p, dp, dp, dp])
    assert sig["admm_hip_residuals"] == (C.c_int, [C.c_void_p, dp, dp, dp, dp])
    assert sig["admm_hip_set_monitor"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert sig["admm_hip_get_monitor"] == (C.c_int, [C.c_void_p, C.c_int32, ip, dp])
    for name in ("admm_hip_energy", "admm_hip_residuals", "admm_hip_set_monitor", "admm_hip_get_monitor"):
        assert getattr(L, name) is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    for decl in ("int admm_hip_energy(admm_hip_ctx *ctx, const double *x, double *totals4, double *per_term);",
                 "int admm_hip_residuals(admm_hip_ctx *ctx, const double *x, const double *z, const double *z_prev, double *out4);",
                 "int admm_hip_set_monitor(admm_hip_ctx *ctx, int32_t mode);",
                 "int admm_hip_get_monitor(admm_hip_ctx *ctx, int32_t cap, int32_t *n, double *records);"):
        assert decl in hdr, decl
    # NULL contexts are refused, not dereferenced
    assert L.admm_hip_set_monitor(None, 1) == -1
    n = C.c_int32(0)
    assert L.admm_hip_get_monitor(None, 0, C.byref(n), None) == -1
    assert Settings().monitor == 0
    assert list(inspect.signature(Solver.energy).parameters) == ["self", "x", "per_term"]
    for m in ("residuals", "set_monitor", "admm_history"):
        assert callable(getattr(Solver, m))


def _parse_host(out):
    d = dict(V=[], T=[], R=[], states={})
    cur = None
    for line in out.strip().split("\n"):
        w = line.split()
        if w[0] == "V": d["V"].append([float(v) for v in w[1:]])
        elif w[0] == "T": d["T"].append([float(v) for v in w[1:]])
        elif w[0] == "R": d["R"].append([int(v) for v in w[1:]])
        elif w[0] == "NR": d["tri_mu"], d["tri_la"] = float(w[2]), float(w[3])
        elif w[0] == "STATE": cur = d["states"].setdefault(w[1], dict(X=[], E=[]))
        elif w[0] == "X": cur["X"].append([float(v) for v in w[1:]])
        elif w[0] == "E": cur["E"].append(float(w[1]))
    return d


def test_cpp_host_energies_match_numpy():
    """tests/cpp/test_energy.cpp --host: the mirror's host EnergyTerm::energy(D, x) of every term of the fixed scene (all eight tet kinds,
    a cloth) against the numpy restatement to 1e-12 (|E_i| + k_i vol_i); the new TriEnergyTerm::energy included, with the reference's
    known answers: 0 at rest and after a rotation."""
    exe = _build_exe("test_energy")
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    d = _parse_host(r.stdout)
    rest = np.array(d["V"]); T = np.array(d["T"])
    tets = T[:, :4].astype(int); kind = T[:, 4].astype(int); mu, la, kappa = T[:, 5], T[:, 6], T[:, 7]
    k = la + 2.0 / 3.0 * mu
    tris = np.array(d["R"])
    assert sorted(set(kind)) == list(range(8)) and len(tris) == 32
    for name, st in d["states"].items():
        x = np.array(st["X"]); E = np.array(st["E"])
        assert len(E) == len(tets) + len(tris)
        F, vol = tet_F(rest, tets, x)
        ref = np.zeros(len(tets))
        for i in range(len(tets)):
            fgh = None
            if kind[i] == pkg.TET_SPLINE_TABLE:
                q = QuadSpline(mu[i], 0.25 * la[i], 0.5 * la[i])
                fgh = (q.f, q.g, q.h)
            ref[i] = tet_energies(F[i:i + 1], vol[i:i + 1], kind[i:i + 1], mu[i:i + 1], la[i:i + 1], k[i:i + 1], kappa[i:i + 1], fgh)[0][0]
        kt = d["tri_la"] + 2.0 / 3.0 * d["tri_mu"]
        rt, st_scale = tri_energies(rest, tris, x, kt)
        ref = np.concatenate([ref, rt]); scale = np.concatenate([k * vol, st_scale])
        err = np.abs(E - ref) / (np.abs(ref) + scale)
        assert err.max() <= 1e-12, (name, int(err.argmax()), err.max())
        if name in ("rest", "rotated"):      # known answers: every energy vanishes in a rigid motion -- except stable Neo-Hookean's,
            zero = np.ones(len(E), bool)     # whose rest value is a constant by construction (alpha != 1, the log term)
            zero[:len(tets)] = kind != pkg.TET_STABLE_NH
            assert np.abs(E[zero]).max() <= 1e-12 * scale.max(), (name, np.abs(E[zero]).max())
            assert np.abs(E[len(tets):]).max() <= 1e-12 * st_scale.max()
        else:
            assert np.abs(E).max() > 1e-3 * scale.max()


# ---------------------------------------------------------------- GPU: energy ----------------------------------------------
def _energy_case(s, rest, x, pushed, lame_tri=None, table_fgh=None):
    ref, scale, S = reference_energies(s, rest, x, lame_tri, table_fgh)
    if S is not None:
        check_state(S, pushed)
    out = s.energy(x, per_term=True)
    E = out["terms"]
    assert E.shape == ref.shape
    err = np.abs(E - ref) / (np.abs(ref) + scale)
    print("energy parity: %d terms, max |E - ref| / (|ref| + k vol) = %.3e (term %d)" % (len(ref), err.max(), int(err.argmax())))
    assert err.max() <= 1e-9, (int(err.argmax()), err.max())
    f = s.flatten()
    nt, nr = len(f["tet_idx"]), len(f["tri_idx"])
    parts = (E[:nt].sum(), E[nt:nt + nr].sum(), E[nt + nr:].sum())
    for key, p in zip(("tets", "tris", "hinges"), parts):
        assert abs(out[key] - p) <= 1e-12 * max(abs(p), 1e-300) or (p == 0.0 and out[key] == 0.0), (key, out[key], p)
    assert abs(out["total"] - E.sum()) <= 1e-12 * abs(E.sum())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("case", ["nh1", "nh3", "mixed5"])
def test_energy_parity_block_shapes(case, pushed):
    """One partial wave (6 tets), a partial block (162), three kinds whose group boundaries fall inside blocks over three blocks (750):
    every term against numpy within 1e-9 (|E_i| + k_i vol_i); per_term in the CALLER's order (the mixed scene adds NH, StVK, linear --
    the library sorts linear first)."""
    if case == "mixed5":
        n = 5; sc = scenes.mixed_cube_scene(n)
    else:
        n = int(case[2]); sc = scenes.cube_scene(n, pkg.TET_NEOHOOKEAN)
    s = sc.make_solver()
    x = (pushed_state if pushed else plain_state)(sc.x, n)
    _energy_case(s, sc.x, x, pushed)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("kind", [pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED, pkg.TET_SPLINE_TABLE, pkg.TET_STABLE_NH])
def test_energy_parity_spline_kinds(kind, pushed):
    """The xu:: splines with kappa != 0, a tabulated user spline (evaluated in numpy through admm_host_spline_table_eval) and stable
    Neo-Hookean on the 162-tet cube."""
    s, verts = kind_solver(3, kind)
    x = (pushed_state if pushed else plain_state)(verts, 3)
    _energy_case(s, verts, x, pushed, table_fgh=table_functions(s) if kind == pkg.TET_SPLINE_TABLE else None)
    s.close()


@pytest.mark.gpu
def test_energy_parity_cloth_and_hinges():
    """Triangles (strain limits ignored, like the reference) and bending hinges at a perturbed state; at rest both vanish."""
    sc = cloth_with_hinges(6)
    s = sc.make_solver()
    x = scenes.perturb(sc.x, 0.02, 1) * np.array([1.1, 1.0, 0.9])
    out = _energy_case(s, sc.x, x, False, lame_tri=sc.tris[0][2])
    assert out["tets"] == 0.0 and out["tris"] > 0.0 and out["hinges"] > 0.0
    rest = s.energy(sc.x, per_term=True)
    assert np.abs(rest["terms"]).max() <= 1e-12 * out["total"]
    s.close()


@pytest.mark.gpu
def test_energy_of_device_resident_state():
    """x = None reads the state the steps left on the device."""
    sc = scenes.cube_scene(3, pkg.TET_NEOHOOKEAN, admm_iters=5)
    s = sc.make_solver()
    s.step()
    a = s.energy()                 # device-resident
    b = s.energy(s.m_x)            # the same positions, uploaded
    assert a["total"] == b["total"] and a["total"] > 0.0
    s.close()


@pytest.mark.gpu
def test_energy_and_residuals_are_bit_reproducible():
    """No floating-point atomics: two calls on the same state return identical bits."""
    rng = np.random.default_rng(3)
    for sc, n in ((scenes.mixed_cube_scene(5), 5), (cloth_with_hinges(6), 1)):
        s = sc.make_solver()
        x = plain_state(sc.x, n)
        a = s.energy(x, per_term=True); b = s.energy(x, per_term=True)
        for key in ("tets", "tris", "hinges", "total"):
            assert a[key] == b[key]
        assert np.array_equal(a["terms"], b["terms"])
        R = s.num_rows()
        z, zp = rng.standard_normal(R), rng.standard_normal(R)
        assert s.residuals(x, z, zp) == s.residuals(x, z, zp)
        s.close()


# ---------------------------------------------------------------- GPU: residual kernel -------------------------------------
def _numpy_residuals(o, x, z, zp):
    Dx = o.D @ x
    return tuple(np.linalg.norm(o.W * v) for v in (Dx - z, z - zp, z, Dx))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed5", "cloth", "one_tet", "gs_pins"])
def test_residual_kernel_against_numpy(case):
    """residuals(x, z, z_prev) with random z, z_prev against numpy |W(Dx - z)| etc.: sums of products in double precision, no SVD, so
    1e-12 relative + 1e-12 |W|_inf |x|_inf.  mixed5 carries 36 pin terms, the cloth hinges and pins; with linsolver 1 pins are no terms."""
    if case == "mixed5":
        sc = scenes.mixed_cube_scene(5)
    elif case == "cloth":
        sc = cloth_with_hinges(6)
    elif case == "one_tet":
        sc = scenes.Scene()
        verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        sc.add_tet_mesh(verts, np.array([[0, 1, 2, 3]], np.int32), Lame.soft_rubber(), pkg.TET_NEOHOOKEAN)
    else:
        sc = scenes.cube_scene(3, pkg.TET_NEOHOOKEAN, linsolver=1)
    s = sc.make_solver()
    o = sc.make_oracle()
    R = s.num_rows()
    assert R == o.R
    if case == "gs_pins":
        assert R == 9 * 162      # no pin rows
    rng = np.random.default_rng(11)
    x = scenes.perturb(sc.x, 0.03, 2).ravel()
    z, zp = rng.standard_normal(R), rng.standard_normal(R)
    got = s.residuals(x, z, zp)
    ref = _numpy_residuals(o, x, z, zp)
    atol = 1e-12 * np.abs(o.W).max() * np.abs(x).max()
    for name, a, b in zip(("primal", "dz", "wz", "wdx"), got, ref):
        print("%s: device %.15e numpy %.15e rel %.2e" % (name, a, b, abs(a - b) / b))
        assert abs(a - b) <= 1e-12 * b + atol, (name, a, b)
    s.close()


# ---------------------------------------------------------------- GPU: the monitor against the oracle ----------------------
# R: the largest |a - b| / (b + max_s b) of primal, dz and the objective over the three scenes against the oracle, as measured on
# the MI355X (see the docstring of test_monitor_matches_oracle_trace); the assertion is 10 x that.
R_MEASURED = 1.078e-8
R_ASSERT = 10.0 * R_MEASURED


def _monitor_scene(name):
    if name == "mixed4":
        return scenes.mixed_cube_scene(4, admm_iters=12)
    if name == "nh5":
        return scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, admm_iters=12)
    return scenes.cloth_scene(6, admm_iters=12)


def _oracle_history(sc, o, s):
    """one frame of the oracle with its trace -> primal, dz, objective per ADMM iteration, in numpy"""
    dt = o.dt
    x0 = o.x.copy(); v = o.v.copy()
    if abs(o.gravity) > 0:
        v[1::3] += dt * o.gravity
    xbar = x0 + dt * v
    tr = []
    o.step(trace=tr)
    zprev = o.D @ x0
    lame_tri = sc.tris[0][2] if sc.tris else None
    primal, dz, obj = [], [], []
    for z, u, b, x in tr:
        primal.append(np.linalg.norm(o.W * (o.D @ x - z)))
        dz.append(np.linalg.norm(o.W * (z - zprev)))
        zprev = z
        E = reference_energies(s, sc.x, x, lame_tri)[0].sum()
        obj.append(E + 0.5 / (dt * dt) * np.sum(o.m * (x - xbar) ** 2))
    return np.array(primal), np.array(dz), np.array(obj)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed4", "nh5", "cloth6"])
def test_monitor_matches_oracle_trace(name):
    """admm_history() of two frames (pcg_tol 1e-12, monitor 2) against the oracle's trace: primal[s] = |W(D x_s - z_s)|, dz[s] =
    |W(z_s - z_{s-1})| with z_{-1} = D x_start, objective[s] = energy(x_s) + inertia in numpy; compared as |a - b| <= R b + R max_s b
    (dz is ~1e-15 at iteration 0 of frame 0).

    Measured on an MI355X (largest ratio per scene over both frames and the three quantities): mixed4 2.7e-10 (dz, frame 0), nh5
    2.8e-9 (dz, frame 0), cloth6 1.08e-8 (objective, frame 0); primal alone stays below 2e-12.  R_MEASURED = 1.078e-8, asserted:
    R_ASSERT = 10 x R_MEASURED = 1.078e-7 -- inside the 1e-7 .. 1e-6 the step parity (x to 1e-7 of the bounding box) suggests, two
    decades under the project's 1e-5 bar."""
    sc = _monitor_scene(name)
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=2)
    o = sc.make_oracle(mode=1)
    worst = 0.0
    for frame in range(2):
        primal, dz, obj = _oracle_history(sc, o, s)
        s.step()
        h = s.admm_history()
        assert all(len(h[k]) == 12 for k in KEYS)
        for key, ref in (("primal", primal), ("dz", dz), ("objective", obj)):
            ratio = np.abs(h[key] - ref) / (ref + ref.max())
            worst = max(worst, ratio.max())
            print("%s frame %d %s: oracle %.6g .. %.6g, max ratio %.3e" % (name, frame, key, ref[0], ref[-1], ratio.max()))
        assert np.allclose(h["objective"], h["energy"] + h["inertia"], rtol=1e-15, atol=0.0)
        assert np.isfinite(h["wz"]).all() and (h["wz"] > 0).all() and (h["wdx"] > 0).all()
    print("%s: measured R = %.3e" % (name, worst))
    assert worst <= R_ASSERT, (worst, R_ASSERT)
    s.close()


@pytest.mark.gpu
def test_monitor_mode_1_leaves_the_objective_slots_zero():
    sc = _monitor_scene("mixed4")
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=1)
    s2 = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=500, monitor=2)
    s.step(); s2.step()
    h, h2 = s.admm_history(), s2.admm_history()
    assert len(h["primal"]) == 12 and (h["primal"] > 0).all()
    for key in ("energy", "inertia", "objective"):
        assert not h[key].any() and h2[key].all()
    # the four norms do not depend on the mode: the same reduction, and the steps themselves are the same to the solver's tolerance
    for key in ("primal", "dz", "wz", "wdx"):
        assert np.allclose(h[key], h2[key], rtol=1e-6, atol=1e-6 * h2[key].max())
    s.close(); s2.close()


# ---------------------------------------------------------------- GPU: the monitor does not disturb the step ---------------
def _run(sc, frames, **kw):
    s = sc.make_solver(**kw)
    for _ in range(frames):
        s.step()
    out = s.m_x.copy(), s.m_v.copy()
    s.close()
    return out


@pytest.mark.gpu
def test_monitor_does_not_change_the_gs_path():
    """linsolver 1 (the bit-reproducible GS path of tests/test_gs_persist.py): m_x, m_v with monitor 2 equal monitor 0 bit for bit."""
    sc = scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, linsolver=1)
    x0, v0 = _run(sc, 3)
    x2, v2 = _run(sc, 3, monitor=2)
    assert np.array_equal(x0, x2) and np.array_equal(v0, v2)


@pytest.mark.gpu
def test_monitor_does_not_change_the_pcg_path():
    """linsolver 0: if two plain runs are bit-identical the monitored one must be as well; otherwise its distance stays within 4x theirs."""
    sc = scenes.mixed_cube_scene(4)
    xa, va = _run(sc, 3)
    xb, vb = _run(sc, 3)
    xm, vm = _run(sc, 3, monitor=2)
    plain = max(np.abs(xa - xb).max(), np.abs(va - vb).max())
    mon = max(np.abs(xa - xm).max(), np.abs(va - vm).max())
    print("plain runs differ by %.3e, the monitored run by %.3e" % (plain, mon))
    if plain == 0.0:
        assert mon == 0.0
    else:
        assert mon <= 4.0 * plain


@pytest.mark.gpu
def test_monitor_switched_off_and_buffers_freed():
    """After set_monitor(0) the next step records nothing; a closed context leaves no device buffer behind."""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = cloth_with_hinges(6, admm_iters=4)
    s = sc.make_solver(monitor=2)
    s.step()
    assert len(s.admm_history()["primal"]) == 4
    s.energy(per_term=True)
    R = s.num_rows()
    s.residuals(s.m_x, np.zeros(R), np.zeros(R))
    s.set_monitor(0)
    s.step()
    h = s.admm_history()
    assert all(len(h[k]) == 0 for k in KEYS)
    s.set_monitor(1)
    s.step()
    assert len(s.admm_history()["primal"]) == 4
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)


@pytest.mark.gpu
def test_monitor_refuses_multi_rank_contexts():
    """world_size > 1: the four entry points return an error with a message instead of a partial sum."""
    sc = scenes.cube_scene(3, pkg.TET_NEOHOOKEAN)
    s = sc.make_solver(world_size=2, rank=0)
    with pytest.raises(pkg.AdmmHipError):
        s.set_monitor(1)
    with pytest.raises(pkg.AdmmHipError):
        s.energy(sc.x)
    R = s.num_rows()
    with pytest.raises(pkg.AdmmHipError):
        s.residuals(sc.x, np.zeros(R), np.zeros(R))
    with pytest.raises(pkg.AdmmHipError):
        s.admm_history()
    s.close()


# ---------------------------------------------------------------- GPU: C++ -------------------------------------------------
@pytest.mark.gpu
def test_cpp_energy_and_monitor():
    """tests/cpp/test_energy.cpp: Solver::energy(x) equals the sum of the mirror's host per-term energies within the per-term bar, and
    with Settings::monitor = 1 admm_history() has admm_iters finite, positive primal residuals."""
    exe = _build_exe("test_energy")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
