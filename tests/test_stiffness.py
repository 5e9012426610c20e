"""The tangent stiffness on the device: admm_hip_stiffness_apply (csrc/tangent.hpp, the per-element algebra in csrc/device_math.hpp),
its Python and C++ faces.  out = K(x) d + shift m o d with K = d2E/dx2 = -df/dx of the energy energy() sums.

The reference has no Hessian (its gradient() throws), so the yardstick is built here, in two legs:
 (a) mpmath: the per-element P(F) of every kind at 60 digits (mp.svd_r, the derivatives of the densities), differentiated as
     dP = [P(F + h dF) - P(F - h dF)] / 2h with h = 1e-20 -- no tangent formula enters, and it is valid at exactly equal stretches, where P
     is smooth in F.  The tabulated spline is the DEVICE's interpolant (the quintic Hermite pieces of admm_host_spline_table_eval on the
     table's own nodes), restated in mp because a difference quotient at h = 1e-20 cannot go through a float64 evaluator;
     test_mp_table_is_the_interpolant_the_device_evaluates holds the restatement to admm_host_spline_table_eval.
 (b) numpy: K d of whole meshes (tets, triangles, hinges) in float64, shown to be the derivative of test_forces.numpy_forces by central
     differences at h and h / 2 (the protocol and the bars of test_forces._fd_case).
tangent_coefs() -- Hs, alpha, beta of one element from its signed stretches, generic over float and mp.mpf -- serves leg (b) and gives
leg (a) its scale h_el; it is held by both legs."""
import ctypes as C
import functools
import inspect
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Lame, Settings, Solver
from test_cpp_api import _build_exe
from test_device_math_host import _rot
from test_energy_monitor import (check_state, cloth_with_hinges, kind_solver, plain_state, pushed_state, signed_stretches, tet_F,
                                 tet_energies)
from test_forces import (ALL_KINDS, SPLINE_KINDS, _one_tet_state, _tet_scene, cloth_states, kind_description, numpy_forces, rigid,
                         stretch_gradient, table_fgh)

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))      # (i, j, the third)
ERR_ARG, ERR_STATE = -1, -4                    # include/admm_hip.h: ADMM_HIP_ERR_ARG, ADMM_HIP_ERR_STATE
FN = 4 + 3 * 1024                              # doubles of one tabulated function (device_math.hpp: kSplineFnDoubles)


# ---------------------------------------------------------------- the coefficients of one element ------------------------------
def uses_abs(kd):
    """the kinds whose density is evaluated at |sigma| (forces.hpp); StVK and stable Neo-Hookean take the signed stretches"""
    return kd not in (pkg.TET_STVK, pkg.TET_STABLE_NH)


def density2(e, kd, mu, la, k, kappa, log, tab=None, grad_only=False):
    """g = dpsi/de [3], H = d2psi/de2 [3][3] and the divided differences al' = (g_i - g_j) / (e_i - e_j), be' = (g_i + g_j) / (e_i + e_j)
    per pair of PAIRS, in closed form (finite at e_i = e_j resp. e_i = -e_j), in the coordinates e the density takes.  Generic in the
    number type.  grad_only: the tabulated spline stops after g (its H, al', be' cost 20 table evaluations more)."""
    J = e[0] * e[1] * e[2]
    dJ = [e[1] * e[2], e[2] * e[0], e[0] * e[1]]
    H = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    al, be = [0, 0, 0], [0, 0, 0]
    nh = kd in (pkg.TET_NEOHOOKEAN, pkg.TET_SPLINE_NH); stvk = kd in (pkg.TET_STVK, pkg.TET_SPLINE_STVK)
    if kd == pkg.TET_LINEAR:
        g = [k * (x - 1) for x in e]
        for q, (i, j, l) in enumerate(PAIRS):
            al[q] = k; be[q] = k * ((e[i] - 1) + (e[j] - 1)) / (e[i] + e[j])
        for i in range(3):
            H[i][i] = k
    elif nh:
        lJ = log(J)
        g = [mu * (x - 1 / x) + la * lJ / x for x in e]
        for i in range(3):
            for j in range(3):
                H[i][j] = la / (e[i] * e[j])
            H[i][i] = mu * (1 + 1 / e[i] ** 2) + la * (1 - lJ) / e[i] ** 2
        for q, (i, j, l) in enumerate(PAIRS):
            al[q] = mu + (mu - la * lJ) / (e[i] * e[j]); be[q] = mu - (mu - la * lJ) / (e[i] * e[j])
    elif stvk:
        trE = (e[0] ** 2 + e[1] ** 2 + e[2] ** 2 - 3) / 2
        g = [x * (mu * (x * x - 1) + la * trE) for x in e]
        for i in range(3):
            for j in range(3):
                H[i][j] = la * e[i] * e[j]
            H[i][i] = mu * (3 * e[i] ** 2 - 1) + la * trE + la * e[i] ** 2
        for q, (i, j, l) in enumerate(PAIRS):
            al[q] = mu * (e[i] ** 2 + e[i] * e[j] + e[j] ** 2 - 1) + la * trE
            be[q] = mu * (e[i] ** 2 - e[i] * e[j] + e[j] ** 2 - 1) + la * trE
    elif kd == pkg.TET_SPLINE_COROTATED:
        tr = e[0] + e[1] + e[2] - 3
        g = [2 * mu * (x - 1) + la * tr for x in e]
        for i in range(3):
            for j in range(3):
                H[i][j] = la
            H[i][i] = 2 * mu + la
        for q, (i, j, l) in enumerate(PAIRS):
            al[q] = 2 * mu; be[q] = (g[i] + g[j]) / (e[i] + e[j])
    elif kd == pkg.TET_STABLE_NH:
        mus = mu * 4 / 3; las = la + mu * 5 / 6; alpha = 1 + mus * 3 / (4 * las)
        IC = e[0] ** 2 + e[1] ** 2 + e[2] ** 2; qq = 1 / (IC + 1)
        a1 = mus * (1 - qq); a2 = 2 * mus * qq * qq; Ja = J - alpha
        g = [a1 * e[i] + las * Ja * dJ[i] for i in range(3)]
        for i in range(3):
            H[i][i] = a1 + a2 * e[i] ** 2 + las * dJ[i] ** 2
        for q, (i, j, l) in enumerate(PAIRS):
            H[i][j] = H[j][i] = a2 * e[i] * e[j] + las * (dJ[i] * dJ[j] + Ja * e[l])
            al[q] = a1 - las * Ja * e[l]; be[q] = a1 + las * Ja * e[l]
    elif kd == pkg.TET_SPLINE_TABLE:
        g = [0, 0, 0]
        for i in range(3):
            j, l = (i + 1) % 3, (i + 2) % 3
            g[i] = tab.d1(0, e[i]) + tab.d1(1, e[i] * e[j]) * e[j] + tab.d1(1, e[i] * e[l]) * e[l] + tab.d1(2, J) * dJ[i]
        if grad_only:
            return g, H, al, be
        for i in range(3):
            j, l = (i + 1) % 3, (i + 2) % 3
            H[i][i] = tab.d2(0, e[i]) + tab.d2(1, e[i] * e[j]) * e[j] ** 2 + tab.d2(1, e[i] * e[l]) * e[l] ** 2 + tab.d2(2, J) * dJ[i] ** 2
        for q, (i, j, l) in enumerate(PAIRS):
            H[i][j] = H[j][i] = tab.d2(1, e[i] * e[j]) * e[i] * e[j] + tab.d1(1, e[i] * e[j]) + tab.d2(2, J) * dJ[i] * dJ[j] + tab.d1(2, J) * e[l]
            al[q] = tab.dd(0, e[i], e[j]) - tab.d1(1, e[i] * e[j]) + e[l] ** 2 * tab.dd(1, e[i] * e[l], e[j] * e[l]) - tab.d1(2, J) * e[l]
            be[q] = (g[i] + g[j]) / (e[i] + e[j])
    else:
        raise KeyError(kd)
    if pkg.TET_SPLINE_NH <= kd <= pkg.TET_SPLINE_COROTATED and kappa != 0:      # c(J) = kappa / 12 ((1 - J) / 6)^3
        t = (1 - J) / 6
        c1 = -kappa * t * t / 24; c2 = kappa * t / 72
        for i in range(3):
            g[i] = g[i] + c1 * dJ[i]
            H[i][i] = H[i][i] + c2 * dJ[i] ** 2
        for q, (i, j, l) in enumerate(PAIRS):
            H[i][j] = H[j][i] = H[i][j] + c2 * dJ[i] * dJ[j] + c1 * e[l]
            al[q] = al[q] - c1 * e[l]; be[q] = be[q] + c1 * e[l]
    return g, H, al, be


def tangent_coefs(s, kd, mu, la, k, kappa, log, tab=None, grad_only=False):
    """p = dpsi/dsigma [3], Hs = d2psi/dsigma2 [3][3], alpha, beta per pair of PAIRS, in the frame of the signed SVD.  For the |sigma|
    kinds U diag(sign) is an SVD with the unsigned stretches in which density2 holds as it stands; carried back that is p_i = s_i g_i,
    Hs_ij = s_i s_j H_ij and (alpha, beta) swapped where s_i s_j < 0."""
    if not uses_abs(kd):
        return density2(list(s), kd, mu, la, k, kappa, log, tab, grad_only)
    sg = [-1 if x < 0 else 1 for x in s]
    g, H, al, be = density2([abs(x) for x in s], kd, mu, la, k, kappa, log, tab, grad_only)
    for q, (i, j, l) in enumerate(PAIRS):
        if sg[i] * sg[j] < 0:
            H[i][j] = H[j][i] = -H[i][j]
            al[q], be[q] = be[q], al[q]
    return [sg[i] * g[i] for i in range(3)], H, al, be


def h_el(H, al, be):
    return max([abs(H[i][j]) for i in range(3) for j in range(3)] + [abs(x) for x in al] + [abs(x) for x in be])


class NpTable:
    """the tabulated spline as the device evaluates it (admm_host_spline_table_eval), float64; the divided difference of F' is the quotient
    where the arguments are 5 % apart and the 5-point Gauss mean of F'' where they are closer"""
    GX, GW = np.polynomial.legendre.leggauss(5)

    def __init__(self, tab):
        self.tab = tab

    def ev(self, which, x, order):
        out = np.zeros(3)
        capi.lib().admm_host_spline_table_eval(capi.dptr(self.tab), which, float(x), capi.dptr(out))
        return out[order]

    def d1(self, which, x): return self.ev(which, x, 1)
    def d2(self, which, x): return self.ev(which, x, 2)

    def dd(self, which, x, y):
        if abs(x - y) > 0.05 * max(abs(x), abs(y)):
            return (self.d1(which, x) - self.d1(which, y)) / (x - y)
        m, r = 0.5 * (x + y), 0.5 * (x - y)
        return 0.5 * sum(w * self.d2(which, m + r * t) for t, w in zip(self.GX, self.GW))


class MpTable:
    """The same interpolant at mp precision: spline_table_eval of csrc/device_math.hpp on the table's own float64 nodes -- quintic Hermite
    pieces in t = ln x, the end nodes' Taylor quadratics in x outside.  The divided difference is the quotient (exact enough at 60 digits
    down to differences of 1e-40) and F'' where the arguments are equal."""

    def __init__(self, tab):
        self.tab = tab

    def ev(self, which, x):
        b = which * FN
        t0, dt, idt = (mp.mpf(float(v)) for v in self.tab[b:b + 3]); n = int(self.tab[b + 3])
        r = (mp.log(x) - t0) * idt
        i = min(max(int(mp.floor(r)), 0), n - 2)
        u = r - i
        a = [mp.mpf(float(v)) for v in self.tab[b + 4 + 3 * i:b + 4 + 3 * i + 6]]
        if u < 0 or u > 1:
            e = a[:3] if u < 0 else a[3:]
            xe = mp.mpf(float(np.exp(float(t0) if u < 0 else float(np.float64(self.tab[b]) + np.float64(self.tab[b + 1]) * (n - 1)))))
            d1 = e[1] / xe; d2 = (e[2] - e[1]) / (xe * xe); dx = x - xe
            return e[0] + dx * (d1 + dx * d2 / 2), d1 + dx * d2, d2
        F0, G0, H0, F1n, G1, H1 = a[0], a[1] * dt, a[2] * dt * dt, a[3], a[4] * dt, a[5] * dt * dt
        dF = F1n - F0
        c = [F0, G0, H0 / 2, 10 * dF - 6 * G0 - 4 * G1 - 3 * H0 / 2 + H1 / 2, -15 * dF + 8 * G0 + 7 * G1 + 3 * H0 / 2 - H1,
             6 * dF - 3 * (G0 + G1) - H0 / 2 + H1 / 2]
        p = sum(c[m] * u ** m for m in range(6))
        pt = sum(m * c[m] * u ** (m - 1) for m in range(1, 6)) * idt
        ptt = sum(m * (m - 1) * c[m] * u ** (m - 2) for m in range(2, 6)) * idt * idt
        return p, pt / x, (ptt - pt) / (x * x)

    def d1(self, which, x): return self.ev(which, x)[1]
    def d2(self, which, x): return self.ev(which, x)[2]

    def dd(self, which, x, y):
        return self.d2(which, x) if x == y else (self.d1(which, x) - self.d1(which, y)) / (x - y)


# ---------------------------------------------------------------- leg (b): K d of whole meshes in numpy -------------------------
def _svd_signed(F):
    U, sv, Vt = np.linalg.svd(F)
    s = sv.copy()
    if np.linalg.det(F) < 0.0:
        s[2] = -s[2]; U = U.copy(); U[:, 2] = -U[:, 2]
    return U, s, Vt


def _element_dP(U, Vt, H, al, be, dF):
    A = U.T @ dF @ Vt.T
    B = np.zeros((3, 3))
    for i in range(3):
        B[i, i] = sum(H[i][j] * A[j, j] for j in range(3))
    for q, (i, j, l) in enumerate(PAIRS):
        B[i, j] = 0.5 * al[q] * (A[i, j] + A[j, i]) + 0.5 * be[q] * (A[i, j] - A[j, i])
        B[j, i] = 0.5 * al[q] * (A[i, j] + A[j, i]) - 0.5 * be[q] * (A[i, j] - A[j, i])
    return U @ B @ Vt


def numpy_stiffness(flat, rest, x, D, tri_k=None, tab=None):
    """-> K(x) d_j [k, nv, 3] and the per-vertex scale of the derived bar [k, nv]:
    sum_{i in v} h_i vol_i |Binv_i|_F^2 max_{u in i} |d_u| over the tets (h_i the largest of the element's |Hs|, |alpha|, |beta|),
    w^2 |rest|_F^2 and stiffness |c|^2 in its place for triangles and hinges."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(D, dtype=np.float64).reshape(-1, len(rest), 3)
    out = np.zeros(D.shape); scale = np.zeros(D.shape[:2])
    dn = np.linalg.norm(D, axis=2)
    tets = flat["tet_idx"]
    if len(tets):
        F, vol = tet_F(rest, tets, x)
        X = rest[tets]
        Binv = np.linalg.inv(np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2))
        ntab = NpTable(tab) if tab is not None else None
        for i in range(len(tets)):
            U, s, Vt = _svd_signed(F[i])
            _, H, al, be = tangent_coefs(s, int(flat["tet_kind"][i]), flat["tet_mu"][i], flat["tet_lambda"][i], flat["tet_k"][i],
                                         flat["tet_kappa"][i], np.log, ntab)
            hs = h_el(H, al, be) * vol[i] * np.sum(Binv[i] ** 2)
            for j in range(len(D)):
                d = D[j][tets[i]]
                dF = np.stack([d[1] - d[0], d[2] - d[0], d[3] - d[0]], axis=1) @ Binv[i]
                G = vol[i] * _element_dP(U, Vt, H, al, be, dF) @ Binv[i].T
                out[j, tets[i, 1]] += G[:, 0]; out[j, tets[i, 2]] += G[:, 1]; out[j, tets[i, 3]] += G[:, 2]; out[j, tets[i, 0]] -= G.sum(axis=1)
                scale[j, tets[i]] += hs * dn[j, tets[i]].max()
    tris = flat["tri_idx"]
    if len(tris):
        X = rest[tris]; p = x[tris]
        e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        n = np.cross(e1, e2); area = 0.5 * np.linalg.norm(n, axis=1)
        u = e1 / np.linalg.norm(e1, axis=1)[:, None]
        w = np.cross(n / (2.0 * area)[:, None], u)
        Dm = np.stack([np.stack([np.sum(e1 * u, 1), np.sum(e1 * w, 1)], 1), np.stack([np.sum(e2 * u, 1), np.sum(e2 * w, 1)], 1)], axis=2)
        Bi = np.linalg.inv(Dm)
        for i in range(len(tris)):
            F = np.stack([p[i, 1] - p[i, 0], p[i, 2] - p[i, 0]], axis=1) @ Bi[i]
            U, sv, Vt = np.linalg.svd(F, full_matrices=False)
            hs = flat["tri_weight"][i] ** 2 * np.sum(flat["tri_rest"][i] ** 2)
            for j in range(len(D)):
                d = D[j][tris[i]]
                dF = np.stack([d[1] - d[0], d[2] - d[0]], axis=1) @ Bi[i]
                A = U.T @ dF @ Vt.T
                om = (A[1, 0] - A[0, 1]) / (sv[0] + sv[1])
                dR = U @ np.array([[0.0, -om], [om, 0.0]]) @ Vt + (dF - U @ (U.T @ dF)) @ Vt.T @ np.diag(1.0 / sv) @ Vt
                G = tri_k * area[i] * (dF - dR) @ Bi[i].T
                out[j, tris[i, 1]] += G[:, 0]; out[j, tris[i, 2]] += G[:, 1]; out[j, tris[i, 0]] -= G.sum(axis=1)
                scale[j, tris[i]] += hs * dn[j, tris[i]].max()
    idx = flat["bend_idx"]
    if len(idx):
        c, st = flat["bend_coef"], flat["bend_stiffness"]
        for j in range(len(D)):
            Dd = np.einsum("hk,hkj->hj", c, D[j][idx])
            for h in range(len(idx)):
                for k in range(4):
                    out[j, idx[h, k]] += st[h] * c[h, k] * Dd[h]
                scale[j, idx[h]] += st[h] * np.sum(c[h] ** 2) * dn[j, idx[h]].max()
    return out, scale


def _directions(rng, shape, k):
    D = rng.standard_normal((k,) + tuple(shape))
    return D / np.linalg.norm(D, axis=2).max(axis=1)[:, None, None]


def _fd_stiffness(name, flat, rest, states, tri_k=None, table=None):
    """central differences of numpy_forces along 8 random directions at h and h / 2 against -K d (test_forces._fd_case one derivative up)"""
    dfgh = table_fgh(table)[1] if table is not None else None
    rng = np.random.default_rng(19)
    edge = np.linalg.norm(rest[flat["tet_idx"][0, 1]] - rest[flat["tet_idx"][0, 0]]) if len(flat["tet_idx"]) else \
        np.linalg.norm(rest[flat["tri_idx"][0, 1]] - rest[flat["tri_idx"][0, 0]])
    h = 4e-4 * edge
    worst = 0.0
    for x in states:
        D = _directions(rng, x.shape, 8)
        Kd = numpy_stiffness(flat, rest, x, D, tri_k, table)[0]
        f = lambda y: numpy_forces(flat, rest, y, tri_k, dfgh)[0]
        for d, ana in zip(D, Kd):
            e1 = np.linalg.norm(-(f(x + h * d) - f(x - h * d)) / (2.0 * h) - ana)
            e2 = np.linalg.norm(-(f(x + 0.5 * h * d) - f(x - 0.5 * h * d)) / h - ana)
            bar = np.linalg.norm(ana)
            worst = max(worst, e2 / bar)
            assert 3.0 <= e1 / e2 <= 5.0, (name, e1, e2, e1 / e2)
            assert e2 <= 1e-6 * bar, (name, e2, bar)
    print("%s: largest discrepancy at h / 2 = %.3e |K d|" % (name, worst))


# ---------------------------------------------------------------- CPU: symbols, leg (b) ----------------------------------------
def test_stiffness_symbol_and_signatures():
    """The entry point exists in libadmm_hip.so with the documented signature and is declared in the header; a NULL context, NULL
    directions and n_vec < 1 are refused; Solver.stiffness_apply has the documented parameters."""
    L = capi.lib()
    sig = {name: (res, args) for name, res, args in capi.SYMBOLS}
    cdp = capi.c_double_p
    assert sig["admm_hip_stiffness_apply"] == (C.c_int, [C.c_void_p, cdp, C.c_int32, cdp, C.c_double, cdp])
    assert L.admm_hip_stiffness_apply is not None
    with open(os.path.join(os.path.dirname(HERE), "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    decl = "int admm_hip_stiffness_apply(admm_hip_ctx *ctx, const double *x, int32_t n_vec, const double *d, double shift, double *out);"
    assert decl in hdr, decl
    out = np.zeros(3)
    assert L.admm_hip_stiffness_apply(None, None, 1, capi.dptr(out), 0.0, capi.dptr(out)) == ERR_ARG
    assert list(inspect.signature(Solver.stiffness_apply).parameters) == ["self", "d", "x", "shift"]
    for word in ("shift", "Single-GPU contexts", "+K d"):
        assert word in Solver.stiffness_apply.__doc__, word


def test_coefficients_carry_the_gradient_of_test_forces():
    """tangent_coefs' p is test_forces.stretch_gradient (the forces' own yardstick), plain and inverted, all eight kinds"""
    rng = np.random.default_rng(3)
    lame = Lame.soft_rubber()
    tab = kind_description(1, pkg.TET_SPLINE_TABLE)[2]
    for kd in ALL_KINDS:
        for _ in range(20):
            s = rng.uniform(0.5, 2.0, 3) * np.array([1.0, 1.0, rng.choice([-1.0, 1.0])])
            kap = 0.3 * lame.lambda_
            p = tangent_coefs(s, kd, lame.mu, lame.lambda_, lame.bulk_modulus(), kap, np.log, NpTable(tab))[0]
            ref = stretch_gradient(s, kd, lame.mu, lame.lambda_, lame.bulk_modulus(), kap, table_fgh(tab)[1])
            assert np.allclose(p, ref, rtol=1e-13, atol=1e-13 * lame.lambda_), (kd, p, ref)


def test_mp_table_is_the_interpolant_the_device_evaluates():
    """MpTable against admm_host_spline_table_eval: F, F', F'' of f, g, h inside the table, at a node, and in both Taylor continuations, to
    1e-12 of their size (the evaluator's own float64 rounding)."""
    tab = kind_description(1, pkg.TET_SPLINE_TABLE)[2]
    m, n = MpTable(tab), NpTable(tab)
    rng = np.random.default_rng(5)
    with mp.workdps(40):
        for which in range(3):
            lo, hi = 0.02 ** (which + 1), 50.0 ** (which + 1)
            xs = list(np.exp(rng.uniform(np.log(lo), np.log(hi), 40))) + [1.0, 0.3 * lo, 1e-3 * lo, 2.0 * hi, 1e3 * hi]
            for x in xs:
                got = [float(v) for v in m.ev(which, mp.mpf(float(x)))]
                ref = [n.ev(which, x, o) for o in range(3)]
                sc = [abs(ref[0]) + abs(ref[1]) * x + abs(ref[2]) * x * x + 1e-300] * 3
                sc = [sc[0], sc[1] / x, sc[2] / (x * x)]
                for o in range(3):
                    assert abs(got[o] - ref[o]) <= 1e-12 * sc[o], (which, x, o, got[o], ref[o])


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_numpy_stiffness_is_the_derivative_of_the_numpy_forces_tets(kind):
    """Leg (b) before any GPU sees it: on the 48-tet Kuhn cube of every kind, at the plain and the pushed (inverted, |sigma| >= 0.1) state,
    the discrepancy between the central difference of test_forces.numpy_forces and -K d falls by 4 +- 25 % from h to h / 2 and is
    <= 1e-6 |K d| at the smaller h."""
    flat, verts, tab = kind_description(2, kind)
    states = (plain_state(verts, 2), pushed_state(verts, 2))
    for x, pushed in zip(states, (False, True)):
        check_state(signed_stretches(tet_F(verts, flat["tet_idx"], x)[0]), pushed)
    _fd_stiffness("kind %d" % kind, flat, verts, states, table=tab)


def test_numpy_stiffness_is_the_derivative_of_the_numpy_forces_cloth():
    """The same for triangles (strain limits ignored) and bending hinges."""
    sc = cloth_with_hinges(4, limits=None)
    s = sc.make_solver(init=False)
    _fd_stiffness("cloth", s.flatten(), sc.x, cloth_states(sc), tri_k=sc.tris[0][2].bulk_modulus())


# ---------------------------------------------------------------- leg (a): the element families in mp ---------------------------
FAMILIES = ("generic", "rest", "rotated rest", "all equal", "two equal", "two nearly equal", "one inverted", "equal and inverted",
            "nearly equal and inverted", "scaled 1e+-3")
N_FAM, N_DIR = 64, 3
DPS = 60
H_MP = mp.mpf("1e-20")
LAME = Lame.soft_rubber()
MU, LA, KK = LAME.mu, LAME.lambda_, LAME.bulk_modulus()
KAPPA = 0.3 * LA


@functools.lru_cache(None)
def family_F():
    """[10][64] deformation gradients U diag(sigma) V^T with random rotations U, V (float64: what every consumer gets), their stretches
    as built, and 3 random dF of unit size per element"""
    rng = np.random.default_rng(11)
    n = N_FAM
    S = {}
    S[0] = rng.uniform(0.5, 2.0, (n, 3))
    S[1] = np.ones((n, 3)); S[2] = np.ones((n, 3))
    S[3] = np.repeat(rng.uniform(0.5, 2.0, (n, 1)), 3, axis=1)
    S[4] = rng.uniform(0.5, 2.0, (n, 3)); S[4][:, 1] = S[4][:, 0]
    S[5] = rng.uniform(0.5, 2.0, (n, 3)); S[5][:, 1] = S[5][:, 0] * (1.0 + np.array([1e-12, 1e-9, 1e-6, 1e-3])[np.arange(n) % 4] * rng.choice([-1.0, 1.0], n))
    S[6] = rng.uniform(0.5, 2.0, (n, 3)); S[6][:, 2] = -rng.uniform(0.1, 1.5, n)
    S[7] = rng.uniform(0.5, 2.0, (n, 3)); S[7][:, 2] = -S[7][:, 1]
    S[8] = rng.uniform(0.5, 2.0, (n, 3)); S[8][:, 2] = -S[8][:, 1] * (1.0 + 1e-9 * rng.uniform(-1.0, 1.0, n))
    S[9] = rng.uniform(0.5, 2.0, (n, 3)) * np.where(np.arange(n) % 2 == 0, 1e3, 1e-3)[:, None]
    F = np.zeros((len(FAMILIES), n, 3, 3))
    for f in range(len(FAMILIES)):
        U, V = _rot(rng, n), _rot(rng, n)
        if f == 1:
            U = V = np.repeat(np.eye(3)[None], n, 0)
        elif f == 2:
            V = np.repeat(np.eye(3)[None], n, 0)
        F[f] = U @ (S[f][:, :, None] * np.eye(3)) @ np.transpose(V, (0, 2, 1))
    for f in (6, 7, 8):      # the inverted families stay in the range the tolerances are derived for (no J <= 0 for the |sigma| kinds)
        check_state(signed_stretches(F[f]), True)
    dF = rng.standard_normal((len(FAMILIES), n, N_DIR, 3, 3))
    dF /= np.linalg.norm(dF, axis=(3, 4))[..., None, None]
    return F, np.stack([S[f] for f in range(len(FAMILIES))]), dF


def _mpm(A):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in A])


def _mp_svd_signed(Fm):
    U, S, V = mp.svd_r(Fm)      # Fm = U diag(S) V, S >= 0 descending
    s = [S[i] for i in range(3)]
    if mp.det(Fm) < 0:
        s[2] = -s[2]
        for r in range(3):
            U[r, 2] = -U[r, 2]
    return U, s, V


@functools.lru_cache(None)
def mp_frames():
    """the signed SVDs of F and of F +- h dF at 60 digits: shared by the eight kinds (the frames do not depend on the density)"""
    F, _, dF = family_F()
    out = {}
    with mp.workdps(DPS):
        for f in range(len(FAMILIES)):
            for i in range(N_FAM):
                Fm = _mpm(F[f, i])
                out[f, i] = _mp_svd_signed(Fm)
                for j in range(N_DIR):
                    dm = _mpm(dF[f, i, j])
                    out[f, i, j] = (_mp_svd_signed(Fm + H_MP * dm), _mp_svd_signed(Fm - H_MP * dm))
    return out


def mp_reference(kd, kappa, tab=None):
    """leg (a) for one kind: dP [10][64][3][3][3] (float64 of the mp difference quotient) and h_el [10][64] from the mp coefficients"""
    fr = mp_frames()
    ref = np.zeros((len(FAMILIES), N_FAM, N_DIR, 3, 3)); hel = np.zeros((len(FAMILIES), N_FAM))
    with mp.workdps(DPS):
        mtab = MpTable(tab) if tab is not None else None
        par = (kd, mp.mpf(MU), mp.mpf(LA), mp.mpf(KK), mp.mpf(kappa), mp.log, mtab)

        def P(frame):
            U, s, V = frame
            return U * mp.diag(tangent_coefs(s, *par, grad_only=True)[0]) * V
        for f in range(len(FAMILIES)):
            for i in range(N_FAM):
                _, H, al, be = tangent_coefs(fr[f, i][1], *par)
                hel[f, i] = float(h_el(H, al, be))
                for j in range(N_DIR):
                    dPm = (P(fr[f, i, j][0]) - P(fr[f, i, j][1])) / (2 * H_MP)
                    ref[f, i, j] = np.array([[float(dPm[r, c]) for c in range(3)] for r in range(3)])
    return ref, hel


def model_args(kd):
    """kernels.hpp: Mat of a kind -> (grp, type)"""
    return {pkg.TET_LINEAR: (0, 0), pkg.TET_NEOHOOKEAN: (1, 0), pkg.TET_STVK: (2, 0), pkg.TET_SPLINE_NH: (4, 0), pkg.TET_SPLINE_STVK: (4, 1),
            pkg.TET_SPLINE_COROTATED: (4, 2), pkg.TET_SPLINE_TABLE: (4, 3), pkg.TET_STABLE_NH: (4, 4)}[kd]


@pytest.fixture(scope="module")
def th(tmp_path_factory):
    """tests/hostmath/tangent_host.cpp compiled with g++, as test_device_math_host.build_hostmath compiles hostmath.cpp"""
    out = os.path.join(str(tmp_path_factory.mktemp("tangent_host")), "libtangent_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "tangent_host.cpp")])
    return C.CDLL(out)


def host_dP(L, grp, typ, mu, la, k, kappa, tab, F, dF):
    """hm_tet_tangent: F [n, 3, 3], dF [n, nd, 3, 3] -> dP [n, nd, 3, 3], coefficients [n, 12]"""
    n, nd = len(F), dF.shape[1]
    Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1))); dFc = np.ascontiguousarray(np.transpose(dF, (0, 1, 3, 2)))
    dP = np.zeros((n, nd, 3, 3)); coef = np.zeros((n, 12)); S = np.zeros((n, 3))
    L.hm_tet_tangent(C.c_int(n), C.c_int(nd), C.c_int(grp), C.c_int(typ), C.c_double(mu), C.c_double(la), C.c_double(k), C.c_double(kappa),
                     None if tab is None else tab.ctypes.data_as(dp), Fc.ctypes.data_as(dp), dFc.ctypes.data_as(dp), dP.ctypes.data_as(dp),
                     coef.ctypes.data_as(dp), S.ctypes.data_as(dp))
    return np.transpose(dP, (0, 1, 3, 2)), coef


# The bar of every family and kind: the local step's 1e-10 oracle bar on a derivative.  ONE relaxation, the tabulated spline, in every
# family alike: its second derivative comes out of a float64 evaluator that forms the quintic Hermite coefficients from differences of
# neighbouring nodes (1024 nodes: the differences are 1e-6 of the values) -- the table's own representation error, the 2e-7 that already
# relaxes check G of test_local_step_edges.py.  Measured: <= 8.4e-11, the other seven kinds <= 3.1e-14.  No family is skipped.
BAR = 1e-10
BAR_TABLE = 2e-7


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_element_tangent_on_the_host_against_mp(kind, th):
    """device_math.hpp's tet_tangent_coef / tet_tangent_apply compiled for the host, 10 families x 64 elements x 3 dF, against leg (a):
    |dP - ref|_F <= 1e-10 h_el |dF|_F.

    Measured (host build), the worst |dP - ref| / (h_el |dF|) over the ten families: linear 2.8e-14, Neo-Hookean 2.4e-14, StVK 3.0e-14, the
    kappa splines 1.6e-14 / 3.1e-14 / 2.0e-14, stable Neo-Hookean 2.8e-14 (the one-inverted, nearly-equal and scaled families; rest 2.5e-16),
    the tabulated spline 8.4e-11; per family: DESIGN.md 4i."""
    F, _, dF = family_F()
    tab = kind_description(1, kind)[2] if kind == pkg.TET_SPLINE_TABLE else None
    kappa = KAPPA if pkg.TET_SPLINE_NH <= kind <= pkg.TET_SPLINE_COROTATED else 0.0
    ref, hel = mp_reference(kind, kappa, tab)
    grp, typ = model_args(kind)
    bar = BAR_TABLE if kind == pkg.TET_SPLINE_TABLE else BAR
    worst = []
    for f, name in enumerate(FAMILIES):
        got, _ = host_dP(th, grp, typ, MU, LA, KK, kappa, tab, F[f], dF[f])
        err = np.linalg.norm(got - ref[f], axis=(2, 3)) / hel[f][:, None]      # |dF| = 1
        worst.append(err.max())
    print("kind %d: worst |dP - ref| / (h_el |dF|) per family: %s  (bar %.0e)" % (kind, " ".join("%.1e" % w for w in worst), bar))
    for name, w in zip(FAMILIES, worst):
        assert w <= bar, (kind, name, w)


def host_energy_grad(L, grp, typ, mu, la, k, kappa, tab, S):
    """hm_tet_energy_grad: signed stretches S [n, 3] -> psi [n], sg [n, 3]"""
    n = len(S)
    Sc = np.ascontiguousarray(S, dtype=np.float64); psi = np.zeros(n); sg = np.zeros((n, 3))
    L.hm_tet_energy_grad(C.c_int(n), C.c_int(grp), C.c_int(typ), C.c_double(mu), C.c_double(la), C.c_double(k), C.c_double(kappa),
                         None if tab is None else tab.ctypes.data_as(dp), Sc.ctypes.data_as(dp), psi.ctypes.data_as(dp), sg.ctypes.data_as(dp))
    return psi, sg


# E: the largest relative deviation of the host-compiled tet_energy_grad from the numpy functions over the eight kinds and the ten families,
# as measured with g++ -O2 on x86-64 (per kind: the docstring of test_element_energy_and_gradient_on_the_host); the assertion is 10 x that.
# Relative: |psi - ref| / max(|ref|, k max(1, |s|^2)) and max_i |sg_i - ref_i| / max(max_i |ref_i|, k max(1, |s|^2)) -- the value's own
# size, with k max(1, |s|^2) as the floor where it cancels (at and near rest psi and g vanish).  The floor alone does not serve as the unit:
# at the stretches of 1e3 of the scaled family the quartic and the c(J) ~ J^3 densities reach 1e12 .. 1e27 k, and one ulp of them is far
# above 1e-12 k |s|^2 without anything being wrong.
E_MEASURED = 4.4e-15
E_ASSERT = 10.0 * E_MEASURED


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_element_energy_and_gradient_on_the_host(kind, th):
    """device_math.hpp's tet_energy_grad -- the ONE dispatch from (grp, type) to a stretch model under energy() and forces() -- compiled for
    the host, at the stretches of the ten families of family_F() (rest, equal, nearly equal, one inverted, equal and inverted, scaled ...),
    taken as they are built (no SVD in between): psi against test_energy_monitor.tet_energies at F = diag(s), s_i g_i against
    test_forces.stretch_gradient and against density2 (through tangent_coefs), the numpy functions the GPU parity tests trust.  Both sides
    are float64 evaluations of the same formulas, so they differ by a few ulp of the value (the order of the sums, fma on one side).

    Measured (host build), the worst relative deviation (E_MEASURED's units) over the ten families, value / gradient: linear 1.5e-16 / 0,
    Neo-Hookean 5.2e-16 / 3.0e-16, StVK 4.0e-16 / 2.1e-16, the kappa splines 1.0e-15 / 6.9e-16 (all three at the 1e+-3-scaled family),
    stable Neo-Hookean 4.3e-16 / 2.2e-16, the tabulated spline 4.2e-15 / 4.4e-15 (the nearly equal families: both sides call the same
    table evaluator, the sums around it differ).  Every kind is three decades under 1e-12; at rest and rotated rest both are 0 or below 1e-17."""
    _, S, _ = family_F()
    tab = kind_description(1, kind)[2] if kind == pkg.TET_SPLINE_TABLE else None
    kappa = KAPPA if pkg.TET_SPLINE_NH <= kind <= pkg.TET_SPLINE_COROTATED else 0.0
    grp, typ = model_args(kind)
    fgh, dfgh = table_fgh(tab) if tab is not None else (None, None)
    ntab = NpTable(tab) if tab is not None else None
    one = np.ones(1)
    worst_psi, worst_sg = [], []
    for f, name in enumerate(FAMILIES):
        psi, sg = host_energy_grad(th, grp, typ, MU, LA, KK, kappa, tab, S[f])
        e_psi = e_sg = 0.0
        for i in range(N_FAM):
            s = S[f][i]
            floor = KK * max(1.0, float(np.sum(s * s)))
            ref_psi = tet_energies(np.diag(s)[None], one, [kind], MU * one, LA * one, KK * one, kappa * one, fgh)[0][0]
            ref_a = stretch_gradient(s, kind, MU, LA, KK, kappa, dfgh)
            ref_b = np.array(tangent_coefs([float(v) for v in s], kind, MU, LA, KK, kappa, np.log, ntab, grad_only=True)[0], dtype=np.float64)
            scale = max(floor, np.abs(ref_a).max())
            e_psi = max(e_psi, abs(psi[i] - ref_psi) / max(floor, abs(ref_psi)))
            e_sg = max(e_sg, np.abs(sg[i] - ref_a).max() / scale, np.abs(sg[i] - ref_b).max() / scale)
        worst_psi.append(e_psi); worst_sg.append(e_sg)
    print("kind %d: worst |psi - ref| / max(|ref|, k max(1, |s|^2)) per family: %s" % (kind, " ".join("%.1e" % w for w in worst_psi)))
    print("kind %d: worst |sg - ref| / max(|ref|, k max(1, |s|^2)) per family:  %s  (bar %.1e)" % (kind, " ".join("%.1e" % w for w in worst_sg), E_ASSERT))
    for name, a, b in zip(FAMILIES, worst_psi, worst_sg):
        assert a <= E_ASSERT and b <= E_ASSERT, (kind, name, a, b)


def test_element_tangent_at_rest_is_linear_elasticity(th):
    """At the rest state and a rigidly rotated one (families 2 and 3) dP = R (2 mu eps + lambda tr(eps) I), eps = sym(R^T dF), for NH, StVK,
    the three xu:: splines with kappa = 0 and stable NH (whose remapped Lame pair is built to meet linear elasticity there), and
    dP = k R sym(R^T dF) for the linear kind; to 1e-12 (mu + lambda) |dF|."""
    F, _, dF = family_F()
    for kd in (pkg.TET_LINEAR, pkg.TET_NEOHOOKEAN, pkg.TET_STVK, pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED, pkg.TET_STABLE_NH):
        grp, typ = model_args(kd)
        for f in (1, 2):
            got, _ = host_dP(th, grp, typ, MU, LA, KK, 0.0, None, F[f], dF[f])
            R = F[f][:, None]
            eps = np.transpose(R, (0, 1, 3, 2)) @ dF[f]
            eps = 0.5 * (eps + np.transpose(eps, (0, 1, 3, 2)))
            tr = np.trace(eps, axis1=2, axis2=3)[..., None, None]
            ref = R @ (KK * eps if kd == pkg.TET_LINEAR else 2.0 * MU * eps + LA * tr * np.eye(3))
            err = np.linalg.norm(got - ref, axis=(2, 3)).max()
            tol = 1e-12 * (KK if kd == pkg.TET_LINEAR else MU + LA)
            print("kind %d %s: |dP - closed form| = %.3e (allowed %.3e)" % (kd, FAMILIES[f], err, tol))
            assert err <= tol, (kd, FAMILIES[f], err, tol)


def test_triangle_tangent_on_the_host_against_mp(th):
    """tri_tangent_frame / tri_tangent_apply against the mp difference quotient of Q(F) = F (F^T F)^(-1/2) (Denman-Beavers free: the 2x2
    square root in closed form at 60 digits), generic, at rest, rotated rest, equal stretches and 1e+-3-scaled: |(dF - dQ) - ref| <=
    1e-10 |dF| max(1, 1 / sigma_min) -- dQ's out-of-plane part divides by the stretches."""
    rng = np.random.default_rng(13)
    n = 16
    sets = []
    for name in ("generic", "rest", "rotated rest", "equal", "scaled"):
        s = rng.uniform(0.5, 2.0, (n, 2))
        if "rest" in name: s[:] = 1.0
        if name == "equal": s[:, 1] = s[:, 0]
        if name == "scaled": s *= np.where(np.arange(n) % 2 == 0, 1e3, 1e-3)[:, None]
        U = _rot(rng, n)[:, :, :2]
        if name == "rest":
            U = np.repeat(np.eye(3)[None, :, :2], n, 0)
        a = rng.uniform(0, 2 * np.pi, n)
        V = np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
        sets.append((name, U @ (s[:, :, None] * np.eye(2)) @ np.transpose(V, (0, 2, 1)), s.min(axis=1)))
    for name, F, smin in sets:
        dF = rng.standard_normal((n, 2, 3, 2)); dF /= np.linalg.norm(dF, axis=(2, 3))[..., None, None]
        Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1))); dFc = np.ascontiguousarray(np.transpose(dF, (0, 1, 3, 2)))
        out = np.zeros((n, 2, 2, 3))
        th.hm_tri_tangent(C.c_int(n), C.c_int(2), Fc.ctypes.data_as(dp), dFc.ctypes.data_as(dp), out.ctypes.data_as(dp))
        got = np.transpose(out, (0, 1, 3, 2))
        worst = 0.0
        with mp.workdps(DPS):
            def Q(Fm):
                Cm = Fm.T * Fm
                s = mp.sqrt(mp.det(Cm)); q = mp.sqrt(Cm[0, 0] + Cm[1, 1] + 2 * s)
                return Fm * ((Cm + s * mp.eye(2)) / q) ** -1
            for i in range(n):
                for j in range(2):
                    Fm, dm = _mpm(F[i]), _mpm(dF[i, j])
                    dQ = (Q(Fm + H_MP * dm) - Q(Fm - H_MP * dm)) / (2 * H_MP)
                    ref = dF[i, j] - np.array([[float(dQ[r, c]) for c in range(2)] for r in range(3)])
                    worst = max(worst, np.linalg.norm(got[i, j] - ref) / max(1.0, 1.0 / smin[i]))
        print("triangles %s: worst |(dF - dQ) - ref| / (|dF| max(1, 1 / sigma_min)) = %.3e (bar 1e-10)" % (name, worst))
        assert worst <= 1e-10, (name, worst)


# ---------------------------------------------------------------- GPU (i): parity in block shapes --------------------------------
def _parity(name, s, rest, x, tri_k=None, table=None, k=3, seed=29):
    flat = s.flatten()
    D = _directions(np.random.default_rng(seed), x.shape, k)
    ref, scale = numpy_stiffness(flat, rest, x, D, tri_k, table)
    out = s.stiffness_apply(D, x)
    assert out.shape == ref.shape
    err = np.linalg.norm(out - ref, axis=2) / scale
    print("%s: stiffness parity, %d vertices x %d directions, max |out_v - ref_v| / scale_v = %.3e (bar 1e-9)" % (name, ref.shape[1], k, err.max()))
    assert err.max() <= 1e-9, (np.unravel_index(err.argmax(), err.shape), err.max())
    return out, ref, scale


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("case", ["one_tet", "nh1", "nh3", "mixed5"])
def test_stiffness_parity_block_shapes(case, pushed):
    """The scenes of test_forces.test_force_parity_block_shapes (one tet; a partial wave; a partial block with records cut after 8 corner
    contributions; three kinds with model boundaries inside the numbering), plain and pushed, 3 directions in one call, against leg (b):
    per vertex |out_v - ref_v| <= 1e-9 sum_{i in v} h_i vol_i |Binv_i|_F^2 max_{u in i} |d_u| -- the force test's bar through one more Binv."""
    sc, n = _tet_scene(case)
    s = sc.make_solver()
    x = _one_tet_state(sc.x, pushed) if case == "one_tet" else (pushed_state if pushed else plain_state)(sc.x, n)
    check_state(signed_stretches(tet_F(sc.x, s.flatten()["tet_idx"], x)[0]), pushed)
    _parity(case, s, sc.x, x)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pushed", [False, True])
@pytest.mark.parametrize("kind", SPLINE_KINDS)
def test_stiffness_parity_spline_kinds(kind, pushed):
    """The xu:: splines with kappa != 0, the tabulated spline and stable Neo-Hookean on the 48-tet cube; the bar as above."""
    s, verts = kind_solver(2, kind)
    x = (pushed_state if pushed else plain_state)(verts, 2)
    _parity("kind %d" % kind, s, verts, x, table=s._spline_tables[0] if kind == pkg.TET_SPLINE_TABLE else None)
    s.close()


@pytest.mark.gpu
def test_stiffness_parity_cloth_and_hinges():
    """Triangles (w^2 |rest|_F^2 in the scale) and hinges (stiffness |c|^2) at two perturbed states."""
    sc = cloth_with_hinges(6)
    s = sc.make_solver()
    k = sc.tris[0][2].bulk_modulus()
    for name, x in zip(("cloth a", "cloth b"), cloth_states(sc)):
        _parity(name, s, sc.x, x, tri_k=k)
    s.close()


# ---------------------------------------------------------------- GPU (ii): wave-mixed degenerate layout -------------------------
UNIT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def _layout(which):
    """positions -> (family, element): "pure" = whole waves of one family, "mixed" = every family in every wave"""
    nf = len(FAMILIES)
    if which == "pure":
        return [(f, i) for f in range(nf) for i in range(N_FAM)]
    return [(f, i) for i in range(N_FAM) for f in range(nf)]


def _device_elements(kind, lay):
    """Disjoint unit tets in device order (Binv = I, vol = 1/6: F = the edge matrix), one per (family, element) of the layout; the three
    dF as three directions.  -> dP [10][64][3][3][3] from the corner contributions (vertex m + 1 gets vol dP[:, m])"""
    F, _, dF = family_F()
    order = _layout(lay)
    n = len(order)
    rest = np.tile(UNIT, (n, 1))
    idx = np.arange(4 * n, dtype=np.int32).reshape(n, 4)
    s = Solver()
    s.add_nodes(rest, np.repeat(meshes.lumped_masses_tets(rest, idx), 3))
    s.add_tets(rest, idx, LAME, kind)
    assert s.initialize(Settings(gravity=0.0))
    x = rest.copy(); D = np.zeros((N_DIR, 4 * n, 3))
    for p, (f, i) in enumerate(order):
        for m in range(3):
            x[4 * p + 1 + m] = F[f, i][:, m]
            D[:, 4 * p + 1 + m] = dF[f, i][:, :, m]
    with np.errstate(all="ignore"):
        out = s.stiffness_apply(D, x)
    s.close()
    dP = np.zeros((len(FAMILIES), N_FAM, N_DIR, 3, 3))
    for p, (f, i) in enumerate(order):
        for m in range(3):
            dP[f, i, :, :, m] = 6.0 * out[:, 4 * p + 1 + m]
        assert np.allclose(out[:, 4 * p], -out[:, 4 * p + 1:4 * p + 4].sum(axis=1), rtol=0, atol=1e-12 * np.abs(out[:, 4 * p:4 * p + 4]).max() + 1e-300)
    return dP


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [pkg.TET_NEOHOOKEAN, pkg.TET_STVK, pkg.TET_LINEAR])
def test_stiffness_at_degenerate_and_wave_mixed_inputs(kind):
    """The ten families of leg (a), 64 elements each, as disjoint unit tets in two layouts -- whole waves of one family, and every family
    in every wave (the signed SVD takes wave votes: a lane's sweeps depend on its neighbours).  Per element against leg (a) with the bar
    of the host test (vol = 1/6 and Binv = I carry it through unchanged: dP = 6 x the corner contribution), and the same element in the
    two layouts to <= 1e-13 h_el |dF| (check H of the local-step tests).

    Measured on an MI355X: against leg (a) at most 1.4e-14 (Neo-Hookean), 1.5e-14 (StVK), 1.6e-14 (linear) h_el |dF|, each in the
    one-inverted family in whole waves (<= 2e-15 with every family in every wave); the two layouts agree to <= 1.6e-14, and bit for
    bit in the rest, two-equal, nearly-equal and both equal-and-inverted families."""
    ref, hel = mp_reference(kind, 0.0)
    got = {lay: _device_elements(kind, lay) for lay in ("pure", "mixed")}
    for lay in ("pure", "mixed"):
        err = np.linalg.norm(got[lay] - ref, axis=(3, 4)) / hel[:, :, None]
        worst = err.max(axis=(1, 2))
        print("kind %d %s: worst |dP - ref| / (h_el |dF|) per family: %s  (bar 1e-10)" % (kind, lay, " ".join("%.1e" % w for w in worst)))
        for name, w in zip(FAMILIES, worst):
            assert w <= BAR, (kind, lay, name, w)
    diff = (np.linalg.norm(got["pure"] - got["mixed"], axis=(3, 4)) / hel[:, :, None]).max(axis=(1, 2))
    print("kind %d: the same element in the two layouts, worst per family: %s  (bar 1e-13)" % (kind, " ".join("%.1e" % w for w in diff)))
    assert diff.max() <= 1e-13, (kind, diff)


# ---------------------------------------------------------------- GPU (iii): the derivative of the device's forces ---------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed5", "cloth"])
def test_device_stiffness_is_the_derivative_of_the_device_forces(case):
    """-(forces(x + h d) - forces(x - h d)) / 2h against stiffness_apply(d, x), 4 directions, device against device, h = 1e-4 edge.  Leg
    (b)'s own central difference at that h gives the truncation error delta_ref (both summed over the vertices); asserted per direction:
    delta_dev <= 2 delta_ref + 1e-9 scale, scale = sum_v scale_v of the parity bar -- the protocol of
    test_forces.test_device_forces_are_the_gradient_of_the_device_energy, no free constant."""
    if case == "mixed5":
        sc = scenes.mixed_cube_scene(5); x = plain_state(sc.x, 5); tri_k = None; edge = 0.2
    else:
        sc = cloth_with_hinges(6); x = cloth_states(sc)[0]; tri_k = sc.tris[0][2].bulk_modulus(); edge = 1.0 / 6.0
    s = sc.make_solver()
    flat = s.flatten()
    D = _directions(np.random.default_rng(31), x.shape, 4)
    Kn, scale_v = numpy_stiffness(flat, sc.x, x, D, tri_k)
    Kd = s.stiffness_apply(D, x)
    h = 1e-4 * edge
    for k, d in enumerate(D):
        dev = -(s.forces(x + h * d) - s.forces(x - h * d)) / (2.0 * h)
        ref = -(numpy_forces(flat, sc.x, x + h * d, tri_k)[0] - numpy_forces(flat, sc.x, x - h * d, tri_k)[0]) / (2.0 * h)
        delta_ref = np.linalg.norm(ref - Kn[k], axis=1).sum()
        delta_dev = np.linalg.norm(dev - Kd[k], axis=1).sum()
        scale = scale_v[k].sum()
        print("%s direction %d: device %.6e, truncation in numpy %.6e, 1e-9 scale %.3e" % (case, k, delta_dev, delta_ref, 1e-9 * scale))
        assert delta_dev <= 2.0 * delta_ref + 1e-9 * scale, (delta_dev, delta_ref, scale)
    s.close()


# ---------------------------------------------------------------- GPU (iv): structure -------------------------------------------
def _structure_scene(kind):
    if kind == "cloth":
        sc = cloth_with_hinges(6)
        return sc.make_solver(), sc.x, cloth_states(sc)[1], sc.tris[0][2].bulk_modulus(), None
    s, verts = kind_solver(2, kind)
    return s, verts, pushed_state(verts, 2), None, (s._spline_tables[0] if kind == pkg.TET_SPLINE_TABLE else None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ALL_KINDS + ["cloth"])
def test_stiffness_structure(kind):
    """On the pushed 48-tet cube of every kind and on the cloth; every scale is leg (b)'s (the per-vertex scale of the parity bar), not the
    device's.
      symmetry        |d1 . K d2 - d2 . K d1| <= 1e-12 |d1| |d2| sum_v scale_v
      translation     |K t|_v <= 1e-12 scale_v for a uniform t
      equivariance    K(x) (om x x) = -om x f(x), f from Solver.forces: to 1e-9 scale_v at the pushed state, to 1e-12 scale_v at a rigidly
                      moved rest state, where both sides vanish -- the twist terms exactly
      rest            d . K d >= -1e-12 |d|^2 sum_v scale_v at the rest state, 8 random d
      shift           apply(d, shift=s) - apply(d, shift=0) = s m o d to 1 ulp of the larger term."""
    s, rest, x, tri_k, table = _structure_scene(kind)
    flat = s.flatten()
    nv = len(rest)
    rng = np.random.default_rng(37)
    D = _directions(rng, x.shape, 2)
    one = np.ones((1, nv, 3)) / np.sqrt(3.0)
    scale = numpy_stiffness(flat, rest, x, one, tri_k, table)[1][0] * np.sqrt(3.0)      # per vertex, for |d_u| = 1
    K = s.stiffness_apply(D, x)
    asym = abs(np.sum(D[0] * K[1]) - np.sum(D[1] * K[0]))
    bar = 1e-12 * np.linalg.norm(D[0]) * np.linalg.norm(D[1]) * scale.sum()
    print("%s: |d1 . K d2 - d2 . K d1| = %.3e (allowed %.3e)" % (kind, asym, bar))
    assert asym <= bar
    t = np.tile(np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]), (nv, 1))
    r = np.linalg.norm(s.stiffness_apply(t, x), axis=1) / scale
    print("%s: translation, max |K t|_v / scale_v = %.3e (allowed 1e-12)" % (kind, r.max()))
    assert r.max() <= 1e-12
    om = np.array([0.4, -0.7, 0.59])
    for name, y, tol in (("pushed", x, 1e-9), ("rigid rest", rigid(rest), 1e-12)):
        sc_y = numpy_stiffness(flat, rest, y, one, tri_k, table)[1][0] * np.sqrt(3.0)
        d = np.cross(om, y)
        lhs = s.stiffness_apply(d, y); rhs = -np.cross(om, s.forces(y))
        r = np.linalg.norm(lhs - rhs, axis=1) / (sc_y * np.linalg.norm(d, axis=1).max())
        print("%s %s: equivariance, max |K (om x x) + om x f|_v / scale_v = %.3e (allowed %.0e)" % (kind, name, r.max(), tol))
        assert r.max() <= tol, (name, r.max())
    sc_r = numpy_stiffness(flat, rest, rest, one, tri_k, table)[1][0] * np.sqrt(3.0)
    D8 = _directions(rng, x.shape, 8)
    K8 = s.stiffness_apply(D8, rest)
    for d, kd in zip(D8, K8):
        q = np.sum(d * kd)
        assert q >= -1e-12 * sc_r.sum(), (kind, q, sc_r.sum())
    print("%s: d . K d at rest, smallest %.3e" % (kind, min(np.sum(d * kd) for d, kd in zip(D8, K8))))
    sh = 576.0
    m = np.asarray(s.m_masses, dtype=np.float64).reshape(nv, 3)
    a0 = s.stiffness_apply(D[0], x); a1 = s.stiffness_apply(D[0], x, shift=sh)
    LD = np.longdouble
    want = LD(sh * m) * LD(D[0])
    resid = np.abs((LD(a1) - LD(a0)) - want).astype(np.float64)
    ulp = np.spacing(np.maximum(np.maximum(np.abs(a0), np.abs(a1)), np.abs(want).astype(np.float64)))
    print("%s: shift, max residual / ulp of the larger term = %.3f" % (kind, (resid / ulp).max()))
    assert (resid <= ulp).all()
    s.close()


# ---------------------------------------------------------------- GPU (v): housekeeping -----------------------------------------
@pytest.mark.gpu
def test_stiffness_housekeeping():
    """Columns of an n_vec = 3 call are bit-identical to three single calls; two identical calls are bit-identical; x = None after
    set_state equals passing that x; the error codes; a scene without tets and one without triangles; a closed context leaves no
    device buffer behind."""
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    L = capi.lib()
    for sc, n in ((scenes.mixed_cube_scene(5, admm_iters=3), 5), (cloth_with_hinges(6, admm_iters=3), 1)):      # no triangles / no tets
        s = sc.make_solver()
        x = plain_state(sc.x, n)
        D = _directions(np.random.default_rng(41), x.shape, 3)
        a = s.stiffness_apply(D, x, shift=3.0)
        assert np.array_equal(a, s.stiffness_apply(D, x, shift=3.0)) and np.abs(a).max() > 0.0 and np.isfinite(a).all()
        for j in range(3):
            single = s.stiffness_apply(D[j], x, shift=3.0)
            assert single.shape == x.shape and np.array_equal(single, a[j]), j
        s.step()
        assert np.array_equal(s.stiffness_apply(D), s.stiffness_apply(D, s.m_x))
        out = np.zeros(D.size); dd = np.ascontiguousarray(D).ravel()
        assert L.admm_hip_stiffness_apply(s._ctx, None, 0, capi.dptr(dd), 0.0, capi.dptr(out)) == ERR_ARG
        assert L.admm_hip_stiffness_apply(s._ctx, None, 1, None, 0.0, capi.dptr(out)) == ERR_ARG
        assert L.admm_hip_stiffness_apply(s._ctx, None, 1, capi.dptr(dd), 0.0, None) == ERR_ARG
        with pytest.raises(ValueError):
            s.stiffness_apply(D[:, :-1], x)
        s.close()
    sc = scenes.cube_scene(3, pkg.TET_NEOHOOKEAN)
    s = sc.make_solver()      # (initialize() uploads no state)
    with pytest.raises(pkg.AdmmHipError) as ei:
        s.stiffness_apply(np.zeros_like(sc.x))
    assert ei.value.code == ERR_STATE
    s.upload()
    D = _directions(np.random.default_rng(47), sc.x.shape, 1)
    assert np.array_equal(s.stiffness_apply(D), s.stiffness_apply(D, sc.x))
    s.close()
    s2 = sc.make_solver(world_size=2, rank=0)
    with pytest.raises(pkg.AdmmHipError) as ei:
        s2.stiffness_apply(np.zeros_like(sc.x), sc.x)
    assert ei.value.code in (ERR_ARG, ERR_STATE)      # mon_refuse: as forces() on a multi-rank context
    s2.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)


@pytest.mark.gpu
def test_stiffness_does_not_disturb_a_step():
    """linsolver 1 (bit-reproducible): two steps with stiffness_apply calls before and between them equal two steps without, bit for
    bit -- the feature touches no step state but the scratch `curr` between steps, as forces() does."""
    sc = scenes.cube_scene(5, pkg.TET_NEOHOOKEAN, linsolver=1)
    out = []
    for call in (False, True):
        s = sc.make_solver()
        D = _directions(np.random.default_rng(43), sc.x.shape, 2)
        for frame in range(2):
            if call:
                s.stiffness_apply(D, plain_state(sc.x, 5))
                if frame:
                    s.stiffness_apply(D[0], shift=576.0)      # the device-resident state of the first step
            s.step()
        out.append((s.m_x.copy(), s.m_v.copy()))
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- GPU (vi): C++ -------------------------------------------------
@pytest.mark.gpu
def test_cpp_stiffness_apply():
    """tests/cpp/test_stiffness.cpp: Solver::stiffness_apply on the 48-tet Neo-Hookean cube equals admm_hip_stiffness_apply bit for bit
    and is symmetric (|d1 . K d2 - d2 . K d1| <= 1e-12 |d1| |d2| sum |K| scale)."""
    exe = _build_exe("test_stiffness")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
