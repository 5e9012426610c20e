"""The positive semi-definite projection of the per-element tangent (device_math.hpp: tet_tangent_psd, tri_tangent_apply_psd), compiled for
the host and held against numpy: the 9x9 (tets) / 6x6 (triangles) operator dP/dF of every element is assembled from the UNPROJECTED host
apply, numpy.linalg.eigh clamps its eigenvalues at 0, and the projected apply must reproduce that matrix.

  entries          |K_psd - clamp(K)|_ij <= 1e-10 h_el (h_el = the largest coefficient of the element, DESIGN.md 4i: the project's
                   per-element bar)
  semi-definite    lambda_min(K_psd) >= -1e-12 h_el
  untouched        at rest and rotated rest the projected coefficients are the unprojected ones, bit for bit

The ten element families of test_stiffness.py and two compressed ones (every stretch in [0.3, 0.8]; the same with one stretch inverted),
64 elements each, all eight kinds.  The test asserts of its own inputs that at least half the elements of the two compressed families are
indefinite by more than 1e-3 h_el before the projection: the check would be empty otherwise."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
from test_device_math_host import _rot
from test_forces import ALL_KINDS, kind_description
from test_stiffness import FAMILIES, KAPPA, KK, LA, MU, N_FAM, family_F, model_args

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
NEW_FAMILIES = ("compressed", "compressed, one inverted")


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    """tests/hostmath/tangent_psd_host.cpp compiled with g++, as test_stiffness.py compiles tangent_host.cpp"""
    out = os.path.join(str(tmp_path_factory.mktemp("tangent_psd_host")), "libtangent_psd_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "tangent_psd_host.cpp")])
    return C.CDLL(out)


@functools.lru_cache(None)
def all_F():
    """[12][64][3][3]: the ten families of test_stiffness.family_F and the two compressed ones"""
    F10 = family_F()[0]
    rng = np.random.default_rng(17)
    n = N_FAM
    extra = []
    for inverted in (False, True):
        S = rng.uniform(0.3, 0.8, (n, 3))
        if inverted:
            S[:, 2] = -S[:, 2]
        extra.append(_rot(rng, n) @ (S[:, :, None] * np.eye(3)) @ np.transpose(_rot(rng, n), (0, 2, 1)))
    return np.concatenate([F10, np.stack(extra)]), FAMILIES + NEW_FAMILIES


def tet_operator(L, psd, grp, typ, kappa, tab, F):
    """-> K [n][9][9] (column j = vec of dP for the unit dF e_j, both column-major), the coefficients as applied and before the
    projection [n][12] (both from the SVD of this call: the host build of signed_svd3 is not bit-reproducible from call to call)"""
    n = len(F)
    Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1)))
    dF = np.ascontiguousarray(np.tile(np.eye(9)[None], (n, 1, 1)))
    dP = np.zeros((n, 9, 9)); coef = np.zeros((n, 12)); raw = np.zeros((n, 12))
    L.hm_tet_tangent_psd(C.c_int(n), C.c_int(9), C.c_int(psd), C.c_int(grp), C.c_int(typ), C.c_double(MU), C.c_double(LA), C.c_double(KK),
                         C.c_double(kappa), None if tab is None else tab.ctypes.data_as(dp), Fc.ctypes.data_as(dp), dF.ctypes.data_as(dp),
                         dP.ctypes.data_as(dp), coef.ctypes.data_as(dp), raw.ctypes.data_as(dp))
    return np.transpose(dP, (0, 2, 1)), coef, raw


def clamp(K):
    K = 0.5 * (K + np.transpose(K, (0, 2, 1)))
    w, V = np.linalg.eigh(K)
    return (V * np.maximum(w, 0.0)[:, None, :]) @ np.transpose(V, (0, 2, 1)), w[:, 0]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_projected_tet_tangent_against_eigh(kind, ph):
    """Measured (host build), worst over the twelve families: |K_psd - clamp(K)| <= 4e-15 h_el for the seven closed-form kinds and the
    tabulated spline alike (the reference is the host's own operator, so the table's representation error cancels), lambda_min >=
    -3e-16 h_el; indefinite by more than 1e-3 h_el before the projection: 64 of 64 elements in both compressed families for every kind."""
    F, names = all_F()
    tab = kind_description(1, kind)[2] if kind == pkg.TET_SPLINE_TABLE else None
    kappa = KAPPA if pkg.TET_SPLINE_NH <= kind <= pkg.TET_SPLINE_COROTATED else 0.0
    grp, typ = model_args(kind)
    for f, name in enumerate(names):
        K0, c0, _ = tet_operator(ph, 0, grp, typ, kappa, tab, F[f])
        K1, c1, raw = tet_operator(ph, 1, grp, typ, kappa, tab, F[f])
        hel = np.abs(c0).max(axis=1)
        asym = np.abs(K0 - np.transpose(K0, (0, 2, 1))).max(axis=(1, 2)) / hel
        ref, lmin0 = clamp(K0)
        err = np.abs(K1 - ref).max(axis=(1, 2)) / hel
        lmin1 = np.linalg.eigvalsh(0.5 * (K1 + np.transpose(K1, (0, 2, 1))))[:, 0] / hel
        indefinite = int((lmin0 < -1e-3 * hel).sum())
        print("kind %d %-26s |K_psd - clamp(K)| / h_el = %.1e, lambda_min(K_psd) / h_el = %.1e, asymmetry of K %.1e, indefinite before: %d of %d"
              % (kind, name, err.max(), lmin1.min(), asym.max(), indefinite, len(hel)))
        if name in NEW_FAMILIES:
            assert 2 * indefinite >= len(hel), (kind, name, indefinite)      # the input condition
        assert err.max() <= 1e-10, (kind, name, err.max())
        assert lmin1.min() >= -1e-12, (kind, name, lmin1.min())
        if name in ("rest", "rotated rest"):
            print("        lowest raw coefficient / h_el = %.1e" % (raw / hel[:, None]).min())
            assert raw.tobytes() == c1.tobytes(), (kind, name, np.abs(raw - c1).max())


def _tri_F(rng, n, s):
    U = _rot(rng, n)[:, :, :2]
    a = rng.uniform(0, 2 * np.pi, n)
    V = np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
    return U @ (s[:, :, None] * np.eye(2)) @ np.transpose(V, (0, 2, 1))


def tri_operator(L, psd, F):
    n = len(F)
    Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1)))
    dF = np.ascontiguousarray(np.tile(np.eye(6)[None], (n, 1, 1)))
    out = np.zeros((n, 6, 6)); frame = np.zeros((n, 4)); raw = np.zeros((n, 4))
    L.hm_tri_tangent_psd(C.c_int(n), C.c_int(6), C.c_int(psd), Fc.ctypes.data_as(dp), dF.ctypes.data_as(dp), out.ctypes.data_as(dp),
                         frame.ctypes.data_as(dp), raw.ctypes.data_as(dp))
    return np.transpose(out, (0, 2, 1)), frame, raw


def test_projected_triangle_tangent_against_eigh(ph):
    """The 6x6 operator I - dQ/dF of the families of test_stiffness.test_triangle_tangent_on_the_host_against_mp and of two compressed
    ones: sigma_1 + sigma_2 < 2 (a negative twist eigenvalue) with both sigma_i < 1 (two negative out-of-plane eigenvalues), and one
    stretch on each side of 1 (one negative out-of-plane eigenvalue: the 2x2 block is projected, not zeroed).  h_el = max(1, 1 / sigma_min),
    the scale of that test.  Measured: <= 2e-15 h_el against eigh, lambda_min >= -2e-16 h_el; every compressed triangle indefinite by
    more than 1e-3 h_el before."""
    rng = np.random.default_rng(19)
    n = 64
    sets = []
    for name in ("generic", "rest", "rotated rest", "equal", "scaled", "compressed", "one stretch below 1"):
        s = rng.uniform(0.5, 2.0, (n, 2))
        if "rest" in name: s[:] = 1.0
        if name == "equal": s[:, 1] = s[:, 0]
        if name == "scaled": s *= np.where(np.arange(n) % 2 == 0, 1e3, 1e-3)[:, None]
        if name == "compressed": s = rng.uniform(0.3, 0.8, (n, 2))
        if name == "one stretch below 1": s = np.stack([rng.uniform(0.3, 0.8, n), rng.uniform(1.3, 2.0, n)], 1)
        F = _tri_F(rng, n, s)
        if name == "rest":
            F = np.repeat(np.eye(3)[None, :, :2], n, 0)
        sets.append((name, F, np.maximum(1.0, 1.0 / s.min(axis=1))))
    for name, F, hel in sets:
        K0, _, _ = tri_operator(ph, 0, F)
        K1, f1, f0 = tri_operator(ph, 1, F)
        ref, lmin0 = clamp(K0)
        err = np.abs(K1 - ref).max(axis=(1, 2)) / hel
        lmin1 = np.linalg.eigvalsh(0.5 * (K1 + np.transpose(K1, (0, 2, 1))))[:, 0] / hel
        indefinite = int((lmin0 < -1e-3 * hel).sum())
        print("triangles %-20s |K_psd - clamp(K)| / h_el = %.1e, lambda_min(K_psd) / h_el = %.1e, indefinite before: %d of %d"
              % (name, err.max(), lmin1.min(), indefinite, n))
        if name in ("compressed", "one stretch below 1"):
            assert 2 * indefinite >= n, (name, indefinite)
        assert err.max() <= 1e-10, (name, err.max())
        assert lmin1.min() >= -1e-12, (name, lmin1.min())
        if name in ("rest", "rotated rest"):
            assert f0.tobytes() == f1.tobytes(), (name, np.abs(f0 - f1).max())
