"""The per-element rest-shape derivative under rest_sensitivity() (device_math.hpp: tet_rest_grad), compiled for the host: for a tet with
the rest edge matrix Dm (Binv = Dm^-1, vol = det Dm / 6), F = Ds(x) Binv, A = Ds(a) Binv, P = dpsi/dF and T = H[A],
    d(-vol P : A)/dDm = Gs Binv^T,    Gs = -vol [ (P : A) I - F^T T - A^T P ],
for all eight kinds over the ten element families of test_stiffness.family_F (64 elements each, 3 multipliers A of unit size each).

  algebra     tet_rest_grad against the same 3x3 algebra in numpy from the host's own P (U diag(sg) V^T of tet_energy_grad) and
              T (tet_tangent_apply).  A rounding bar: 1e-12 vol (|P : A| + |F| |T| + |A| |P|); at rest and rotated rest, where P is what
              rounding leaves, the magnitude carries the floor k max(1, |s|^2) |A| of test_adjoint_host.py.
  derivative  Gs Binv^T against central differences of the host's own s = -vol P : A in the nine entries of Dm (Ds(x), Ds(a) fixed;
              Dm = I + 0.2 N, N standard normal, det Dm > 0).  Steps 4e-3 2^-i, i = 0..3: the largest h = 4e-3 2^-i, i >= 1, at which
              the quotient changes less from h to h / 2 than from 2h to h (or has stopped changing: both changes below 1e-10 of the
              magnitude, the quotient of a function whose third derivative vanishes there); asserted
              |value - q(h / 2)| <= 4 |q(h) - q(h / 2)| + 1e-9 magnitude |Binv|_F.
              NO FAMILY IS LEFT OUT: a step would have to cross sigma_i = 0 or a flip, and the inverted families keep |sigma_3| >= 0.1
              against relative steps of 4e-3; where two stretches are equal in size (equal, nearly equal, equal and inverted) every
              density is a symmetric smooth function of the singular values of F (of sigma^2 and J for StVK and stable Neo-Hookean), so
              -vol P : A is smooth in Dm there and the quotient converges.
  rest state  at F = I (the family "rest"): Gs = vol T to the rounding bar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
from test_forces import ALL_KINDS, kind_description
from test_stiffness import FAMILIES, KAPPA, KK, LA, MU, family_F, model_args

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
BAR = 1e-12
WITH_KAPPA = (pkg.TET_SPLINE_NH, pkg.TET_SPLINE_STVK, pkg.TET_SPLINE_COROTATED)
H0, N_LADDER = 4e-3, 4


@pytest.fixture(scope="module")
def rs(tmp_path_factory):
    """tests/hostmath/rest_sens_host.cpp compiled with g++, as test_adjoint_host.py compiles param_sens_host.cpp"""
    out = os.path.join(str(tmp_path_factory.mktemp("rest_sens_host")), "librest_sens_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "rest_sens_host.cpp")])
    return C.CDLL(out)


def host_rest_grad(L, grp, typ, mu, la, k, kappa, tab, F, A, vol):
    """hm_tet_rest_grad: F [n, 3, 3], A [n, nd, 3, 3], vol [n] -> S [n, 3], P [n, 3, 3], T, Gs [n, nd, 3, 3], s [n, nd]"""
    n, nd = len(F), A.shape[1]
    Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1))); Ac = np.ascontiguousarray(np.transpose(A, (0, 1, 3, 2)))
    vc = np.ascontiguousarray(vol, dtype=np.float64)
    S = np.zeros((n, 3)); P = np.zeros((n, 3, 3)); T = np.zeros((n, nd, 3, 3)); Gs = np.zeros((n, nd, 3, 3)); s = np.zeros((n, nd))
    L.hm_tet_rest_grad(C.c_int(n), C.c_int(nd), C.c_int(grp), C.c_int(typ), C.c_double(mu), C.c_double(la), C.c_double(k), C.c_double(kappa),
                       None if tab is None else tab.ctypes.data_as(dp), Fc.ctypes.data_as(dp), Ac.ctypes.data_as(dp), vc.ctypes.data_as(dp),
                       S.ctypes.data_as(dp), P.ctypes.data_as(dp), T.ctypes.data_as(dp), Gs.ctypes.data_as(dp), s.ctypes.data_as(dp))
    return S, np.transpose(P, (0, 2, 1)), np.transpose(T, (0, 1, 3, 2)), np.transpose(Gs, (0, 1, 3, 2)), s


def numpy_Gs(F, A, P, T, vol):
    """-vol [(P : A) I - F^T T - A^T P] per element and multiplier, and the magnitude |P : A| + |F| |T| + |A| |P| (times vol)"""
    pa = np.einsum("nij,ndij->nd", P, A)
    Ft = np.transpose(F, (0, 2, 1))[:, None]
    At = np.transpose(A, (0, 1, 3, 2))
    G = -vol[:, None, None, None] * (pa[..., None, None] * np.eye(3) - Ft @ T - At @ P[:, None])
    fro = lambda M: np.linalg.norm(M, axis=(-2, -1))
    mag = vol[:, None] * (np.abs(pa) + fro(F)[:, None] * fro(T) + fro(A) * fro(P)[:, None])
    return G, mag


def rest_matrices(n):
    rng = np.random.default_rng(83)
    Dm = np.eye(3)[None] + 0.2 * rng.standard_normal((n, 3, 3))
    assert (np.linalg.det(Dm) > 0.1).all()
    return Dm


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_rest_gradient_on_the_host(kind, rs):
    """Measured (host build, g++ -O2), the worst ratio to the bar over the ten families and the eight kinds: algebra 1.4e-2 (1.4e-14 of
    the magnitude; exactly 0 at rest), rest state 7.3e-3 (stable Neo-Hookean; the closed-form kinds exactly 0), derivative 8.3e-2 = 1 / 12
    in every family and kind alike -- the error of a central difference at h / 2 is (q(h) - q(h / 2)) / 3, which is where the value
    stands: the quotient's own error, none of the formula's.  (Against the additive term alone the distance is up to 1.4e4: the
    quotients stand 1.4e-5 of the magnitude off the value at these steps.)  Every element took the first step of the ladder."""
    F_all, _, dF_all = family_F()
    tab = kind_description(1, kind)[2] if kind == pkg.TET_SPLINE_TABLE else None
    kappa = KAPPA if kind in WITH_KAPPA else 0.0
    grp, typ = model_args(kind)
    args = (rs, grp, typ, MU, LA, KK, kappa, tab)
    n = F_all.shape[1]
    Dm0 = rest_matrices(n)
    B0 = np.linalg.inv(Dm0)
    vol0 = np.linalg.det(Dm0) / 6.0
    worst_a, worst_d, worst_r, worst_add = [], [], [], []
    for f, name in enumerate(FAMILIES):
        F, A = F_all[f], dF_all[f]
        # ---- algebra
        S, P, T, Gs, _ = host_rest_grad(*args, F, A, vol0)
        G_np, mag = numpy_Gs(F, A, P, T, vol0)
        if name in ("rest", "rotated rest"):
            mag = mag + (vol0 * KK * np.maximum(1.0, np.sum(S * S, axis=1)))[:, None] * np.linalg.norm(A, axis=(2, 3))
        ra = (np.abs(Gs - G_np).max(axis=(2, 3)) / (BAR * mag)).max()
        worst_a.append(ra)
        # ---- rest state
        if name == "rest":
            worst_r.append((np.abs(Gs - vol0[:, None, None, None] * T).max(axis=(2, 3)) / (BAR * mag)).max())
        # ---- derivative: Ds(x) = F Dm0 and Ds(a) = A Dm0 fixed, Dm moves
        Dsx, Dsa = F @ Dm0, A @ Dm0[:, None]
        Fb, Ab = Dsx @ B0, Dsa @ B0[:, None]
        _, Pb, Tb, Gb, _ = host_rest_grad(*args, Fb, Ab, vol0)
        value = Gb @ np.transpose(B0, (0, 2, 1))[:, None]                      # [n, nd, 3, 3]: d s / d Dm(j, k)
        magd = numpy_Gs(Fb, Ab, Pb, Tb, vol0)[1] * np.linalg.norm(B0, axis=(1, 2))[:, None]
        q = np.zeros((N_LADDER,) + value.shape)
        for i in range(N_LADDER):
            h = H0 * 0.5 ** i
            for j in range(3):
                for k in range(3):
                    sv = []
                    for sign in (1.0, -1.0):
                        Dm = Dm0.copy(); Dm[:, j, k] += sign * h
                        B = np.linalg.inv(Dm)
                        sv.append(host_rest_grad(*args, Dsx @ B, Dsa @ B[:, None], np.linalg.det(Dm) / 6.0)[4])
                    q[i, :, :, j, k] = (sv[0] - sv[1]) / (2.0 * h)
        m4 = magd[..., None, None]
        err = np.full(value.shape, np.inf); chosen = np.zeros(value.shape, bool); add = np.zeros(value.shape)
        for i in range(1, N_LADDER - 1):
            d_prev, d_next = np.abs(q[i - 1] - q[i]), np.abs(q[i] - q[i + 1])
            ok = ~chosen & ((d_next < d_prev) | ((d_prev <= 1e-10 * m4) & (d_next <= 1e-10 * m4)))
            bar = 4.0 * d_next + 1e-9 * m4
            err = np.where(ok, np.abs(value - q[i + 1]) / bar, err)
            add = np.where(ok, np.abs(value - q[i + 1]) / (1e-9 * m4), add)
            chosen |= ok
        assert chosen.all(), (kind, name, "no step of the ladder at which the quotient converges", int((~chosen).sum()))
        worst_d.append(err.max()); worst_add.append(add.max())
    print("kind %d: algebra, worst |Gs - numpy| / bar per family:      %s" % (kind, " ".join("%.1e" % w for w in worst_a)))
    print("kind %d: derivative, worst |value - q| / bar per family:    %s" % (kind, " ".join("%.1e" % w for w in worst_d)))
    print("kind %d: derivative, |value - q| / (1e-9 magnitude) alone:  %s" % (kind, " ".join("%.1e" % w for w in worst_add)))
    print("kind %d: rest state, worst |Gs - vol T| / bar:              %s" % (kind, " ".join("%.1e" % w for w in worst_r)))
    for name, a, d in zip(FAMILIES, worst_a, worst_d):
        assert a <= 1.0 and d <= 1.0, (kind, name, a, d)
    assert worst_r and worst_r[0] <= 1.0, (kind, worst_r)


def test_symbols_and_signatures():
    """the two entry points are declared, bound and documented on every face"""
    from admm_elastic_amd import capi
    from admm_elastic_amd.solver import Solver
    names = [s[0] for s in capi.SYMBOLS]
    assert "admm_hip_rest_sensitivity" in names and "admm_hip_adjoint_held" in names
    root = os.path.dirname(HERE)
    with open(os.path.join(root, "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    assert "int admm_hip_rest_sensitivity(" in hdr and "int admm_hip_adjoint_held(" in hdr
    assert "admm_hip_rest_sensitivity" in Solver.rest_sensitivity.__doc__ and "admm_hip_adjoint_held" in Solver.step_adjoint.__doc__
    with open(os.path.join(root, "admm-elastic_amd", "host", "include", "Solver.hpp")) as fh:
        hpp = fh.read()
    assert "rest_sensitivity(" in hpp and "adjoint_held(" in hpp
