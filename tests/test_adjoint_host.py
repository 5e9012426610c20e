"""The per-element parameter derivative under param_sensitivity() and step_adjoint() (device_math.hpp: tet_param_grad), compiled for the
host: d(s o g)/d theta, theta = (mu, la, kappa) as a tet's Mat stores them, for all eight kinds over the ten element families of
test_stiffness.family_F (64 elements each, through the host's signed SVD).

  reference     central differences in theta of the host's own tet_energy_grad at the same stretches, steps of theta / 2 (1 where the
                kind's theta is 0).  s o g is linear in theta, so the quotient is exact up to rounding.
  bar           |d sg / d theta_p - quotient| <= 1e-12 unit / |theta_p|, a rounding bar: a kind that misses it is not linear as claimed.
  identity      |mu d_mu + la d_la + kappa d_kappa - sg| <= 1e-12 (|mu d_mu| + |la d_la| + |kappa d_kappa| + |sg|) for the six
                kinds with device parameters
  parameterless the three columns of the linear tet and the tabulated spline are exactly 0, as is the kappa column of every kind that
                does not read kappa

unit = max_i |sg_i| of the element, as the issue of this feature states the bar -- in eight of the ten families.  At rest and rotated rest
s o g vanishes while its terms do not (stable Neo-Hookean at unit mu: mu_s s (1 - q) = 1 against la_s (J - alpha) dJ = -1), so what is
left of s o g there is the rounding of those terms, 1e-16 k or exactly 0, and 1e-12 of THAT is 1e-28 k or 0: no float64 evaluation of the
terms meets it, linear or not.  In those two families the unit is max(max_i |sg_i|, k max(1, |s|^2)), the floor
test_stiffness.test_element_energy_and_gradient_on_the_host uses where the value cancels, and the identity's magnitudes carry the same
floor."""
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
PARAMETERLESS = (pkg.TET_LINEAR, pkg.TET_SPLINE_TABLE)


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    """tests/hostmath/param_sens_host.cpp compiled with g++, as test_newton_host.py compiles tangent_psd_host.cpp"""
    out = os.path.join(str(tmp_path_factory.mktemp("param_sens_host")), "libparam_sens_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "param_sens_host.cpp")])
    return C.CDLL(out)


def host_param_grad(L, grp, typ, mu, la, k, kappa, tab, F, h):
    """hm_tet_param_grad: F [n, 3, 3] -> S [n, 3], sg [n, 3], dsg [n, 3, 3] (parameter, stretch), the quotients [n, 3, 3]"""
    n = len(F)
    Fc = np.ascontiguousarray(np.transpose(F, (0, 2, 1)))
    hc = np.ascontiguousarray(h, dtype=np.float64)
    S = np.zeros((n, 3)); sg = np.zeros((n, 3)); dsg = np.zeros((n, 3, 3)); fd = np.zeros((n, 3, 3))
    L.hm_tet_param_grad(C.c_int(n), C.c_int(grp), C.c_int(typ), C.c_double(mu), C.c_double(la), C.c_double(k), C.c_double(kappa),
                        None if tab is None else tab.ctypes.data_as(dp), Fc.ctypes.data_as(dp), hc.ctypes.data_as(dp), S.ctypes.data_as(dp),
                        sg.ctypes.data_as(dp), dsg.ctypes.data_as(dp), fd.ctypes.data_as(dp))
    return S, sg, dsg, fd


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_parameter_derivative_against_central_differences(kind, ps):
    """Measured (host build, g++ -O2), the worst |d sg / d theta - quotient| |theta| / unit and the worst identity defect over the ten
    families: Neo-Hookean 5.3e-16 / 1.5e-16, StVK 4.6e-16 / 1.7e-16, the kappa splines 6.5e-16 / 2.1e-16, stable Neo-Hookean 6.0e-16 /
    4.4e-16 (rest and rotated rest, in the floored unit: <= 4.2e-17, Neo-Hookean and StVK at rest exactly 0); the linear tet and the
    tabulated spline: every column exactly 0."""
    F = family_F()[0]
    tab = kind_description(1, kind)[2] if kind == pkg.TET_SPLINE_TABLE else None
    kappa = KAPPA if kind in WITH_KAPPA else 0.0
    theta = np.array([MU, LA, kappa])
    h = np.where(theta != 0.0, 0.5 * theta, 1.0)
    grp, typ = model_args(kind)
    worst_d, worst_i = [], []
    for f, name in enumerate(FAMILIES):
        S, sg, dsg, fd = host_param_grad(ps, grp, typ, MU, LA, KK, kappa, tab, F[f], h)
        floor = KK * np.maximum(1.0, np.sum(S * S, axis=1))
        at_rest = name in ("rest", "rotated rest")
        unit = np.maximum(np.abs(sg).max(axis=1), floor) if at_rest else np.abs(sg).max(axis=1)
        if kind in PARAMETERLESS:
            assert not dsg.any(), (kind, name)
            assert (np.abs(fd).max(axis=(1, 2)) <= BAR * np.maximum(unit, floor)).all(), (kind, name)      # (two inlined copies of one evaluation: rounding apart)
            worst_d.append(0.0); worst_i.append(0.0)
            continue
        if kind not in WITH_KAPPA:
            assert not dsg[:, 2].any(), (kind, name)
        e = 0.0
        for p in range(3):      # (a theta of 0, the kappa of a kind that reads none: the step, 1, stands for |theta|)
            e = max(e, (np.abs(dsg[:, p] - fd[:, p]).max(axis=1) * (abs(theta[p]) if theta[p] != 0.0 else 1.0) / unit).max())
        terms = theta[None, :, None] * dsg
        defect = np.abs(terms.sum(axis=1) - sg).max(axis=1)
        mag = (np.abs(terms).sum(axis=1) + np.abs(sg)).max(axis=1) + (floor if at_rest else 0.0)
        worst_d.append(e); worst_i.append((defect / mag).max())
    print("kind %d: worst |d sg/d theta - quotient| |theta| / unit per family: %s" % (kind, " ".join("%.1e" % w for w in worst_d)))
    print("kind %d: worst identity defect / magnitudes per family:            %s  (bar %.0e)" % (kind, " ".join("%.1e" % w for w in worst_i), BAR))
    for name, a, b in zip(FAMILIES, worst_d, worst_i):
        assert a <= BAR and b <= BAR, (kind, name, a, b)


def test_symbols_and_signatures():
    """the two entry points are declared, bound and documented on every face"""
    from admm_elastic_amd import capi
    from admm_elastic_amd.solver import Solver
    names = [s[0] for s in capi.SYMBOLS]
    assert "admm_hip_param_sensitivity" in names and "admm_hip_step_adjoint" in names
    root = os.path.dirname(HERE)
    with open(os.path.join(root, "include", "admm_hip.h")) as fh:
        hdr = fh.read()
    assert "int admm_hip_param_sensitivity(" in hdr and "int admm_hip_step_adjoint(" in hdr
    for fn in (Solver.param_sensitivity, Solver.step_adjoint):
        assert "admm_hip_" in fn.__doc__
