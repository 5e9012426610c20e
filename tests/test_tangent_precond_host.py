"""The host side of the two-level tangent preconditioner (csrc/tangent_precond.hpp), no GPU:

  the inverse    device_math.hpp: tc_invert, the routine k_tc_invert runs, compiled for the host (tests/hostmath/tc_invert_host.cpp: one
                 thread, an empty barrier -- the device's arithmetic) against numpy.  SPD matrices with CONSTRUCTED condition numbers
                 (Q diag(logspace) Q^T, Q from a QR of a seeded Gaussian): |X A - I|_max <= 64 n eps cond -- the backward error of
                 Cholesky is c n eps |A|, so the residual of the inverse is c n eps cond; 64 covers c and the n eps cond of numpy's own
                 product X A.  Dropped columns, and the two ways a matrix is "not positive definite".
  the plan       admm_host_tangent_plan (oc_plan.cpp: tangent_plan): recursive coordinate bisection."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Solver

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def tc(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("tc_invert_host")), "libtc_invert_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "tc_invert_host.cpp")])
    L = C.CDLL(out)
    L.hm_tc_drop.restype = C.c_double
    return L


def invert(L, A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = len(A)
    X = np.full((n, n), np.nan)
    dropped = C.c_int(-1)
    ok = L.hm_tc_invert(C.c_int(n), A.ctypes.data_as(dp), X.ctypes.data_as(dp), C.byref(dropped))
    return ok, dropped.value, X


def spd(n, cond, seed, lowest=None):
    """Q diag(w) Q^T with w = logspace(0, -log10 cond): condition number cond by construction; lowest: replaces the smallest eigenvalue"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    w = np.logspace(0.0, -np.log10(cond), n)
    if lowest is not None:
        w[-1] = lowest
    A = (Q * w) @ Q.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("n", [12, 96, 768])
@pytest.mark.parametrize("cond", [1e2, 1e6, 1e10])
def test_inverse_against_numpy(tc, n, cond):
    """Measured (host build): |X A - I|_max between 7.5e-5 and 1.4e-2 of n eps cond over the nine cases (bar 64); X is
    symmetric to the bit and agrees with numpy.linalg.inv to the same bound relative to |X|_max (<= 1.2e-7 at cond 1e10)."""
    A = spd(n, cond, 100 + n)
    ok, dropped, X = invert(tc, A)
    res = np.abs(X @ A - np.eye(n)).max()
    ref = np.linalg.inv(A)
    dev = np.abs(X - ref).max() / np.abs(ref).max()
    bar = 64 * n * EPS * cond
    print("n = %d, cond = %.0e (numpy: %.3e): |X A - I|_max = %.3e = %.2e n eps cond (bar 64), |X - inv| / |inv|_max = %.3e"
          % (n, cond, np.linalg.cond(A), res, res / (n * EPS * cond), dev))
    assert ok == 1 and dropped == 0
    assert res <= bar, (res, bar)
    assert dev <= bar, (dev, bar)
    assert X.tobytes() == X.T.copy().tobytes()


@pytest.mark.parametrize("n", [12, 96])
def test_dropped_columns(tc, n):
    """Three zeroed rows and columns: three dropped columns, zero rows and columns of X, and the inverse of the rest to the bar of
    test_inverse_against_numpy.  A diagonal of 2^-41 of the largest is dropped as well, one of 2^-39 is kept."""
    cond = 1e6
    A = spd(n, cond, 7)
    z = [1, n // 2, n - 1]
    A[z, :] = 0.0; A[:, z] = 0.0
    ok, dropped, X = invert(tc, A)
    rest = np.setdiff1d(np.arange(n), z)
    assert ok == 1 and dropped == 3
    assert (X[z, :] == 0.0).all() and (X[:, z] == 0.0).all()
    sub = A[np.ix_(rest, rest)]
    res = np.abs(X[np.ix_(rest, rest)] @ sub - np.eye(len(rest))).max()
    bar = 64 * n * EPS * np.linalg.cond(sub)
    print("n = %d: 3 dropped, |X A - I|_max on the rest = %.3e (bar %.3e)" % (n, res, bar))
    assert res <= bar, (res, bar)
    assert tc.hm_tc_drop() == 2.0 ** -40
    D = np.diag(np.concatenate([[1.0, 2.0 ** -41, 2.0 ** -39], np.full(n - 3, 0.5)]))
    ok, dropped, X = invert(tc, D)
    assert ok == 1 and dropped == 1 and X[1, 1] == 0.0 and abs(X[2, 2] * 2.0 ** -39 - 1.0) <= 8 * EPS and X[0, 0] == 1.0      # (1 / sqrt(2^-39) is rounded)
    ok, dropped, X = invert(tc, np.zeros((n, n)))      # everything held
    assert ok == 1 and dropped == n and (X == 0.0).all()


@pytest.mark.parametrize("n", [12, 96])
def test_not_positive_definite(tc, n):
    """An indefinite matrix (one eigenvalue -0.05, the others in [0.5, 1], every diagonal entry positive), a singular one (B B^T of rank
    n - 6), a negative diagonal entry and a NaN: verdict 0 and X = 0 exactly."""
    ind = spd(n, 2.0, 11, lowest=-0.05)
    assert (np.diag(ind) > 0).all() and np.linalg.eigvalsh(ind)[0] < -0.04
    B = np.random.default_rng(13).standard_normal((n, n - 6))
    sing = B @ B.T
    neg = spd(n, 1e2, 17); neg[3, 3] = -1.0
    nan = spd(n, 1e2, 19); nan[2, 5] = nan[5, 2] = np.nan
    for name, A in (("indefinite", ind), ("singular", sing), ("negative diagonal", neg), ("NaN", nan)):
        ok, dropped, X = invert(tc, A)
        assert ok == 0, name
        assert (X == 0.0).all(), name


def _cloth_grid(n):
    g = np.arange(n + 1) / n
    X, Y = np.meshgrid(g, 1.5 * g, indexing="ij")
    return np.stack([X.ravel(), np.zeros(X.size), Y.ravel()], axis=1)


def _sibling_sizes(sizes):
    """the sizes of the two halves at every node of the bisection tree over a power-of-two list of leaves"""
    out = []
    while len(sizes) > 1:
        out += [(sizes[i], sizes[i + 1]) for i in range(0, len(sizes), 2)]
        sizes = [sizes[i] + sizes[i + 1] for i in range(0, len(sizes), 2)]
    return out


@pytest.mark.parametrize("mesh,G", [("kuhn5", 8), ("kuhn5", 4), ("kuhn3", 4), ("kuhn3", 1), ("kuhn3", 64), ("cloth12", 8), ("kuhn5", 6)])
def test_plan(mesh, G):
    """Every vertex in exactly one aggregate; G aggregates, none empty, ascending inside one; siblings of the bisection differ by at most
    one vertex (G a power of two); two calls return the same arrays; a split is along the longest extent: the first one separates the
    vertices at a coordinate of that axis.  G = 6: the parts get 3 / 6 and 1 / 3 + 2 / 3 shares."""
    xyz = meshes.kuhn_cube(5)[0] if mesh == "kuhn5" else meshes.kuhn_cube(3)[0] if mesh == "kuhn3" else _cloth_grid(12)
    nv = len(xyz)
    assert nv == {"kuhn5": 216, "kuhn3": 64, "cloth12": 169}[mesh]
    ptr, vert = Solver.tangent_plan(xyz, G)
    ptr2, vert2 = Solver.tangent_plan(xyz, G)
    assert ptr.tobytes() == ptr2.tobytes() and vert.tobytes() == vert2.tobytes()
    assert len(ptr) == G + 1 and ptr[0] == 0 and ptr[-1] == nv
    sizes = np.diff(ptr)
    assert (sizes >= 1).all()
    assert sorted(vert.tolist()) == list(range(nv))
    for g in range(G):
        a = vert[ptr[g]:ptr[g + 1]]
        assert (np.diff(a) > 0).all()
    if G & (G - 1) == 0:
        for a, b in _sibling_sizes(sizes.tolist()):
            assert abs(a - b) <= 1, (a, b)
    else:
        assert sizes.max() - sizes.min() <= 2, sizes
    if G >= 2:
        ax = int(np.argmax(np.ptp(xyz, axis=0)))
        left = vert[:ptr[G // 2]]; right = vert[ptr[G // 2]:]
        assert xyz[left, ax].max() <= xyz[right, ax].min()
    print("%s, G = %d: sizes %s" % (mesh, G, sizes.tolist()))


def test_plan_refusals():
    xyz = meshes.kuhn_cube(1)[0]
    for G in (0, 65, len(xyz) + 1):
        with pytest.raises(capi.AdmmHipError):
            Solver.tangent_plan(xyz, G)
