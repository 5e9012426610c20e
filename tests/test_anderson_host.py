"""The small regularised solve of the Anderson acceleration (device_math.hpp: aa_small_solve, the function k_aa_solve calls), compiled for
the host and held against numpy.linalg.solve on the same regularised system (H + 1e-10 (tr H / n) I) theta = b.

  sizes          n = 1 .. 8
  systems        H = A^T A, b = A^T f for A [200][n] and f random; A with independent random columns, and with nearly dependent columns
                 (column j = column 0 + eps_j noise, eps down to 1e-6: cond(H) up to 1e12 and beyond, what a stalled ADMM run produces)
  compared       per entry, relative to the largest entry of numpy's theta
  way out        exactly dependent columns of an exactly representable matrix (the regularised pivot still positive: solved, finite), a
                 zero matrix, a negative diagonal and a NaN entry of H or b must return 0 with theta zero ("clear the ring")

MEASURED on the host (g++ -O2, x86-64): well conditioned (random columns, cond(H) 2.4) max 5.2e-16 of |theta|_inf; nearly dependent
columns (cond(H) up to 1.4e13, the regularisation leaves about 1e10 n), max 1.5e-6 -- Cholesky against numpy's LU at cond * eps.  Asserted
at 10 x: 5.2e-15 and 1.5e-5.

Exactly dependent NON-ZERO columns do not take the way out under the stated regularisation: the last pivot is 1e-10 tr H / n (1 + the
share of the dependent column), far above the rounding of the elimination, so the solve succeeds with a finite theta -- asserted as
such.  The way out is reached by a Gram matrix that is exactly zero (dependent columns that are all zero: a history that stalled to
the bit), by an indefinite or non-finite one, and by a non-finite right-hand side."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
BOUND_RANDOM = 5.2e-15
BOUND_DEPENDENT = 1.5e-5


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("anderson_host")), "libanderson_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "anderson_host.cpp")])
    lib = C.CDLL(out)
    lib.hm_aa_small_solve.restype = C.c_int
    lib.hm_aa_reg.restype = C.c_double
    return lib


def solve(L, H, b):
    H = np.ascontiguousarray(H, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    n = len(b)
    th = np.full(8, 7.0)
    ok = L.hm_aa_small_solve(C.c_int(n), H.ctypes.data_as(dp), b.ctypes.data_as(dp), th.ctypes.data_as(dp))
    return ok, th


def reference(H, b, reg):
    n = len(b)
    return np.linalg.solve(H + reg * (np.trace(H) / n) * np.eye(n), b)


def systems(dependent):
    rng = np.random.default_rng(23 if dependent else 11)
    for n in range(1, 9):
        for rep in range(12):
            A = rng.standard_normal((200, n))
            if dependent:
                eps = 10.0 ** rng.uniform(-6.0, -2.0, n)
                A = A[:, :1] + eps[None, :] * A
                A[:, 0] = A[:, 0] / (1.0 + eps[0])
            f = rng.standard_normal(200)
            yield n, A.T @ A, A.T @ f


@pytest.mark.parametrize("dependent", [False, True], ids=["random", "nearly-dependent"])
def test_small_solve_matches_numpy(L, dependent):
    reg = L.hm_aa_reg()
    assert reg == 1e-10
    worst = 0.0; cond = 0.0
    for n, H, b in systems(dependent):
        ok, th = solve(L, H, b)
        assert ok == 1
        assert np.all(th[n:] == 0.0)
        ref = reference(H, b, reg)
        worst = max(worst, np.abs(th[:n] - ref).max() / np.abs(ref).max())
        cond = max(cond, np.linalg.cond(H))
    print("aa_small_solve vs numpy.linalg.solve (%s): max %.3e of |theta|_inf, cond(H) up to %.1e" % ("dependent" if dependent else "random", worst, cond))
    if dependent:
        assert cond >= 1e12      # (the family does reach the ill-conditioned systems it is meant to)
    assert worst <= (BOUND_DEPENDENT if dependent else BOUND_RANDOM)


def test_small_solve_ways_out(L):
    # exactly dependent columns with exactly representable entries: H is singular, the regularisation makes it solvable
    A = np.array([[1.0, 2.0], [2.0, 4.0], [-1.0, -2.0]])
    H = A.T @ A; b = A.T @ np.array([1.0, 0.5, 0.25])
    ok, th = solve(L, H, b)
    assert ok == 1 and np.all(np.isfinite(th))
    ref = reference(H, b, 1e-10)
    assert np.abs(th[:2] - ref).max() <= 1e-3 * np.abs(ref).max()      # (cond 1e10 against LU: only that both solve the same system)
    # the ways out: theta zero, the caller clears its ring
    bad = []
    bad.append((np.zeros((3, 3)), np.ones(3)))                                       # zero pivot
    bad.append((np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2)))                     # indefinite: second pivot negative
    bad.append((np.array([[-1.0]]), np.ones(1)))                                     # negative diagonal
    Hn = np.eye(4); Hn[2, 1] = Hn[1, 2] = np.nan
    bad.append((Hn, np.ones(4)))                                                     # NaN entry of H
    bad.append((np.eye(3), np.array([1.0, np.nan, 1.0])))                            # NaN entry of b
    bad.append((np.diag([np.inf, np.inf]), np.ones(2)))                                   # infinite pivot
    bad.append((np.eye(2), np.array([np.inf, 1.0])))                                 # infinite theta
    for H, b in bad:
        ok, th = solve(L, H, b)
        assert ok == 0, (H, b)
        assert np.all(th == 0.0)
    for n in (0, 9):      # sizes outside 1 .. 8
        th = np.full(8, 7.0)
        assert L.hm_aa_small_solve(C.c_int(n), np.eye(9).ctypes.data_as(dp), np.ones(9).ctypes.data_as(dp), th.ctypes.data_as(dp)) == 0
        assert np.all(th == 0.0)
