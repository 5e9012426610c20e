"""The blocked dense inverse of the two-level tangent preconditioner (csrc/tangent_coarse.hpp; Solver.set_tangent_coarse("blocked")),
no GPU: the routines the k_tcb_ kernels call, compiled for the host (tests/hostmath/tcb_invert_host.cpp: one thread walks the blocks of
every launch in the device's launch order, an empty barrier -- the device's arithmetic) against numpy and against the one-block routine
(tests/hostmath/tc_invert_host.cpp).

THE MATRICES are test_tangent_precond_host.py's: SPD with CONSTRUCTED condition numbers 1e2, 1e6, 1e10.  THE BAR is its bar:
|X A - I|_max <= 64 n eps cond -- the backward error of a Cholesky solve is c n eps |A| whatever the blocking -- and, for two inverses that
both meet it, |X_b - X_o|_max <= 64 n eps cond |X_o|_max.  Sizes: 1, 12, T - 1, T, T + 1, 2 T + 1, 384, 768 with T = 64 the tile.

The matrices and numpy's figures are built once per (n, cond) and shared (matrix())."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from test_tangent_precond_host import EPS, dp, spd

HERE = os.path.dirname(os.path.abspath(__file__))
T = 64
SIZES = [1, 12, T - 1, T, T + 1, 2 * T + 1, 384, 768]
CONDS = [1e2, 1e6, 1e10]


def _build(tmp, src, name, extra=()):
    out = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *extra, "-I", os.path.join(HERE, "hostmath"), "-o", out, os.path.join(HERE, "hostmath", src)])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(blocked at T = 64, blocked at T = 32, one-block)"""
    tmp = str(tmp_path_factory.mktemp("tcb_invert_host"))
    return (_build(tmp, "tcb_invert_host.cpp", "libtcb64.so"), _build(tmp, "tcb_invert_host.cpp", "libtcb32.so", ["-DADMM_TCB_TILE=32"]),
            _build(tmp, "tc_invert_host.cpp", "libtc.so"))


def invert(fn, A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = len(A)
    X = np.full((n, n), np.nan)
    dropped = C.c_int(-1)
    ok = fn(C.c_int(n), A.ctypes.data_as(dp), X.ctypes.data_as(dp), C.byref(dropped))
    return ok, dropped.value, X


@functools.lru_cache(maxsize=None)
def matrix(n, cond):
    """the SPD matrix of (n, cond); n = 1: the 1 x 1 matrix [1]"""
    A = spd(n, cond, 100 + n)
    A.setflags(write=False)
    return A


def dropped_case(n):
    """cond 1e6 with three zeroed rows and columns: one in the first tile, one on a tile boundary (or mid-way below a tile), one in the
    last (partial) tile -> (A, the zeroed indices)"""
    A = spd(n, 1e6, 7)
    z = sorted({1, n // 2 if n < T else T - 1 if n == T + 1 else T, n - 1})
    A[z, :] = 0.0; A[:, z] = 0.0
    return A, z


BAD_SIZES = [12, T + 9, 2 * T + 9]      # one tile; two and three tiles whose last, partial tile has 9 rows (at T = 32: three and five tiles)


def first_bad_pivot(A):
    """numpy's replay of the rule: the step at which the right-looking Cholesky of the scaled matrix meets a pivot below 16 n eps or
    not finite; -1: the diagonal scan ends it before any pivot; None: none"""
    n = len(A)
    d = np.diag(A).copy()
    if not np.isfinite(d).all() or (d < -2.0 ** -40 * d.max()).any():
        return -1
    s = 1.0 / np.sqrt(d)
    S = A * s[:, None] * s[None, :]
    with np.errstate(all="ignore"):
        for j in range(n):
            if not S[j, j] >= 16 * n * EPS or not np.isfinite(S[j, j]):
                return j
            c = S[j + 1:, j] / np.sqrt(S[j, j])
            S[j + 1:, j + 1:] -= np.outer(c, c)
    return None


def bad_cases(n):
    """not positive definite or not finite: name -> (matrix, the rows the defect must be found in: None, or (lo, hi) -- asserted against
    first_bad_pivot).  Apart from the two global cases the defect sits at (p, q) = (3, 5), in the FIRST tile; at (n - 2, n - 5), both in
    the LAST tile of a multi-tile n (BAD_SIZES: the last tile holds rows n - 9 .. n - 1 at T = 64 and at T = 32), where only the last
    k_tcb_potrf of the chain can find it; and at (n - 2, 5), an off-diagonal entry of the tile (last, first): a NaN / Inf there travels
    through the panel of step 0 and the updates into the last diagonal tile.  (A negative diagonal entry is the scan's to find.)"""
    out = {}
    ind = spd(n, 2.0, 11, lowest=-0.05)
    assert (np.diag(ind) > 0).all() and np.linalg.eigvalsh(ind)[0] < -0.04
    out["indefinite"] = (ind, None)
    B = np.random.default_rng(13).standard_normal((n, n - 6))
    out["rank n - 6"] = (B @ B.T, None)
    last = (n - 9, n - 1) if n > T else (0, n - 1)
    for where, (p, q), rows in (("first tile", (3, 5), (0, 5)), ("last tile", (n - 2, n - 5), last), ("tile (last, first)", (n - 2, 5), last)):
        neg = spd(n, 1e2, 17); neg[p, p] = -1.0
        nan = spd(n, 1e2, 19); nan[p, q] = nan[q, p] = np.nan
        inf = spd(n, 1e2, 23); inf[p, q] = inf[q, p] = np.inf
        ind2 = spd(n, 1e2, 29); ind2[p, q] = ind2[q, p] = 2.0      # a 2 x 2 minor with |a_pq| > sqrt(a_pp a_qq): indefinite, found at pivot max(p, q)
        assert ind2[p, p] * ind2[q, q] < 4.0
        out.update({"negative diagonal, %s" % where: (neg, (-1, -1)), "NaN, %s" % where: (nan, rows), "Inf, %s" % where: (inf, rows),
                    "indefinite minor, %s" % where: (ind2, rows)})
    for name, (A, rows) in out.items():
        j = first_bad_pivot(A)
        assert j is not None and (rows is None or rows[0] <= j <= rows[1]), (name, j, rows)
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cond", CONDS)
def test_inverse_against_numpy_and_one_block(libs, n, cond):
    """|X A - I|_max <= 64 n eps cond, X symmetric to the bit, and |X_b - X_o|_max <= 64 n eps cond |X_o|_max against the one-block
    routine on the same matrix.

    Measured (host build, 24 cases): |X A - I|_max between 9.9e-7 and 3.6e-4 of the bar, |X_b - X_o| between 8.8e-14 and 2.4e-5 of its
    bar (0 at n = 1); DESIGN.md 4o."""
    A = matrix(n, cond)
    ok, dropped, X = invert(libs[0].hm_tcb_invert, A)
    ok1, dropped1, X1 = invert(libs[2].hm_tc_invert, A)
    res = np.abs(X @ A - np.eye(n)).max()
    dev = np.abs(X - X1).max() / np.abs(X1).max()
    bar = 64 * n * EPS * cond
    print("n = %d, cond = %.0e: |X A - I|_max = %.3e = %.2e of the bar; |X_b - X_o| / |X_o|_max = %.3e = %.2e of the bar" % (n, cond, res, res / bar, dev, dev / bar))
    assert (ok, dropped) == (1, 0) == (ok1, dropped1)
    assert res <= bar, (res, bar)
    assert dev <= bar, (dev, bar)
    assert X.tobytes() == X.T.copy().tobytes()


@pytest.mark.parametrize("n", [12, T + 1, 2 * T + 1, 384])
def test_dropped_columns(libs, n):
    """Three zeroed rows and columns (first tile, a tile boundary, the last partial tile): dropped == 3, those rows and columns of X
    zero, the rest the inverse of the rest at the bar; the one-block routine drops the same."""
    A, z = dropped_case(n)
    ok, dropped, X = invert(libs[0].hm_tcb_invert, A)
    ok1, dropped1, X1 = invert(libs[2].hm_tc_invert, A)
    rest = np.setdiff1d(np.arange(n), z)
    assert (ok, dropped) == (1, 3) == (ok1, dropped1)
    assert (X[z, :] == 0.0).all() and (X[:, z] == 0.0).all()
    sub = A[np.ix_(rest, rest)]
    res = np.abs(X[np.ix_(rest, rest)] @ sub - np.eye(len(rest))).max()
    bar = 64 * n * EPS * np.linalg.cond(sub)
    print("n = %d, zeroed %s: |X A - I|_max on the rest = %.3e (bar %.3e)" % (n, z, res, bar))
    assert res <= bar, (res, bar)
    assert X.tobytes() == X.T.copy().tobytes()
    ok, dropped, X = invert(libs[0].hm_tcb_invert, np.zeros((n, n)))      # everything held
    assert ok == 1 and dropped == n and (X == 0.0).all()


@pytest.mark.parametrize("n", BAD_SIZES)
def test_not_positive_definite(libs, n):
    """Indefinite, rank n - 6, a negative diagonal entry, a NaN, an Inf and an indefinite 2 x 2 minor; the defect in the first tile (the
    verdict word has to travel through every later phase), in the last tile (cleared by the last potrf of the chain) and in the tile
    (last, first) (carried there by panel and update) -- bad_cases asserts by a numpy replay where each is found: verdict 0 and X = 0
    exactly, the one-block routine's verdict."""
    for name, (A, _) in bad_cases(n).items():
        ok, dropped, X = invert(libs[0].hm_tcb_invert, A)
        ok1, _, X1 = invert(libs[2].hm_tc_invert, A)
        assert ok == 0 == ok1, name
        assert (X == 0.0).all() and (X1 == 0.0).all(), name


@pytest.mark.parametrize("n", [T - 1, 2 * T + 1, 384])
@pytest.mark.parametrize("cond", CONDS)
def test_tile_independence(libs, n, cond):
    """The same text at T = 32: the two results agree at the forward-error bar, and the verdicts of the bad matrices agree."""
    assert libs[0].hm_tcb_tile() == T and libs[1].hm_tcb_tile() == 32
    A = matrix(n, cond)
    ok, dropped, X = invert(libs[0].hm_tcb_invert, A)
    ok2, dropped2, X2 = invert(libs[1].hm_tcb_invert, A)
    dev = np.abs(X - X2).max() / np.abs(X).max()
    bar = 64 * n * EPS * cond
    print("n = %d, cond = %.0e: |X_64 - X_32| / |X_64|_max = %.3e = %.2e of the bar" % (n, cond, dev, dev / bar))
    assert (ok, dropped) == (1, 0) == (ok2, dropped2)
    assert dev <= bar, (dev, bar)
    assert X2.tobytes() == X2.T.copy().tobytes()
    if cond == CONDS[0] and n == 2 * T + 1:
        for name, (B, _) in bad_cases(2 * T + 9).items():
            ok2, _, X2 = invert(libs[1].hm_tcb_invert, B)
            assert ok2 == 0 and (X2 == 0.0).all(), name
