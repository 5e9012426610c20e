"""The dense Rayleigh-Ritz of the block eigensolver (device_math.hpp: modal_geneig, modal_rr -- the functions k_modal_rr calls, one text
for device and host) compiled for the host, where ONE thread replays the device's phases in order, against numpy.linalg.eigh of the
Cholesky-reduced pencil L^-1 G_A L^-T (G_M = L L^T, after the same unit-diagonal scaling).

  sizes          n = 1 .. 48
  well cond.     G_M = B^T B for B [200][n] random, G_A random symmetric
  nearly dep.    column j of B = column 0 + eps_j noise, eps down to 1e-5: cond(G_M) up to 1e12 after scaling -- what a stalled P produces
  clustered      G_A = C^-T diag(ev) C^-1 with exactly repeated and 1e-10-clustered ev
  compared       eigenvalues, relative to the largest |ev|; C^T G_M C = I (max norm)

MEASURED on the host (g++ -O2, x86-64) / asserted at 10 x:
  well conditioned   eigenvalues 1.4e-14 / 1.4e-13      C^T G_M C - I  1.4e-14 / 1.4e-13
  nearly dependent   eigenvalues 2.8e-6  / 2.8e-5       C^T G_M C - I  6.7e-6  / 6.7e-5     (cond(scaled G_M) up to 3.7e12: eps cond)
  clustered          eigenvalues 2.1e-15 / 2.1e-14      C^T G_M C - I  1.7e-15 / 1.7e-14

The failure rule: an exactly singular, an indefinite and a non-finite G_M report failure with ev and C zero; modal_rr on a singular G_M
whose leading 2 nb block is regular succeeds on the restart path (P dropped: its rows of C are zero)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
BOUND = {"random": (1.4e-13, 1.4e-13), "dependent": (2.8e-5, 6.7e-5), "clustered": (2.1e-14, 1.7e-14)}


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("modal_host")), "libmodal_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(HERE, "hostmath"), "-o", out,
                           os.path.join(HERE, "hostmath", "modal_host.cpp")])
    lib = C.CDLL(out)
    lib.hm_modal_pivot.restype = C.c_double
    lib.hm_modal_start.restype = C.c_double
    return lib


def geneig(L, GA, GM):
    GA = np.ascontiguousarray(GA, dtype=np.float64); GM = np.ascontiguousarray(GM, dtype=np.float64)
    n = len(GA)
    ev = np.full(n, 7.0); Cm = np.full((n, n), 7.0)
    ok = L.hm_sym_geneig(C.c_int(n), GA.ctypes.data_as(dp), GM.ctypes.data_as(dp), ev.ctypes.data_as(dp), Cm.ctypes.data_as(dp))
    return ok, ev, Cm


def reference(GA, GM):
    d = 1.0 / np.sqrt(np.diag(GM))
    Lc = np.linalg.cholesky(GM * d[:, None] * d[None, :])
    Y = np.linalg.solve(Lc, GA * d[:, None] * d[None, :])
    H = np.linalg.solve(Lc, Y.T).T
    return np.linalg.eigvalsh(0.5 * (H + H.T))


def systems(kind):
    rng = np.random.default_rng({"random": 5, "dependent": 7, "clustered": 9}[kind])
    for n in range(1, 49):
        B = rng.standard_normal((200, n))
        if kind == "dependent" and n > 1:
            eps = 10.0 ** rng.uniform(-5.0, -2.0, n)
            B = B[:, :1] + eps[None, :] * B
            B[:, 0] = B[:, 0] / (1.0 + eps[0])
        GM = B.T @ B
        if kind == "clustered":
            ev = np.sort(rng.standard_normal(n))
            ev[n // 2:] = ev[n // 2]                                  # exactly repeated
            ev[:n // 4] = ev[0] * (1.0 + 1e-10 * np.arange(n // 4))      # a cluster
            X = np.linalg.inv(np.linalg.cholesky(GM)).T               # X^T GM X = I
            Xi = np.linalg.inv(X)
            GA = Xi.T @ np.diag(ev) @ Xi
        else:
            R = rng.standard_normal((n, n))
            GA = B.T @ (rng.standard_normal(200)[:, None] * B) if kind == "dependent" else R + R.T
        yield n, 0.5 * (GA + GA.T), GM


@pytest.mark.parametrize("kind", ["random", "dependent", "clustered"])
def test_geneig_matches_numpy(L, kind):
    worst_ev = worst_orth = cond = 0.0
    for n, GA, GM in systems(kind):
        ok, ev, Cm = geneig(L, GA, GM)
        assert ok == 1, n
        ref = reference(GA, GM)
        assert np.all(np.diff(ev) >= 0.0)
        worst_ev = max(worst_ev, np.abs(ev - ref).max() / np.abs(ref).max())
        worst_orth = max(worst_orth, np.abs(Cm.T @ GM @ Cm - np.eye(n)).max())
        d = 1.0 / np.sqrt(np.diag(GM))
        cond = max(cond, np.linalg.cond(GM * d[:, None] * d[None, :]))
    print("modal_geneig vs numpy (%s): eigenvalues %.3e of max |ev|, C^T G_M C - I %.3e, cond(scaled G_M) up to %.1e" % (kind, worst_ev, worst_orth, cond))
    if kind == "dependent":
        assert cond >= 1e11      # (the family does reach the ill-conditioned matrices it is meant to)
    assert worst_ev <= BOUND[kind][0]
    assert worst_orth <= BOUND[kind][1]


def test_failure_rule(L):
    assert L.hm_modal_pivot() == 64.0 * np.finfo(np.float64).eps
    bad = []
    B = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, 0.0], [-1.0, -2.0, 3.0]])      # columns 0 and 1 exactly dependent, exactly representable
    bad.append(B.T @ B)
    bad.append(np.array([[1.0, 2.0], [2.0, 1.0]]))                          # indefinite
    bad.append(np.array([[1.0, 0.0], [0.0, -1.0]]))                         # a negative diagonal
    bad.append(np.zeros((3, 3)))
    Mn = np.eye(4); Mn[2, 1] = Mn[1, 2] = np.nan
    bad.append(Mn)
    bad.append(np.diag([1.0, np.inf]))
    for GM in bad:
        n = len(GM)
        ok, ev, Cm = geneig(L, np.eye(n), GM)
        assert ok == 0, GM
        assert np.all(ev == 0.0) and np.all(Cm == 0.0)
    An = np.eye(3); An[0, 2] = An[2, 0] = np.nan                            # a non-finite G_A
    ok, ev, Cm = geneig(L, An, np.eye(3))
    assert ok == 0 and np.all(ev == 0.0) and np.all(Cm == 0.0)


def test_restart_path(L):
    """S = [X W P] with P = a copy of X (exactly dependent, exactly representable): G_M is singular, its leading 2 nb block regular"""
    nb = 3
    rng = np.random.default_rng(3)
    XW = np.round(rng.standard_normal((40, 2 * nb)) * 8.0) / 8.0
    S = np.concatenate([XW, XW[:, :nb]], axis=1)
    Aop = np.diag(np.arange(1.0, 41.0))
    GA = np.ascontiguousarray(S.T @ Aop @ S); GM = np.ascontiguousarray(S.T @ S)
    th = np.full(nb, 7.0); Cm = np.full((3 * nb, nb), 7.0); rst = C.c_int(5)
    used = L.hm_modal_rr(C.c_int(nb), C.c_int(3 * nb), GA.ctypes.data_as(dp), GM.ctypes.data_as(dp), th.ctypes.data_as(dp), Cm.ctypes.data_as(dp), C.byref(rst))
    assert used == 2 * nb and rst.value == 1
    assert np.all(Cm[2 * nb:] == 0.0)
    ref = reference(GA[:2 * nb, :2 * nb], GM[:2 * nb, :2 * nb])[:nb]      # (a well-conditioned 6 x 6 pencil: 1e-13 is the bar of the random family)
    assert np.abs(th - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(Cm.T @ GM @ Cm - np.eye(nb)).max() <= 1e-13
    # without P in use nothing restarts; a failure on [X W] as well returns 0 with everything zero
    used = L.hm_modal_rr(C.c_int(nb), C.c_int(2 * nb), GA.ctypes.data_as(dp), GM.ctypes.data_as(dp), th.ctypes.data_as(dp), Cm.ctypes.data_as(dp), C.byref(rst))
    assert used == 2 * nb and rst.value == 0
    Z = np.zeros((3 * nb, 3 * nb))
    used = L.hm_modal_rr(C.c_int(nb), C.c_int(3 * nb), GA.ctypes.data_as(dp), Z.ctypes.data_as(dp), th.ctypes.data_as(dp), Cm.ctypes.data_as(dp), C.byref(rst))
    assert used == 0 and rst.value == 1 and np.all(th == 0.0) and np.all(Cm == 0.0)


def test_start_block_hash(L):
    """the default start block: the integer hash, restated in numpy (tests/test_modes.py builds its `init` from this restatement)"""
    from test_modes import start_block
    X = start_block(3, 11)
    for c in range(3):
        for v in range(11):
            for j in range(3):
                assert X[c, v, j] == L.hm_modal_start(C.c_uint(c), C.c_uint(v), C.c_uint(j))
    assert np.abs(X).max() < 1.0
