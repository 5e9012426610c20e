"""The adjoint of a step through the C++ mirror: tests/cpp/test_adjoint.cpp, driven the way test_newton_cpp.py drives its binary, and
held against the Python binding on the same scene."""
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
from admm_elastic_amd.solver import Lame, Settings, Solver
from test_cpp_api import _build_exe


def test_cpp_adjoint_builds():
    """Solver::step_adjoint and Solver::param_sensitivity exist and link."""
    _build_exe("test_adjoint")


def _cube48():
    """the mesh of tests/cpp/test_adjoint.cpp, built the same way"""
    n, h = 2, 0.5
    vid = lambda i, j, k: (i * (n + 1) + j) * (n + 1) + k
    verts = np.array([[h * i, h * j, h * k] for i in range(n + 1) for j in range(n + 1) for k in range(n + 1)])
    perms = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    tets = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                for p in range(6):
                    c = [i, j, k]; idx = [vid(*c)]
                    for q in range(3):
                        c[perms[p][q]] += 1; idx.append(vid(*c))
                    if p in (1, 2, 5):
                        idx[2], idx[3] = idx[3], idx[2]
                    tets.append(idx)
    return verts, np.array(tets, np.int32)


@pytest.mark.gpu
def test_cpp_step_adjoint_matches_the_python_binding(tmp_path):
    """The pinned 48-tet Neo-Hookean cube: one step of 5 ADMM iterations, the polish, step_adjoint with the same dL/dx and dL/dv on both
    faces.  Every vector the C++ mirror returns (the state, lam, xbar, x_prev, v_prev, masses) equals the Python binding's to 1e-14 of its
    largest entry, the per-tet parameter outputs to 1e-14 of theirs, and info likewise: both faces drive the same library."""
    exe = _build_exe("test_adjoint")
    path = os.path.join(str(tmp_path), "cpp_adjoint.txt")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.loadtxt(path)
    verts, tets = _cube48()
    nv, nt, n3 = len(verts), len(tets), 3 * len(verts)
    s = Solver()
    s.add_nodes(verts, np.full(n3, 0.05))
    s.add_tets(verts, tets, Lame(1.0e5, 0.35), pkg.TET_NEOHOOKEAN)
    pins = [int(v) for v in np.nonzero(verts[:, 0] < 1e-9)[0]]
    s.set_pins(pins, [verts[v] for v in pins])
    st = Settings(); st.admm_iters = 5; st.linsolver = 1      # (the pins of the sweeps: held exactly, the same problem on both faces)
    assert s.initialize(st)
    s.step()
    fm = np.ones(nv, bool); fm[pins] = False
    mg = np.linalg.norm(np.full(int(fm.sum()), 0.05 * st.gravity))
    s.newton_polish(max_iters=20, grad_tol=1e-8 * mg, cg_tol=1e-10, cg_max=2000)
    i = np.arange(n3)
    out = s.step_adjoint(np.sin(1.0 + 3.0 * i), np.cos(2.0 + 5.0 * i), tol=1e-12, max_iters=4000)
    want = [s.m_x.ravel(), s.m_v.ravel()] + [out[k].ravel() for k in ("lam", "xbar", "x_prev", "v_prev", "masses")] + [out["tets"].ravel()]
    s.close()
    assert got.size == 7 * n3 + 4 * nt + 6
    off = 0
    worst = 0.0
    for name, w in zip(("m_x", "m_v", "lam", "xbar", "x_prev", "v_prev", "masses", "tets"), want):
        g = got[off:off + w.size]; off += w.size
        e = np.abs(g - w).max() / np.abs(w).max()
        worst = max(worst, e)
        assert e <= 1e-14, (name, e)
    info = out["info"]
    tail = got[off:]
    print("C++ mirror against the Python binding: worst |difference| / scale = %.3e; info %s" % (worst, tail))
    assert int(tail[0]) == info["iterations"] and bool(tail[1]) == info["converged"]
    for g, k in zip(tail[2:], ("residual", "rhs_norm", "stationarity", "shift")):
        assert abs(g - info[k]) <= 1e-14 * max(abs(info[k]), 1e-300) or (k == "residual" and abs(g - info[k]) <= 1e-14), (k, g, info[k])
