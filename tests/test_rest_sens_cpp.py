"""The rest-shape and held-vertex gradients through the C++ mirror: tests/cpp/test_rest_sens.cpp, driven the way test_adjoint_cpp.py drives
its binary, and held against the Python binding on the same scene."""
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
from admm_elastic_amd.solver import Lame, Settings, Solver
from test_adjoint_cpp import _cube48
from test_cpp_api import _build_exe


def test_cpp_rest_sens_builds():
    """Solver::rest_sensitivity and Solver::adjoint_held exist and link."""
    _build_exe("test_rest_sens")


@pytest.mark.gpu
def test_cpp_rest_and_held_match_the_python_binding(tmp_path):
    """The pinned 48-tet Neo-Hookean cube of test_adjoint_cpp.py (pins of the sweeps): one step of 5 ADMM iterations, the polish,
    step_adjoint with the same dL/dx and dL/dv on both faces.  lam, rest = rest_sensitivity(lam) at the state and held, as the C++
    mirror returns them (written as %.17g, which round-trips a double), have the BITS of step_adjoint(rest=True, held=True) of the
    Python binding: both faces drive the same library with the same description.  Measured on an MI355X: every difference exactly 0."""
    exe = _build_exe("test_rest_sens")
    path = os.path.join(str(tmp_path), "cpp_rest_sens.txt")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.loadtxt(path)
    verts, tets = _cube48()
    nv, n3 = len(verts), 3 * len(verts)
    s = Solver()
    s.add_nodes(verts, np.full(n3, 0.05))
    s.add_tets(verts, tets, Lame(1.0e5, 0.35), pkg.TET_NEOHOOKEAN)
    pins = [int(v) for v in np.nonzero(verts[:, 0] < 1e-9)[0]]
    s.set_pins(pins, [verts[v] for v in pins])
    st = Settings(); st.admm_iters = 5; st.linsolver = 1
    assert s.initialize(st)
    s.step()
    fm = np.ones(nv, bool); fm[pins] = False
    mg = np.linalg.norm(np.full(int(fm.sum()), 0.05 * st.gravity))
    s.newton_polish(max_iters=20, grad_tol=1e-8 * mg, cg_tol=1e-10, cg_max=2000)
    i = np.arange(n3)
    out = s.step_adjoint(np.sin(1.0 + 3.0 * i), np.cos(2.0 + 5.0 * i), tol=1e-12, max_iters=4000, params=False, rest=True, held=True)
    s.close()
    assert got.size == 3 * n3
    for j, name in enumerate(("lam", "rest", "held")):
        g, w = got[j * n3:(j + 1) * n3], out[name].ravel()
        print("%s: largest |C++ - Python| / largest entry = %.3e" % (name, np.abs(g - w).max() / np.abs(w).max()))
    for j, name in enumerate(("lam", "rest", "held")):
        assert got[j * n3:(j + 1) * n3].tobytes() == out[name].ravel().tobytes(), name
    assert np.abs(out["rest"]).max() > 0.0 and np.abs(out["held"][pins]).max() > 0.0
