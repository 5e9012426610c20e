"""The blocked coarse inverse of the two-level tangent preconditioner through the C++ mirror: tests/cpp/test_tangent_coarse.cpp, driven
the way test_tangent_precond_cpp.py drives its binary, and held against the Python binding on the same scene."""
import os
import subprocess

import numpy as np
import pytest

import admm_elastic_amd as pkg
from admm_elastic_amd.solver import Lame, Settings, Solver
from test_adjoint_cpp import _cube48
from test_cpp_api import _build_exe


def test_cpp_tangent_coarse_builds():
    """Solver::set_tangent_coarse and Solver::tangent_coarse exist and link."""
    _build_exe("test_tangent_coarse")


@pytest.mark.gpu
def test_cpp_blocked_solve_matches_the_python_binding(tmp_path):
    """The scene of test_tangent_precond_cpp.py: Solver::tangent_solve with set_tangent_precond(TwoLevel, 2) and
    set_tangent_coarse(Blocked), and with OneBlock, as the C++ mirror returns them (written as %.17g, which round-trips a double), have
    the BITS and the iteration counts of the Python binding with set_tangent_coarse("blocked") / "one_block": both faces drive the same
    library with the same description.  The binary itself checks the residual, the reports of tangent_coarse() and tangent_precond() and
    that one-block after blocked has the bits of one-block before."""
    exe = _build_exe("test_tangent_coarse")
    path = os.path.join(str(tmp_path), "cpp_tangent_coarse.txt")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.loadtxt(path)
    verts, tets = _cube48()
    nv, n3 = len(verts), 3 * len(verts)
    s = Solver()
    s.add_nodes(verts, np.full(n3, 0.05))
    s.add_tets(verts, tets, Lame(1.0e5, 0.35), pkg.TET_NEOHOOKEAN)
    pins = [int(v) for v in np.nonzero((verts[:, 0] < 1e-9) & (verts[:, 1] < 1e-9))[0]]
    s.set_pins(pins, [verts[v] for v in pins])
    st = Settings(); st.admm_iters = 5; st.linsolver = 0
    assert s.initialize(st)
    x = np.stack([0.9 * verts[:, 0], 0.8 * verts[:, 1] + 0.1 * verts[:, 0], 0.85 * verts[:, 2]], axis=1)
    rhs = np.sin(1.0 + 3.0 * np.arange(n3))
    s.set_tangent_precond("two_level", 2)
    yo, io = s.tangent_solve(rhs, x, tol=1e-12, max_iters=2000)
    s.set_tangent_coarse("blocked")
    yb, ib = s.tangent_solve(rhs, x, tol=1e-12, max_iters=2000)
    info, co = s.tangent_precond(), s.tangent_coarse()
    s.close()
    assert got.size == 2 * n3 + 2
    print("Python: blocked %d iterations, one-block %d; C++: %d, %d; largest |C++ - Python| blocked %.3e, one-block %.3e; %s %s"
          % (ib["iterations"], io["iterations"], got[-2], got[-1], np.abs(got[:n3] - yb.ravel()).max(), np.abs(got[n3:2 * n3] - yo.ravel()).max(), info, co))
    assert info == dict(kind="two_level", aggregates=2, coarse_dim=24, coarse_dropped=0, coarse_ok=True, setup_passes=2), info
    assert co == dict(solver="blocked", tile=64, launches=7), co
    assert (int(got[-2]), int(got[-1])) == (ib["iterations"], io["iterations"])
    assert got[:n3].tobytes() == yb.ravel().tobytes()
    assert got[n3:2 * n3].tobytes() == yo.ravel().tobytes()
