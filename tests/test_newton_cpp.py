"""The Newton polish through the C++ mirror: tests/cpp/test_newton.cpp, driven the way test_cpp_api.py drives its binaries."""
import subprocess

import pytest

from test_cpp_api import _build_exe


def test_cpp_newton_builds():
    """Solver::newton_polish, Solver::tangent_solve and the stiffness_apply overload exist and link."""
    _build_exe("test_newton")


@pytest.mark.gpu
def test_cpp_newton_polish():
    """One step of 5 ADMM iterations on the pinned 48-tet Neo-Hookean cube, then Solver::newton_polish: the objective does not rise,
    |g_free| recomputed from Solver::forces reaches grad_tol, m_v stays (m_x - x_prev) / dt, pinned vertices stay; Solver::tangent_solve's
    residual recomputed with Solver::stiffness_apply(psd, hold_pins) is <= 2 tol |rhs|."""
    exe = _build_exe("test_newton")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
