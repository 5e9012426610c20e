"""Modal analysis through the C++ mirror: tests/cpp/test_modes.cpp, driven the way test_newton_cpp.py drives its binary."""
import subprocess

import pytest

from test_cpp_api import _build_exe


def test_cpp_modes_builds():
    """Solver::modes and the block argument of the stiffness_apply overload exist and link."""
    _build_exe("test_modes")


@pytest.mark.gpu
def test_cpp_modes():
    """The pinned 48-tet Neo-Hookean cube at a compressed state, Solver::modes(4): the residuals recomputed through
    Solver::stiffness_apply(psd, hold_pins) meet 2 tol, the block pass has the single pass's bytes, Phi^T M Phi = I."""
    exe = _build_exe("test_modes")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
