"""Anderson acceleration through the C++ mirror: tests/cpp/test_anderson.cpp, driven the way test_cpp_api.py drives its binaries."""
import subprocess

import pytest

from test_cpp_api import _build_exe


def test_cpp_anderson_builds():
    """Settings::anderson, Solver::set_anderson and Solver::anderson_history exist and link."""
    _build_exe("test_anderson")


@pytest.mark.gpu
def test_cpp_anderson():
    """-aa 3 -it 20 on the pinned 18-tet Neo-Hookean cantilever under gravity: Settings::parse_args reads the window, anderson_history() has
    one record per iteration with a plain accepted first one and extrapolated states behind it, the step ends nearer to the 600-iteration
    step than the plain 20-iteration step, a window of 9 is refused, and with the window 0 again a step leaves no records."""
    exe = _build_exe("test_anderson")
    r = subprocess.run([exe, "-aa", "3", "-it", "20"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
