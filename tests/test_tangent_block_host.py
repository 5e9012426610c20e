"""The block entry points of the tangent solves (admm_hip_tangent_solve_block, admm_hip_step_adjoint_block) on every face of the project,
without a GPU: exported by the library, declared in include/admm_hip.h, bound in capi.py, mirrored in Python and C++, documented; the
argument checks that need no device."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("admm_hip_tangent_solve_block", "admm_hip_step_adjoint_block")
ERR_ARG = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_symbols_and_signatures():
    """both entry points are exported, declared, bound and mirrored"""
    from admm_elastic_amd import capi
    from admm_elastic_amd.solver import Solver
    bound = {s[0]: s for s in capi.SYMBOLS}
    hdr = _read("include", "admm_hip.h")
    L = capi.lib()
    for name in NAMES:
        assert name in bound and hasattr(L, name)
        assert "int %s(" % name in hdr
    assert len(bound[NAMES[0]][2]) == 11 and len(bound[NAMES[1]][2]) == 17      # the arguments of the declarations
    assert NAMES[0] in Solver.tangent_solve_block.__doc__ and NAMES[1] in Solver.step_adjoint_block.__doc__
    hpp = _read("admm-elastic_amd", "host", "include", "Solver.hpp")
    cpp = _read("admm-elastic_amd", "host", "src", "Solver.cpp")
    assert "tangent_solve_block(" in hpp and "step_adjoint_block(" in hpp
    assert NAMES[0] + "(" in cpp and NAMES[1] + "(" in cpp


def test_documented():
    """README, DESIGN and INTEGRATION name both entry points; DESIGN carries the resource table of every new kernel"""
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "tangent_solve_block" in text and "step_adjoint_block" in text, doc
    design = _read("DESIGN.md")
    for kernel in ("k_nw_cg_init_block", "k_nw_cg_init2_block", "k_nw_cg_step_block", "k_nw_cg_dir_block", "k_nw_true_resid_block",
                   "k_nw_resid_final_block", "k_newton_gather_block<true>"):
        assert kernel in design, kernel


def test_null_context_and_k_below_one_are_refused():
    from admm_elastic_amd import capi
    L = capi.lib()
    d = capi.dptr
    a = np.ones(12); y = np.zeros(12); i4 = np.zeros(4); i6 = np.zeros(6); b3 = np.zeros(3)
    for k in (1, 0, -3):
        assert L.admm_hip_tangent_solve_block(None, None, k, d(a), 1.0, 3, 1e-10, 10, d(y), d(i4), d(b3)) == ERR_ARG
        assert L.admm_hip_step_adjoint_block(None, k, d(a), None, 0, 1e-10, 10, *([None] * 8), d(i6), d(b3)) == ERR_ARG
    assert b"NULL" in L.admm_hip_last_error()
