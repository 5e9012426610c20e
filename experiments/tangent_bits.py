"""The bits of every solve on the frozen tangent, for comparing two builds of the library (profiles/tangent_refactor.txt): one line per
call with the sha256 of its outputs and of its info, on the cases tet1, mixed162 and cloth of tests/test_newton.py.

    python experiments/tangent_bits.py > THIS.txt
    ADMM_HIP_LIB=/path/to/other/libadmm_hip.so python experiments/tangent_bits.py > OTHER.txt        (diff the two)

tangent_solve with Jacobi and with the two-level preconditioner (both coarse inverses), tangent_solve_block for k = 2 and 17, modes for
k = 3, and -- after two steps and a polish -- newton_polish's records, step_adjoint and step_adjoint_block with k = 3."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()[:16]


def flat_info(info):
    """a dict of scalars, arrays and lists of dicts -> a repr with the floats in hex"""
    if isinstance(info, dict):
        return [(k, flat_info(info[k])) for k in sorted(info)]
    if isinstance(info, (list, tuple)):
        return [flat_info(i) for i in info]
    if isinstance(info, np.ndarray):
        return info.tobytes().hex()
    return float(info).hex() if isinstance(info, float) else info


def line(name, what, arrays, info):
    print("%-8s %-34s out %s info %s  %s" % (name, what, sha(*arrays), sha(flat_info(info)), brief(info)))


def brief(info):
    if isinstance(info, dict) and "columns" in info:
        return "iterations %s blocked %s" % ([c["iterations"] for c in info["columns"]], info["blocked"])
    if isinstance(info, dict) and "iterations" in info:
        return "iterations %s" % info["iterations"]
    return ""


def main():
    import torch  # noqa: F401  (first, as in bench.py)
    from test_energy_monitor import cloth_with_hinges
    from test_newton import _rhs, open_case
    for name in ("tet1", "mixed162", "cloth"):
        s, flat, c, tab = open_case(name)
        nv = len(c["x"])
        G = 1 if nv < 8 else 4
        rng = np.random.default_rng(7)
        rhs = _rhs(c)
        R = rng.standard_normal((17,) + c["x"].shape)
        hold = len(c["pins"]) > 0
        y, i = s.tangent_solve(rhs, c["x"], hold_pins=hold)
        line(name, "tangent_solve jacobi", [y], i)
        for coarse in ("one_block", "blocked"):
            s.set_tangent_precond("two_level", aggregates=G)
            s.set_tangent_coarse(coarse)
            y, i = s.tangent_solve(rhs, c["x"], hold_pins=hold)
            line(name, "tangent_solve two_level " + coarse, [y], i)
        s.set_tangent_coarse("one_block")
        s.set_tangent_precond("jacobi")
        for k in (2, 17):
            Y, i = s.tangent_solve_block(R[:k], c["x"], hold_pins=hold)
            line(name, "tangent_solve_block k=%d" % k, [Y], i)
        if 3 * 3 <= 3 * (nv - len(c["pins"])):
            lam, phi, i = s.modes(3, c["x"], shift=100.0, guard=0, hold_pins=hold, max_iters=200)
            line(name, "modes k=3", [lam, phi], i)
        # two steps and a polish from the case's state, then the adjoints at the polished state (the polish refuses strain limits)
        if name == "cloth":
            s.close()
            s = cloth_with_hinges(12, limits=None).make_solver()
        s.m_x[:] = c["x"].reshape(s.m_x.shape)
        s.m_v[:] = 0.0
        s.step()
        s.step()
        rec = s.newton_polish(max_iters=5)
        line(name, "newton_polish records", [s.m_x.copy(), s.m_v.copy()], rec)
        L = rng.standard_normal((3,) + c["x"].shape)
        a = s.step_adjoint(L[0], L[1])
        line(name, "step_adjoint", [a[k] for k in ("lam", "xbar", "x_prev", "v_prev", "masses", "tets", "tris", "hinges")], a["info"])
        b = s.step_adjoint_block(L, 0.5 * L)
        line(name, "step_adjoint_block k=3", [b[k] for k in ("lam", "xbar", "x_prev", "v_prev", "masses", "tets", "tris", "hinges")], b["info"])
        s.close()


if __name__ == "__main__":
    main()
