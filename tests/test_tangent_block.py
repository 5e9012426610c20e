"""Tangent solves for a stack of right-hand sides (csrc/newton.hpp: the block PCG): tangent_solve_block and step_adjoint_block against
the single calls, bit for bit.

The block PCG runs k independent CG recurrences that share every launch; a column that has ended leaves the launches through a column
list kept on the device.  The yardstick of every test here is therefore the single call on the same column: y, lam, every gradient and
every info field are compared with == on the bits.

THE COLUMNS (columns()) are built to end at different times: M o (an affine displacement), a zero column, a unit load on one free
vertex, a column supported on the held vertices only (zero once the pins are held; a tiny random one on a body without pins), and
random columns r scaled 1e-6 .. 1e6, every second one replaced by A^m r, m = 1 .. 4, A = K_psd(x) + M / dt^2 with the pins held (through
stiffness_apply_ex).  A right-hand side A^m r carries little of the soft end of the spectrum, which is what a CG with a stop test
relative to |rhs| spends its last iterations on: such a column ends well before a random one.  Columns of another content (affine,
unit load, random at any scale) end within a few per cent of each other.

Cases: tet1 (4 vertices, one block), mixed162 (pins), cloth (the triangle and hinge ranges of the block pass) and the 13^3-cell mixed
cube (2 744 vertices = 11 vertex blocks: xcd_block's remainder path, nw_reduce over several partials)."""
import functools

import numpy as np
import pytest

import admm_elastic_amd as pkg
import scenes
from admm_elastic_amd import capi
from test_adjoint import NH, polished
from test_newton import _rhs, compressed_state, dense_K, free_mask, open_case, reference

gpu = pytest.mark.gpu
ERR_ARG = -1


# ---------------------------------------------------------------- cases and columns ------------------------------------------------
def open_block_case(name):
    """open_case of test_newton.py, plus "cube13": scenes.mixed_cube_scene(13) at its compressed state -> (solver, case dict)"""
    if name != "cube13":
        s, flat, c, tab = open_case(name)
        return s, c
    sc = scenes.mixed_cube_scene(13)
    return sc.make_solver(), dict(rest=sc.x, x=compressed_state(sc.x, 13), pins=sorted(sc.pins))


def columns(s, c, k, seed=53):
    """[k, n_verts, 3]: the column kinds of the module docstring, in an order that mixes them at every k"""
    rest = np.asarray(c["rest"], dtype=np.float64)
    nv = len(rest)
    fm = free_mask(c)
    m = np.asarray(s.m_masses, dtype=np.float64).reshape(nv, 3)
    rng = np.random.default_rng(seed)
    A = np.eye(3) * 0.1 + 0.05 * rng.standard_normal((3, 3))
    affine = m * (rest @ A + np.array([0.02, -0.01, 0.03]))
    unit = np.zeros((nv, 3)); unit[int(np.nonzero(fm)[0][-1]), 1] = 1.0
    held = np.zeros((nv, 3))
    if (~fm).any():
        held[~fm] = rng.standard_normal((int((~fm).sum()), 3))
    else:
        held = 1e-9 * rng.standard_normal((nv, 3))
    out = [affine, np.zeros((nv, 3)), unit, held]
    scales = 10.0 ** np.linspace(-6.0, 6.0, max(k - 4, 2))
    shift = 1.0 / s._settings.timestep_s ** 2
    j = 0
    while len(out) < k:
        r = rng.standard_normal((nv, 3))
        for _ in range((1 + j // 2 % 4) if j % 2 == 1 else 0):      # A^m r, m = 1 .. 4: the soft end of the spectrum is damped in it
            r = s.stiffness_apply_ex(r, c["x"], shift=shift, psd=True, hold_pins=True)
            r /= np.abs(r).max()
        out.append(scales[j % len(scales)] * r)
        j += 1
    return np.ascontiguousarray(np.stack(out[:k]))


def singles(s, rhs, x, **kw):
    return [s.tangent_solve(r, x, **kw) for r in rhs]


def broke(info, max_iters):
    """the column ended in a CG breakdown: not converged, short of max_iters, a right-hand side that is not zero"""
    return (not info["converged"]) and info["iterations"] < max_iters and info["rhs_norm"] > 0.0


def assert_columns_equal(Y, info, ref, what):
    for j, (y1, i1) in enumerate(ref):
        assert Y[j].tobytes() == y1.tobytes(), (what, j, float(np.abs(Y[j] - y1).max()))
        assert info["columns"][j] == i1, (what, j, info["columns"][j], i1)


def assert_column_list(info, max_iters):
    cols = info["columns"]
    ends = [i["iterations"] + (1 if broke(i, max_iters) else 0) for i in cols]
    assert info["blocked"]
    assert info["column_passes"] == sum(ends), (info["column_passes"], ends)
    assert info["block_iterations"] == max(ends), (info["block_iterations"], ends)


# ---------------------------------------------------------------- 1, 2: column = single solve; the column list ---------------------
@gpu
@pytest.mark.parametrize("name,ks", [("tet1", (1, 2, 16, 17)), ("mixed162", (1, 2, 16, 17)), ("cloth", (2, 16)), ("cube13", (16, 17))])
def test_every_column_is_its_single_solve(name, ks):
    """Y[j] and every info field of column j (iterations, converged, residual, rhs_norm) equal tangent_solve(rhs[j]) called alone, on
    the bits; column_passes == sum_j (iterations_j + [column j ended by breakdown]) and block_iterations == max_j of the same; for
    k = 17 (two slabs: 16 columns and 1) block_iterations is the longer slab's.  On cube13 the inputs are asserted to exercise the
    list: the single solves' iteration counts take at least three distinct positive values and the smallest positive one is below
    0.7 of the largest."""
    s, c = open_block_case(name)
    tol, max_iters = 1e-10, (4000 if name == "cube13" else 1000)
    for k in ks:
        rhs = columns(s, c, k)
        ref = singles(s, rhs, c["x"], tol=tol, max_iters=max_iters)
        Y, info = s.tangent_solve_block(rhs, c["x"], tol=tol, max_iters=max_iters)
        its = [i["iterations"] for _, i in ref]
        print("%s k = %d: iterations %s, block_iterations %d, column_passes %d" % (name, k, its, info["block_iterations"], info["column_passes"]))
        assert_columns_equal(Y, info, ref, (name, k))
        if k <= 16:
            assert_column_list(info, max_iters)
        else:
            ends = [i["iterations"] + (1 if broke(i, max_iters) else 0) for i in info["columns"]]
            assert info["column_passes"] == sum(ends) and info["block_iterations"] == max(max(ends[:16]), max(ends[16:]))
        if name == "cube13" and k == 16:
            pos = sorted(set(i for i in its if i > 0))
            assert len(pos) >= 3 and pos[0] < 0.7 * pos[-1], ("the columns do not end at different times: the list is not exercised", its)
        Y2, info2 = s.tangent_solve_block(rhs, c["x"], tol=tol, max_iters=max_iters)      # a second call has the bits
        assert Y2.tobytes() == Y.tobytes() and info2 == info
    s.close()


@gpu
def test_a_zero_solve_after_a_solve_that_ended_on_an_odd_iteration():
    """A right-hand side of zero ends at the set-up of the solve: 0 iterations, y = 0, residual 0, rhs_norm 0 -- also when the solve
    before it left its scalars behind at any parity (solves of 1 .. 6 iterations before it), single and block."""
    s, c = open_block_case("mixed162")
    rhs = _rhs(c)
    zero = np.zeros_like(rhs)
    want = dict(iterations=0, converged=True, residual=0.0, rhs_norm=0.0)
    for n in range(1, 7):
        _, i0 = s.tangent_solve(rhs, c["x"], tol=1e-12, max_iters=n)
        assert i0["iterations"] == n
        y, i1 = s.tangent_solve(zero, c["x"])
        assert i1 == want and not y.any(), (n, i1)
        s.tangent_solve_block(np.stack([rhs, 0.5 * rhs]), c["x"], tol=1e-12, max_iters=n)
        Y, ib = s.tangent_solve_block(np.stack([zero, zero]), c["x"])
        assert ib["columns"] == [want, want] and not Y.any() and ib["column_passes"] == 0 and ib["block_iterations"] == 0, (n, ib)
    s.close()


# ---------------------------------------------------------------- 3: breakdown and cap per column -----------------------------------
@functools.lru_cache(None)
def indefinite_shift(f=0.5):
    """the construction of test_newton.test_tangent_solve_breakdown_returns_the_iterate_before_it: shift = -f mu_min of the pencil (K, M)
    on the free rows of the unprojected dense matrix of mixed162"""
    s, flat, c, tab = open_case("mixed162")
    f3 = np.repeat(free_mask(c), 3)
    K0 = dense_K(flat, c["rest"], c["x"], psd=False)[np.ix_(f3, f3)]
    isq = 1.0 / np.sqrt(np.asarray(s.m_masses, dtype=np.float64)[f3])
    s.close()
    mu = np.linalg.eigvalsh(K0 * isq[:, None] * isq[None, :])
    assert mu[0] < 0.0
    return -f * mu[0]


@gpu
def test_breakdown_and_cap_per_column():
    """mixed162, psd=False, shift = -0.5 mu_min: eight columns (zero, held vertices only, six random ones scaled 1e-6 .. 1e6).  Every
    column equals its single solve on the bits; the reported residual is that of the returned y (recomputed through stiffness_apply_ex,
    1e-6 relative): the iterate before the breakdown; asserted of the inputs: at least one column ends unconverged after >= 1
    iterations and before max_iters.  With max_iters = 3 every column that is not zero reports 3 iterations and converged = False."""
    s, c = open_block_case("mixed162")
    fm = free_mask(c)
    shift = indefinite_shift()
    rng = np.random.default_rng(59)
    nv = len(c["rest"])
    held = np.zeros((nv, 3)); held[~fm] = rng.standard_normal((int((~fm).sum()), 3))
    rhs = np.stack([np.zeros((nv, 3)), held] + [sc * rng.standard_normal((nv, 3)) for sc in 10.0 ** np.linspace(-6.0, 6.0, 6)])
    kw = dict(shift=shift, psd=False, tol=1e-10, max_iters=400)
    ref = singles(s, rhs, c["x"], **kw)
    Y, info = s.tangent_solve_block(rhs, c["x"], **kw)
    print("breakdown: %s; block_iterations %d, column_passes %d" % ([(i["iterations"], i["converged"]) for _, i in ref], info["block_iterations"], info["column_passes"]))
    assert_columns_equal(Y, info, ref, "breakdown")
    assert_column_list(info, 400)
    AY = s.stiffness_apply_ex(Y, c["x"], shift=shift, hold_pins=True, block=True)
    for j, i in enumerate(info["columns"]):
        assert np.isfinite(Y[j]).all() and (Y[j][~fm] == 0.0).all()
        rn = np.linalg.norm(rhs[j][fm])
        if rn > 0.0:
            rel = np.linalg.norm((rhs[j] - AY[j])[fm]) / rn
            assert abs(i["residual"] - rel) <= 1e-6 * rel, (j, i["residual"], rel)
    assert any(broke(i, 400) and i["iterations"] >= 1 for i in info["columns"]), "no column broke down after its first iteration: the path is not exercised"
    kw["max_iters"] = 3
    ref3 = singles(s, rhs, c["x"], **kw)
    Y3, info3 = s.tangent_solve_block(rhs, c["x"], **kw)
    assert_columns_equal(Y3, info3, ref3, "max_iters = 3")
    for j, i in enumerate(info3["columns"]):
        if i["rhs_norm"] > 0.0:
            assert i["iterations"] == 3 and not i["converged"], (j, i)
    assert info3["block_iterations"] == 3
    s.close()


# ---------------------------------------------------------------- 4: against a dense solve -----------------------------------------
@gpu
def test_block_solve_against_dense_solve():
    """mixed162: every column against numpy.linalg.solve of the assembled projected reference + shift M on the free rows, at the bar of
    test_newton.test_tangent_solve_against_dense_solve: |y - y_ref| <= 1e-6 kappa |y_ref|."""
    name = "mixed162"
    s, c = open_block_case(name)
    _, K, _ = reference(name)
    fm = np.repeat(free_mask(c), 3)
    shift = 1.0 / s._settings.timestep_s ** 2
    A = (K + shift * np.diag(s.m_masses))[np.ix_(fm, fm)]
    kappa = np.linalg.cond(A)
    rhs = columns(s, c, 8)
    Y, info = s.tangent_solve_block(rhs, c["x"], tol=1e-12, max_iters=2000)
    s.close()
    for j in range(len(rhs)):
        b = rhs[j].ravel()[fm]
        if not b.any():
            assert not Y[j].any()
            continue
        ref = np.linalg.solve(A, b)
        err = np.linalg.norm(Y[j].ravel()[fm] - ref) / np.linalg.norm(ref)
        print("column %d: |y - y_ref| / |y_ref| = %.3e (bar 1e-6 kappa = %.3e), %d iterations" % (j, err, 1e-6 * kappa, info["columns"][j]["iterations"]))
        assert info["columns"][j]["converged"]
        assert err <= 1e-6 * kappa, (j, err, kappa)


# ---------------------------------------------------------------- 5: the adjoint ---------------------------------------------------
VEC = ("lam", "xbar", "x_prev", "v_prev", "masses", "tets", "tris", "hinges")


@gpu
def test_step_adjoint_block_is_five_step_adjoints():
    """After a step and the polish on the 162-tet cantilever of test_adjoint.py: step_adjoint_block with k = 5 losses (dL_dv given)
    equals five step_adjoint calls on the bits in lam, xbar, x_prev, v_prev, masses, tets, tris, hinges and every info field; with
    rest=True, held=True also in rest and held; a step_adjoint call afterwards returns the bits of one made before."""
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished("cantilever162")
    rng = np.random.default_rng(67)
    k = 5
    Lx = rng.standard_normal((k,) + sc.x.shape) * (10.0 ** np.arange(-2, 3))[:, None, None]
    Lv = rng.standard_normal((k,) + sc.x.shape)
    Lx[3] = 0.0; Lv[3] = 0.0      # a loss that does not depend on the state: its column ends at the set-up
    kw = dict(tol=1e-11, max_iters=3000)
    before = [s.step_adjoint(Lx[j], Lv[j], rest=True, held=True, **kw) for j in range(k)]
    out = s.step_adjoint_block(Lx, Lv, rest=True, held=True, **kw)
    plain = s.step_adjoint_block(Lx, Lv, **kw)
    after = s.step_adjoint(Lx[0], Lv[0], rest=True, held=True, **kw)
    s.close()
    assert out["info"]["blocked"] and "rest" not in plain and "held" not in plain
    print("adjoint: iterations %s, block_iterations %d, column_passes %d" % ([i["iterations"] for i in out["info"]["columns"]],
                                                                              out["info"]["block_iterations"], out["info"]["column_passes"]))
    for j in range(k):
        for key in VEC + ("rest", "held"):
            assert out[key][j].tobytes() == before[j][key].tobytes(), (j, key)
            if key in VEC:
                assert plain[key][j].tobytes() == before[j][key].tobytes(), (j, key)
        assert out["info"]["columns"][j] == before[j]["info"], (j, out["info"]["columns"][j], before[j]["info"])
    assert plain["info"] == out["info"]
    assert out["info"]["columns"][3]["iterations"] == 0 and not out["lam"][3].any()
    assert_column_list(dict(out["info"]), 3000)
    for key in VEC + ("rest", "held"):
        assert after[key].tobytes() == before[0][key].tobytes(), key
    assert after["info"] == before[0]["info"]


# ---------------------------------------------------------------- 6: nothing else moves --------------------------------------------
@gpu
def test_block_solves_do_not_disturb_a_run():
    """3 frames of the on-chip PCG (k_pcg2) with tangent_solve_block and step_adjoint_block between the frames: m_x and m_v
    bit-identical to the same run without those calls."""
    out = []
    for probe in (False, True):
        sc = scenes.mixed_cube_scene(3, linsolver=0)
        s = sc.make_solver()
        xs = []
        for _ in range(3):
            s.step()
            xs.append(s.m_x.copy()); xs.append(s.m_v.copy())
            if probe:
                xp = compressed_state(sc.x, 3)
                R = np.stack([np.ones_like(xp), np.zeros_like(xp), scenes.perturb(xp, 1.0, 3)])
                Y, info = s.tangent_solve_block(R, xp, tol=1e-8)
                assert np.isfinite(Y).all() and info["blocked"]
                o = s.step_adjoint_block(R, 0.5 * R, tol=1e-8)
                assert np.isfinite(o["lam"]).all() and np.isfinite(o["tets"]).all()
        out.append(np.concatenate(xs))
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


@gpu
def test_modes_and_block_apply_keep_their_bits():
    """modes() and stiffness_apply_ex(block=True) after a block solve (which shares the block pass, its scratch and its argument
    structures with them) return the bits they returned before it."""
    s, c = open_block_case("mixed162")
    D = columns(s, c, 6, seed=71)
    a0 = s.stiffness_apply_ex(D, c["x"], shift=3.0, psd=True, hold_pins=True, block=True)
    lam0, phi0, i0 = s.modes(3, c["x"], tol=1e-6, max_iters=200)
    s.tangent_solve_block(columns(s, c, 16), c["x"], tol=1e-10)
    a1 = s.stiffness_apply_ex(D, c["x"], shift=3.0, psd=True, hold_pins=True, block=True)
    lam1, phi1, i1 = s.modes(3, c["x"], tol=1e-6, max_iters=200)
    s.close()
    assert a1.tobytes() == a0.tobytes()
    assert lam1.tobytes() == lam0.tobytes() and phi1.tobytes() == phi0.tobytes()
    assert i1["iterations"] == i0["iterations"] and i1["residual"].tobytes() == i0["residual"].tobytes()


# ---------------------------------------------------------------- 7: the two-level fallback ----------------------------------------
@gpu
def test_two_level_fallback():
    """With set_tangent_precond("two_level") the block entry points solve column after column: blocked is False and each column equals
    the single two-level solve on the bits (solve and adjoint); back on "jacobi" the block solve is blocked again."""
    s, c = open_block_case("mixed162")
    s.set_tangent_precond("two_level", 4)
    rhs = columns(s, c, 6)
    ref = singles(s, rhs, c["x"], tol=1e-10)
    Y, info = s.tangent_solve_block(rhs, c["x"], tol=1e-10)
    assert not info["blocked"] and s.tangent_precond()["coarse_dim"] > 0
    assert_columns_equal(Y, info, ref, "two_level")
    assert info["block_iterations"] == max(i["iterations"] for _, i in ref) and info["column_passes"] == sum(i["iterations"] for _, i in ref)
    s.set_tangent_precond("jacobi")
    Yj, infoj = s.tangent_solve_block(rhs, c["x"], tol=1e-10)
    assert infoj["blocked"]
    assert_columns_equal(Yj, infoj, singles(s, rhs, c["x"], tol=1e-10), "jacobi again")
    s.close()
    sc, s, rec, x_prev, xbar, fm, m3, tri_k, grad_tol = polished("cantilever162")
    s.set_tangent_precond("two_level", 4)
    rng = np.random.default_rng(73)
    Lx = rng.standard_normal((3,) + sc.x.shape)
    before = [s.step_adjoint(Lx[j], tol=1e-11) for j in range(3)]
    out = s.step_adjoint_block(Lx, tol=1e-11)
    s.close()
    assert not out["info"]["blocked"]
    for j in range(3):
        for key in VEC:
            assert out[key][j].tobytes() == before[j][key].tobytes(), (j, key)
        assert out["info"]["columns"][j] == before[j]["info"]


# ---------------------------------------------------------------- 8: refusals ------------------------------------------------------
@gpu
def test_block_refusals():
    """tangent_solve_block / step_adjoint_block refuse what tangent_solve / step_adjoint refuse, with the same codes: multi-GPU
    settings; for the adjoint colliders, strain-limited triangles, slide pins and a state no step has run on; k < 1 and bad shapes."""
    def same_refusal(call_single, call_block):
        with pytest.raises(capi.AdmmHipError) as e1:
            call_single()
        with pytest.raises(capi.AdmmHipError) as e2:
            call_block()
        assert e2.value.code == e1.value.code, (e1.value, e2.value)

    def adjoint_refused(s):
        x0, v0 = s.m_x.copy(), s.m_v.copy()
        n = s.m_x.size // 3
        same_refusal(lambda: s.step_adjoint(np.ones((n, 3))), lambda: s.step_adjoint_block(np.ones((2, n, 3))))
        s.download()
        assert s.m_x.tobytes() == x0.tobytes() and s.m_v.tobytes() == v0.tobytes()
        s.close()
    s = scenes.cloth_scene(6, limits=None, floor=-1.0, linsolver=1).make_solver(); s.step(); adjoint_refused(s)      # a floor
    s = scenes.cloth_scene(6).make_solver(); s.step(); adjoint_refused(s)                              # strain-limited triangles
    sc = scenes.cloth_scene(6, limits=None); sc.slides[3] = (sc.x[3].copy(), np.array([0.0, 1.0, 0.0]))
    s = sc.make_solver(); s.step(); adjoint_refused(s)                                                 # slide pins
    s = scenes.cube_scene(2, NH).make_solver(); s.upload(); adjoint_refused(s)                         # before its first step
    sc = scenes.cube_scene(2, NH)
    s = sc.make_solver(world_size=2, rank=0)                                                           # multi-GPU settings
    n = len(sc.x)
    same_refusal(lambda: s.tangent_solve(np.ones((n, 3)), sc.x), lambda: s.tangent_solve_block(np.ones((2, n, 3)), sc.x))
    same_refusal(lambda: s.step_adjoint(np.ones((n, 3))), lambda: s.step_adjoint_block(np.ones((2, n, 3))))
    s.close()
    s = sc.make_solver()
    same_refusal(lambda: s.tangent_solve(np.ones((n, 3))), lambda: s.tangent_solve_block(np.ones((2, n, 3))))      # no state, x=None
    s.step()
    for bad in (np.ones((n, 3)), np.ones((2, n + 1, 3)), np.ones((2, n, 2)), np.ones((0, n, 3)), np.ones(6 * n)):
        with pytest.raises(ValueError):
            s.tangent_solve_block(bad, sc.x)
        with pytest.raises(ValueError):
            s.step_adjoint_block(bad)
    with pytest.raises(ValueError):
        s.step_adjoint_block(np.ones((2, n, 3)), np.ones((3, n, 3)))
    L = capi.lib()
    one = np.ones(3 * n); y = np.zeros(3 * n); i4 = np.zeros(4); i6 = np.zeros(6); b3 = np.zeros(3)
    d = capi.dptr
    for k in (0, -1):
        assert L.admm_hip_tangent_solve_block(s._ctx, None, k, d(one), 1.0, 3, 1e-10, 100, d(y), d(i4), d(b3)) == ERR_ARG
        assert L.admm_hip_step_adjoint_block(s._ctx, k, d(one), None, 0, 1e-10, 100, *([None] * 8), d(i6), d(b3)) == ERR_ARG
    assert L.admm_hip_tangent_solve_block(s._ctx, None, 1, d(one), 1.0, 4, 1e-10, 100, d(y), d(i4), d(b3)) == ERR_ARG      # unknown flag
    assert L.admm_hip_tangent_solve_block(s._ctx, None, 1, d(one), 1.0, 3, -1.0, 100, d(y), d(i4), d(b3)) == ERR_ARG       # tol < 0
    assert L.admm_hip_tangent_solve_block(s._ctx, None, 1, d(one), 1.0, 3, 1e-10, 0, d(y), d(i4), d(b3)) == ERR_ARG        # max_iters < 1
    assert L.admm_hip_step_adjoint_block(s._ctx, 1, d(one), None, 4, 1e-10, 100, *([None] * 8), d(i6), d(b3)) == ERR_ARG   # unknown flag
    assert L.admm_hip_step_adjoint_block(s._ctx, 1, d(one), None, 0, 1e-10, 100, *([None] * 8), d(i6), None) == ERR_ARG    # no block_info
    s.close()


@gpu
def test_block_buffers_are_freed_with_the_context():
    """a closed context leaves no device buffer behind after block solves of 2, then 17 columns (the buffers grow once)"""
    import ctypes as C
    n0, n1 = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n0), None))
    sc = scenes.cube_scene(3, NH, admm_iters=4)
    s = sc.make_solver()
    s.step()
    for k in (2, 17):
        s.tangent_solve_block(np.ones((k,) + sc.x.shape), tol=1e-8)
        s.step_adjoint_block(np.ones((k,) + sc.x.shape), tol=1e-8)
    s.close()
    capi.check(capi.lib().admm_hip_device_buffers(C.byref(n1), None))
    assert n1.value == n0.value, (n0.value, n1.value)
