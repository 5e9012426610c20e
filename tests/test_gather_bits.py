"""The gather of the right-hand side (k_gather_rhs) keeps a vertex's whole record list in flight: indices of up to 32 records at
once, records 16 at a time.  Its sums are those of the reference instantiation -- acc += rec[e_0], rec[e_1], ... in list order,
padding included -- so after one local step the two must return the SAME BITS of b (admm_hip_regather_rhs).  Scenes: every
width from 4 up with pins (blob), a list far wider than one batch (fan), a partly empty last slice with a one-record vertex,
the triangle path (cloth), and the instantiations that read the ADMM loop's stop word."""
import numpy as np
import pytest

import admm_elastic_amd as pkg
from admm_elastic_amd import capi, meshes
from admm_elastic_amd.solver import Lame
import scenes

pytestmark = pytest.mark.gpu


def deformed(sc, amp, seed):
    rng = np.random.default_rng(seed)
    x = sc.x @ np.array([[1.15, 0.1, 0.0], [0.0, 0.9, 0.05], [0.02, 0.0, 1.05]]).T
    return (x + amp * rng.standard_normal(x.shape)).ravel()


def positive(verts, tets):
    """tets with the orientation of meshes.kuhn_cube"""
    kv, kt = meshes.kuhn_cube(1)
    sign = np.sign(meshes.tet_volumes(kv, kt)[0])
    t = np.array(tets, dtype=np.int32)
    flip = np.sign(meshes.tet_volumes(verts, t)) != sign
    t[flip] = t[flip][:, [0, 2, 1, 3]]
    return t


def fan_scene(m=48, n=46):
    """2 m n >= 4352 tets that share one apex: the apex is a corner of every tet of >= 17 chunks of 256"""
    gx, gz = np.meshgrid(np.linspace(-1.0, 1.0, m + 1), np.linspace(-1.0, 1.0, n + 1), indexing="ij")
    ring = np.stack([gx.ravel(), np.ones(gx.size), gz.ravel()], 1)
    verts = np.concatenate([np.zeros((1, 3)), ring])
    i, k = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    a = 1 + (i * (n + 1) + k).ravel(); b = a + (n + 1); c = b + 1; d = a + 1
    z = np.zeros_like(a)
    tets = positive(verts, np.concatenate([np.stack([z, a, b, c], 1), np.stack([z, a, c, d], 1)]))
    sc = scenes.Scene()
    sc.add_tet_mesh(verts, tets, Lame.soft_rubber(), pkg.TET_NEOHOOKEAN)
    for v in (1, 1 + n, verts.shape[0] - 1):
        sc.pins[int(v)] = verts[v].copy()
    return sc, tets


def ragged_scene():
    """126 vertices: the second 64-vertex slice holds 62; vertex 125 is a corner of one tet only, hence of one record"""
    verts, tets = meshes.kuhn_cube(4)
    assert verts.shape[0] == 125
    face = next(f for f in meshes.surface_faces(tets) if np.all(verts[f, 1] > 1.0 - 1e-9))
    verts = np.concatenate([verts, [verts[face].mean(axis=0) + np.array([0.0, 0.2, 0.0])]])
    tets = np.concatenate([tets, positive(verts, [[face[0], face[1], face[2], 125]])]).astype(np.int32)
    sc = scenes.Scene()
    sc.add_tet_mesh(verts, tets, Lame.soft_rubber(), pkg.TET_STVK)
    assert np.count_nonzero(tets == 125) == 1 and verts.shape[0] % 64 == 62
    return sc


def both_gathers(sc, stop_word=False, **kw):
    s = sc.make_solver(**kw)
    if stop_word:
        s.set_admm_stop(1e-3)
        s.step()          # (a step with the early exit on the device: the stop-word instantiations in their place)
    x = deformed(sc, 0.02, 5)
    u0 = 0.05 * np.random.default_rng(12).standard_normal(s.num_rows())
    Mxbar = np.random.default_rng(7).standard_normal(x.size)
    z, u, b = s.local_step(x, u0, Mxbar)
    assert np.isfinite(b).all() and np.abs(b - Mxbar).max() > 0.0
    b_new = s.regather_rhs(u0, reference=False, stop_word=stop_word)
    b_ref = s.regather_rhs(u0, reference=True, stop_word=stop_word)
    assert np.array_equal(b, b_new)            # the entry runs the step's schedule on the step's inputs
    assert np.array_equal(b_new, b_ref), np.abs(b_new - b_ref).max()
    assert np.array_equal(b, b_ref)
    # ... and leaves the context as the local step left it
    assert np.array_equal(s.regather_rhs(u0), b_new)
    return s


def test_blob_with_pins():
    sc = scenes.blob_scene(30)
    assert len(sc.pins) > 0
    both_gathers(sc)


def test_fan_list_wider_than_one_batch():
    sc, tets = fan_scene()
    assert len(tets) >= 4352
    _, st = capi.chunk_reduce(len(sc.x), tets, [0, 0, len(tets), len(tets), len(tets), len(tets)], np.zeros((len(tets), 4, 3)))
    assert st["chunks"] >= 17 and st["max_list"] > 32, st      # more than the 32 indices of one batch, from >= 17 chunks
    both_gathers(sc)


def test_partly_empty_last_slice_and_single_record():
    both_gathers(ragged_scene())


def test_cloth_triangle_path():
    both_gathers(scenes.cloth_scene(30))


def test_stop_word_instantiation():
    sc = scenes.mixed_cube_scene(6, admm_iters=5)
    s = both_gathers(sc, stop_word=True)
    assert s.admm_stop()["tol"] == 1e-3
