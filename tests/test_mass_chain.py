"""meshes.lumped_masses_tets_grad, the chain rule of lumped_masses_tets, against central differences on kuhn_cube(2) with jittered
vertices.  The masses are cubic in X, so the central difference at h is exact up to c h^2 and Richardson's (4 q(h / 2) - q(h)) / 3
removes that term exactly: what is left is rounding.  Asserted relative 1e-9 (of the gradient's largest entry)."""
import numpy as np

from admm_elastic_amd import meshes


def test_lumped_masses_gradient_against_richardson():
    """Measured: 1.3e-11 of the largest entry."""
    verts, tets = meshes.kuhn_cube(2)
    rng = np.random.default_rng(89)
    verts = verts + 0.05 * rng.standard_normal(verts.shape)
    w = rng.standard_normal(len(verts))      # L = w . m
    g = meshes.lumped_masses_tets_grad(verts, tets, w)
    assert g.shape == verts.shape
    loss = lambda X: float(np.dot(w, meshes.lumped_masses_tets(X, tets)))

    def quotient(h):
        q = np.zeros(verts.shape)
        for v in range(len(verts)):
            for j in range(3):
                Xp, Xm = verts.copy(), verts.copy()
                Xp[v, j] += h; Xm[v, j] -= h
                q[v, j] = (loss(Xp) - loss(Xm)) / (2.0 * h)
        return q
    h = 1e-2
    rich = (4.0 * quotient(0.5 * h) - quotient(h)) / 3.0
    err = np.abs(g - rich).max() / np.abs(rich).max()
    print("lumped_masses_tets_grad against Richardson(h = %.0e): %.3e of the largest entry (bar 1e-9)" % (h, err))
    assert err <= 1e-9, err
    # another density scales the gradient; the gradient of the total mass in a translation is 0
    assert np.allclose(meshes.lumped_masses_tets_grad(verts, tets, w, density=2.0), g * (2.0 / 1522.0), rtol=1e-14, atol=0.0)
    assert np.abs(meshes.lumped_masses_tets_grad(verts, tets, np.ones(len(verts))).sum(axis=0)).max() <= 1e-9 * np.abs(g).max()
