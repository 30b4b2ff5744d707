"""The NumPy restatement of the StVK membrane (tests/stvk_numpy.py) checked on its own: derivatives against central differences, invariance
under rigid motions, and the rest triangle rebuilt from three lengths."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stvk_numpy as sn  # noqa: E402


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _face(rng):
    l = np.array([1.0, 1.3, 0.8]) * (1 + 0.1 * rng.random(3))
    Di = sn.dminv_from_lengths(*l)
    X = np.zeros((3, 3))
    X[:, :2] = np.array([[0.0, 0.0], [l[0], 0.0], sn.dm_from_lengths(*l)[:, 1]])
    return X, Di


def test_gradient_and_hessian_match_central_differences():
    rng = np.random.default_rng(0)
    X, Di = _face(rng)
    x = X + 0.2 * rng.normal(size=(3, 3))
    mu, lam, A0 = 3.0e5, 2.0e5, 0.37
    g = sn.face_grad(x, Di, A0, mu, lam)
    H = sn.face_hess(x, Di, A0, mu, lam)
    h = 1e-6
    gfd = np.zeros(9); Hfd = np.zeros((9, 9))
    for k in range(9):
        d = np.zeros(9); d[k] = h
        xp, xm = x + d.reshape(3, 3), x - d.reshape(3, 3)
        gfd[k] = (sn.face_energy(xp, Di, A0, mu, lam) - sn.face_energy(xm, Di, A0, mu, lam)) / (2 * h)
        Hfd[:, k] = (sn.face_grad(xp, Di, A0, mu, lam) - sn.face_grad(xm, Di, A0, mu, lam)).ravel() / (2 * h)
    assert np.abs(g.ravel() - gfd).max() <= 1e-7 * np.abs(g).max()
    assert np.abs(H - Hfd).max() <= 1e-7 * np.abs(H).max()
    assert np.allclose(H, H.T, rtol=0, atol=1e-12 * np.abs(H).max())


def test_rigid_motions_of_the_rest_shape_have_no_energy_or_gradient():
    rng = np.random.default_rng(1)
    f2v, X, li, V = sn.grid_cloth(4, 0.01)
    Dis = sn.dminv_all(li)
    for _ in range(3):
        x = X @ _rot(rng).T + rng.normal(size=3)
        assert abs(sn.energy(x, f2v, Dis, V, 3e5, 2e5)) < 1e-18
        assert np.abs(sn.gradient(x, f2v, Dis, V, 3e5, 2e5)).max() < 1e-9


def test_dm_from_lengths_reproduces_the_rest_triangle():
    rng = np.random.default_rng(2)
    for _ in range(20):
        P = rng.normal(size=(3, 3))
        l = [np.linalg.norm(P[0] - P[1]), np.linalg.norm(P[1] - P[2]), np.linalg.norm(P[2] - P[0])]
        Dm = sn.dm_from_lengths(*l)
        X0, X1, X2 = np.zeros(2), Dm[:, 0], Dm[:, 1]
        assert np.isclose(np.linalg.norm(X0 - X1), l[0], rtol=1e-13)
        assert np.isclose(np.linalg.norm(X1 - X2), l[1], rtol=1e-13)
        assert np.isclose(np.linalg.norm(X2 - X0), l[2], rtol=1e-13)
        assert Dm[1, 1] > 0
        # F of the triangle itself is an isometry: F^T F = I
        F = np.stack([P[1] - P[0], P[2] - P[0]], 1) @ np.linalg.inv(Dm)
        assert np.allclose(F.T @ F, np.eye(2), atol=1e-12)


def test_uniform_deformation_energy_is_area_times_psi_and_clamped_hessian_is_psd():
    rng = np.random.default_rng(3)
    f2v, X, li, V = sn.grid_cloth(3, 0.02)
    Dis = sn.dminv_all(li)
    Fh = np.eye(3, 2) + 0.2 * rng.normal(size=(3, 2))
    x = X[:, :2] @ Fh.T
    e = sn.energy(x, f2v, Dis, V, 3e5, 2e5)
    assert np.isclose(e, V.sum() * sn.psi(Fh, 3e5, 2e5), rtol=1e-12)
    xc = X.copy(); xc[:, 0] *= 0.7   # compressed: the exact block is indefinite, the clamped one is not
    assert np.linalg.eigvalsh(sn.hessian(xc, f2v, Dis, V, 3e5, 2e5)).min() < 0
    w = np.linalg.eigvalsh(sn.hessian(xc, f2v, Dis, V, 3e5, 2e5, clamp=True))
    assert w.min() >= -1e-10 * w.max()
