"""tests/berr.py, the yardstick of the first-pass tests (test_gpu_direct_first_pass.py): its long-double backward errors against mpmath at
50 digits, and a planted perturbation of known size reported back within a factor of 2."""
import mpmath
import numpy as np
import pytest
import scipy.sparse as sp

import berr


def _system(n, seed, density=0.2):
    rng = np.random.default_rng(seed)
    H = sp.random(n, n, density=density, random_state=rng, format="csr") * 10.0 ** rng.uniform(-3, 3)
    H = H + sp.diags(rng.uniform(1.0, 4.0, n) * (abs(H).sum(axis=1).A1 + 1.0))
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 5)
    return sp.csr_matrix(H), b


def _mp(v):
    return [mpmath.mpf(float(t)) for t in v]


def _mp_berrs(H, x, b):
    """both backward errors at 50 significant digits (the float64 entries are exact in mpmath)"""
    with mpmath.workdps(50):
        n = H.shape[0]
        xm, bm = _mp(x), _mp(b)
        Hc = H.tocsr()
        r, absrow, den_c = [], [], []
        for i in range(n):
            acc, accabs, accx = mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0)
            for q in range(Hc.indptr[i], Hc.indptr[i + 1]):
                h = mpmath.mpf(float(Hc.data[q])); j = Hc.indices[q]
                acc += h * xm[j]; accabs += abs(h); accx += abs(h) * abs(xm[j])
            r.append(bm[i] - acc); absrow.append(accabs); den_c.append(accx + abs(bm[i]))
        n2 = lambda v: mpmath.sqrt(mpmath.fsum(t * t for t in v))
        nw = n2(r) / (max(absrow) * n2(xm) + n2(bm))
        cw = max(abs(r[i]) / den_c[i] for i in range(n))
        return float(nw), float(cw)


@pytest.mark.parametrize("n,seed", [(5, 0), (17, 1), (33, 2), (60, 3)])
def test_berr_matches_mpmath(n, seed):
    H, b = _system(n, seed)
    x = np.linalg.solve(H.toarray(), b)                          # a float64 answer: backward errors of a few ulps
    x_far = x * (1 + 1e-9 * np.random.default_rng(seed).standard_normal(n))
    for xx in (x, x_far):
        nw, cw = _mp_berrs(H, xx, b)
        assert nw > 0 and cw > 0
        # the long-double residual carries ~11 digits more than float64: the helper is right to a few 1e-3 of a value of 1e-17
        assert abs(berr.normwise_berr(H, xx, b) - nw) <= 1e-3 * nw + 1e-30, (berr.normwise_berr(H, xx, b), nw)
        assert abs(berr.componentwise_berr(H, xx, b) - cw) <= 1e-3 * cw + 1e-30, (berr.componentwise_berr(H, xx, b), cw)
    with mpmath.workdps(50):
        assert abs(float(berr.inf_norm(H)) - float(max(mpmath.fsum(abs(mpmath.mpf(float(v))) for v in H.getrow(i).data) for i in range(n)))) \
            <= 1e-15 * float(berr.inf_norm(H))


@pytest.mark.parametrize("n,seed,delta", [(40, 4, 1e-9), (60, 5, 1e-13), (25, 6, 1e-6)])
def test_berr_reports_a_planted_perturbation(n, seed, delta):
    """x = H^-1 b exactly (in long double), then x + dx with H dx sized so the backward error IS delta: the helper reports it within 2x"""
    H, _ = _system(n, seed)
    rng = np.random.default_rng(seed + 100)
    x_true = rng.standard_normal(n)
    b = np.asarray(berr._csr(H) @ x_true.astype(berr.LD), dtype=np.float64)
    xt = berr.x_ref(H, b)
    assert berr.normwise_berr(H, xt, b) < 1e-16 and berr.componentwise_berr(H, xt, b) < 1e-15     # (x rounded to float64)
    Hn = float(berr.inf_norm(H))
    # normwise: a residual of norm delta (|H| |x| + |b|) along a random direction
    rdir = rng.standard_normal(n); rdir /= np.linalg.norm(rdir)
    target = delta * (Hn * np.linalg.norm(xt) + np.linalg.norm(b))
    dx = np.linalg.solve(H.toarray(), -target * rdir)            # H (xt + dx) = b - target * rdir
    got = berr.normwise_berr(H, xt + dx, b)
    assert delta / 2 <= got <= 2 * delta, (got, delta)
    # componentwise: every residual component delta (|H||x| + |b|)_i, signs random
    den = abs(H) @ np.abs(xt) + np.abs(b)
    dx = np.linalg.solve(H.toarray(), -delta * den * rng.choice([-1.0, 1.0], n))
    got = berr.componentwise_berr(H, xt + dx, b)
    assert delta / 2 <= got <= 2 * delta, (got, delta)


def test_x_ref_is_refined():
    """x_ref beats plain SuperLU on an ill-conditioned system (cond 1e7): the FORWARD error against mpmath's solution at 40 digits is that of
    cond x the long-double eps (1e-12), where SuperLU's is cond x the double eps"""
    import scipy.sparse.linalg as spl
    n = 40
    rng = np.random.default_rng(9)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, -7, n)) @ Q.T
    H = sp.csr_matrix(A)
    b = rng.standard_normal(n)
    with mpmath.workdps(40):
        xm = mpmath.lu_solve(mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in A]), mpmath.matrix(_mp(b)))
        xm = np.array([float(t) for t in xm])
    fe = lambda x: np.abs(x - xm).max() / np.abs(xm).max()
    x0 = spl.splu(sp.csc_matrix(H)).solve(b)
    xr = berr.x_ref(H, b)
    assert fe(xr) < 1e-11 and fe(x0) > 100 * fe(xr), (fe(xr), fe(x0))
