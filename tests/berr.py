"""High-precision backward errors of a linear solve, computed on the host (test infrastructure).

The residual r = b - H x and the norms are formed in np.longdouble (80-bit extended on x86: 64-bit significand), so the rounding of the
check itself stays three decades below the errors it measures.  normwise_berr is the engine's own definition of
tsl_solve_stats.backward_error, |b - Hx|_2 / (|H|_inf |x|_2 + |b|_2); componentwise_berr is the Oettli-Prager value."""
import numpy as np
import scipy.sparse as sp

# without an extended long double every quantity below would be rounded like the solve it checks: fail loudly instead of measuring nothing
assert np.finfo(np.longdouble).eps < 1e-18, "tests/berr.py needs an 80-bit (or wider) np.longdouble"

LD = np.longdouble


def _csr(H):
    H = sp.csr_matrix(H)
    return sp.csr_matrix((H.data.astype(LD), H.indices, H.indptr), shape=H.shape)


def residual(H, x, b):
    """b - H x in long double (H sparse or dense, x / b float64 or long double vectors)"""
    x = np.asarray(x, dtype=LD); b = np.asarray(b, dtype=LD)
    return b - _csr(H) @ x


def inf_norm(H):
    """|H|_inf = max_i sum_j |H_ij|, summed in long double"""
    A = _csr(H)
    return LD(abs(A).sum(axis=1).max()) if A.nnz else LD(0)


def _norm2(v):
    v = np.asarray(v, dtype=LD)
    return np.sqrt(np.dot(v, v))


def normwise_berr(H, x, b):
    """|b - H x|_2 / (|H|_inf |x|_2 + |b|_2), every step in long double; returned as float"""
    r = residual(H, x, b)
    den = inf_norm(H) * _norm2(x) + _norm2(b)
    return float(_norm2(r) / den) if den > 0 else 0.0


def componentwise_berr(H, x, b):
    """Oettli-Prager: max_i |r_i| / (|H| |x| + |b|)_i (rows where the denominator vanishes count only if their residual does not)"""
    r = np.abs(residual(H, x, b))
    den = abs(_csr(H)) @ np.abs(np.asarray(x, dtype=LD)) + np.abs(np.asarray(b, dtype=LD))
    pos = den > 0
    if np.any(r[~pos] > 0):
        return float("inf")
    return float(np.max(r[pos] / den[pos])) if pos.any() else 0.0


def x_ref(H, b, passes=3):
    """SuperLU's solution refined `passes` times with long-double residuals: the reference solution of H x = b"""
    import scipy.sparse.linalg as spl
    lu = spl.splu(sp.csc_matrix(H, dtype=np.float64))
    x = lu.solve(np.asarray(b, dtype=np.float64)).astype(LD)
    for _ in range(passes):
        x = x + lu.solve(np.asarray(residual(H, x, b), dtype=np.float64)).astype(LD)
    return np.asarray(x, dtype=np.float64)
