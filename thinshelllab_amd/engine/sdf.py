"""Sampling of distance fields for BaseScene.set_sdfs (no counterpart in the reference): a few analytic signed distance functions, the sampler that
lays a grid over a box, and the check that a solid keeps clear of its grid's border.

A field function takes points (..., 3) in the field's own frame and returns the signed distance (...,), negative inside the solid.  The engine reads
the samples as the control values of a uniform cubic B-spline: a sampled plane is reproduced exactly, a curved field is smoothed by about h^2 / 6
times its Laplacian (a ball of radius R sits about h^2 / (3 R) deeper); there is no prefilter."""
import numpy as np


def ball(radius, centre=(0.0, 0.0, 0.0)):
    c = np.asarray(centre, np.float64)
    return lambda p: np.linalg.norm(np.asarray(p, np.float64) - c, axis=-1) - radius


def rounded_box(half_extents, radius, centre=(0.0, 0.0, 0.0)):
    """the box of csrc/k_box.hpp: the core box of the half extents grown by the radius"""
    c, h = np.asarray(centre, np.float64), np.asarray(half_extents, np.float64)

    def fn(p):
        q = np.abs(np.asarray(p, np.float64) - c) - h
        return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0) - radius
    return fn


def torus(major, minor, axis=2, centre=(0.0, 0.0, 0.0)):
    """a ring of tube radius `minor` about the circle of radius `major` in the plane normal to `axis`"""
    c = np.asarray(centre, np.float64)
    a, b = [i for i in range(3) if i != axis]

    def fn(p):
        q = np.asarray(p, np.float64) - c
        return np.hypot(np.hypot(q[..., a], q[..., b]) - major, q[..., axis]) - minor
    return fn


def union(*fns):
    """the solid that is any of the solids (the minimum of the fields: exact outside, a lower bound of the distance inside)"""
    return lambda p: np.minimum.reduce([f(p) for f in fns])


def sample(fn, lo, hi, h):
    """(grid, origin): samples of fn at origin + h (i, j, k), laid so that the valid region of the spline (1 <= t < n - 2 grid cells) covers the box
    [lo, hi]: origin = lo - h, n_a = ceil((hi_a - lo_a) / h) + 4.  The grid is C-ordered float64, the argument of BaseScene.set_sdfs."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (h > 0.0 and np.isfinite(h) and np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"sample: a spacing {h:g} > 0 and a box lo <= hi are needed (lo {lo.tolist()}, hi {hi.tolist()})")
    n = np.ceil((hi - lo) / h - 1e-9).astype(np.int64) + 4
    origin = lo - h
    ax = [origin[a] + h * np.arange(n[a]) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)
    return np.ascontiguousarray(fn(P), dtype=np.float64), origin


def border_clear(grid, r, eps):
    """True when every sample with an index below 3 or at or above n_a - 3 along some axis is at least r + eps.  By the convex-hull property of the
    spline the field is then at least eps outside the solid {phi < r} all along the boundary of the valid region: no vertex can reach the solid's
    shell from outside the grid."""
    g = np.asarray(grid, np.float64)
    inner = np.zeros(g.shape, bool)
    inner[3:g.shape[0] - 3, 3:g.shape[1] - 3, 3:g.shape[2] - 3] = True
    return bool((g[~inner] >= r + eps).all())
