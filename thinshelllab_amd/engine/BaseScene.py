"""Scene state + implicit-Euler driver: host-side counterpart of ``BaseScene``
(/root/reference/code/engine/BaseScene.py).

Python keeps what the task scenes / Grad / trajopt scripts touch (fields, bodies, gripper, frozen sets) and
hands the hot path to ``libtsl_hip.so`` through ``TslContext``:
  time_step            -> tsl_step            (BaseScene.py:1327-1370)
  compute_energy       -> tsl_energy          (:427-451)
  compute_residual_and_Hessian / compute_Hessian -> tsl_assemble (:976-1052)
  H.solve              -> tsl_solve           (sparse_solver.py:85-105)
State lives once, in global HBM tensors; per-body fields are views (no pushup/pushdown copies).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import gripper_single
from .field import Field, ScalarField
from .frames import compose, frame_targets, quat_normalize, validate_frames, validate_poses
from .gripper_single import quat_to_rotmat
from .gripper_tactile import gripper
from .model_elastic_offset import Elastic
from .model_elastic_tactile import Elastic as tactile
from .model_fold_offset import Cloth


@dataclass
class Body:
    v_start: int
    v_end: int
    f_start: int
    f_end: int


def validate_handles(tot_NV, vertex_ids, weights=None):
    """The checks of tsl_set_handles on the host, with its messages: returns (int32 vertex ids, float64 weights or None) or raises ValueError naming
    the offender -- a vertex outside [0, tot_NV), a vertex with more than one handle, a negative or non-finite weight."""
    v = np.asarray(vertex_ids)
    if v.ndim != 1 or (v.size and not np.issubdtype(v.dtype, np.integer)):
        raise ValueError(f"set_handles: vertex ids must be a flat list of integers (got shape {v.shape}, dtype {v.dtype})")
    v = v.astype(np.int64)
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != v.shape:
            raise ValueError(f"set_handles: {w.size} weights for {v.size} handles")
    seen = set()
    for i, vi in enumerate(v.tolist()):
        if vi < 0 or vi >= tot_NV:
            raise ValueError(f"set_handles: vertex {vi} out of range [0, {tot_NV})")
        if vi in seen:
            raise ValueError(f"set_handles: vertex {vi} has more than one handle")
        seen.add(vi)
        if w is not None and not (w[i] >= 0.0 and np.isfinite(w[i])):
            raise ValueError(f"set_handles: weight {w[i]:g} of vertex {vi} is negative or not finite")
    return v.astype(np.int32), w


def validate_surface_handles(tot_NF, face_ids, bary, weights=None):
    """The checks of tsl_set_handles_on_faces on the host, with its messages: returns (int32 face ids, float64 coordinates (n, 3), float64 weights or
    None) or raises ValueError naming the offender -- a face outside [0, tot_NF), a barycentric coordinate that is not finite or outside [0, 1], a
    triple whose sum differs from 1 by more than 1e-9, a negative or non-finite weight.  The coordinates are used as given, not renormalised."""
    f = np.asarray(face_ids)
    if f.ndim != 1 or (f.size and not np.issubdtype(f.dtype, np.integer)):
        raise ValueError(f"set_surface_handles: face ids must be a flat list of integers (got shape {f.shape}, dtype {f.dtype})")
    f = f.astype(np.int64)
    b = np.asarray(bary, dtype=np.float64)
    if b.shape != (f.size, 3):
        raise ValueError(f"set_surface_handles: barycentric coordinates of shape {b.shape} for {f.size} handles (expected ({f.size}, 3))")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != f.shape:
            raise ValueError(f"set_surface_handles: {w.size} weights for {f.size} handles")
    for i, fi in enumerate(f.tolist()):
        if fi < 0 or fi >= tot_NF:
            raise ValueError(f"set_surface_handles: face {fi} of handle {i} out of range [0, {tot_NF})")
        for a in range(3):
            if not (np.isfinite(b[i, a]) and 0.0 <= b[i, a] <= 1.0):
                raise ValueError(f"set_surface_handles: barycentric coordinate {b[i, a]:g} of handle {i} (face {fi}) is not finite or outside [0, 1]")
        tot = (b[i, 0] + b[i, 1]) + b[i, 2]
        if not abs(tot - 1.0) <= 1e-9:
            raise ValueError(f"set_surface_handles: barycentric coordinates ({b[i, 0]:g}, {b[i, 1]:g}, {b[i, 2]:g}) of handle {i} (face {fi}) sum to {tot:.12g}, not 1")
        if w is not None and not (w[i] >= 0.0 and np.isfinite(w[i])):
            raise ValueError(f"set_surface_handles: weight {w[i]:g} of handle {i} (face {fi}) is negative or not finite")
    return f.astype(np.int32), np.ascontiguousarray(b), w


def validate_ties(tot_NV, faces_tab, vertex_ids, face_ids, bary, weights=None):
    """The checks of tsl_set_ties on the host, with its messages: returns (int32 vertex ids, int32 face ids, float64 coordinates (n, 3), float64
    weights or None) or raises ValueError naming the offender -- a face outside [0, tot_NF), a vertex outside [0, tot_NV), a vertex that is a corner of
    its own face, a barycentric coordinate that is not finite or outside [0, 1], a triple whose sum differs from 1 by more than 1e-9, a negative or
    non-finite weight.  faces_tab: the scene's global face table (tot_NF, 3).  The coordinates are used as given, not renormalised."""
    v = np.asarray(vertex_ids)
    f = np.asarray(face_ids)
    for name, a in (("vertex", v), ("face", f)):
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"set_ties: {name} ids must be a flat list of integers (got shape {a.shape}, dtype {a.dtype})")
    if v.shape != f.shape:
        raise ValueError(f"set_ties: {v.size} vertices for {f.size} faces")
    v = v.astype(np.int64); f = f.astype(np.int64)
    b = np.asarray(bary, dtype=np.float64)
    if b.shape != (f.size, 3):
        raise ValueError(f"set_ties: barycentric coordinates of shape {b.shape} for {f.size} ties (expected ({f.size}, 3))")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != f.shape:
            raise ValueError(f"set_ties: {w.size} weights for {f.size} ties")
    faces_tab = np.asarray(faces_tab).reshape(-1, 3)
    tot_NF = len(faces_tab)
    for i, (vi, fi) in enumerate(zip(v.tolist(), f.tolist())):
        if fi < 0 or fi >= tot_NF:
            raise ValueError(f"set_ties: face {fi} of tie {i} out of range [0, {tot_NF})")
        if vi < 0 or vi >= tot_NV:
            raise ValueError(f"set_ties: vertex {vi} of tie {i} (face {fi}) out of range [0, {tot_NV})")
        if vi in faces_tab[fi].tolist():
            raise ValueError(f"set_ties: vertex {vi} of tie {i} is a corner of its own face {fi}")
        for a in range(3):
            if not (np.isfinite(b[i, a]) and 0.0 <= b[i, a] <= 1.0):
                raise ValueError(f"set_ties: barycentric coordinate {b[i, a]:g} of tie {i} (face {fi}, vertex {vi}) is not finite or outside [0, 1]")
        tot = (b[i, 0] + b[i, 1]) + b[i, 2]
        if not abs(tot - 1.0) <= 1e-9:
            raise ValueError(f"set_ties: barycentric coordinates ({b[i, 0]:g}, {b[i, 1]:g}, {b[i, 2]:g}) of tie {i} (face {fi}, vertex {vi}) sum to {tot:.12g}, not 1")
        if w is not None and not (w[i] >= 0.0 and np.isfinite(w[i])):
            raise ValueError(f"set_ties: weight {w[i]:g} of tie {i} (face {fi}, vertex {vi}) is negative or not finite")
    return v.astype(np.int32), f.astype(np.int32), np.ascontiguousarray(b), w


SHAPE_MAX = 8   # colliders of one kind: one bit each in a vertex's mask byte (csrc/shape_host.hpp)
TSL_MAX_COLLIDERS = TSL_MAX_SPHERES = TSL_MAX_CAPSULES = TSL_MAX_BOXES = TSL_MAX_SDFS = SHAPE_MAX
SDF_DIM_MIN, SDF_DIM_MAX, SDF_SAMPLES_MAX = 4, 512, 1 << 26   # (csrc/sdf_host.hpp)


def _check_shape(who, noun, j, mu, radius=None):
    """the radius (where the kind has one) and the friction coefficient of shape j, with the messages of csrc/shape_host.hpp"""
    if radius is not None and not (np.isfinite(radius) and radius > 0.0):
        raise ValueError(f"{who}: radius {radius:g} of {noun} {j} is not finite and positive")
    if not (mu >= 0.0 and np.isfinite(mu)):
        raise ValueError(f"{who}: friction coefficient {mu:g} of {noun} {j} is negative or not finite")


def _check_count(who, noun, n):
    if n > SHAPE_MAX:
        raise ValueError(f"{who}: {n} {noun}s: at most {SHAPE_MAX}")


def _check_k(who, name, k):
    """the stiffness of a collider kind as a float, with the message of tsl_set_param"""
    k = float(k)
    if not (k >= 0.0 and np.isfinite(k)):
        raise ValueError(f"{who}: {name} must be finite and >= 0 (got {k:g})")
    return k


def _shape_mask(who, noun, tot_NV, n, vertex_ids):
    """The uint8 mask (tot_NV), bit j: shape j acts on the vertex.  vertex_ids None: every shape on every vertex; else one entry per shape, None (all
    vertices) or a list of global vertex ids; ValueError for a wrong number of lists or an id out of range"""
    mask = np.full(tot_NV, (1 << n) - 1, np.uint8)
    if vertex_ids is not None:
        if len(vertex_ids) != n:
            raise ValueError(f"{who}: {len(vertex_ids)} vertex lists for {n} {noun}s")
        mask[:] = 0
        for j, ids in enumerate(vertex_ids):
            if ids is None:
                mask |= np.uint8(1 << j)
                continue
            v = np.asarray(ids, dtype=np.int64).reshape(-1)
            for vi in v.tolist():
                if vi < 0 or vi >= tot_NV:
                    raise ValueError(f"{who}: vertex {vi} of {noun} {j} out of range [0, {tot_NV})")
            mask[v] |= np.uint8(1 << j)
    return mask


def validate_colliders(tot_NV, normals, offsets, mu, vertex_ids=None):
    """The checks of tsl_set_colliders on the host, with the messages of csrc/collider_host.hpp: returns (unit normals (n, 3), offsets (n), mu (n),
    uint8 mask (tot_NV)) or raises ValueError naming the offender -- more than SHAPE_MAX colliders, a zero or non-finite normal, a non-finite
    offset, a negative or non-finite friction coefficient, a vertex id out of range.  vertex_ids None: every collider acts on every vertex; else one
    entry per collider, None (all vertices) or a list of global vertex ids."""
    o = np.asarray(offsets, dtype=np.float64).reshape(-1)
    n = len(o)
    nr = np.asarray(normals, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    m = np.asarray(mu, dtype=np.float64).reshape(-1)
    if nr.shape != (n, 3) or m.shape != (n,):
        raise ValueError(f"set_colliders: {len(nr)} normals and {m.size} friction coefficients for {n} offsets")
    _check_count("set_colliders", "collider", n)
    unit = np.zeros((n, 3))
    for j in range(n):
        length = float(np.sqrt((nr[j, 0] * nr[j, 0] + nr[j, 1] * nr[j, 1]) + nr[j, 2] * nr[j, 2]))
        if not (np.isfinite(length) and length > 0.0):
            raise ValueError(f"set_colliders: normal ({nr[j, 0]:g}, {nr[j, 1]:g}, {nr[j, 2]:g}) of collider {j} is zero or not finite")
        if not np.isfinite(o[j]):
            raise ValueError(f"set_colliders: offset {o[j]:g} of collider {j} is not finite")
        _check_shape("set_colliders", "collider", j, m[j])
        unit[j] = nr[j] / length
    return unit, o.copy(), m.copy(), _shape_mask("set_colliders", "collider", tot_NV, n, vertex_ids)


def validate_wind(n_cloth_faces, tot_NF, c_n, c_t, face_ids=None, weights=None):
    """The checks of tsl_set_wind and of the keys "wind_cn" / "wind_ct" on the host, with the messages of csrc/wind_host.hpp: returns (c_n, c_t, int32
    face ids (n), weights (n)) or raises ValueError naming the offender -- a negative or non-finite coefficient, a face outside [0, tot_NF), a
    surface face of a body (the cloth faces are the first n_cloth_faces of the scene's face table), a face listed twice, a negative or non-finite
    weight.  face_ids None: every cloth face in ascending order; weights None: 1 each."""
    cs = []
    for name, v in (("wind_cn", c_n), ("wind_ct", c_t)):
        v = float(v)
        if not (v >= 0.0 and np.isfinite(v)):
            raise ValueError(f"set_wind: {name} must be finite and >= 0 (got {v:g})")
        cs.append(v)
    f = np.arange(n_cloth_faces, dtype=np.int32) if face_ids is None else np.asarray(face_ids, dtype=np.int64).reshape(-1)
    n = len(f)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (n,):
        raise ValueError(f"set_wind: {w.size} weights for {n} faces")
    first = {}
    for i in range(n):
        fi = int(f[i])
        if fi < 0 or fi >= tot_NF:
            raise ValueError(f"set_wind: face {fi} of entry {i} out of range [0, {tot_NF})")
        if fi >= n_cloth_faces:
            raise ValueError(f"set_wind: face {fi} of entry {i} is a surface face of a body, not a cloth face (cloth faces are [0, {n_cloth_faces}))")
        if fi in first:
            raise ValueError(f"set_wind: face {fi} is listed twice (entries {first[fi]} and {i})")
        first[fi] = i
        if not (w[i] >= 0.0 and np.isfinite(w[i])):
            raise ValueError(f"set_wind: weight {w[i]:g} of entry {i} (face {fi}) is negative or not finite")
    return cs[0], cs[1], f.astype(np.int32), w.copy()


def validate_wind_velocity(W):
    """the wind velocity as a (3,) array, or ValueError naming the component that is not finite (the message of csrc/wind_host.hpp)"""
    W = np.asarray(W, dtype=np.float64).reshape(-1)
    if W.shape != (3,):
        raise ValueError(f"set_wind_velocity: {W.size} components, not 3")
    for a in range(3):
        if not np.isfinite(W[a]):
            raise ValueError(f"set_wind_velocity: component {a} of the wind velocity ({W[0]:g}, {W[1]:g}, {W[2]:g}) is not finite")
    return W.copy()


def validate_spheres(tot_NV, centres, radii, mu, vertex_ids=None):
    """The checks of tsl_set_spheres on the host, with the messages of csrc/sphere_host.hpp: returns (centres (n, 3), radii (n), mu (n), uint8 mask
    (tot_NV)) or raises ValueError naming the offender -- more than SHAPE_MAX spheres, a non-finite centre, a radius that is not finite and
    positive, a negative or non-finite friction coefficient, a vertex id out of range.  vertex_ids None: every sphere acts on every vertex; else one
    entry per sphere, None (all vertices) or a list of global vertex ids."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    n = len(r)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    m = np.asarray(mu, dtype=np.float64).reshape(-1)
    if c.shape != (n, 3) or m.shape != (n,):
        raise ValueError(f"set_spheres: {len(c)} centres and {m.size} friction coefficients for {n} radii")
    _check_count("set_spheres", "sphere", n)
    for j in range(n):
        if not np.isfinite(c[j]).all():
            raise ValueError(f"set_spheres: centre ({c[j, 0]:g}, {c[j, 1]:g}, {c[j, 2]:g}) of sphere {j} is not finite")
        _check_shape("set_spheres", "sphere", j, m[j], r[j])
    return c.copy(), r.copy(), m.copy(), _shape_mask("set_spheres", "sphere", tot_NV, n, vertex_ids)


CAPSULE_MIN_LEN = 1e-9


def _capsule_ends_check(who, what, a, b, j):
    """the message of csrc/capsule_host.hpp for the endpoints of capsule j (what: "" or "previous "), or None"""
    for name, e in (("a", a), ("b", b)):
        if not np.isfinite(e).all():
            return f"{who}: {what}endpoint {name} ({e[0]:g}, {e[1]:g}, {e[2]:g}) of capsule {j} is not finite"
    ln = float(np.sqrt(((b - a) ** 2).sum()))
    if not ln >= CAPSULE_MIN_LEN:
        return f"{who}: {what}segment of capsule {j} is {ln:g} m long: at least {CAPSULE_MIN_LEN:g} m"
    return None


def validate_capsules(tot_NV, ends_a, ends_b, radii, mu, vertex_ids=None):
    """The checks of tsl_set_capsules on the host, with the messages of csrc/capsule_host.hpp: returns (a (n, 3), b (n, 3), radii (n), mu (n), uint8
    mask (tot_NV)) or raises ValueError naming the offender -- more than SHAPE_MAX capsules, a non-finite endpoint, a segment shorter than
    1e-9 m, a radius that is not finite and positive, a negative or non-finite friction coefficient, a vertex id out of range.  vertex_ids None:
    every capsule acts on every vertex; else one entry per capsule, None (all vertices) or a list of global vertex ids."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    n = len(r)
    a = np.asarray(ends_a, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    b = np.asarray(ends_b, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    m = np.asarray(mu, dtype=np.float64).reshape(-1)
    if a.shape != (n, 3) or b.shape != (n, 3) or m.shape != (n,):
        raise ValueError(f"set_capsules: {len(a)} endpoints a, {len(b)} endpoints b and {m.size} friction coefficients for {n} radii")
    _check_count("set_capsules", "capsule", n)
    for j in range(n):
        bad = _capsule_ends_check("set_capsules", "", a[j], b[j], j)
        if bad:
            raise ValueError(bad)
        _check_shape("set_capsules", "capsule", j, m[j], r[j])
    return a.copy(), b.copy(), r.copy(), m.copy(), _shape_mask("set_capsules", "capsule", tot_NV, n, vertex_ids)


def _box_pose_check(who, what, c, q, j, noun="box"):
    """the message of csrc/box_host.hpp's box_pose_check for the pose of box j (what: "" or "previous "; noun: what carries the pose -- the sampled
    fields take the same rule), or None"""
    if not np.isfinite(c).all():
        return f"{who}: {what}centre ({c[0]:g}, {c[1]:g}, {c[2]:g}) of {noun} {j} is not finite"
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) if np.isfinite(q).all() else float("nan")
    if not (n > 0.0 and math.isfinite(n)):
        return f"{who}: {what}quaternion ({q[0]:g}, {q[1]:g}, {q[2]:g}, {q[3]:g}) of {noun} {j} is zero or not finite"
    return None


def validate_boxes(tot_NV, centres, quats, half_extents, radii, mu, vertex_ids=None):
    """The checks of tsl_set_boxes on the host, with the messages of csrc/box_host.hpp: returns (centres (n, 3), unit quaternions (n, 4), half extents
    (n, 3), radii (n), mu (n), uint8 mask (tot_NV)) or raises ValueError naming the offender -- more than SHAPE_MAX boxes, a non-finite centre, a
    zero or non-finite quaternion, a negative or non-finite half extent, a radius that is not finite and positive, a negative or non-finite friction
    coefficient, a vertex id out of range.  vertex_ids None: every box acts on every vertex; else one entry per box, None (all vertices) or a list
    of global vertex ids."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    n = len(r)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    q = np.array(quats, dtype=np.float64).reshape(-1, 4) if n else np.zeros((0, 4))
    h = np.asarray(half_extents, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    m = np.asarray(mu, dtype=np.float64).reshape(-1)
    if c.shape != (n, 3) or q.shape != (n, 4) or h.shape != (n, 3) or m.shape != (n,):
        raise ValueError(f"set_boxes: {len(c)} centres, {len(q)} quaternions, {len(h)} half extents and {m.size} friction coefficients for {n} radii")
    if n > SHAPE_MAX:
        raise ValueError(f"set_boxes: {n} boxes: at most {SHAPE_MAX}")
    for j in range(n):
        bad = _box_pose_check("set_boxes", "", c[j], q[j], j)
        if bad:
            raise ValueError(bad)
        if not (np.isfinite(h[j]).all() and (h[j] >= 0.0).all()):
            raise ValueError(f"set_boxes: half extents ({h[j, 0]:g}, {h[j, 1]:g}, {h[j, 2]:g}) of box {j} are negative or not finite")
        _check_shape("set_boxes", "box", j, m[j], r[j])
        q[j] = quat_normalize(q[j])
    if vertex_ids is not None and len(vertex_ids) != n:
        raise ValueError(f"set_boxes: {len(vertex_ids)} vertex lists for {n} boxes")
    return c.copy(), q, h.copy(), r.copy(), m.copy(), _shape_mask("set_boxes", "box", tot_NV, n, vertex_ids)


def validate_sdfs(tot_NV, grids, origins, spacings, centres, quats, offsets, mu, vertex_ids=None):
    """The checks of tsl_set_sdfs on the host, with the messages of csrc/sdf_host.hpp: returns (grids (list of C-ordered float64 arrays), origins (n, 3),
    spacings (n), centres (n, 3), unit quaternions (n, 4), offsets (n), mu (n), uint8 mask (tot_NV)) or raises ValueError naming the offender -- more
    than SHAPE_MAX fields, a grid that is not 3-d, a dimension below 4 or above 512, more than 2^26 samples in total, a spacing that is not finite and
    positive, a non-finite origin, offset, centre or sample, a zero or non-finite quaternion, a negative or non-finite friction coefficient, a vertex
    id out of range.  vertex_ids None: every field acts on every vertex; else one entry per field, None (all vertices) or a list of global vertex ids."""
    g = [np.array(a, dtype=np.float64, order="C") for a in grids]
    n = len(g)
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    h = np.asarray(spacings, dtype=np.float64).reshape(-1)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    q = np.array(quats, dtype=np.float64).reshape(-1, 4) if n else np.zeros((0, 4))
    r = np.asarray(offsets, dtype=np.float64).reshape(-1)
    m = np.asarray(mu, dtype=np.float64).reshape(-1)
    if o.shape != (n, 3) or h.shape != (n,) or c.shape != (n, 3) or q.shape != (n, 4) or r.shape != (n,) or m.shape != (n,):
        raise ValueError(f"set_sdfs: {len(o)} origins, {h.size} spacings, {len(c)} centres, {len(q)} quaternions, {r.size} offsets and {m.size} friction coefficients for {n} grids")
    if n > SHAPE_MAX:
        raise ValueError(f"set_sdfs: {n} fields: at most {SHAPE_MAX}")
    tot = 0
    for j in range(n):
        if g[j].ndim != 3:
            raise ValueError(f"set_sdfs: the grid of field {j} has {g[j].ndim} axes, not 3")
        for a in range(3):
            if not SDF_DIM_MIN <= g[j].shape[a] <= SDF_DIM_MAX:
                raise ValueError(f"set_sdfs: dimension {g[j].shape[a]} of axis {a} of field {j} is below {SDF_DIM_MIN} or above {SDF_DIM_MAX}")
        tot += g[j].size
        if tot > SDF_SAMPLES_MAX:
            raise ValueError(f"set_sdfs: {tot} samples up to field {j}: at most {SDF_SAMPLES_MAX} in total")
        if not (h[j] > 0.0 and np.isfinite(h[j])):
            raise ValueError(f"set_sdfs: spacing {h[j]:g} of field {j} is not finite and positive")
        if not np.isfinite(o[j]).all():
            raise ValueError(f"set_sdfs: origin ({o[j, 0]:g}, {o[j, 1]:g}, {o[j, 2]:g}) of field {j} is not finite")
        if not np.isfinite(r[j]):
            raise ValueError(f"set_sdfs: offset {r[j]:g} of field {j} is not finite")
        bad = _box_pose_check("set_sdfs", "", c[j], q[j], j, "field")
        if bad:
            raise ValueError(bad)
        _check_shape("set_sdfs", "field", j, m[j])
        q[j] = quat_normalize(q[j])
    for j in range(n):
        if not np.isfinite(g[j]).all():
            i0, i1, i2 = (int(e) for e in np.argwhere(~np.isfinite(g[j]))[0])
            raise ValueError(f"set_sdfs: sample ({i0}, {i1}, {i2}) of field {j} is not finite ({g[j][i0, i1, i2]:g})")
    if vertex_ids is not None and len(vertex_ids) != n:
        raise ValueError(f"set_sdfs: {len(vertex_ids)} vertex lists for {n} fields")
    return g, o.copy(), h.copy(), c.copy(), q, r.copy(), m.copy(), _shape_mask("set_sdfs", "field", tot_NV, n, vertex_ids)


class _SystemMatrix:
    """Stand-in for ``SparseMatrix`` (sparse_solver.py): the matrix itself lives inside the context."""

    def __init__(self, sys):
        self._sys = sys
        self.n = sys.tot_NV * 3

    def clear_all(self):
        pass

    def solve(self, b):
        x, _ = self._sys._ensure_ctx().solve(b.contiguous().to(self._sys.device, torch.float64))
        return x

    def to_csr(self):
        return self._sys._ensure_ctx().matrix_csr()


class BaseScene:
    _newton_cap = 1000   # BaseScene.py:1342
    _plastic = 0         # base timestep_finish does not update ref angles (:1321-1325)
    spd_literal = False  # True: the forward projections run the reference's own projector (linalg.py:15-148) instead of the converged eigen-clamp
    contact_ee = False   # True: edge-edge contact between the surface edges of different bodies next to the reference's vertex-triangle contact

    def __init__(self, cloth_size=0.1, dt=5e-3, enable_gripper=True, device="cuda:0"):
        # BaseScene.py:31-60
        self.dt = dt
        self.h = self.dt
        self.cloth_cnt = 2
        self.elastic_cnt = 3
        self.cloth_size = cloth_size
        self.elastic_size = [0.06, 0.015, 0.015]
        self.cloth_N = 31
        self.elastic_Nx = 16
        self.elastic_Ny = 16
        self.elastic_Nz = 2
        self.enable_gripper = enable_gripper
        self.k_contact = 1000
        self.eps_contact = 0.001
        self.eps_v = 0.01
        self.max_n_constraints = 100000
        self.damping = 1.0
        self.extra_obj = False
        self.effector_cnt = -1
        self.grid_h = 0.003
        if isinstance(device, str) and device.startswith("cuda") and not torch.cuda.is_available():
            device = "cpu"  # host-only use (tables, poses); any engine call will raise (no CPU path)
        self.device = torch.device(device)
        self._ctx = None
        self._dirty = set()
        self.last_stats = {}
        # soft handles (set_handles): vertex ids, weights, targets and the stiffness k_handle, kept here and pushed to the engine context lazily
        self._handle_v = np.zeros(0, np.int32)
        self._handle_f = None    # set_surface_handles: global face ids and barycentric coordinates (n, 3); None while the list is a vertex list
        self._handle_b = None
        self._handle_w = None
        self._handle_t = np.zeros((0, 3))
        self.k_handle = 0.0
        # ties (set_ties, sew): vertex ids, face ids, barycentric coordinates, weights and the stiffness k_tie, kept here and pushed to the engine context lazily
        self._tie_v = np.zeros(0, np.int32)
        self._tie_f = np.zeros(0, np.int32)
        self._tie_b = np.zeros((0, 3))
        self._tie_w = None
        self.k_tie = 0.0
        # half-space colliders (set_colliders): unit normals, offsets, friction coefficients, the per-vertex mask and the stiffness k_collider, kept
        # here and pushed to the engine context lazily
        self._col_n = np.zeros((0, 3))
        self._col_o = np.zeros(0)
        self._col_mu = np.zeros(0)
        self._col_mask = np.zeros(0, np.uint8)
        self.k_collider = 0.0
        # sphere colliders (set_spheres): _sph_c the centres for the next step, _sph_cp the centres of the last completed step (where the balls are at the
        # start of the next one), _sph_cp_step the previous centres that the last completed step used (the tape records it); radii, friction
        # coefficients, the per-vertex mask and the stiffness k_sphere, kept here and pushed to the engine context lazily
        self._sph_c = np.zeros((0, 3))
        self._sph_cp = np.zeros((0, 3))
        self._sph_cp_step = np.zeros((0, 3))
        self._sph_R = np.zeros(0)
        self._sph_mu = np.zeros(0)
        self._sph_mask = np.zeros(0, np.uint8)
        self.k_sphere = 0.0
        # capsule colliders (set_capsules): _cap_e the endpoints (n, 2, 3) for the next step, _cap_ep those of the last completed step (where the rods are
        # at the start of the next one), _cap_ep_step the previous endpoints that the last completed step used (the tape records it); radii, friction
        # coefficients, the per-vertex mask and the stiffness k_capsule, kept here and pushed to the engine context lazily
        self._cap_e = np.zeros((0, 2, 3))
        self._cap_ep = np.zeros((0, 2, 3))
        self._cap_ep_step = np.zeros((0, 2, 3))
        self._cap_R = np.zeros(0)
        self._cap_mu = np.zeros(0)
        self._cap_mask = np.zeros(0, np.uint8)
        self.k_capsule = 0.0
        # rounded-box colliders (set_boxes): _box_c, _box_q the poses (centres (n, 3), unit quaternions (n, 4)) for the next step, _box_cp, _box_qp those of
        # the last completed step (where the boxes are at the start of the next one), _box_cp_step, _box_qp_step the previous poses that the last
        # completed step used (the tape records them); half extents, radii, friction coefficients, the per-vertex mask and the stiffness k_box, kept
        # here and pushed to the engine context lazily
        self._box_c = self._box_cp = self._box_cp_step = np.zeros((0, 3))
        self._box_q = self._box_qp = self._box_qp_step = np.zeros((0, 4))
        self._box_h = np.zeros((0, 3))
        self._box_r = np.zeros(0)
        self._box_mu = np.zeros(0)
        self._box_mask = np.zeros(0, np.uint8)
        self.k_box = 0.0
        # sampled distance-field colliders (set_sdfs): the poses as for the boxes (_sdf_c, _sdf_q for the next step, _sdf_cp, _sdf_qp of the last completed
        # step, _sdf_cp_step, _sdf_qp_step the previous poses that the last completed step used); grids, origins, spacings, offsets, friction
        # coefficients, the per-vertex mask and the stiffness k_sdf, kept here and pushed to the engine context lazily
        self._sdf_c = self._sdf_cp = self._sdf_cp_step = np.zeros((0, 3))
        self._sdf_q = self._sdf_qp = self._sdf_qp_step = np.zeros((0, 4))
        self._sdf_grids = []
        self._sdf_o = np.zeros((0, 3))
        self._sdf_h = np.zeros(0)
        self._sdf_r = np.zeros(0)
        self._sdf_mu = np.zeros(0)
        self._sdf_mask = np.zeros(0, np.uint8)
        self.k_sdf = 0.0
        # wind (set_wind): the listed cloth faces and their weights, the two drag coefficients and the wind velocity of the next step, kept here and
        # pushed to the engine context lazily
        self._wind_f = np.zeros(0, np.int32)
        self._wind_w = np.zeros(0)
        self.wind_cn = 0.0
        self.wind_ct = 0.0
        self._wind_W = np.zeros(3)
        # rigid frames of the handles (set_handle_frames): frame and local point of every handle, position and unit quaternion of every frame
        self._frame_of = np.zeros(0, np.int32)
        self._frame_local = np.zeros((0, 3))
        self._frame_pos = np.zeros((0, 3))
        self._frame_quat = np.zeros((0, 4))

        self.init_scene_parameters()
        if self.effector_cnt == -1:
            self.effector_cnt = self.elastic_cnt
        self.gravity = ScalarField([0.0, 0.0, -9.8], lambda f: self._refresh_gravity())
        self.mu_cloth_elastic = ScalarField(1.0, lambda f: self._set_param("mu_cloth_elastic", f.value))
        self.cloths = []
        self.elastics = []
        self.tot_NV = ((self.cloth_N + 1) ** 2) * self.cloth_cnt
        self.init_objects()
        NV = self.tot_NV
        dev = self.device
        # BaseScene.py:69-88
        self.pos = Field(torch.zeros((NV, 3), dtype=torch.float64, device=dev))
        self.vel = Field(torch.zeros((NV, 3), dtype=torch.float64, device=dev))
        self.prev_pos = Field(torch.zeros((NV, 3), dtype=torch.float64, device=dev))
        self.x1 = Field(torch.zeros((NV, 3), dtype=torch.float64, device=dev))
        self.mass = Field(torch.zeros(NV, dtype=torch.float64))
        self.tot_NF = 0
        for c in self.cloths:
            c.offset_faces = self.tot_NF
            self.tot_NF += c.NF
        for e in self.elastics:
            e.offset_faces = self.tot_NF
            self.tot_NF += e.n_surfaces
        self.frozen = Field(torch.zeros(NV * 3, dtype=torch.int32), lambda f: self._dirty.add("frozen"))
        self.faces = Field(torch.zeros((self.tot_NF, 3), dtype=torch.int32))
        self.border_flag = Field(torch.zeros(NV, dtype=torch.int32), lambda f: self._dirty.add("border"))
        self.ext_force = Field(torch.zeros((NV, 3), dtype=torch.float64), lambda f: self._dirty.add("ext_force"))
        self.x32 = Field(torch.zeros((NV, 3), dtype=torch.float32))
        self.f_vis = Field(torch.zeros(self.tot_NF * 3, dtype=torch.int32))
        # BaseScene.py:91-99
        self.body_list = []
        for c in self.cloths:
            self.body_list.append(Body(c.offset, c.offset + c.NV, c.offset_faces, c.offset_faces + c.NF))
        for e in self.elastics:
            self.body_list.append(Body(e.offset, e.offset + e.n_verts, e.offset_faces, e.offset_faces + e.n_surfaces))
        for i, c in enumerate(self.cloths):
            c.body_idx = i; c._idx = i; c._sys = self
        for i, e in enumerate(self.elastics):
            e.body_idx = i + self.cloth_cnt; e._sys = self
        self.nc = ScalarField(0, dtype=torch.int32)
        self.E = ScalarField(0.0)
        self.F = Field(torch.zeros(NV * 3, dtype=torch.float64, device=dev))
        self.H = _SystemMatrix(self)
        self.tmp_z_frozen = Field(torch.zeros(NV * 3, dtype=torch.float64, device=dev))
        # plastic rest angles of all cloths, one tensor; each cloth's field is a view
        n_cf = sum(c.NF for c in self.cloths)
        self._ref_angle = torch.zeros((max(n_cf, 1), 3), dtype=torch.float64, device=dev)
        self._bind_bodies()
        # gripper (BaseScene.py:166-172)
        if enable_gripper:
            self.gripper = gripper(self.dt, self.elastics[1].n_verts, self.elastics[1].frozen_cnt, self.elastics[1].surf_point,
                                   int((self.effector_cnt - 1) // 2))
        elif self.elastic_cnt > 1:
            self.gripper = gripper_single.gripper(self.dt, self.elastics[1].n_verts, self.elastics[1].frozen_cnt, self.elastics[1].surf_point,
                                                  self.effector_cnt - 1)
        self.action_dim = 3 * (self.effector_cnt - 1)
        if not enable_gripper:
            self.action_dim = int(6 * (self.effector_cnt - 1))
        if self.effector_cnt - 1 > 0:
            self.n_obs_cloth = 4
            self.n_obs_elastic = 16
            self.n_sample_cloth = self.cloths[0].N // 4   # BaseScene.py:187-191
            self.m_sample_cloth = self.cloths[0].M // 4
            self.obs_dim = (self.n_obs_cloth * self.n_obs_cloth * self.cloth_cnt + self.n_obs_elastic * self.elastic_cnt) * 6 + 7 * self.gripper.n_part
            self.observation = Field(torch.zeros(self.obs_dim, dtype=torch.float64))
            self.tot_force = Field(torch.zeros((self.effector_cnt - 1, 3), dtype=torch.float64))

    # ------------------------------------------------------------------ construction helpers
    def _bind_bodies(self):
        """make per-body state fields views of the global arrays (replaces pushup/pushdown_property)."""
        fs = 0
        for c in self.cloths:
            sl = slice(c.offset, c.offset + c.NV)
            for name, glob in (("pos", self.pos), ("vel", self.vel), ("prev_pos", self.prev_pos)):
                old = getattr(c, name).t
                glob.t[sl].copy_(old.to(glob.t.device))
                getattr(c, name).t = glob.t[sl]
            old = c.ref_angle.t
            self._ref_angle[fs:fs + c.NF].copy_(old.to(self._ref_angle.device))
            c.ref_angle.t = self._ref_angle[fs:fs + c.NF]
            fs += c.NF
        for e in self.elastics:
            sl = slice(e.offset, e.offset + e.n_verts)
            for name, glob in (("F_x", self.pos), ("F_v", self.vel), ("F_x_prev", self.prev_pos)):
                old = getattr(e, name).t
                glob.t[sl].copy_(old.to(glob.t.device))
                getattr(e, name).t = glob.t[sl]

    def init_objects(self):
        # BaseScene.py:196-211
        rho = 4e1
        for i in range(self.cloth_cnt):
            self.cloths.append(Cloth(self.cloth_N, self.dt, self.cloth_size, self.tot_NV, rho, i * ((self.cloth_N + 1) ** 2)))
        self.elastic_offset = ((self.cloth_N + 1) ** 2) * self.cloth_cnt
        tmp_tot = self.elastic_offset
        self.elastics.append(Elastic(self.dt, self.elastic_size[0], tmp_tot, self.elastic_Nx, self.elastic_Ny, self.elastic_Nz))
        tmp_tot += self.elastic_Nx * self.elastic_Ny * self.elastic_Nz
        for i in range(1, self.elastic_cnt):
            self.elastics.append(tactile(self.dt, tmp_tot, self.elastic_size[i] / 0.03))
            tmp_tot += self.elastics[i].n_verts
        self.tot_NV = tmp_tot

    def init_scene_parameters(self):
        # BaseScene.py:213-225
        self.dt = 5e-3
        self.h = self.dt
        self.cloth_cnt = 1
        self.elastic_cnt = 3
        self.elastic_size = [0.06, 0.015, 0.015]
        self.cloth_N = 15
        self.k_contact = 500
        self.eps_contact = 0.0004
        self.eps_v = 0.01
        self.max_n_constraints = 10000
        self.damping = 1.0

    def init_all(self):
        self.init()
        self.init_property()
        self.set_frozen()
        self.set_ext_force()
        self.update_visual()

    def init(self):
        # BaseScene.py:235-242
        self.cloths[0].init(-0.03, -0.03, 0.000399)
        self.elastics[0].init(-0.03, -0.03, -0.004)
        self.elastics[1].init(-0.02, 0., 0.0105, True)
        self.elastics[2].init(-0.02, 0., -0.0105, False)
        self.gripper.init(self, np.array([[-0.02, 0., 0.0]]))

    def reset_pos(self):
        self.init()

    def reset(self):
        # BaseScene.py:252-268
        self.reset_pos()
        self.set_ext_force()
        self.set_frozen()
        self.update_visual()
        if self._ctx is not None:
            self._ctx.contact_reset()

    def init_property(self):
        # BaseScene.py:361-383: gravity per body, masses, faces; (re)creates the engine context
        g = np.asarray(self.gravity[None], dtype=np.float64)
        for c in self.cloths:
            c.gravity.t.copy_(torch.as_tensor(g))
        if self.elastic_cnt > 0:
            self.elastics[0].gravity.t.copy_(torch.as_tensor(g))
        for i in range(1, self.effector_cnt):
            self.elastics[i].gravity.t.zero_()
        for i in range(self.effector_cnt, self.elastic_cnt):
            self.elastics[i].gravity.t.copy_(torch.as_tensor(g))
        m = np.zeros(self.tot_NV)
        for c in self.cloths:
            m[c.offset:c.offset + c.NV] = c.mass
        for e in self.elastics:
            m[e.offset:e.offset + e.n_verts] = e.F_m.to_numpy()
        self.mass.from_numpy(m)
        f = np.zeros((self.tot_NF, 3), np.int32)
        for c in self.cloths:
            f[c.offset_faces:c.offset_faces + c.NF] = c.f2v.to_numpy() + c.offset
        for e in self.elastics:
            f[e.offset_faces:e.offset_faces + e.n_surfaces] = e.f2v.to_numpy() + e.offset
        self.faces.from_numpy(f)
        self.f_vis.from_numpy(f.reshape(-1))
        self._close_ctx()

    def _gravity_array(self):
        g = np.zeros((self.tot_NV, 3))
        for c in self.cloths:
            g[c.offset:c.offset + c.NV] = c.gravity.to_numpy()
        for e in self.elastics:
            g[e.offset:e.offset + e.n_verts] = e.gravity.to_numpy()
        return g

    def _refresh_gravity(self):
        self._dirty.add("gravity")

    def _ext_force_array(self):
        f = self.ext_force.to_numpy().copy()
        for c in self.cloths:
            f[c.offset:c.offset + c.NV] += c.manipulate_force.to_numpy()
        for e in self.elastics:
            f[e.offset:e.offset + e.n_verts] += e.ext_force.to_numpy()
        return f

    # ------------------------------------------------------------------ static-friction loss (BaseScene.py:732-775)
    def _friction_slip(self, constraints=None, pos=None):
        """tangential slip of every constraint of the current step: (constraints, u (nc, 2), r (nc,), sliding mask r > 0.9 dt eps_v)
        -- the quantities both static_friction_loss variants start from (BaseScene.py:745-750, Scene_pick.py:205-211).  Host side:
        the reference never calls these kernels (analytic_grad_single.py:231 is commented out), they complete the named surface."""
        import numpy as np
        c = self._ensure_ctx().constraints() if constraints is None else constraints
        if constraints is None and self.contact_ee:   # the vertex-triangle slots only (the edge-edge ones follow them)
            n_vf = self._ctx.contact_counts()[0]
            c = {k: v[:n_vf] for k, v in c.items()}
        x = self.pos.to_numpy() if pos is None else pos
        idx, w = c["idx"], c["w"]
        T = c["T"].reshape(-1, 2, 3)
        x_c = (x[idx[:, :3]] * w[:, :, None]).sum(1)
        dx = x[idx[:, 3]] - x_c - c["dx0"]
        u = np.einsum("nij,nj->ni", T, dx)
        r = np.linalg.norm(u, axis=1)
        return c, T, u, r, r > self.dt * self.eps_v * 0.9

    def static_friction_loss(self, analy_grad, step, constraints=None, pos=None):
        """BaseScene.py:732-775: pos_grad[step, idx[i1]] += u_3d w1[i1] f_loss_ratio k for every sliding constraint,
        u_3d = T^T u, w1 = (-w0, -w1, -w2, 1)"""
        import numpy as np
        c, T, u, r, sl = self._friction_slip(constraints, pos)
        if not sl.any():
            return
        u3 = np.einsum("nij,ni->nj", T, u)
        w1 = np.concatenate([-c["w"], np.ones((len(r), 1))], 1)
        g = analy_grad.pos_grad.to_numpy()
        add = u3[:, None, :] * w1[:, :, None] * (analy_grad.f_loss_ratio * c["k"])[:, None, None]
        for i1 in range(4):
            np.add.at(g[step], c["idx"][sl, i1], add[sl, i1])
        analy_grad.pos_grad.from_numpy(g)

    # contact relationship of contact_analysis (BaseScene.py:818-835); scenes override
    def contact_pairs(self):
        pairs = []
        for i in range(self.cloth_cnt):
            for j in range(self.cloth_cnt):
                if abs(i - j) == 1:
                    pairs.append((self.cloths[i].body_idx, self.cloths[j].offset, self.cloths[j].offset + self.cloths[j].NV, 0.1))
                    pairs.append((self.cloths[j].body_idx, self.cloths[i].offset, self.cloths[i].offset + self.cloths[i].NV, 0.1))
        for i in range(self.cloth_cnt):
            for j in range(self.elastic_cnt):
                mu = None if j != 0 else 0.2
                pairs.append((self.cloths[i].body_idx, self.elastics[j].offset, self.elastics[j].offset + self.elastics[j].n_verts, mu))
                pairs.append((self.elastics[j].body_idx, self.cloths[i].offset, self.cloths[i].offset + self.cloths[i].NV, mu))
        return pairs

    # ------------------------------------------------------------------ engine context
    def _close_ctx(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def _ensure_ctx(self):
        if self._ctx is None:
            from ..context import TslContext
            self._ctx = TslContext(
                tot_NV=self.tot_NV, dt=self.dt, mass=self.mass.to_numpy(), gravity=self._gravity_array(), frozen=self.frozen.to_numpy(),
                cloths=[c._desc() for c in self.cloths], elastics=[e._desc() for e in self.elastics], faces=self.faces.to_numpy(),
                bodies=[(b.v_start, b.v_end, b.f_start, b.f_end) for b in self.body_list], pairs=self.contact_pairs(),
                k_contact=self.k_contact, eps_contact=self.eps_contact, eps_v=self.eps_v, damping=self.damping,
                max_n_constraints=self.max_n_constraints, grid_h=self.grid_h, device=str(self.device))
            self._ctx.set_param("mu_cloth_elastic", self.mu_cloth_elastic.value)
            if hasattr(self, "mu_cloth_cloth"):
                self._ctx.set_param("mu_cloth_cloth", self.mu_cloth_cloth.value)
            if getattr(self, "grid_extent", None):
                self._ctx.set_param("grid_extent", self.grid_extent)
            self._ctx.set_param("newton_cap", self._newton_cap)
            self._ctx.set_param("plastic", self._plastic)
            self._ctx.set_param("spd_literal", int(bool(self.spd_literal)))
            if self.contact_ee:
                self._ctx.set_param("contact_ee", 1)
            for i, c in enumerate(self.cloths):
                for k, v in c._stvk_params():
                    self._ctx.set_param(f"cloth{i}.{k}", v)
            self._ctx.set_ext_force(self._ext_force_array())
            if self.n_handle:
                self._push_handles()
            if self.n_tie:
                self._push_ties()
            if self.n_collider:
                self._push_colliders()
            if self.n_sphere:
                self._push_spheres()
            if self.n_capsule:
                self._push_capsules()
            if self.n_box:
                self._push_boxes()
            if self.n_sdf:
                self._push_sdfs()
            if self.n_wind:
                self._push_wind()
            self._dirty.clear()
        if self._dirty:
            if "ties" in self._dirty:
                self._push_ties()
            if "colliders" in self._dirty:
                self._push_colliders()
            elif "collider_offsets" in self._dirty:
                self._ctx.set_collider_offsets(self._col_o)
            if "spheres" in self._dirty:
                self._push_spheres()
            elif "sphere_centres" in self._dirty:
                self._ctx.set_sphere_centres(self._sph_c, self._sph_cp)
            if "capsules" in self._dirty:
                self._push_capsules()
            elif "capsule_ends" in self._dirty:
                self._ctx.set_capsule_ends(self._cap_e[:, 0], self._cap_e[:, 1], self._cap_ep[:, 0], self._cap_ep[:, 1])
            if "boxes" in self._dirty:
                self._push_boxes()
            elif "box_poses" in self._dirty:
                self._ctx.set_box_poses(self._box_c, self._box_q, self._box_cp, self._box_qp)
            if "sdfs" in self._dirty:
                self._push_sdfs()
            elif "sdf_poses" in self._dirty:
                self._ctx.set_sdf_poses(self._sdf_c, self._sdf_q, self._sdf_cp, self._sdf_qp)
            if "wind" in self._dirty:
                self._push_wind()
            elif "wind_velocity" in self._dirty:
                self._ctx.set_wind_velocity(self._wind_W)
            if "handles" in self._dirty:
                self._push_handles()
            else:
                if "handle_targets" in self._dirty:
                    self._ctx.set_handle_targets(self._handle_t)
                if "handle_frames" in self._dirty:
                    self._push_frames()
                elif "frame_poses" in self._dirty:
                    self._ctx.set_frame_poses(self._frame_pos, self._frame_quat)
            if "frozen" in self._dirty:
                self._ctx.set_frozen(self.frozen.to_numpy())
            if "border" in self._dirty:
                self._ctx.set_border(self.border_flag.to_numpy())
            if "ext_force" in self._dirty:
                self._ctx.set_ext_force(self._ext_force_array())
            if "gravity" in self._dirty:
                self._ctx.set_gravity(self._gravity_array())
            self._dirty.clear()
        return self._ctx

    def _set_param(self, key, value):
        if self._ctx is not None:
            self._ctx.set_param(key, value)

    # ------------------------------------------------------------------ frozen / external force
    def set_spd_literal(self, on):
        """Select the projector of the forward assembly: True the reference's Householder + QR sweeps (SPD_Projector, linalg.py:15-148), False
        (default) the converged eigen-clamp.  Applies to a live engine context at once and to one created later."""
        self.spd_literal = bool(on)
        if self._ctx is not None:
            self._ctx.set_param("spd_literal", int(self.spd_literal))

    def set_contact_ee(self, on):
        """Edge-edge contact (no counterpart in the reference): True appends edge-edge constraints behind the vertex-triangle ones at every detection,
        False (default) keeps vertex-triangle contact only.  Applies to a live engine context at once and to one created later."""
        self.contact_ee = bool(on)
        if self._ctx is not None:
            self._ctx.set_param("contact_ee", int(self.contact_ee))

    # ------------------------------------------------------------------ soft handles (no counterpart in the reference)
    @property
    def n_handle(self):
        return len(self._handle_v) if self._handle_f is None else len(self._handle_f)

    def set_handles(self, vertex_ids, k, weights=None):
        """Target springs on vertices: E_h = 1/2 k sum_i w_i |x_{v_i} - t_i|^2 with global vertex ids v_i (at most one handle per vertex), stiffness
        k >= 0 in N/m and weights w_i >= 0 (None: all 1).  An empty list removes the handles.  The targets start at zero: set_handle_targets.
        The lists are checked here, before any library call; the engine context receives them at its next use."""
        v, w = validate_handles(self.tot_NV, vertex_ids, weights)
        k = float(k)
        if not (k >= 0.0 and np.isfinite(k)):
            raise ValueError(f"set_handles: k_handle must be finite and >= 0 (got {k:g})")
        self._handle_v, self._handle_w, self.k_handle = v, w, k
        self._handle_f = self._handle_b = None   # (a scene holds a vertex list or a face list)
        self._handle_t = np.zeros((len(v), 3))
        self._frame_of, self._frame_local = np.zeros(0, np.int32), np.zeros((0, 3))   # (the handle list changed: the frames go with it)
        self._frame_pos, self._frame_quat = np.zeros((0, 3)), np.zeros((0, 4))
        self._dirty.add("handles")

    def set_surface_handles(self, face_ids, bary, k, weights=None):
        """Target springs on points of faces: E_h = 1/2 k sum_i w_i |p_i - t_i|^2 with p_i = sum_a b_a x_{v_a} the point of barycentric coordinates
        bary[i] on the global face face_ids[i] = (v_0, v_1, v_2) of self.faces (a cloth face or a surface face of a body; Cloth.locate gives both for
        a material point of a cloth).  Any number of handles may share a face or a vertex.  It replaces the handle list, as set_handles does -- each
        drops the other's list and the frames; an empty list removes the handles.  The targets start at zero: set_handle_targets.  The lists are
        checked here, before any library call; the engine context receives them at its next use."""
        f, b, w = validate_surface_handles(self.tot_NF, face_ids, bary, weights)
        k = float(k)
        if not (k >= 0.0 and np.isfinite(k)):
            raise ValueError(f"set_surface_handles: k_handle must be finite and >= 0 (got {k:g})")
        self._handle_f, self._handle_b, self._handle_w, self.k_handle = f, b, w, k
        self._handle_v = np.zeros(0, np.int32)
        self._handle_t = np.zeros((len(f), 3))
        self._frame_of, self._frame_local = np.zeros(0, np.int32), np.zeros((0, 3))   # (the handle list changed: the frames go with it)
        self._frame_pos, self._frame_quat = np.zeros((0, 3)), np.zeros((0, 4))
        self._dirty.add("handles")

    def handle_points(self):
        """(n, 3): the points the handles act on at the current positions -- sum_a b_a x_{v_a} of a face list, x_{v_i} of a vertex list (host arithmetic
        on a copy of the positions: the grasp of set_handle_frames needs no engine context; TslContext.handle_points is the library's read-out)"""
        x = self.pos.to_numpy()
        if self._handle_f is None:
            return x[self._handle_v]
        fv = self.faces.to_numpy()[self._handle_f]
        b = self._handle_b
        return (b[:, 0:1] * x[fv[:, 0]] + b[:, 1:2] * x[fv[:, 1]]) + b[:, 2:3] * x[fv[:, 2]]

    def set_handle_targets(self, targets):
        """world-space targets (n, 3) of the next energy, assembly, time step or reverse step"""
        t = np.array(targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else targets, dtype=np.float64)
        if t.shape != (self.n_handle, 3):
            raise ValueError(f"set_handle_targets: targets of shape {t.shape} for {self.n_handle} handles (expected ({self.n_handle}, 3))")
        self._handle_t = self._framed(t)
        self._dirty.add("handle_targets")

    def handle_force(self):
        """(n, 3): the force k w_i (t_i - x_{v_i}) every handle applies to the cloth at the current positions"""
        return self._ensure_ctx().handle_force(self.pos.t)

    def _push_handles(self):
        if self._handle_f is None:
            self._ctx.set_handles(self._handle_v, self._handle_w)
        else:
            self._ctx.set_handles_on_faces(self._handle_f, self._handle_b, self._handle_w)
        self._ctx.set_param("k_handle", self.k_handle)
        self._ctx.set_handle_targets(self._handle_t)
        self._push_frames()

    # ------------------------------------------------------------------ ties (no counterpart in the reference)
    @property
    def n_tie(self):
        return len(self._tie_v)

    def set_ties(self, vertex_ids, face_ids, bary, k, weights=None):
        """Springs between material points: tie i binds the global vertex vertex_ids[i] to the point with barycentric coordinates bary[i] on the global
        face face_ids[i] of self.faces (a cloth face or a surface face of a FEM body), E = 1/2 k sum_i w_i |x_v - sum_a b_a x_{t_a}|^2 with stiffness
        k >= 0 in N/m and weights w_i >= 0 (None: all 1).  Any number of ties may share a vertex or a face; the vertex must not be a corner of its
        face.  An empty list removes the ties.  A member of a SceneGroup sets its ties before the group is created."""
        v, f, b, w = validate_ties(self.tot_NV, self.faces.to_numpy(), vertex_ids, face_ids, bary, weights)
        k = float(k)
        if not (k >= 0.0 and np.isfinite(k)):
            raise ValueError(f"set_ties: k_tie must be finite and >= 0 (got {k:g})")
        self._tie_v, self._tie_f, self._tie_b, self._tie_w, self.k_tie = v, f, b, w, k
        self._dirty.add("ties")

    def sew(self, verts_a, verts_b, k, weights=None):
        """Vertex-to-vertex stitches: vertex verts_a[i] is tied to vertex verts_b[i] -- to the lowest-numbered face that contains verts_b[i], with a
        one-hot coordinate on it.  Replaces the tie list (set_ties)."""
        va = np.asarray(verts_a, np.int64).reshape(-1)
        vb = np.asarray(verts_b, np.int64).reshape(-1)
        if va.shape != vb.shape:
            raise ValueError(f"sew: {va.size} vertices onto {vb.size} vertices")
        tab = self.faces.to_numpy().reshape(-1, 3)
        faces, bary = [], np.zeros((len(vb), 3))
        for i, t in enumerate(vb.tolist()):
            hit = np.nonzero((tab == t).any(axis=1))[0]
            if not len(hit):
                raise ValueError(f"sew: vertex {t} (pair {i}) lies on no face of the scene")
            faces.append(int(hit[0]))
            bary[i, int(np.nonzero(tab[hit[0]] == t)[0][0])] = 1.0
        self.set_ties(va, np.array(faces, np.int64), bary, k, weights)

    def tie_force(self):
        """(n, 3): the force -k w_i r_i every tie applies to its vertex at the current positions"""
        return self._ensure_ctx().tie_force(self.pos.t)

    def tie_residuals(self):
        """(n, 3): r_i = x_v - sum_a b_a x_{t_a} at the current positions"""
        return self._ensure_ctx().tie_residuals(self.pos.t)

    def _push_ties(self):
        self._ctx.set_ties(self._tie_v, self._tie_f, self._tie_b, self._tie_w)
        self._ctx.set_param("k_tie", self.k_tie)

    # ------------------------------------------------------------------ half-space colliders (no counterpart in the reference)
    @property
    def n_collider(self):
        return len(self._col_o)

    def set_colliders(self, normals, offsets, mu, k, vertex_ids=None):
        """Up to 8 half-spaces n_j . x < o_j (the solid side) with friction coefficients mu_j >= 0 and one stiffness k >= 0 in N/m: a floor, a
        ramp, a plate that moves along its normal (set_collider_offsets before every step).  The shell is eps_contact thick, the friction is
        regularised with eps_v dt.  vertex_ids None: every collider acts on every vertex; else one entry per collider, None or a list of global
        vertex ids.  The normals are normalised and stay fixed; an empty list removes the colliders.  The lists are checked here, before any
        library call."""
        n, o, m, mask = validate_colliders(self.tot_NV, normals, offsets, mu, vertex_ids)
        k = _check_k("set_colliders", "k_collider", k)
        self._col_n, self._col_o, self._col_mu, self._col_mask, self.k_collider = n, o, m, mask, k
        self._dirty.add("colliders")

    def set_collider_offsets(self, offsets):
        """the offsets o_j of the next step (or energy, assembly, reverse step)"""
        o = np.asarray(offsets, dtype=np.float64).reshape(-1)
        if o.shape != (self.n_collider,):
            raise ValueError(f"set_collider_offsets: {o.size} offsets for {self.n_collider} colliders")
        for j in range(len(o)):
            if not np.isfinite(o[j]):
                raise ValueError(f"set_collider_offsets: offset {o[j]:g} of collider {j} is not finite")
        self._col_o = o.copy()
        self._dirty.add("collider_offsets")

    def collider_force(self):
        """(n, 3): the net force every plane applies to the cloth at the current positions and start-of-step positions (a plate under a resting cloth
        reads its weight along the normal)"""
        return self._ensure_ctx().collider_force(self.pos.t, self.prev_pos.t)

    def _push_colliders(self):
        self._ctx.set_colliders(self._col_n, self._col_o, self._col_mu, self._col_mask if self.n_collider else None)
        self._ctx.set_param("k_collider", self.k_collider)

    # ------------------------------------------------------------------ sphere colliders (no counterpart in the reference)
    @property
    def n_sphere(self):
        return len(self._sph_R)

    def set_spheres(self, centres, radii, mu, k, vertex_ids=None):
        """Up to 8 solid balls (centre, radius > 0, friction coefficient mu_j >= 0) with the cloth outside and one stiffness k >= 0 in N/m: a
        fingertip, a pusher, a mandrel, a roller that drags the sheet (set_sphere_centres before every step).  The shell is eps_contact thick, the
        friction is regularised with eps_v dt and acts on the slip relative to the ball.  vertex_ids None: every sphere acts on every vertex; else
        one entry per sphere, None or a list of global vertex ids.  The balls start at rest (previous centres = centres); the radii stay fixed; an
        empty list removes the spheres.  The lists are checked here, before any library call."""
        c, r, m, mask = validate_spheres(self.tot_NV, centres, radii, mu, vertex_ids)
        k = _check_k("set_spheres", "k_sphere", k)
        self._sph_c, self._sph_cp, self._sph_cp_step = c, c.copy(), c.copy()
        self._sph_R, self._sph_mu, self._sph_mask, self.k_sphere = r, m, mask, k
        self._dirty.add("spheres")

    def _check_centres(self, what, centres):
        c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        if c.shape != (self.n_sphere, 3):
            raise ValueError(f"set_sphere_centres: {len(c)} {what}s for {self.n_sphere} spheres")
        for j in range(len(c)):
            if not np.isfinite(c[j]).all():
                raise ValueError(f"set_sphere_centres: {what} ({c[j, 0]:g}, {c[j, 1]:g}, {c[j, 2]:g}) of sphere {j} is not finite")
        return c.copy()

    def set_sphere_centres(self, centres, prev_centres=None):
        """the centres c_j of the next step (or energy, assembly, reverse step).  Where the balls were at the start of that step is kept by the scene:
        the centres of the last completed step.  prev_centres overrides it (a tape puts a recorded step back; a caller restarts a rollout)."""
        c = self._check_centres("centre", centres)
        if prev_centres is not None:
            self._sph_cp = self._check_centres("previous centre", prev_centres)
        self._sph_c = c
        self._dirty.add("sphere_centres")

    def sphere_force(self):
        """(n, 3): the net force every ball applies to the cloth at the current positions and start-of-step positions (a ball under a resting cloth
        reads the weight it carries)"""
        return self._ensure_ctx().sphere_force(self.pos.t, self.prev_pos.t)

    def _push_spheres(self):
        self._ctx.set_spheres(self._sph_c, self._sph_R, self._sph_mu, self._sph_mask if self.n_sphere else None)
        self._ctx.set_sphere_centres(self._sph_c, self._sph_cp)
        self._ctx.set_param("k_sphere", self.k_sphere)

    def _spheres_step_done(self):
        """a step is complete: its centres are where the balls are at the start of the next one"""
        if self.n_sphere:
            self._sph_cp_step = self._sph_cp
            self._sph_cp = self._sph_c.copy()
            self._dirty.add("sphere_centres")

    # ------------------------------------------------------------------ capsule colliders (no counterpart in the reference)
    @property
    def n_capsule(self):
        return len(self._cap_R)

    def set_capsules(self, ends_a, ends_b, radii, mu, k, vertex_ids=None):
        """Up to 8 solid rods with round ends (endpoints a_j, b_j at least 1e-9 m apart, radius > 0, friction coefficient mu_j >= 0) with the cloth
        outside and one stiffness k >= 0 in N/m: a finger, a rod the cloth is folded over, a roller of finite length, a bar that sweeps a sheet
        (set_capsule_ends before every step; the two endpoints move independently).  The shell is eps_contact thick, the friction is regularised
        with eps_v dt and acts on the slip relative to the rod's material point under the vertex.  vertex_ids None: every capsule acts on every
        vertex; else one entry per capsule, None or a list of global vertex ids.  The rods start at rest (previous endpoints = endpoints); the radii
        stay fixed; an empty list removes the capsules.  The lists are checked here, before any library call."""
        a, b, r, m, mask = validate_capsules(self.tot_NV, ends_a, ends_b, radii, mu, vertex_ids)
        k = _check_k("set_capsules", "k_capsule", k)
        e = np.stack([a, b], axis=1)
        self._cap_e, self._cap_ep, self._cap_ep_step = e, e.copy(), e.copy()
        self._cap_R, self._cap_mu, self._cap_mask, self.k_capsule = r, m, mask, k
        self._dirty.add("capsules")

    def _check_ends(self, what, a, b):
        a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
        b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
        if a.shape != (self.n_capsule, 3) or b.shape != (self.n_capsule, 3):
            raise ValueError(f"set_capsule_ends: {len(a)} {what}endpoints a and {len(b)} {what}endpoints b for {self.n_capsule} capsules")
        for j in range(len(a)):
            bad = _capsule_ends_check("set_capsule_ends", what, a[j], b[j], j)
            if bad:
                raise ValueError(bad)
        return np.stack([a, b], axis=1)

    def set_capsule_ends(self, a, b, prev_a=None, prev_b=None):
        """the endpoints a_j, b_j of the next step (or energy, assembly, reverse step).  Where the rods were at the start of that step is kept by the
        scene: the endpoints of the last completed step.  prev_a and prev_b together override it (a tape puts a recorded step back; a caller
        restarts a rollout); one without the other is refused."""
        if (prev_a is None) != (prev_b is None):
            raise ValueError("set_capsule_ends: previous endpoints " + ("a without previous endpoints b" if prev_b is None else "b without previous endpoints a"))
        e = self._check_ends("", a, b)
        if prev_a is not None:
            self._cap_ep = self._check_ends("previous ", prev_a, prev_b)
        self._cap_e = e
        self._dirty.add("capsule_ends")

    def capsule_force(self):
        """(n, 6): the net force every rod applies to the cloth at the current positions and start-of-step positions, and its torque about the rod's
        midpoint (a level rod under a resting cloth reads the weight it carries and how unevenly it carries it)"""
        return self._ensure_ctx().capsule_force(self.pos.t, self.prev_pos.t)

    def _push_capsules(self):
        self._ctx.set_capsules(self._cap_e[:, 0], self._cap_e[:, 1], self._cap_R, self._cap_mu, self._cap_mask if self.n_capsule else None)
        self._ctx.set_capsule_ends(self._cap_e[:, 0], self._cap_e[:, 1], self._cap_ep[:, 0], self._cap_ep[:, 1])
        self._ctx.set_param("k_capsule", self.k_capsule)

    def _capsules_step_done(self):
        """a step is complete: its endpoints are where the rods are at the start of the next one"""
        if self.n_capsule:
            self._cap_ep_step = self._cap_ep
            self._cap_ep = self._cap_e.copy()
            self._dirty.add("capsule_ends")

    # ------------------------------------------------------------------ rounded-box colliders (no counterpart in the reference)
    @property
    def n_box(self):
        return len(self._box_r)

    def set_boxes(self, centres, quats, half_extents, radii, mu, k, vertex_ids=None):
        """Up to 8 solid boxes with rounded edges and corners (centre, quaternion (s, x, y, z), half extents >= 0 of the core box, rounding radius > 0,
        friction coefficient mu_j >= 0) with the cloth outside and one stiffness k >= 0 in N/m: a table top whose edge the cloth hangs over, a shelf,
        a step, a gripper jaw, a plate that tilts (set_box_poses or move_boxes before every step).  The solid is the core box grown by the radius;
        there is no sharp box.  The shell is eps_contact thick, the friction is regularised with eps_v dt and acts on the slip relative to the
        box's material point under the vertex.  A vertex inside the core box, deeper than the radius, feels nothing: the limit of the model.
        vertex_ids None: every box acts on every vertex; else one entry per box, None or a list of global vertex ids.  The boxes start at rest
        (previous poses = poses); half extents and radii stay fixed; an empty list removes the boxes.  The lists are checked here, before any
        library call."""
        c, q, h, r, m, mask = validate_boxes(self.tot_NV, centres, quats, half_extents, radii, mu, vertex_ids)
        k = _check_k("set_boxes", "k_box", k)
        self._box_c, self._box_cp, self._box_cp_step = c, c.copy(), c.copy()
        self._box_q, self._box_qp, self._box_qp_step = q, q.copy(), q.copy()
        self._box_h, self._box_r, self._box_mu, self._box_mask, self.k_box = h, r, m, mask, k
        self._dirty.add("boxes")

    def _check_box_poses(self, what, centres, quats):
        c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        q = np.array(quats, dtype=np.float64).reshape(-1, 4)
        if c.shape != (self.n_box, 3) or q.shape != (self.n_box, 4):
            raise ValueError(f"set_box_poses: {len(c)} {what}centres and {len(q)} {what}quaternions for {self.n_box} boxes")
        for j in range(len(c)):
            bad = _box_pose_check("set_box_poses", what, c[j], q[j], j)
            if bad:
                raise ValueError(bad)
            q[j] = quat_normalize(q[j])
        return c.copy(), q

    def set_box_poses(self, centres, quats, prev_centres=None, prev_quats=None):
        """the poses of the next step (or energy, assembly, reverse step).  Where the boxes were at the start of that step is kept by the scene: the
        poses of the last completed step.  prev_centres and prev_quats together override it (a tape puts a recorded step back; a caller restarts a
        rollout); one without the other is refused."""
        if (prev_centres is None) != (prev_quats is None):
            raise ValueError("set_box_poses: previous " + ("centres without previous quaternions" if prev_quats is None else "quaternions without previous centres"))
        c, q = self._check_box_poses("", centres, quats)
        if prev_centres is not None:
            self._box_cp, self._box_qp = self._check_box_poses("previous ", prev_centres, prev_quats)
        self._box_c, self._box_q = c, q
        self._dirty.add("box_poses")

    def move_boxes(self, delta_pos, delta_theta):
        """the poses of the next step from those in place: c += delta_pos, R <- exp([delta_theta]x) R per box (frames.compose: world-frame rotation
        vectors applied on the left, the convention of box_pose_grad)"""
        dp = np.asarray(delta_pos, dtype=np.float64).reshape(-1, 3)
        dth = np.asarray(delta_theta, dtype=np.float64).reshape(-1, 3)
        if dp.shape != (self.n_box, 3) or dth.shape != (self.n_box, 3):
            raise ValueError(f"move_boxes: {len(dp)} translations and {len(dth)} rotation vectors for {self.n_box} boxes")
        if self.n_box:
            self.set_box_poses(*compose(self._box_c, self._box_q, dp, dth))

    def box_force(self):
        """(n, 6): the net force every box applies to the cloth at the current positions and start-of-step positions, and its torque about the box's
        centre (a level plate under a resting cloth reads the weight it carries and where it carries it)"""
        return self._ensure_ctx().box_force(self.pos.t, self.prev_pos.t)

    def _push_boxes(self):
        self._ctx.set_boxes(self._box_c, self._box_q, self._box_h, self._box_r, self._box_mu, self._box_mask if self.n_box else None)
        self._ctx.set_box_poses(self._box_c, self._box_q, self._box_cp, self._box_qp)
        self._ctx.set_param("k_box", self.k_box)

    def _boxes_step_done(self):
        """a step is complete: its poses are where the boxes are at the start of the next one"""
        if self.n_box:
            self._box_cp_step, self._box_qp_step = self._box_cp, self._box_qp
            self._box_cp, self._box_qp = self._box_c.copy(), self._box_q.copy()
            self._dirty.add("box_poses")

    # ------------------------------------------------------------------ sampled distance-field colliders (no counterpart in the reference)
    @property
    def n_sdf(self):
        return len(self._sdf_r)

    def set_sdfs(self, grids, origins, spacings, centres, quats, offsets, mu, k, vertex_ids=None):
        """Up to 8 solids given as sampled distance fields, with the cloth outside and one stiffness k >= 0 in N/m: a mould a sheet is formed into, a bowl,
        a ring, a shoulder -- any solid, concave ones included (engine/sdf.py samples analytic fields).  grids[j]: a 3-d array of samples in C order,
        every dimension in [4, 512]; origins[j]: the local position of sample (0, 0, 0); spacings[j] > 0; the solid is {phi < offsets[j]} with phi the
        cubic B-spline over the samples (the samples are its control values: a curved field is smoothed by about h^2/6 times its Laplacian).  Poses:
        centre and quaternion (s, x, y, z) (set_sdf_poses or move_sdfs before every step); friction mu_j >= 0 acts on the slip relative to the field's
        material point under the vertex.  Outside 1 <= t < n - 2 grid cells a vertex feels nothing: keep the solid inside (sdf.border_clear).
        vertex_ids None: every field acts on every vertex; else one entry per field, None or a list of global vertex ids.  The fields start at rest
        (previous poses = poses); an empty list removes them.  The lists are checked here, before any library call."""
        g, o, h, c, q, r, m, mask = validate_sdfs(self.tot_NV, grids, origins, spacings, centres, quats, offsets, mu, vertex_ids)
        k = _check_k("set_sdfs", "k_sdf", k)
        self._sdf_c, self._sdf_cp, self._sdf_cp_step = c, c.copy(), c.copy()
        self._sdf_q, self._sdf_qp, self._sdf_qp_step = q, q.copy(), q.copy()
        self._sdf_grids, self._sdf_o, self._sdf_h, self._sdf_r, self._sdf_mu, self._sdf_mask, self.k_sdf = g, o, h, r, m, mask, k
        self._dirty.add("sdfs")

    def _check_sdf_poses(self, what, centres, quats):
        c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        q = np.array(quats, dtype=np.float64).reshape(-1, 4)
        if c.shape != (self.n_sdf, 3) or q.shape != (self.n_sdf, 4):
            raise ValueError(f"set_sdf_poses: {len(c)} {what}centres and {len(q)} {what}quaternions for {self.n_sdf} fields")
        for j in range(len(c)):
            bad = _box_pose_check("set_sdf_poses", what, c[j], q[j], j, "field")
            if bad:
                raise ValueError(bad)
            q[j] = quat_normalize(q[j])
        return c.copy(), q

    def set_sdf_poses(self, centres, quats, prev_centres=None, prev_quats=None):
        """the poses of the next step (or energy, assembly, reverse step).  Where the fields were at the start of that step is kept by the scene: the
        poses of the last completed step.  prev_centres and prev_quats together override it (a tape puts a recorded step back; a caller restarts a
        rollout); one without the other is refused."""
        if (prev_centres is None) != (prev_quats is None):
            raise ValueError("set_sdf_poses: previous " + ("centres without previous quaternions" if prev_quats is None else "quaternions without previous centres"))
        c, q = self._check_sdf_poses("", centres, quats)
        if prev_centres is not None:
            self._sdf_cp, self._sdf_qp = self._check_sdf_poses("previous ", prev_centres, prev_quats)
        self._sdf_c, self._sdf_q = c, q
        self._dirty.add("sdf_poses")

    def move_sdfs(self, delta_pos, delta_theta):
        """the poses of the next step from those in place: c += delta_pos, R <- exp([delta_theta]x) R per field (frames.compose: world-frame rotation
        vectors applied on the left, the convention of sdf_pose_grad)"""
        dp = np.asarray(delta_pos, dtype=np.float64).reshape(-1, 3)
        dth = np.asarray(delta_theta, dtype=np.float64).reshape(-1, 3)
        if dp.shape != (self.n_sdf, 3) or dth.shape != (self.n_sdf, 3):
            raise ValueError(f"move_sdfs: {len(dp)} translations and {len(dth)} rotation vectors for {self.n_sdf} fields")
        if self.n_sdf:
            self.set_sdf_poses(*compose(self._sdf_c, self._sdf_q, dp, dth))

    def sdf_force(self):
        """(n, 6): the net force every field's solid applies to the cloth at the current positions and start-of-step positions, and its torque about
        the field's centre"""
        return self._ensure_ctx().sdf_force(self.pos.t, self.prev_pos.t)

    def _push_sdfs(self):
        self._ctx.set_sdfs(self._sdf_grids, self._sdf_o, self._sdf_h, self._sdf_c, self._sdf_q, self._sdf_r, self._sdf_mu, self._sdf_mask if self.n_sdf else None)
        self._ctx.set_sdf_poses(self._sdf_c, self._sdf_q, self._sdf_cp, self._sdf_qp)
        self._ctx.set_param("k_sdf", self.k_sdf)

    def _sdfs_step_done(self):
        """a step is complete: its poses are where the fields are at the start of the next one"""
        if self.n_sdf:
            self._sdf_cp_step, self._sdf_qp_step = self._sdf_cp, self._sdf_qp
            self._sdf_cp, self._sdf_qp = self._sdf_c.copy(), self._sdf_q.copy()
            self._dirty.add("sdf_poses")

    # ------------------------------------------------------------------ wind (no counterpart in the reference)
    @property
    def n_wind(self):
        return len(self._wind_f)

    def set_wind(self, c_n, c_t, face_ids=None, weights=None):
        """Opt-in wind: lagged linear aerodynamic drag on cloth faces.  A listed face f with the start-of-step area vector a (area A0, normal n0) feels
        the force w_f A0 (c_n n0 n0^T + c_t (I - n0 n0^T)) (W - u), u its centroid velocity over the step and W the wind velocity
        (set_wind_velocity, one per step and scene); c_n, c_t >= 0 in N s / m^3 are the normal and the tangential drag coefficient.  face_ids None:
        every cloth face (Cloth.faces() gives one cloth's); else global ids of cloth faces, each once; weights None: 1 each.  An empty list removes
        the wind; with c_n = c_t = 0 nothing is launched.  Not modelled: drag quadratic in speed, a wind that varies in space (the weights are the
        only spatial handle), faces of FEM bodies (refused), gradients for the weights.  The lists are checked here, before any library call."""
        n_cf = sum(c.NF for c in self.cloths)
        self.wind_cn, self.wind_ct, self._wind_f, self._wind_w = validate_wind(n_cf, self.tot_NF, c_n, c_t, face_ids, weights)
        self._dirty.add("wind")

    def set_wind_velocity(self, W):
        """the wind velocity (3,), m / s, of the steps from now on (a Grad tape records it per step)"""
        self._wind_W = validate_wind_velocity(W)
        self._dirty.add("wind_velocity")

    def wind_force(self):
        """(3,): the net force the wind applies to the cloth at the current positions and start-of-step positions"""
        return self._ensure_ctx().wind_force(self.pos.t, self.prev_pos.t)

    def _push_wind(self):
        self._ctx.set_wind(self._wind_f, self._wind_w)
        self._ctx.set_wind_velocity(self._wind_W)
        self._ctx.set_param("wind_cn", self.wind_cn)
        self._ctx.set_param("wind_ct", self.wind_ct)

    # ------------------------------------------------------------------ rigid frames for the handles (no counterpart in the reference)
    @property
    def n_frame(self):
        return len(self._frame_pos)

    def set_handle_frames(self, frame_ids, local_points=None, n_frames=None):
        """Put handles on rigid frames: handle i belongs to frame frame_ids[i] in [0, n_frames) with the local point local_points[i], or stays a free
        handle with a world target (frame id -1).  The target of a framed handle is c + R(q) r_i with the frame's pose (c, q) (set_frame_poses,
        move_frames).  n_frames None: largest id + 1; n_frames = 0 (or all ids -1 with n_frames None) removes the frames.  local_points None grasps
        the handled points where they are: r_i = R^T (p_i - c) at the current poses.  Poses are kept when the number of frames stays, and
        start at the identity at the origin otherwise.  The lists are checked here, before any library call."""
        f = np.asarray(frame_ids)
        if n_frames is None:
            n_frames = int(f.max()) + 1 if f.ndim == 1 and f.size and np.issubdtype(f.dtype, np.integer) else 0
        if int(n_frames) != self.n_frame:
            pos, quat = np.zeros((int(max(n_frames, 0)), 3)), np.tile([1.0, 0.0, 0.0, 0.0], (int(max(n_frames, 0)), 1))
        else:
            pos, quat = self._frame_pos, self._frame_quat
        if local_points is None:
            local_points = np.zeros((self.n_handle, 3))
            if f.shape == (self.n_handle,) and self.n_handle:
                x = self.handle_points()
                for i, fi in enumerate(f.tolist()):
                    if 0 <= fi < len(pos):
                        local_points[i] = quat_to_rotmat(quat[fi]).T @ (x[i] - pos[fi])
        f, r = validate_frames(self.n_handle, f, local_points, n_frames)
        self._frame_of, self._frame_local, self._frame_pos, self._frame_quat = f, r, pos, quat
        self._handle_t = self._framed(self._handle_t)
        self._dirty.add("handle_frames")

    def set_frame_poses(self, pos, quat):
        """position (n_frame, 3) and quaternion (n_frame, 4) = (s, x, y, z) of every frame, in the convention of gripper_single.quat_to_rotmat; the
        quaternions are normalised, a zero or non-finite one raises.  Moves the targets of the framed handles for the next energy, assembly, time
        step or reverse step; the engine context receives the poses at its next use."""
        self._frame_pos, self._frame_quat = validate_poses(self.n_frame, pos, quat)
        self._handle_t = self._framed(self._handle_t)
        self._dirty.add("frame_poses")

    def frame_poses(self):
        """(positions (n_frame, 3), unit quaternions (n_frame, 4)), copies"""
        return self._frame_pos.copy(), self._frame_quat.copy()

    def move_frames(self, delta_pos, delta_theta):
        """c <- c + delta_pos, q <- exp(delta_theta / 2) (x) q renormalised, per frame: delta_theta (n_frame, 3) is a world-frame rotation vector
        applied on the left, the variable of the rotation block of frame_grad"""
        dp, dt = np.asarray(delta_pos, dtype=np.float64), np.asarray(delta_theta, dtype=np.float64)
        if dp.shape != (self.n_frame, 3) or dt.shape != (self.n_frame, 3):
            raise ValueError(f"move_frames: steps of shape {dp.shape} and {dt.shape} for {self.n_frame} frames (expected ({self.n_frame}, 3) twice)")
        self.set_frame_poses(*compose(self._frame_pos, self._frame_quat, dp, dt))

    def frame_wrench(self):
        """(n_frame, 6): force and moment about the frame's position that the handles of every frame apply to the cloth at the current positions"""
        return self._ensure_ctx().frame_wrench(self.pos.t)

    def _framed(self, t):
        """the targets t with the rows of framed handles at c + R r (the host's copy of what k_frame_targets writes)"""
        return frame_targets(t, self._frame_of, self._frame_local, self._frame_pos, self._frame_quat) if self.n_frame else t

    def _push_frames(self):
        if self.n_frame or getattr(self._ctx, "n_frame", 0):
            self._ctx.set_handle_frames(self._frame_of, self._frame_local, self.n_frame)
            self._ctx.set_frame_poses(self._frame_pos, self._frame_quat)

    def set_frozen_kernel(self):
        # BaseScene.py:1445-1463
        fr = self.frozen.t.view(-1, 3)
        e0 = self.elastics[0]
        fr[e0.offset:e0.offset + e0.n_verts] = 1
        for j in (1, 2):
            e = self.elastics[j]
            fr[e.offset:e.offset + e.n_verts][torch.as_tensor(e.bound_mask())] = 1

    def set_frozen(self):
        self.frozen.t.zero_()
        self.set_frozen_kernel()
        self._dirty.add("frozen")

    def set_ext_force(self):
        self.ext_force.t.zero_()
        for c in self.cloths:
            c.clear_manipulation()
        self._dirty.add("ext_force")

    def update_visual(self):
        self.x32.t.copy_(self.pos.t.detach().to("cpu", torch.float32))

    # ------------------------------------------------------------------ stepping
    def push_down_pos(self):
        pass  # per-body arrays are views of self.pos

    def push_down_vel(self):
        pass

    def pushup_property(self, dest, src, offset):
        if dest.t.data_ptr() != src.t.data_ptr():  # already aliased when src is a bound body field
            dest.t[offset:offset + src.t.shape[0]].copy_(src.t.to(dest.t.device))

    def _state(self):
        return self.pos.t, self.prev_pos.t, self.vel.t, self._ref_angle

    def compute_energy(self):
        e = self._ensure_ctx().energy(*self._state())
        self.E[None] = e
        return e

    def compute_residual_and_Hessian(self, check_PD=False, iter=0, spd=True):
        self._ensure_ctx().assemble(*self._state(), spd=spd, grad=self.F.t)
        return True

    def compute_Hessian(self, spd=True):
        self._ensure_ctx().assemble(*self._state(), spd=spd, grad=None)

    def calc_vn(self):
        pass  # part of contact detection inside the context

    def contact_analysis(self):
        pass

    def update_ref_angle(self):
        self._ensure_ctx().update_ref_angle(self.pos.t, self._ref_angle)

    def time_step(self, f_contact, frame_idx, force_stick=True):
        """BaseScene.time_step (BaseScene.py:1327-1370).  ``f_contact`` is ``geometry.projection_query``; the
        detection it stands for runs inside tsl_step (None disables contact)."""
        ctx = self._ensure_ctx()
        ctx.set_param("contact", 0.0 if f_contact is None else 1.0)
        st = ctx.step(*self._state())
        self._spheres_step_done()
        self._capsules_step_done()
        self._boxes_step_done()
        self._sdfs_step_done()
        self.last_stats = st
        self.nc[None] = st["nc"]
        self.E[None] = st["energy"]
        return st

    def action(self, step, delta_pos, delta_rot, delta_dis=None):
        # BaseScene.py:1489-1500
        self.gripper.step_simple(delta_pos, delta_rot)
        self.gripper.update_bound(self)

    # ------------------------------------------------------------------ adjoint helpers (BaseScene.py:270-315)
    def copy_pos_kernel(self, target_pos, step):
        self.pos.t.copy_(target_pos.t[step])

    def copy_prev_pos_kernel(self, target_pos, step):
        self.prev_pos.t.copy_(target_pos.t[step - 1])

    def copy_pos_only(self, target_pos, step):
        self.copy_pos_kernel(target_pos, step)
        self.copy_prev_pos_kernel(target_pos, step + 1)

    def copy_pos_and_refangle(self, analy_grad, step):
        self.copy_pos_kernel(analy_grad.pos_buffer, step)
        self.copy_prev_pos_kernel(analy_grad.pos_buffer, step)
        rb = analy_grad.ref_angle_buffer.t[step - 1].reshape(-1, 3)
        self._ref_angle[: rb.shape[0]].copy_(rb)

    def copy_refangle(self, analy_grad, step):
        rb = analy_grad.ref_angle_buffer.t[step].reshape(-1, 3)
        self._ref_angle[: rb.shape[0]].copy_(rb)

    # ------------------------------------------------------------------ misc surface kept for the scripts
    def compute_reward(self):
        c = self.cloths[0]
        return float(c.pos.t[:, 2].sum().item())

    def check_pos_nan(self):
        return bool(torch.isnan(self.pos.t).any().item())

    def gather_force(self):
        """BaseScene.py:1541-1549: sum of Elastic.get_force over the gripper-driven vertices of every effector pad"""
        f = self._ensure_ctx().elastic_force(self.pos.t, torch.empty_like(self.pos.t)).cpu().numpy()
        tot = np.zeros((self.effector_cnt - 1, 3))
        for j in range(1, self.effector_cnt):
            e = self.elastics[j]
            tot[j - 1] = f[e.offset:e.offset + e.n_verts][e.bound_mask()].sum(0)
        self.tot_force.from_numpy(tot)
        return tot

    def check_early_stop(self, frame, ifprint=False, RL=False):
        # BaseScene.py:1559-1584
        if self.check_pos_nan():
            if ifprint:
                print("exist nan")
            return True
        if self.effector_cnt - 1 <= 0:
            return False
        tot = self.gather_force()
        for i in range(self.effector_cnt - 1):
            if (np.abs(tot[i]) > 10).any():
                if ifprint:
                    print("too much force")
                return True
            if np.sqrt((tot[i] ** 2).sum()) < 0.2 and frame > 10 and not RL:
                if ifprint:
                    print("no contact")
                return True
        return False

    def get_observation_kernel(self):
        # BaseScene.py:1586-1619 (cloth samples index pos[jj * cloth_N + kk] -- cloth_N, not M + 1 -- and the elastic sample
        # index (n_verts // n_obs_elastic) * j - 1 is -1 for j = 0, i.e. the last vertex: both kept; on non-square cloths such as
        # the 15x7 balancing sheet the cloth index runs past NV -- an unchecked out-of-range read in the reference, zeros here)
        obs = np.zeros(self.obs_dim)
        no = self.n_obs_cloth
        for i, c in enumerate(self.cloths):
            x = c.pos.to_numpy(); v = c.vel.to_numpy()
            for j in range(no):
                for k in range(no):
                    xx = i * no * no + j * no + k
                    jj = self.n_sample_cloth // 2 + j * self.n_sample_cloth
                    kk = self.m_sample_cloth // 2 + k * self.m_sample_cloth
                    q = jj * self.cloth_N + kk
                    if q < c.NV:
                        obs[xx * 6:xx * 6 + 3] = x[q]
                        obs[xx * 6 + 3:xx * 6 + 6] = v[q]
        for i, e in enumerate(self.elastics):
            x = e.F_x.to_numpy(); v = e.F_v.to_numpy()
            for j in range(self.n_obs_elastic):
                xx = no * no * self.cloth_cnt + i * self.n_obs_elastic + j
                ii = (e.n_verts // self.n_obs_elastic) * j - 1
                obs[xx * 6:xx * 6 + 3] = x[ii]
                obs[xx * 6 + 3:xx * 6 + 6] = v[ii]
        base = (no * no * self.cloth_cnt + self.elastic_cnt * self.n_obs_elastic) * 6
        gp = self.gripper.pos.to_numpy(); gr = self.gripper.rot.to_numpy()
        for j in range(self.gripper.n_part):
            obs[base + j * 7: base + j * 7 + 3] = gp[j]
            obs[base + j * 7 + 3: base + j * 7 + 7] = gr[j]
        self.observation.from_numpy(obs)
        return obs

    def get_observation(self):
        return self.get_observation_kernel()

    def save_state(self, save_path):
        torch.save({'pos': self.pos.to_torch('cpu'), 'vel': self.vel.to_torch('cpu')}, save_path)

    def load_state(self, save_path):
        data = torch.load(save_path)
        self.pos.t.copy_(data['pos'].to(self.pos.t.device))
        self.vel.t.copy_(data['vel'].to(self.vel.t.device))
        self.update_ref_angle()   # BaseScene.py:1376-1384: the loaded pose also moves the plastic rest angles
        self.update_visual()
