"""Thin object wrapper over the C ABI: owns one ``tsl_ctx`` (one scene on one GPU).

State (pos / prev_pos / vel / ref_angle) stays in caller-owned torch tensors resident in HBM; this
class only passes ``data_ptr()``s.  torch is plumbing here (device memory, streams), not compute.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import Body, ClothDesc, ContactPair, ElasticDesc, SceneDesc, SolveStats, StepStats, check


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(t):
    """device/host pointer of a torch tensor or numpy array (or None)."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous(), "tensor must be contiguous"
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def scene_desc(*, tot_NV, dt, mass, gravity, frozen, cloths=(), elastics=(), faces=None, bodies=(), pairs=(),
               k_contact=1000.0, eps_contact=1e-3, eps_v=0.01, damping=1.0, max_n_constraints=10000, grid_h=0.003, device=None):
    """The ``SceneDesc`` that tsl_ctx_create reads, and the list of objects its pointers refer to (keep it alive as long as the description is used).
    Host work only: neither a GPU nor the library is needed (`device` is accepted and ignored, so that the arguments are those of TslContext).
    cloths: dicts with N, M, NV, NF, v_offset, dx, mass, Kl, Ka, Kb, k_angle, f2v, counter_face, counter_point, rest_area, rest_len
    elastics: dicts with kind, n_verts, n_cells, v_offset, mu, lam, alpha, tets, B, W
    bodies: (v_start, v_end, f_start, f_end); pairs: (b_idx, v_start, v_end, mu or None[, factor on mu_cloth_elastic])"""
    keep = []
    cl = (ClothDesc * max(len(cloths), 1))()
    for i, c in enumerate(cloths):
        arrs = [_np(c["f2v"], np.int32), _np(c["counter_face"], np.int32), _np(c["counter_point"], np.int32),
                _np(c["rest_area"], np.float64), _np(c["rest_len"], np.float64)]
        keep += arrs
        cl[i] = ClothDesc(c["N"], c["M"], c["NV"], c["NF"], c["v_offset"], c["dx"], c["mass"], c["Kl"], c["Ka"], c["Kb"], c["k_angle"],
                          *[a.ctypes.data for a in arrs])
    el = (ElasticDesc * max(len(elastics), 1))()
    for i, e in enumerate(elastics):
        arrs = [_np(e["tets"], np.int32), _np(e["B"], np.float64), _np(e["W"], np.float64)]
        keep += arrs
        el[i] = ElasticDesc(e["kind"], e["n_verts"], e["n_cells"], e["v_offset"], e["mu"], e["lam"], e["alpha"], *[a.ctypes.data for a in arrs])
    bd = (Body * max(len(bodies), 1))()
    for i, b in enumerate(bodies):
        bd[i] = Body(*[int(x) for x in b])
    pr = (ContactPair * max(len(pairs), 1))()
    for i, p in enumerate(pairs):
        mu = p[3]   # float: fixed; None: live mu_cloth_elastic; "cloth_cloth": live mu_cloth_cloth
        factor = float(p[4]) if len(p) > 4 else 0.0
        kind = 0 if isinstance(mu, (int, float)) else (2 if mu == "cloth_cloth" else 1)
        pr[i] = ContactPair(int(p[0]), int(p[1]), int(p[2]), kind, float(mu) if kind == 0 else factor)
    faces = _np(faces if faces is not None else np.zeros((0, 3)), np.int32)
    mass = _np(mass, np.float64); gravity = _np(gravity, np.float64); frozen = _np(frozen, np.int32)
    assert mass.shape == (tot_NV,) and gravity.shape == (tot_NV, 3) and frozen.shape == (3 * tot_NV,)
    d = SceneDesc(tot_NV, len(faces), dt, k_contact, eps_contact, eps_v, damping, int(max_n_constraints),
                  len(cloths), cl, len(elastics), el, len(bodies), bd, len(pairs), pr,
                  mass.ctypes.data, gravity.ctypes.data, faces.ctypes.data, frozen.ctypes.data, grid_h)
    keep += [cl, el, bd, pr, faces, mass, gravity, frozen]
    return d, keep


class TslContext:
    def __init__(self, *, device="cuda:0", **scene):
        """scene: the keyword arguments of scene_desc (tot_NV, dt, mass, gravity, frozen, cloths, elastics, faces, bodies, pairs and the scalars)"""
        self.L = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.TslLibraryError("no HIP device visible: thinshelllab_amd has no CPU path")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        d, self._keep = scene_desc(**scene)
        self.tot_NV = int(d.tot_NV)
        self.h = C.c_void_p()
        check(self.L.tsl_ctx_create(C.byref(d), C.byref(self.h)), "tsl_ctx_create")
        self.n_body = d.n_body
        self.n_cface = sum(d.cloths[i].NF for i in range(d.n_cloth))
        self.dt = scene["dt"]
        self.max_n_constraints = d.max_n_constraints
        self.L.tsl_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        # solver switches for A/B runs of unchanged drivers: TSL_PARAMS="key=value,key=value" (keys of tsl_set_param)
        for kv in os.environ.get("TSL_PARAMS", "").split(","):
            if "=" in kv:
                k, v = kv.split("=", 1)
                self.set_param(k.strip(), float(v))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            g = getattr(self, "_group", None)
            if g is not None:   # member of a scene group: the group goes first (the members get buffers of their own again)
                g.close()
            self.L.tsl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters
    def set_param(self, key, value):
        check(self.L.tsl_set_param(self.h, key.encode(), float(value)), f"tsl_set_param({key})")

    def set_frozen(self, frozen):
        f = _np(frozen, np.int32)
        check(self.L.tsl_set_frozen(self.h, f.ctypes.data), "tsl_set_frozen")

    def set_ext_force(self, f):
        f = _np(f, np.float64)
        check(self.L.tsl_set_ext_force(self.h, f.ctypes.data), "tsl_set_ext_force")

    def set_gravity(self, g):
        g = _np(g, np.float64)
        check(self.L.tsl_set_gravity(self.h, g.ctypes.data), "tsl_set_gravity")

    # ---- soft handles (tsl_set_handles; stiffness: set_param("k_handle", k))
    def set_handles(self, verts, weights=None):
        """n handles on the global vertex ids `verts` (at most one per vertex), weights None: all 1; an empty list removes them.  Targets start at zero."""
        v = _np(verts, np.int32).reshape(-1)
        w = None if weights is None else _np(weights, np.float64).reshape(-1)
        assert w is None or w.shape == v.shape, (v.shape, w.shape)
        check(self.L.tsl_set_handles(self.h, v.ctypes.data if len(v) else None, None if w is None or not len(v) else w.ctypes.data, len(v)), "tsl_set_handles")
        self.n_handle = len(v)
        self.n_frame = 0   # (the library drops the frames with the handle list)

    def set_handles_on_faces(self, faces, bary, weights=None):
        """n handles at the barycentric points `bary` (n, 3) of the global face ids `faces` (any number per face or vertex), weights None: all 1; an
        empty list removes them.  Replaces a vertex list, drops the frames; targets start at zero."""
        f = _np(faces, np.int32).reshape(-1)
        b = _np(bary, np.float64).reshape(-1, 3)
        w = None if weights is None else _np(weights, np.float64).reshape(-1)
        assert b.shape == (len(f), 3) and (w is None or w.shape == f.shape), (f.shape, b.shape)
        n = len(f)
        check(self.L.tsl_set_handles_on_faces(self.h, f.ctypes.data if n else None, b.ctypes.data if n else None,
                                              None if w is None or not n else w.ctypes.data, n), "tsl_set_handles_on_faces")
        self.n_handle = n
        self.n_frame = 0   # (the library drops the frames with the handle list)

    def handle_points(self, pos):
        """(n, 3) the points the handles act on at the state pos: sum_a b_a x_{v_a} of a face list, x_{v_i} of a vertex list"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_handle", 0), 3))
        check(self.L.tsl_handle_points(self.h, _ptr(pos), out.ctypes.data), "tsl_handle_points")
        return out

    def set_handle_targets(self, targets):
        t = _np(targets, np.float64)
        assert t.shape == (getattr(self, "n_handle", 0), 3), t.shape
        if len(t):
            check(self.L.tsl_set_handle_targets(self.h, t.ctypes.data), "tsl_set_handle_targets")

    def handle_force(self, pos):
        """(n, 3) k_handle w_i (t_i - x_{v_i}): the force every handle applies to the cloth at the state pos (frozen dofs not masked)"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_handle", 0), 3))
        check(self.L.tsl_handle_force(self.h, _ptr(pos), out.ctypes.data), "tsl_handle_force")
        return out

    def handle_grad(self, p=None):
        """(n, 3) contribution of one reverse step to d(loss)/d(target): k_handle w_i p_{v_i} on free dofs, 0 on frozen ones; p None: the solution of
        the last adjoint_step, else a 3 * tot_NV device vector"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_handle", 0), 3))
        check(self.L.tsl_handle_grad(self.h, _ptr(p), out.ctypes.data), "tsl_handle_grad")
        return out

    # ---- rigid frames of the handles (tsl_set_handle_frames)
    def set_handle_frames(self, frame_of_handle, local_points, n_frame):
        """frame of every handle (-1: free) and its local point (n_handle, 3); n_frame = 0 removes all frames.  Poses start at the identity."""
        n_frame = int(n_frame)
        if n_frame == 0:
            check(self.L.tsl_set_handle_frames(self.h, None, None, 0), "tsl_set_handle_frames")
        else:
            f = _np(frame_of_handle, np.int32).reshape(-1)
            r = _np(local_points, np.float64)
            assert f.shape == (getattr(self, "n_handle", 0),) and r.shape == (len(f), 3), (f.shape, r.shape)
            check(self.L.tsl_set_handle_frames(self.h, f.ctypes.data if len(f) else None, r.ctypes.data if len(f) else None, n_frame), "tsl_set_handle_frames")
        self.n_frame = n_frame

    def set_frame_poses(self, pos, quat):
        """positions (n_frame, 3) and quaternions (n_frame, 4) = (s, x, y, z), normalised by the library; rewrites the targets of the framed handles"""
        c = _np(pos, np.float64)
        q = _np(quat, np.float64)
        assert c.shape == (getattr(self, "n_frame", 0), 3) and q.shape == (len(c), 4), (c.shape, q.shape)
        if len(c):
            self.refresh_stream()
            check(self.L.tsl_set_frame_poses(self.h, c.ctypes.data, q.ctypes.data), "tsl_set_frame_poses")

    def handle_targets(self):
        """(n, 3) the targets as they stand: what was set for free handles, c + R r for framed ones"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_handle", 0), 3))
        check(self.L.tsl_handle_targets(self.h, out.ctypes.data), "tsl_handle_targets")
        return out

    def frame_wrench(self, pos):
        """(n_frame, 6) force and moment about the frame's position that its handles apply to the cloth at the state pos (frozen dofs not masked)"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_frame", 0), 6))
        check(self.L.tsl_frame_wrench(self.h, _ptr(pos), out.ctypes.data), "tsl_frame_wrench")
        return out

    def frame_grad(self, p=None):
        """(n_frame, 6) contribution of one reverse step to d(loss)/d(position) and d(loss)/d(world rotation vector applied on the left) of every
        frame; p None: the solution of the last adjoint_step, else a 3 * tot_NV device vector"""
        self.refresh_stream()
        out = np.zeros((getattr(self, "n_frame", 0), 6))
        check(self.L.tsl_frame_grad(self.h, _ptr(p), out.ctypes.data), "tsl_frame_grad")
        return out

    # ---- ties (tsl_set_ties; stiffness: set_param("k_tie", k))
    def set_ties(self, verts, faces, bary, weights=None):
        """n ties: global vertex verts[i] to the barycentric point bary[i] of the global face faces[i]; weights None: all 1; an empty list removes them"""
        v = _np(verts, np.int32).reshape(-1)
        f = _np(faces, np.int32).reshape(-1)
        b = _np(bary, np.float64).reshape(-1, 3)
        w = None if weights is None else _np(weights, np.float64).reshape(-1)
        n = len(v)
        assert f.shape == v.shape and b.shape == (n, 3) and (w is None or w.shape == v.shape), (v.shape, f.shape, b.shape)
        check(self.L.tsl_set_ties(self.h, v.ctypes.data if n else None, f.ctypes.data if n else None, b.ctypes.data if n else None,
                                  None if w is None or not n else w.ctypes.data, n), "tsl_set_ties")

    def tie_count(self):
        out = C.c_int32(0)
        check(self.L.tsl_tie_count(self.h, C.byref(out)), "tsl_tie_count")
        return int(out.value)

    def tie_force(self, pos):
        """(n, 3) -k_tie w_i r_i: the force every tie applies to its vertex at the state pos (frozen dofs not masked)"""
        self.refresh_stream()
        out = np.zeros((self.tie_count(), 3))
        check(self.L.tsl_tie_force(self.h, _ptr(pos), out.ctypes.data), "tsl_tie_force")
        return out

    def tie_residuals(self, pos):
        """(n, 3) r_i = x_v - sum_a b_a x_{t_a} at the state pos"""
        self.refresh_stream()
        out = np.zeros((self.tie_count(), 3))
        check(self.L.tsl_tie_residuals(self.h, _ptr(pos), out.ctypes.data), "tsl_tie_residuals")
        return out

    def tie_grad(self, pos, p=None):
        """(n,) contribution of one reverse step to d(loss)/d(w_i) at the tape state pos; p None: the solution of the last adjoint_step, else a
        3 * tot_NV device vector"""
        self.refresh_stream()
        out = np.zeros(self.tie_count())
        check(self.L.tsl_tie_grad(self.h, _ptr(pos), _ptr(p), out.ctypes.data), "tsl_tie_grad")
        return out

    # ---- what the four collider kinds share: kind is "collider", "sphere", "capsule" or "box"
    def _shape_count(self, kind):
        out = C.c_int32(0)
        check(getattr(self.L, f"tsl_{kind}_count")(self.h, C.byref(out)), f"tsl_{kind}_count")
        return int(out.value)

    def _shape_force(self, kind, per, pos, prev_pos):
        self.refresh_stream()
        out = np.zeros((self._shape_count(kind), per))
        check(getattr(self.L, f"tsl_{kind}_force")(self.h, _ptr(pos), _ptr(prev_pos), out.ctypes.data), f"tsl_{kind}_force")
        return out

    def _shape_grad(self, kind, per, pos, prev_pos, p):
        self.refresh_stream()
        out = np.zeros((self._shape_count(kind), per))
        check(getattr(self.L, f"tsl_{kind}_grad")(self.h, _ptr(pos), _ptr(prev_pos), _ptr(p), out.ctypes.data), f"tsl_{kind}_grad")
        return out

    # ---- half-space colliders (tsl_set_colliders; stiffness: set_param("k_collider", k))
    def set_colliders(self, normals, offsets, mu, vertex_mask=None):
        """n half-spaces n_j . x < o_j with friction mu_j; vertex_mask (tot_NV,) uint8, bit j: collider j acts on the vertex, None: all on all; an empty
        list removes them.  The normals are normalised by the library and stay fixed."""
        nr = _np(normals, np.float64).reshape(-1, 3)
        o = _np(offsets, np.float64).reshape(-1)
        m = _np(mu, np.float64).reshape(-1)
        n = len(o)
        assert nr.shape == (n, 3) and m.shape == (n,), (nr.shape, o.shape, m.shape)
        vm = None if vertex_mask is None else _np(vertex_mask, np.uint8).reshape(-1)
        assert vm is None or vm.shape == (self.tot_NV,), vm.shape
        check(self.L.tsl_set_colliders(self.h, nr.ctypes.data if n else None, o.ctypes.data if n else None, m.ctypes.data if n else None, n,
                                       None if vm is None else vm.ctypes.data), "tsl_set_colliders")

    def set_collider_offsets(self, offsets):
        o = _np(offsets, np.float64).reshape(-1)
        assert o.shape == (self.collider_count(),), o.shape
        if len(o):
            check(self.L.tsl_set_collider_offsets(self.h, o.ctypes.data), "tsl_set_collider_offsets")

    def collider_count(self):
        return self._shape_count("collider")

    def collider_force(self, pos, prev_pos):
        """(n, 3) -sum_v g_v: the net force every plane applies to the cloth at the state (pos, prev_pos) (frozen dofs not masked)"""
        return self._shape_force("collider", 3, pos, prev_pos)

    def collider_grad(self, pos, prev_pos, p=None):
        """(n, 2) contribution of one reverse step to d(loss)/d(offset) and d(loss)/d(mu) of every collider at the tape state (x_s, x_{s-1}) with the
        offsets of step s in place; p None: the solution of the last adjoint_step, else a 3 * tot_NV device vector"""
        return self._shape_grad("collider", 2, pos, prev_pos, p)

    # ---- sphere colliders (tsl_set_spheres; stiffness: set_param("k_sphere", k))
    def set_spheres(self, centres, radii, mu, vertex_mask=None):
        """n solid balls (centre c_j, radius R_j, friction mu_j) with the cloth outside; vertex_mask (tot_NV,) uint8, bit j: sphere j acts on the vertex,
        None: all on all; an empty list removes them.  The previous centres are set to the centres; the radii stay fixed."""
        r = _np(radii, np.float64).reshape(-1)
        n = len(r)
        ce = _np(centres, np.float64).reshape(-1, 3)
        m = _np(mu, np.float64).reshape(-1)
        assert ce.shape == (n, 3) and m.shape == (n,), (ce.shape, r.shape, m.shape)
        vm = None if vertex_mask is None else _np(vertex_mask, np.uint8).reshape(-1)
        assert vm is None or vm.shape == (self.tot_NV,), vm.shape
        check(self.L.tsl_set_spheres(self.h, ce.ctypes.data if n else None, r.ctypes.data if n else None, m.ctypes.data if n else None, n,
                                     None if vm is None else vm.ctypes.data), "tsl_set_spheres")

    def set_sphere_centres(self, centres, prev_centres=None):
        """the centres of the next energy / assembly / step / reverse step and where the balls were at the start of that step (None: the centres)"""
        n = self.sphere_count()
        ce = _np(centres, np.float64).reshape(-1, 3)
        cp = None if prev_centres is None else _np(prev_centres, np.float64).reshape(-1, 3)
        assert ce.shape == (n, 3) and (cp is None or cp.shape == (n, 3)), (ce.shape, n)
        if n:
            check(self.L.tsl_set_sphere_centres(self.h, ce.ctypes.data, None if cp is None else cp.ctypes.data), "tsl_set_sphere_centres")

    def sphere_count(self):
        return self._shape_count("sphere")

    def sphere_force(self, pos, prev_pos):
        """(n, 3) -sum_v g_v: the net force every ball applies to the cloth at the state (pos, prev_pos) (frozen dofs not masked)"""
        return self._shape_force("sphere", 3, pos, prev_pos)

    def sphere_grad(self, pos, prev_pos, p=None):
        """(n, 8) contribution of one reverse step to d(loss)/d(centre (3), previous centre (3), mu, R) of every sphere at the tape state (x_s, x_{s-1}) with
        the centres of step s in place; p None: the solution of the last adjoint_step, else a 3 * tot_NV device vector"""
        return self._shape_grad("sphere", 8, pos, prev_pos, p)

    # ---- capsule colliders (tsl_set_capsules; stiffness: set_param("k_capsule", k))
    def set_capsules(self, ends_a, ends_b, radii, mu, vertex_mask=None):
        """n solid rods with round ends (endpoints a_j, b_j, radius R_j, friction mu_j) with the cloth outside; vertex_mask (tot_NV,) uint8, bit j: capsule
        j acts on the vertex, None: all on all; an empty list removes them.  The previous endpoints are set to the endpoints; the radii stay fixed."""
        r = _np(radii, np.float64).reshape(-1)
        n = len(r)
        a = _np(ends_a, np.float64).reshape(-1, 3)
        b = _np(ends_b, np.float64).reshape(-1, 3)
        m = _np(mu, np.float64).reshape(-1)
        assert a.shape == (n, 3) and b.shape == (n, 3) and m.shape == (n,), (a.shape, b.shape, r.shape, m.shape)
        vm = None if vertex_mask is None else _np(vertex_mask, np.uint8).reshape(-1)
        assert vm is None or vm.shape == (self.tot_NV,), vm.shape
        check(self.L.tsl_set_capsules(self.h, a.ctypes.data if n else None, b.ctypes.data if n else None, r.ctypes.data if n else None,
                                      m.ctypes.data if n else None, n, None if vm is None else vm.ctypes.data), "tsl_set_capsules")

    def set_capsule_ends(self, ends_a, ends_b, prev_a=None, prev_b=None):
        """the endpoints of the next energy / assembly / step / reverse step and where the rods were at the start of that step (both None: the endpoints)"""
        n = self.capsule_count()
        a = _np(ends_a, np.float64).reshape(-1, 3)
        b = _np(ends_b, np.float64).reshape(-1, 3)
        pa = None if prev_a is None else _np(prev_a, np.float64).reshape(-1, 3)
        pb = None if prev_b is None else _np(prev_b, np.float64).reshape(-1, 3)
        assert a.shape == (n, 3) and b.shape == (n, 3) and (pa is None or pa.shape == (n, 3)) and (pb is None or pb.shape == (n, 3)), (a.shape, b.shape, n)
        if n:
            check(self.L.tsl_set_capsule_ends(self.h, a.ctypes.data, b.ctypes.data, None if pa is None else pa.ctypes.data, None if pb is None else pb.ctypes.data),
                  "tsl_set_capsule_ends")

    def capsule_count(self):
        return self._shape_count("capsule")

    def capsule_force(self, pos, prev_pos):
        """(n, 6): [0:3] -sum_v g_v, the net force every rod applies to the cloth at the state (pos, prev_pos), [3:6] -sum_v (x_v - m) x g_v, its torque
        about the rod's midpoint (frozen dofs not masked)"""
        return self._shape_force("capsule", 6, pos, prev_pos)

    def capsule_grad(self, pos, prev_pos, p=None):
        """(n, 14) contribution of one reverse step to d(loss)/d(a (3), b (3), previous a (3), previous b (3), mu, R) of every capsule at the tape state
        (x_s, x_{s-1}) with the endpoints of step s in place; p None: the solution of the last adjoint_step, else a 3 * tot_NV device vector"""
        return self._shape_grad("capsule", 14, pos, prev_pos, p)

    # ---- rounded-box colliders (tsl_set_boxes; stiffness: set_param("k_box", k))
    def set_boxes(self, centres, quats, half_extents, radii, mu, vertex_mask=None):
        """n solid boxes with rounded edges and corners (centre c_j, quaternion (s, x, y, z), half extents h_j >= 0 of the core box, rounding radius r_j > 0,
        friction mu_j) with the cloth outside; vertex_mask (tot_NV,) uint8, bit j: box j acts on the vertex, None: all on all; an empty list removes
        them.  The quaternions are normalised by the library; the previous poses are set to the poses; half extents and radii stay fixed."""
        r = _np(radii, np.float64).reshape(-1)
        n = len(r)
        ce = _np(centres, np.float64).reshape(-1, 3)
        qu = _np(quats, np.float64).reshape(-1, 4)
        he = _np(half_extents, np.float64).reshape(-1, 3)
        m = _np(mu, np.float64).reshape(-1)
        assert ce.shape == (n, 3) and qu.shape == (n, 4) and he.shape == (n, 3) and m.shape == (n,), (ce.shape, qu.shape, he.shape, r.shape, m.shape)
        vm = None if vertex_mask is None else _np(vertex_mask, np.uint8).reshape(-1)
        assert vm is None or vm.shape == (self.tot_NV,), vm.shape
        check(self.L.tsl_set_boxes(self.h, ce.ctypes.data if n else None, qu.ctypes.data if n else None, he.ctypes.data if n else None,
                                   r.ctypes.data if n else None, m.ctypes.data if n else None, n, None if vm is None else vm.ctypes.data), "tsl_set_boxes")

    def set_box_poses(self, centres, quats, prev_centres=None, prev_quats=None):
        """the poses of the next energy / assembly / step / reverse step and where the boxes were at the start of that step (both None: the poses)"""
        n = self.box_count()
        ce = _np(centres, np.float64).reshape(-1, 3)
        qu = _np(quats, np.float64).reshape(-1, 4)
        pc = None if prev_centres is None else _np(prev_centres, np.float64).reshape(-1, 3)
        pq = None if prev_quats is None else _np(prev_quats, np.float64).reshape(-1, 4)
        assert ce.shape == (n, 3) and qu.shape == (n, 4) and (pc is None or pc.shape == (n, 3)) and (pq is None or pq.shape == (n, 4)), (ce.shape, qu.shape, n)
        if n:
            check(self.L.tsl_set_box_poses(self.h, ce.ctypes.data, qu.ctypes.data, None if pc is None else pc.ctypes.data, None if pq is None else pq.ctypes.data),
                  "tsl_set_box_poses")

    def box_count(self):
        return self._shape_count("box")

    def box_force(self, pos, prev_pos):
        """(n, 6): [0:3] -sum_v g_v, the net force every box applies to the cloth at the state (pos, prev_pos), [3:6] -sum_v (x_v - c) x g_v, its torque
        about the box's centre (frozen dofs not masked)"""
        return self._shape_force("box", 6, pos, prev_pos)

    def box_grad(self, pos, prev_pos, p=None):
        """(n, 14) contribution of one reverse step to d(loss)/d(c (3), theta (3), previous c (3), previous theta (3), mu, r) of every box at the tape state
        (x_s, x_{s-1}) with the poses of step s in place (theta: world-frame rotation vectors applied on the left); p None: the solution of the last
        adjoint_step, else a 3 * tot_NV device vector"""
        return self._shape_grad("box", 14, pos, prev_pos, p)

    # ---- sampled distance-field colliders (tsl_set_sdfs; stiffness: set_param("k_sdf", k))
    def set_sdfs(self, grids, origins, spacings, centres, quats, offsets, mu, vertex_mask=None):
        """n solids {phi < offset} with the cloth outside, phi the cubic B-spline over grids[j] (a 3-d array of samples, every dimension in [4, 512], C
        order) with spacing spacings[j] and origins[j] the local position of sample (0, 0, 0); centre c_j, quaternion (s, x, y, z), friction mu_j;
        vertex_mask (tot_NV,) uint8, bit j: field j acts on the vertex, None: all on all; an empty list removes them and frees the samples.  The
        quaternions are normalised by the library; the previous poses are set to the poses; samples, spacings, origins and offsets stay fixed."""
        g = [np.ascontiguousarray(_np(a, np.float64)) for a in grids]
        n = len(g)
        assert all(a.ndim == 3 for a in g), [a.shape for a in g]
        dims = np.array([a.shape for a in g], np.int32).reshape(-1, 3)
        smp = np.concatenate([a.reshape(-1) for a in g]) if n else np.zeros(0)
        o = _np(origins, np.float64).reshape(-1, 3)
        h = _np(spacings, np.float64).reshape(-1)
        ce = _np(centres, np.float64).reshape(-1, 3)
        qu = _np(quats, np.float64).reshape(-1, 4)
        r = _np(offsets, np.float64).reshape(-1)
        m = _np(mu, np.float64).reshape(-1)
        assert o.shape == (n, 3) and h.shape == (n,) and ce.shape == (n, 3) and qu.shape == (n, 4) and r.shape == (n,) and m.shape == (n,), (n, o.shape, h.shape, ce.shape, qu.shape, r.shape, m.shape)
        vm = None if vertex_mask is None else _np(vertex_mask, np.uint8).reshape(-1)
        assert vm is None or vm.shape == (self.tot_NV,), vm.shape
        ptr = lambda a: a.ctypes.data if n else None
        check(self.L.tsl_set_sdfs(self.h, ptr(smp), ptr(dims), ptr(o), ptr(h), ptr(ce), ptr(qu), ptr(r), ptr(m), n, None if vm is None else vm.ctypes.data), "tsl_set_sdfs")

    def set_sdf_poses(self, centres, quats, prev_centres=None, prev_quats=None):
        """the poses of the next energy / assembly / step / reverse step and where the fields were at the start of that step (both None: the poses)"""
        n = self.sdf_count()
        ce = _np(centres, np.float64).reshape(-1, 3)
        qu = _np(quats, np.float64).reshape(-1, 4)
        pc = None if prev_centres is None else _np(prev_centres, np.float64).reshape(-1, 3)
        pq = None if prev_quats is None else _np(prev_quats, np.float64).reshape(-1, 4)
        assert ce.shape == (n, 3) and qu.shape == (n, 4) and (pc is None or pc.shape == (n, 3)) and (pq is None or pq.shape == (n, 4)), (ce.shape, qu.shape, n)
        if n:
            check(self.L.tsl_set_sdf_poses(self.h, ce.ctypes.data, qu.ctypes.data, None if pc is None else pc.ctypes.data, None if pq is None else pq.ctypes.data),
                  "tsl_set_sdf_poses")

    def sdf_count(self):
        return self._shape_count("sdf")

    def sdf_force(self, pos, prev_pos):
        """(n, 6): [0:3] -sum_v g_v, the net force every field's solid applies to the cloth at the state (pos, prev_pos), [3:6] -sum_v (x_v - c) x g_v, its
        torque about the field's centre (frozen dofs not masked)"""
        return self._shape_force("sdf", 6, pos, prev_pos)

    def sdf_grad(self, pos, prev_pos, p=None):
        """(n, 14) contribution of one reverse step to d(loss)/d(c (3), theta (3), previous c (3), previous theta (3), mu, offset) of every field at the tape
        state (x_s, x_{s-1}) with the poses of step s in place (theta: world-frame rotation vectors applied on the left); p None: the solution of the
        last adjoint_step, else a 3 * tot_NV device vector"""
        return self._shape_grad("sdf", 14, pos, prev_pos, p)

    # ---- wind (tsl_set_wind; coefficients: set_param("wind_cn", c_n), set_param("wind_ct", c_t))
    def set_wind(self, faces=None, weights=None):
        """lagged aerodynamic drag on the cloth faces `faces` (global face ids, each once) with the weights `weights` (None: 1 each); faces None: every
        cloth face in ascending order; an empty list removes the wind"""
        w = None if weights is None else _np(weights, np.float64).reshape(-1)
        if faces is None:
            assert w is None or w.shape == (self.n_cface,), w.shape
            check(self.L.tsl_set_wind(self.h, None, None if w is None else w.ctypes.data, -1), "tsl_set_wind")
            return
        f = _np(faces, np.int32).reshape(-1)
        n = len(f)
        assert w is None or w.shape == (n,), (w.shape, n)
        check(self.L.tsl_set_wind(self.h, f.ctypes.data if n else None, None if (w is None or not n) else w.ctypes.data, n), "tsl_set_wind")

    def set_wind_velocity(self, W):
        """the wind velocity (3,) of the next energy / assembly / step / reverse step"""
        W = _np(W, np.float64).reshape(-1)
        assert W.shape == (3,), W.shape
        check(self.L.tsl_set_wind_velocity(self.h, W.ctypes.data), "tsl_set_wind_velocity")

    def wind_count(self):
        out = C.c_int32(0)
        check(self.L.tsl_wind_count(self.h, C.byref(out)), "tsl_wind_count")
        return int(out.value)

    def wind_force(self, pos, prev_pos):
        """(3,) -sum_f M_f r_f: the net force the wind applies to the cloth at the state (pos, prev_pos) (frozen dofs not masked)"""
        self.refresh_stream()
        out = np.zeros(3)
        check(self.L.tsl_wind_force(self.h, _ptr(pos), _ptr(prev_pos), out.ctypes.data), "tsl_wind_force")
        return out

    def wind_grad(self, pos, prev_pos, p=None):
        """(5,) contribution of one reverse step to d(loss)/d(W (3), c_n, c_t) at the tape state (x_s, x_{s-1}) with the wind velocity of step s in
        place; p None: the solution of the last adjoint_step, else a 3 * tot_NV device vector"""
        self.refresh_stream()
        out = np.zeros(5)
        check(self.L.tsl_wind_grad(self.h, _ptr(pos), _ptr(prev_pos), _ptr(p), out.ctypes.data), "tsl_wind_grad")
        return out

    # ---- engine calls
    def energy(self, pos, prev_pos, vel, ref_angle):
        self.refresh_stream()
        e = C.c_double(0)
        check(self.L.tsl_energy(self.h, _ptr(pos), _ptr(prev_pos), _ptr(vel), _ptr(ref_angle), C.byref(e)), "tsl_energy")
        return e.value

    def assemble(self, pos, prev_pos, vel, ref_angle, spd=True, grad=None):
        self.refresh_stream()
        check(self.L.tsl_assemble(self.h, _ptr(pos), _ptr(prev_pos), _ptr(vel), _ptr(ref_angle), int(spd), _ptr(grad)), "tsl_assemble")

    def solve(self, rhs, x=None):
        self.refresh_stream()
        if x is None:
            x = torch.empty_like(rhs)
        st = SolveStats()
        check(self.L.tsl_solve(self.h, _ptr(rhs), _ptr(x), C.byref(st)), "tsl_solve")
        return x, st.as_dict()

    def step(self, pos, prev_pos, vel, ref_angle):
        self.refresh_stream()
        st = StepStats()
        check(self.L.tsl_step(self.h, _ptr(pos), _ptr(prev_pos), _ptr(vel), _ptr(ref_angle), C.byref(st)), "tsl_step")
        return st.as_dict()

    def contact_detect(self, pos, prev_pos):
        self.refresh_stream()
        nc = C.c_int32(0)
        check(self.L.tsl_contact_detect(self.h, _ptr(pos), _ptr(prev_pos), C.byref(nc)), "tsl_contact_detect")
        return nc.value

    def contact_counts(self):
        """(vertex-triangle, edge-edge) constraints of the last detection; the edge-edge ones ("contact_ee" = 1) follow the others in the list"""
        out = (C.c_int32 * 2)()
        check(self.L.tsl_contact_counts(self.h, out), "tsl_contact_counts")
        return int(out[0]), int(out[1])

    def contact_reset(self):
        check(self.L.tsl_contact_reset(self.h), "tsl_contact_reset")

    def update_ref_angle(self, pos, ref_angle):
        check(self.L.tsl_update_ref_angle(self.h, _ptr(pos), _ptr(ref_angle)), "tsl_update_ref_angle")

    def adjoint_step(self, step, T, pos_buffer, pos_grad, ref_angle_buffer, angleref_grad, tmp_z_frozen, damping=1.0):
        self.refresh_stream()
        st = SolveStats()
        check(self.L.tsl_adjoint_step(self.h, int(step), int(T), _ptr(pos_buffer), _ptr(pos_grad), _ptr(ref_angle_buffer), _ptr(angleref_grad),
                                      _ptr(tmp_z_frozen), float(damping), C.byref(st)), "tsl_adjoint_step")
        return st.as_dict()

    def elastic_force(self, pos, out):
        check(self.L.tsl_elastic_force(self.h, _ptr(pos), _ptr(out)), "tsl_elastic_force")
        return out

    def friction_grad(self, pos):
        out = C.c_double(0)
        check(self.L.tsl_friction_grad(self.h, _ptr(pos), C.byref(out)), "tsl_friction_grad")
        return out.value

    def param_grad(self, pos, ref_angle):
        """{kb, mu, lam} contributions of the last adjoint_step (system identification)"""
        out = (C.c_double * 3)()
        check(self.L.tsl_param_grad(self.h, _ptr(pos), _ptr(ref_angle), out), "tsl_param_grad")
        return dict(kb=out[0], mu=out[1], lam=out[2])

    def param_grads(self, pos, ref_angle, keys, p=None):
        """{key: sum over the free dofs of p . d(force)/d(key)} at the tape state pos (tsl_param_grad_keys): keys as tsl_set_param spells them
        ("cloth<i>.Kl|Ka|Kb|stvk_mu|stvk_lam", "elastic<i>.mu|lam", "k_contact", "mu_cloth_elastic", "mu_cloth_cloth", "k_handle", "k_tie"); p None: the solution of the last
        adjoint_step, else a 3 * tot_NV device vector"""
        keys = list(keys)
        if not keys:
            return {}
        self.refresh_stream()
        arr = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
        out = (C.c_double * len(keys))()
        check(self.L.tsl_param_grad_keys(self.h, _ptr(pos), _ptr(ref_angle), _ptr(p), arr, len(keys), out), "tsl_param_grad_keys")
        return {k: out[j] for j, k in enumerate(keys)}

    # ---- introspection (tests)
    def matrix(self):
        """(row_ptr, col, vals[nnzb,3,3]) of the masked system matrix of the last assemble (static part)."""
        nb = C.c_int32(0); nnzb = C.c_int32(0)
        check(self.L.tsl_matrix_nnzb(self.h, C.byref(nb), C.byref(nnzb)), "tsl_matrix_nnzb")
        rp = np.zeros(nb.value + 1, np.int32); col = np.zeros(nnzb.value, np.int32); vals = np.zeros((nnzb.value, 3, 3), np.float64)
        check(self.L.tsl_matrix_export(self.h, rp.ctypes.data, col.ctypes.data, vals.ctypes.data), "tsl_matrix_export")
        return rp, col, vals

    def matrix_import(self, vals):
        """write vals[nnzb,3,3] -- the pattern and order of matrix() -- into the static part of the operator (until the next assemble or step)"""
        rp, col, _ = self.matrix()
        v = np.ascontiguousarray(vals, dtype=np.float64)
        assert v.shape == (len(col), 3, 3), (v.shape, len(col))
        check(self.L.tsl_matrix_import(self.h, v.ctypes.data), "tsl_matrix_import")

    def matrix_csr(self):
        import scipy.sparse as sp
        rp, col, vals = self.matrix()
        n = 3 * (len(rp) - 1)
        return sp.bsr_matrix((vals, col, rp), shape=(n, n)).tocsr()

    # ---- the iterative hierarchy taken apart (tests): tsl_mg_info / tsl_mg_export / tsl_mg_apply / tsl_solve_with
    MG_ARRAYS = dict(A=(0, np.float64), Dinv=(1, np.float64), omega=(2, np.float64), A32=(3, np.float32), S32=(4, np.float32), Cinv=(5, np.float32),
                     bad=(6, np.int32), Binv=(7, np.float32), bad_body=(8, np.int32), rowpos=(9, np.int32))
    MG_KINDS = ("inner", "dense", "one_workgroup", "per_sweep")

    def mg_info(self):
        """{"hierarchies": [{v_offset, N0, M0, levels: [{N, M, kind}]}], "bodies": [n3, ...]} of the preconditioner as the next solve runs it"""
        self.refresh_stream()
        out = np.zeros(256, np.int32)
        n = check(self.L.tsl_mg_info(self.h, out.ctypes.data, len(out)), "tsl_mg_info")
        v = [int(t) for t in out[:n]]
        H, B, k = v[0], v[1], 2
        hs = []
        for _ in range(H):
            h = dict(v_offset=v[k], N0=v[k + 1], M0=v[k + 2], levels=[])
            nl = v[k + 3]; k += 4
            for _ in range(nl):
                h["levels"].append(dict(N=v[k], M=v[k + 1], kind=self.MG_KINDS[v[k + 2]])); k += 3
            hs.append(h)
        return dict(hierarchies=hs, bodies=v[k:k + B])

    def mg_export(self, what, hierarchy=0, level=0, size=None):
        """array `what` (a key of MG_ARRAYS) of one level (-1: level 0) of one hierarchy, or of dense body `hierarchy`, flat, as the cycle reads it"""
        self.refresh_stream()
        code, dt = self.MG_ARRAYS[what]
        cap = int(size) if size is not None else 9 * self.tot_NV * 225
        out = np.zeros(cap, dt)
        n = check(self.L.tsl_mg_export(self.h, int(hierarchy), int(level), code, out.ctypes.data, cap), f"tsl_mg_export({what})")
        return out[:n].copy()

    def mg_apply(self, r, z=None):
        """z = M^-1 r with the preconditioner a PCG iteration would apply (device vectors, 3 * tot_NV, the caller's vertex order)"""
        self.refresh_stream()
        if z is None:
            z = torch.empty_like(r)
        check(self.L.tsl_mg_apply(self.h, _ptr(r), _ptr(z)), "tsl_mg_apply")
        return z

    def solve_with(self, method, rhs, cap=0, x=None):
        """one solver of the hierarchy alone: 0 PCG (active preconditioner), 1 MINRES, 2 GMRES, 3 BiCGStab; cap 0: "cg_maxit" """
        self.refresh_stream()
        if x is None:
            x = torch.empty_like(rhs)
        st = SolveStats()
        check(self.L.tsl_solve_with(self.h, int(method), int(cap), _ptr(rhs), _ptr(x), C.byref(st)), "tsl_solve_with")
        return x, st.as_dict()

    # ---- the operator of the Krylov solvers taken apart (tests): tsl_op_export / tsl_op_apply / tsl_pcg_trace
    OP_ARRAYS = dict(slice_off=(0, np.int32), slice_len=(1, np.int32), colidx=(2, np.int32), perm=(3, np.int32), rowpos=(4, np.int32), diag_perm=(5, np.int32),
                     vals=(6, np.float64), vals_full=(7, np.float64), fzmask=(8, np.uint8), mdt2=(9, np.float64), Dinv=(10, np.float64), c_diag=(11, np.float64),
                     cr_ptr=(12, np.int32), cr_ent=(13, np.int32), cr_rows=(14, np.int32))

    def op_export(self, what):
        """array `what` (a key of OP_ARRAYS) as the next solve reads it, flat, in the solver's row order; empty where a scene without constraints has none"""
        self.refresh_stream()
        code, dt = self.OP_ARRAYS[what]
        if what in ("vals", "vals_full", "colidx"):
            so = self.op_export("slice_off")
            cap = int(so[-1]) * (1 if what == "colidx" else 9)
        elif what in ("cr_ent", "cr_rows"):
            cap = 16 * (self.max_n_constraints + self.tie_count())
        else:
            cap = 9 * self.tot_NV + 64
        out = np.zeros(max(cap, 1), dt)
        n = check(self.L.tsl_op_export(self.h, code, out.ctypes.data, cap), f"tsl_op_export({what})")
        return out[:n].copy()

    def op_apply(self, kernel, x, y=None):
        """(y, dot, partials) of y = H x by product kernel `kernel` (0..9, tsl_hip.h); x, y device vectors in the caller's vertex order"""
        self.refresh_stream()
        if y is None:
            y = torch.empty_like(x)
        part = np.zeros(self.tot_NV + 64)
        dot = C.c_double(0)
        n = check(self.L.tsl_op_apply(self.h, int(kernel), _ptr(x), _ptr(y), C.byref(dot), part.ctypes.data, len(part)), "tsl_op_apply")
        return y, dot.value, part[:n].copy()

    def pcg_trace(self, rhs, n_iter, use_graph=False):
        """the state of a PCG run on rhs after n_iter iterations that nothing stops: dict of x, r, z, p, p_prev, Ap (solver order), part_pAp, part_rz,
        part_rr, the scalar record and the chunk of the captured graph"""
        self.refresh_stream()
        n3 = 3 * self.tot_NV
        cap = self.tot_NV + 2048
        vec = np.zeros((6, n3)); part = np.zeros((3, cap)); npart = np.zeros(3, np.int32); sc = np.zeros(11)
        chunk = check(self.L.tsl_pcg_trace(self.h, _ptr(rhs), int(n_iter), int(bool(use_graph)), vec.ctypes.data, part.ctypes.data, cap, npart.ctypes.data, sc.ctypes.data),
                      "tsl_pcg_trace")
        out = dict(zip(("x", "r", "z", "p", "p_prev", "Ap"), vec))
        out.update(part_pAp=part[0, :npart[0]].copy(), part_rz=part[1, :npart[1]].copy(), part_rr=part[2, :npart[2]].copy(), chunk=chunk)
        out.update(zip(("rzh0", "rzh1", "thresh2", "bb", "rr_last", "rz_last", "pAp_last"), sc[:7]))
        out.update(flag=int(sc[7]), iters=int(sc[8]), n_part1=int(sc[9]), n_part2=int(sc[10]))
        return out

    def constraints(self):
        m = self.max_n_constraints + self.tie_count()   # (the tie slots lie behind the detected ones)
        idx = np.zeros((m, 4), np.int32); w = np.zeros((m, 3)); k = np.zeros(m); dx0 = np.zeros((m, 3)); T = np.zeros((m, 6)); n = np.zeros((m, 3)); mu = np.zeros(m)
        cnt = check(self.L.tsl_constraints_export(self.h, idx.ctypes.data, w.ctypes.data, k.ctypes.data, dx0.ctypes.data, T.ctypes.data, n.ctypes.data,
                                                  mu.ctypes.data, m), "tsl_constraints_export")
        return dict(idx=idx[:cnt], w=w[:cnt], k=k[:cnt], dx0=dx0[:cnt], T=T[:cnt], n=n[:cnt], mu=mu[:cnt])

    def contact_blocks(self, masked=True):
        m = self.max_n_constraints + self.tie_count()
        blk = np.zeros((m, 12, 12))
        cnt = check(self.L.tsl_contact_blocks_export(self.h, blk.ctypes.data, m, int(masked)), "tsl_contact_blocks_export")
        return blk[:cnt]

    def operator_csr(self):
        """full solve operator: static masked matrix + matrix-free contact blocks, as scipy CSR"""
        import scipy.sparse as sp
        A = self.matrix_csr().tolil()
        cons = self.constraints()
        blk = self.contact_blocks(True)
        for c in range(len(blk)):
            idx = cons["idx"][c]
            dofs = np.concatenate([3 * idx[k] + np.arange(3) for k in range(4)])
            for r in range(12):
                for cc in range(12):
                    if blk[c, r, cc] != 0.0:
                        A[dofs[r], dofs[cc]] += blk[c, r, cc]
        return A.tocsr()

    def proj_export(self):
        nb = max(self.n_body, 1)
        flag = np.zeros((nb, self.tot_NV), np.int32); dr = np.zeros((nb, self.tot_NV), np.int32)
        pidx = np.zeros((nb, self.tot_NV, 3), np.int32); pw = np.zeros((nb, self.tot_NV, 3))
        check(self.L.tsl_proj_export(self.h, flag.ctypes.data, dr.ctypes.data, pidx.ctypes.data, pw.ctypes.data), "tsl_proj_export")
        return flag, dr, pidx, pw

    def proj_import(self, flag, dr):
        flag = _np(flag, np.int32); dr = _np(dr, np.int32)
        check(self.L.tsl_proj_import(self.h, flag.ctypes.data, dr.ctypes.data), "tsl_proj_import")

    def set_border(self, border):
        b = _np(border, np.int32)
        assert b.shape == (self.tot_NV,)
        check(self.L.tsl_set_border(self.h, b.ctypes.data), "tsl_set_border")

    def refresh_stream(self):
        """engine calls are ordered against torch's CURRENT stream of the context's device (it may change between calls)"""
        self.L.tsl_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def spd_project(self, blocks, D):
        check(self.L.tsl_spd_project(self.h, _ptr(blocks), blocks.numel() // (D * D), D), "tsl_spd_project")

    def profile_reset(self, enable=True):
        check(self.L.tsl_profile_reset(self.h, int(bool(enable))), "tsl_profile_reset")

    def profile_read(self):
        ms = C.c_double(0); n = C.c_int64(0); b = C.c_int64(0)
        check(self.L.tsl_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(b)), "tsl_profile_read")
        ev = C.c_double(0)
        check(self.L.tsl_profile_read_events(self.h, C.byref(ev)), "tsl_profile_read_events")
        return dict(ms_per_launch=ms.value, launches=n.value, bytes_per_launch=b.value, ms_per_launch_events=ev.value)

    def bench_direct(self, cls, reps=20):
        """kernel class of the sparse direct path replayed back to back (0 Gauss-Jordan inversions on the block-step path, 1 Schur GEMM + extend-add, 2 G = W F12 GEMM, 3 inversions in the LDS kernel, 4 gemv sweeps of one application, 5 inversions in the persistent dataflow kernel)"""
        out = (C.c_double * 4)()
        check(self.L.tsl_bench_direct(self.h, int(cls), int(reps), out), "tsl_bench_direct")
        return dict(us_per_launch=out[0], flops_per_launch=out[1], bytes_per_launch=out[2], launches=int(out[3]))

    def direct_info(self):
        out = (C.c_double * 10)()
        check(self.L.tsl_direct_info(self.h, out), "tsl_direct_info")
        keys = ("plans", "factorizations", "applications", "perturbed_pivots", "plan_seconds", "supernodes", "levels", "batches", "flops_per_factorization", "front_bytes")
        return dict(zip(keys, [float(v) for v in out]))

    def direct_counters(self):
        out = (C.c_double * 13)()
        check(self.L.tsl_direct_counters(self.h, out, 13), "tsl_direct_counters")
        keys = ("flow_launches", "flow_aborts", "plan_cache_hits", "panel_bytes", "schur_bytes", "g_bytes", "schur_entries", "plans_parked",
                "berr_seen", "berr_accepted", "berr_max", "berr_rel_max", "tiles_guarded")
        return dict(zip(keys, [float(v) for v in out]))

    def bench_spmv(self, variant=20, reps=500):
        """microseconds per launch of `reps` back-to-back operator launches between one hipEvent pair (20 = k_pcg_spmv)"""
        us = C.c_double(0)
        check(self.L.tsl_bench_spmv(self.h, int(variant), int(reps), C.byref(us)), "tsl_bench_spmv")
        return us.value
