"""Synthetic floor scene (no reference counterpart, whose tables are frozen 16 x 16 x 2 tetrahedral bodies): one N x N cloth over a half-space
collider (BaseScene.set_colliders) -- collider 0 is the floor n = (0, 0, 1) at height ``floor_z`` -- and no table body, no contact pair, no
constraint slot.  ``tilt`` adds collider 1, a plane through the origin tilted by that angle about the x axis, n = (0, sin tilt, cos tilt), whose
tangent pair is orthonormal; with ``on_ramp`` the cloth starts lying in that plane's shell (the floor then lies ``ramp_drop`` below and never
acts).  The cloth starts ``depth`` inside the shell of the plane it lies on; None: where the plane carries its weight, m g cos(tilt) / k per vertex."""
import numpy as np

from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.04, N=8, k_collider=2e3, mu=0.5, tilt=None, on_ramp=False, floor_z=0.0, depth=None, ramp_drop=1.0, Kb=100.0, k_angle=3.14, stvk=None,
                 device="cuda:0", newton_cap=50):
        self._N = N
        self._newton_cap = newton_cap
        self._floor = dict(k=float(k_collider), mu=float(mu), tilt=None if tilt is None else float(tilt), on_ramp=bool(on_ramp), z=float(floor_z), depth=None if depth is None else float(depth),
                           drop=float(ramp_drop))
        assert not on_ramp or tilt is not None, "on_ramp needs a tilt"
        super().__init__(cloth_size=cloth_size, enable_gripper=False, device=device)
        self.cloths[0].Kb[None] = Kb
        self.cloths[0].k_angle[None] = k_angle
        if stvk:   # (stvk_mu, stvk_lam) in N/m: the StVK membrane
            self.cloths[0].stvk_mu[None], self.cloths[0].stvk_lam[None] = stvk
            self.cloths[0].membrane[None] = 1.0

    def init_scene_parameters(self):
        self.dt = 5e-3
        self.h = self.dt
        self.cloth_cnt = 1
        self.elastic_cnt = 0
        self.cloth_N = self._N
        self.cloth_M = self._N
        self.k_contact = 10000
        self.eps_contact = 0.0004
        self.eps_v = 0.01
        self.max_n_constraints = 16
        self.damping = 1.0

    def init_objects(self):
        self.cloths.append(Cloth(self.cloth_N, self.dt, self.cloth_size, 0, 4e1, 0, False, self.cloth_M))
        self.tot_NV = self.cloths[0].NV

    def plane_list(self):
        """(normals, offsets, mu) of the scene's colliders"""
        f = self._floor
        normals, offsets = [[0.0, 0.0, 1.0]], [f["z"] - (f["drop"] if f["on_ramp"] else 0.0)]
        if f["tilt"] is not None:
            normals.append([0.0, np.sin(f["tilt"]), np.cos(f["tilt"])])
            offsets.append(0.0)
        return np.array(normals), np.array(offsets), np.full(len(offsets), f["mu"])

    def init(self):
        f = self._floor
        c = self.cloths[0]
        depth = f["depth"]
        if depth is None:
            depth = c.mass * 9.8 * (np.cos(f["tilt"]) if f["on_ramp"] else 1.0) / f["k"] if f["k"] > 0 else 0.0
        rest = self.eps_contact - depth   # distance to the plane the cloth lies on
        c.init(-0.5 * self.cloth_size, -0.5 * self.cloth_size, 0.0)
        p = c.pos.to_numpy()
        if f["on_ramp"]:   # the flat sheet turned about the x axis into the tilted plane, then lifted along its normal
            s, co = np.sin(f["tilt"]), np.cos(f["tilt"])
            y = p[:, 1].copy()
            p[:, 1] = co * y + s * rest
            p[:, 2] = -s * y + co * rest
        else:
            p[:, 2] = f["z"] + rest
        c.pos.from_numpy(p)

    def init_all(self):
        super().init_all()
        if self.n_collider == 0:   # (a caller's own list, set before, stays)
            normals, offsets, mu = self.plane_list()
            self.set_colliders(normals, offsets, mu, self._floor["k"])

    def contact_pairs(self):
        return []

    def set_frozen_kernel(self):
        pass

    def action(self, step, delta_pos=None, delta_rot=None, delta_dis=None):
        pass
