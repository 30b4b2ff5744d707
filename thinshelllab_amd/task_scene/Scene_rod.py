"""Synthetic rod scene (no reference counterpart, whose rods are meshed bodies): one N x N cloth with its four corners frozen over one capsule
collider (BaseScene.set_capsules) under its middle -- a horizontal rod along x of radius ``radius`` whose top lies ``push`` above the flat sheet's
plane -- and no body, no contact pair, no constraint slot.  The rod is shorter than the sheet's side: its ends lie 0.7 of a grid spacing beyond
the last vertex over the barrel, so that the next vertex of the middle row lies over the cap, 0.3 of a spacing from the end; the barrel and both
caps touch vertices.  The rod is moved with ``set_capsule_ends`` before every step (its endpoints are independent: it may translate and yaw); its
slip against the sheet drags the sheet by friction, differently along its length when it turns."""
import numpy as np

from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.04, N=8, k_capsule=2e3, mu=0.5, radius=0.005, push=0.0, half_length=None, Kb=100.0, k_angle=3.14, stvk=None, device="cuda:0",
                 newton_cap=50):
        self._N = N
        self._newton_cap = newton_cap
        if half_length is None:
            half_length = (N // 4 + 0.7) * cloth_size / N
        self._rod = dict(k=float(k_capsule), mu=float(mu), R=float(radius), push=float(push), L=float(half_length))
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

    def rod(self):
        """(a (1, 3), b (1, 3), radius (1,), mu (1,)) of the scene's rod: along x under the middle of the flat sheet (z = 0), its top `push` above the
        sheet's plane"""
        r = self._rod
        z = r["push"] - r["R"]
        return np.array([[-r["L"], 0.0, z]]), np.array([[r["L"], 0.0, z]]), np.array([r["R"]]), np.array([r["mu"]])

    def centre_vertex(self):
        """global id of the vertex in the middle of the grid (N even: the grid has one)"""
        c = self.cloths[0]
        return c.offset + (c.N // 2) * (c.M + 1) + c.M // 2

    def init(self):
        c = self.cloths[0]
        c.init(-0.5 * self.cloth_size, -0.5 * self.cloth_size, 0.0)

    def init_all(self):
        super().init_all()
        if self.n_capsule == 0:   # (a caller's own list, set before, stays)
            a, b, radius, mu = self.rod()
            self.set_capsules(a, b, radius, mu, self._rod["k"])

    def contact_pairs(self):
        return []

    def set_frozen_kernel(self):
        fr = self.frozen.t.view(-1, 3)
        for v in self.cloths[0].corner_ids():
            fr[v] = 1

    def action(self, step, delta_pos=None, delta_rot=None, delta_dis=None):
        pass
