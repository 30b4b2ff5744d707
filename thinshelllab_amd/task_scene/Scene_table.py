"""Synthetic table scene (no reference counterpart, whose table tops are meshed bodies): one N x N cloth lies with one half on a rounded plate
(BaseScene.set_boxes) and hangs with the other half over the plate's edge -- the long edge of the plate's core runs along y a tenth of a grid
spacing short of the sheet's middle column, so that this column lies over the rounded edge where it still touches, the columns before it over
the face; the plate ends short of the sheet's two end rows -- and no body, no contact pair, no constraint slot.  The two corners of the sheet that lie on the plate are frozen (``pin="plate"``; ``pin="all"`` freezes all
four, for a sheet that is stretched over the plate's edge, not hanging over it).  The plate's top (shell included) lies
``push`` above the flat sheet's plane.  The plate is moved with ``set_box_poses`` or ``move_boxes`` before every step: it may translate and tilt;
its slip against the sheet drags the sheet by friction, differently across its face when it turns."""
import numpy as np

from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.04, N=8, k_box=2e3, mu=0.5, radius=0.002, thickness=0.001, push=0.0, Kb=100.0, k_angle=3.14, stvk=None, pin="plate",
                 device="cuda:0", newton_cap=50):
        assert pin in ("plate", "all"), pin
        self._pin = pin
        self._N = N
        self._newton_cap = newton_cap
        dx = cloth_size / N
        # the core box: from 0.3 dx beyond the sheet's side at x = -cloth_size / 2 to 0.1 dx short of its middle column, 0.3 dx and the radius short of
        # the sheet's ends in y
        half = np.array([0.25 * cloth_size + 0.1 * dx, 0.5 * cloth_size - 0.3 * dx - radius, thickness])
        self._plate = dict(k=float(k_box), mu=float(mu), r=float(radius), push=float(push), h=half, cx=-0.25 * cloth_size - 0.2 * dx)
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

    def plate(self):
        """(centre (1, 3), quaternion (1, 4), half extents (1, 3), radius (1,), mu (1,)) of the scene's plate: level, its rounded top `push` above the
        flat sheet's plane (z = 0)"""
        p = self._plate
        z = p["push"] - p["r"] - p["h"][2]
        return np.array([[p["cx"], 0.0, z]]), np.array([[1.0, 0.0, 0.0, 0.0]]), p["h"][None].copy(), np.array([p["r"]]), np.array([p["mu"]])

    def centre_vertex(self):
        """global id of the vertex in the middle of the grid (N even: the grid has one); it lies over the plate's edge"""
        c = self.cloths[0]
        return c.offset + (c.N // 2) * (c.M + 1) + c.M // 2

    def hanging_vertex(self):
        """global id of the vertex in the middle of the sheet's free side, the one farthest beyond the plate's edge"""
        x = self.pos.to_numpy()
        far = np.flatnonzero(np.abs(x[:, 0] - x[:, 0].max()) < 1e-12)
        return int(far[np.argmin(np.abs(x[far, 1]))])

    def init(self):
        c = self.cloths[0]
        c.init(-0.5 * self.cloth_size, -0.5 * self.cloth_size, 0.0)

    def init_all(self):
        super().init_all()
        if self.n_box == 0:   # (a caller's own list, set before, stays)
            c, q, h, r, mu = self.plate()
            self.set_boxes(c, q, h, r, mu, self._plate["k"])

    def contact_pairs(self):
        return []

    def set_frozen_kernel(self):
        fr = self.frozen.t.view(-1, 3)
        x = self.pos.to_numpy()
        for v in self.cloths[0].corner_ids():
            if self._pin == "all" or x[v, 0] < 0.0:
                fr[v] = 1

    def action(self, step, delta_pos=None, delta_rot=None, delta_dis=None):
        pass
