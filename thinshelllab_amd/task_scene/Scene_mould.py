"""Synthetic mould scene (no reference counterpart, whose moulds are meshed bodies with every vertex frozen): one N x N cloth lies over a flat-lying
ring -- a torus about the z axis, sampled with engine/sdf.py and set with BaseScene.set_sdfs -- and no body, no contact pair, no constraint slot.
The ring's top lies ``push`` above the flat sheet's plane; its hole makes the solid concave, which no analytic collider kind can be.  ``pin="all"``
freezes the sheet's four corners (a sheet stretched over the mould), ``pin="side"`` the two at x < 0.  The mould is moved with ``set_sdf_poses`` or
``move_sdfs`` before every step: it may rise, translate and tilt; its slip against the sheet drags the sheet by friction."""
import numpy as np

from ..engine import sdf
from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.04, N=8, k_sdf=2e3, mu=0.5, major=None, minor=None, spacing=None, push=0.0, Kb=100.0, k_angle=3.14, stvk=None, pin="all",
                 device="cuda:0", newton_cap=50):
        assert pin in ("side", "all"), pin
        self._pin = pin
        self._N = N
        self._newton_cap = newton_cap
        major = 0.3 * cloth_size if major is None else major
        minor = 0.1 * cloth_size if minor is None else minor
        self._mould = dict(k=float(k_sdf), mu=float(mu), major=float(major), minor=float(minor), push=float(push), h=float(0.5 * minor if spacing is None else spacing))
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

    def mould(self):
        """(grid, origin (3,), spacing, centre (1, 3), quaternion (1, 4), offset (1,), mu (1,)) of the scene's ring: level, its top `push` above the flat
        sheet's plane (z = 0); the grid reaches three spacings beyond the ring, so that the solid keeps clear of the border (sdf.border_clear)"""
        m = self._mould
        ext = np.array([m["major"] + m["minor"], m["major"] + m["minor"], m["minor"]]) + 3.0 * m["h"]
        grid, origin = sdf.sample(sdf.torus(m["major"], m["minor"], axis=2), -ext, ext, m["h"])
        return grid, origin, m["h"], np.array([[0.0, 0.0, m["push"] - m["minor"]]]), np.array([[1.0, 0.0, 0.0, 0.0]]), np.array([0.0]), np.array([m["mu"]])

    def centre_vertex(self):
        """global id of the vertex in the middle of the grid (N even: the grid has one); it lies over the ring's hole"""
        c = self.cloths[0]
        return c.offset + (c.N // 2) * (c.M + 1) + c.M // 2

    def init(self):
        c = self.cloths[0]
        c.init(-0.5 * self.cloth_size, -0.5 * self.cloth_size, 0.0)

    def init_all(self):
        super().init_all()
        if self.n_sdf == 0:   # (a caller's own list, set before, stays)
            grid, origin, h, c, q, r, mu = self.mould()
            assert sdf.border_clear(grid, r[0], self.eps_contact), "the ring reaches the border of its grid"
            self.set_sdfs([grid], [origin], [h], c, q, r, mu, self._mould["k"])

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
