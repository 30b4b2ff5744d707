"""Synthetic seam scene (no reference counterpart): two N x N cloths lying edge to edge.  Cloth 0 has a pinned row (i = 0); cloth 1 is sewn to
cloth 0's free edge (row i = N) by BaseScene.sew -- one vertex-to-vertex tie per vertex of its row 0 -- and hangs from it under gravity.  No contact
pairs: the two cloths meet only in the ties.  ``tube=True`` is one cloth rolled into a ring whose row 0 is sewn to its own row N (the rest shape is
flat); the row opposite the seam is pinned."""
import numpy as np

from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.04, N=12, k_tie=2e5, tube=False, Kb=100.0, k_angle=3.14, perturb=1e-4, stvk=None, device="cuda:0", newton_cap=50):
        self._N = N
        self._tube = bool(tube)
        self._perturb = perturb
        self._newton_cap = newton_cap
        super().__init__(cloth_size=cloth_size, enable_gripper=False, device=device)
        for c in self.cloths:
            c.Kb[None] = Kb
            c.k_angle[None] = k_angle
            if stvk:   # (stvk_mu, stvk_lam) in N/m: the StVK membrane on every cloth
                c.stvk_mu[None], c.stvk_lam[None] = stvk
                c.membrane[None] = 1.0
        self._k_tie0 = float(k_tie)

    def init_scene_parameters(self):
        self.dt = 5e-3
        self.h = self.dt
        self.cloth_cnt = 1 if self._tube else 2
        self.elastic_cnt = 0
        self.cloth_N = self._N
        self.cloth_M = self._N
        self.k_contact = 10000
        self.eps_contact = 0.0004
        self.eps_v = 0.01
        self.max_n_constraints = 16
        self.damping = 1.0

    def init_objects(self):
        nv = (self.cloth_N + 1) ** 2
        for i in range(self.cloth_cnt):
            self.cloths.append(Cloth(self.cloth_N, self.dt, self.cloth_size, 0, 4e1, i * nv, False, self.cloth_M))
        self.tot_NV = nv * self.cloth_cnt

    def seam_pairs(self):
        """(vertices sewn, vertices they are sewn to): cloth 1's row 0 onto cloth 0's row N; the tube: row 0 onto row N of the one cloth"""
        c0 = self.cloths[0]
        W = c0.M + 1
        a = (c0 if self._tube else self.cloths[1]).offset + np.arange(W)
        b = c0.offset + c0.N * W + np.arange(W)
        return a, b

    def init(self):
        N = self._N
        for q, c in enumerate(self.cloths):
            c.init(q * self.cloth_size, 0.0, 0.0)
            p = c.pos.to_numpy()
            i, j = np.meshgrid(np.arange(c.N + 1), np.arange(c.M + 1), indexing="ij")
            if self._tube:   # a ring of circumference N dx around the y axis: row N comes back to row 0
                R = N * c.dx / (2.0 * np.pi)
                th = (2.0 * np.pi * i / N).reshape(-1)
                p[:, 0] = R * np.sin(th)
                p[:, 2] = R * (np.cos(th) - 1.0)
            elif self._perturb:
                p[:, 2] = (self._perturb * np.sin(7.0 * i + 3.0 * q) * np.cos(5.0 * j)).reshape(-1)
                p[i.reshape(-1) == (c.N if q == 0 else 0), 2] = 0.0   # (the two rows of the seam start on each other)
            c.pos.from_numpy(p)

    def init_all(self):
        super().init_all()
        if self.n_tie == 0:   # (the seam; a caller's own list, set before, stays)
            self.sew(*self.seam_pairs(), self._k_tie0)

    def contact_pairs(self):
        return []

    def set_frozen_kernel(self):
        c = self.cloths[0]
        fr = self.frozen.t.view(-1, 3)
        row = c.N // 2 if self._tube else 0
        fr[c.offset + row * (c.M + 1): c.offset + (row + 1) * (c.M + 1)] = 1

    def action(self, step, delta_pos=None, delta_rot=None, delta_dis=None):
        pass
