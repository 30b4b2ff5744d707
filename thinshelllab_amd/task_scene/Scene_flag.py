"""Synthetic flag scene (no reference counterpart, which has no load from the medium): one N x N cloth that hangs in the x-z plane from the two
corners of its top edge, under gravity, in a side wind (BaseScene.set_wind on every face of the cloth) -- no body, no contact
pair, no constraint slot.  The default coefficients (200 and 20 N s / m^3) make the drag of a 1 m / s wind about half the flag's weight.  The wind velocity is set with ``set_wind_velocity`` before every step."""
import numpy as np

from ..engine.BaseScene import BaseScene
from ..engine.model_fold_offset import Cloth


class Scene(BaseScene):
    _newton_cap = 50

    def __init__(self, cloth_size=0.08, N=16, c_n=200.0, c_t=20.0, wind=(0.3, 1.0, 0.1), Kb=100.0, k_angle=3.14, stvk=None, device="cuda:0", newton_cap=50):
        self._N = N
        self._newton_cap = newton_cap
        self._wind = dict(c_n=float(c_n), c_t=float(c_t), W=np.asarray(wind, dtype=np.float64).reshape(3).copy())
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

    def init(self):
        c = self.cloths[0]
        c.init(-0.5 * self.cloth_size, 0.0, 0.0)
        p = c.pos.to_numpy()   # the flat sheet (x, y, 0) turned about the x axis into the x-z plane: grid index i runs along x, j hangs down
        c.pos.from_numpy(np.stack([p[:, 0], np.zeros(len(p)), -p[:, 1]], axis=1))

    def hung_vertices(self):
        """global ids of the two corners the flag hangs from: (i, j) = (0, 0) and (N, 0)"""
        ids = self.cloths[0].corner_ids()
        return [ids[0], ids[2]]

    def free_edge(self):
        """global ids of the vertices of the bottom edge j = M"""
        c = self.cloths[0]
        return [c.offset + i * (c.M + 1) + c.M for i in range(c.N + 1)]

    def init_all(self):
        super().init_all()
        if self.n_wind == 0:   # (a caller's own list, set before, stays)
            self.set_wind(self._wind["c_n"], self._wind["c_t"])
            self.set_wind_velocity(self._wind["W"])

    def contact_pairs(self):
        return []

    def set_frozen_kernel(self):
        fr = self.frozen.t.view(-1, 3)
        for v in self.hung_vertices():
            fr[v] = 1

    def action(self, step, delta_pos=None, delta_rot=None, delta_dis=None):
        pass
