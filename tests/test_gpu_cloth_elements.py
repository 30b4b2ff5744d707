"""The cloth kernels alone (csrc/k_cloth.hpp: k_cloth_normals, k_cloth_grad_face / _hinge, k_cloth_quirk, k_cloth_hess_face / _hinge, k_cloth_gather,
hinge_energy / cface_energy, k_cloth_update_ref; k_pg_face / k_pg_hinge of csrc/k_param.hpp) against the mpmath restatement tests/cloth_numpy.py,
through folds.  Contexts hold cloths only, built from the tables of init_mesh: no faces table, no pairs, gravity 0, prev_pos = pos, vel = 0,
membrane 0, and a mass so small that m / dt^2 is lost in every block (the references add it all the same).

Bound (tet_numpy.bound): |gpu - mp|_F <= 8 max(e64, 4 u |mp|_F) per element quantity and per 3 x 3 vertex-pair sub-block of an element block;
a vertex's gradient and a vertex pair's block of the assembled matrix take the mp sum of their elements and the sum of their bounds.  e64 is the
largest error against mp of the float64 restatement over the state, its six coordinate rotations, eight copies with every coordinate moved by
one ulp and two with the cosine of every face pair that is coplanar by construction moved by one ulp (cloth_numpy.Reference says why); a
projected block adds 64 u |block|_F inside the max.  Every state passes cloth_numpy.decisions_safe on the CPU (tests/test_cloth_numpy.py); no
element is skipped or masked.  Each state runs with (Kl, Ka, Kb) = (Kl, 0, 0), (0, Ka, 0), (0, 0, Kb) and all three, free and with three frozen vertices,
under spd 0 / 1 / 2.  Every test prints its largest |gpu - mp| / bound per quantity."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloth_numpy as cn  # noqa: E402
from test_gpu_tet_elements import Ratios, _dev  # noqa: E402

pytestmark = pytest.mark.gpu


class ClothRatios(Ratios):
    label = "cloth elements"


class Ctx:
    """a cloths-only context of a state and the calls the tests make"""
    def __init__(self, st, frozen_verts=()):
        self.st, self.nv = st, st.nv
        fz = np.zeros(3 * st.nv, np.int32)
        for v in frozen_verts:
            fz[3 * v:3 * v + 3] = 1
        self.ctx = cn.cloth_context(st.cloths, st.nv, fz)
        self.pos = _dev(st.x)
        self.prev, self.vel = self.pos.clone(), torch.zeros_like(self.pos)   # (named: a temporary's memory is handed to the next allocation before the engine reads it)
        self.ref = _dev(np.concatenate(st.ra))

    def close(self):
        self.ctx.close()

    def constants(self, combo):
        for i, c in enumerate(self.st.cloths):
            for on, key, v in zip(cn.COMBOS[combo], ("Kl", "Ka", "Kb"), (c.Kl, c.Ka, c.Kb)):
                self.ctx.set_param("cloth%d.%s" % (i, key), v if on else 0.0)

    def assemble(self, spd):
        from thinshelllab_amd._lib import check
        from thinshelllab_amd.context import _ptr
        g = torch.zeros(3 * self.nv, dtype=torch.float64, device="cuda")
        self.ctx.refresh_stream()
        check(self.ctx.L.tsl_assemble(self.ctx.h, _ptr(self.pos), _ptr(self.prev), _ptr(self.vel), _ptr(self.ref), int(spd), _ptr(g)),
              "tsl_assemble")
        torch.cuda.synchronize()
        return self.ctx.matrix_csr().toarray(), g.cpu().numpy()

    def energy(self):
        return self.ctx.energy(self.pos, self.prev, self.vel, self.ref)


def _run_state(key, spd2_combos=tuple(cn.COMBOS)):
    ref = cn.reference(key)
    st = ref.st
    R = ClothRatios()
    for frozen in ((), cn.frozen_of(st)):
        C = Ctx(st, frozen)
        tag = " frozen" if frozen else ""
        for combo in cn.COMBOS:
            C.constants(combo)
            for spd in (0, 1, 2):
                if spd == 2 and combo not in spd2_combos:
                    continue
                e = cn.expected(ref, combo, spd, frozen, 7)
                A, g = C.assemble(spd)
                # PSD: spd 2 projects every face block, the hinge blocks are d2 g g^T; under spd 1 the springs alone are a sum of clamped blocks
                cn.check_assembly(e, A, g, R, "spd%d %s%s" % (spd, combo, tag), psd=(spd == 2 or (spd == 1 and combo == "Kl")))
            e = cn.expected(ref, combo, 0, frozen, 7)
            cn.ratio(R, "energy", abs(float(mp.mpf(C.energy()) - e.E)), e.Eb)
        # per-key sums (the kernels take no constant: asked once, with all three set) and the force of the elastic bodies, of which there are none
        got = C.ctx.param_grads(C.pos, C.ref, list(e.keys), p=_dev(e.p.ravel()))
        for k, (want, bnd) in e.keys.items():
            cn.ratio(R, "key " + k.split(".")[1] + tag, abs(float(mp.mpf(got[k]) - want)), bnd)
        f = torch.ones(3 * st.nv, dtype=torch.float64, device="cuda")
        assert not C.ctx.elastic_force(C.pos, f).cpu().numpy().any()
        C.close()
    R.check(key)


SMALL = [k for k in cn.GPU_KEYS if k.split("/")[0] in ("1x1", "2x1", "1x2", "3x2")]
LARGE = [k for k in cn.GPU_KEYS if k not in SMALL]


@pytest.mark.parametrize("key", SMALL)
def test_small_meshes_match_mpmath_through_folds(key):
    """1 x 1 (fewer than three faces: the rows of the quirk table beyond the cloth), 2 x 1, 1 x 2, 3 x 2 (both cell parities, so the wrongly tabled
    slots), cells of 1 / 150 m and 1e-4 m, every mesh in every state: rest, turned rest, ripples of +-1.0e-4, +-1.3e-3, +-1.5e-3 rad (below, just
    below and just above the switch from the series to acos; not on 1 x 1, which has no grid line to fold a zigzag about), folds of +-90,
    +-170 degrees and +-(pi - 1e-3) with reference angles 0, the fold's own and its opposite (1 x 1: about its diagonal), stretch x 1.5,
    compression x 0.5 (spring blocks indefinite), a sliver shear, a smooth bump"""
    _run_state(key)


@pytest.mark.parametrize("key", LARGE)
def test_launch_edges_and_a_second_cloth_match_mpmath(key):
    """8 x 8 = 128 faces (one full workgroup of the face kernels), + a 1 x 1 second cloth = 130 (tail), 10 x 10 = 200 faces and 280 hinges (the hinge
    kernels' edge at 256), + a 3 x 2 second cloth with its own cell size, constants, v_offset and reference angles (Q + cid * 90, face_start and
    cid decide its values), cells of 1 / 150 m and 1e-4 m.  The 10 x 10 meshes rippled and folded by 90 degrees, the 8 x 8 meshes also with the
    bump, compressed and folded to -(pi - 1e-3) against an opposite reference angle.  spd 0 and 1 run with each constant alone and all three,
    the whole-block projection (spd 2, one mp eigen-solve of a 9 x 9 block per face and combination) with Kb alone and all three."""
    _run_state(key, spd2_combos=("Kb", "all"))


@pytest.mark.parametrize("key", cn.PLASTIC_KEYS)
def test_update_ref_angle_at_the_plastic_threshold(key):
    """folds at 0.5, 0.99, 1.01 and 2 times the plastic threshold of each of two cloths, both signs: the new reference angle of every hinge
    against mp, every other slot untouched"""
    ref = cn.reference(key)
    st = ref.st
    C = Ctx(st)
    R = ClothRatios()
    C.ctx.update_ref_angle(C.pos, C.ref)
    torch.cuda.synchronize()
    got = C.ref.cpu().numpy().reshape(-1, 3)
    f0 = 0
    for i, c in enumerate(st.cloths):
        e64 = ref.e64(i, lambda ev, part: cn._sel(ev, part, ["newref"]), None)
        new = got[f0:f0 + c.NF]
        touched = np.zeros((c.NF, 3), bool)
        for h, (f, l) in enumerate(c.hinges):
            touched[f, l] = True
            want = ref.mp[i]["newref"][h]
            cn.ratio(R, "ref_angle", abs(float(mp.mpf(float(new[f, l])) - want)), cn.bound(mp.mpf(float(e64[h])), abs(want)))
        assert np.array_equal(new[~touched], st.ra[i][~touched])
        f0 += c.NF
    C.close()
    R.check(key)
