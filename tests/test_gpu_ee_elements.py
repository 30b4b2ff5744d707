"""The edge-edge contact kernels alone ("contact_ee" = 1; csrc/k_contact.hpp: ee_qualifies / k_ee_build for the records, k_contact_assemble_coop<LIT, true>,
k_ee_energy, k_ee_backprop, k_contact_mask, the row lists and k_contact_row_gather; k_contact_zfrozen_gather of csrc/k_adjoint.hpp) against the mpmath
restatement tests/ee_elements_numpy.py.  Probe scenes: one target edge and one query edge crossing over it per probe, each an edge of a surface triangle
whose third vertex is folded away from the other edge, probes 0.02 m apart, carried by tetrahedra with mu = lam = 0; m and dt are powers of two; a pair
of bodies per kind of mu.  Every vertex carries the border flag: the vertex-triangle projection of a query vertex lands on the rim of the target triangle
and lists nothing (contact_counts() == (0, n)).  Detection runs at a benign state with prev != pos and only delivers the slots; the exported records are
then data.  Assembly runs at an evaluation state with prev = pos, vel = 0, gravity 0.

Bound (tet_numpy.bound, as tests/test_gpu_contact_elements.py): |gpu - mp|_F <= 8 max(e64, 4 u |mp|_F) per quantity, per 3 x 3 sub-block, per vertex, per
record; e64 over the state, its six rotations and eight one-ulp jitters (records: the jitters alone; the exactly parallel state: jitters that keep the
y and z of an edge's two vertices the same bits, so that a x b stays zero); a projected block takes the whole block's float64 error + 64 u |unprojected block|_F.  Every state
passes ee_elements_numpy.decisions_safe on the CPU (tests/test_ee_elements_numpy.py); no slot is skipped or masked.  Every test prints its largest
|gpu - mp| / bound per quantity."""
import copy
import functools
import os
import sys

import mpmath as mp
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_numpy as cn  # noqa: E402
import ee_elements_numpy as ee  # noqa: E402
from test_gpu_tet_elements import Ratios, _dev  # noqa: E402

pytestmark = pytest.mark.gpu


class EERatios(Ratios):
    label = "edge-edge elements"


class Ctx:
    """a probe context (an ee_elements_numpy.Scene by name, or a Merged) and the calls the tests make"""
    def __init__(self, name, cap=None, detect=True, lagged=True, sc=None, counts=None):
        self.name, self.sc = name, ee.scene(name) if sc is None else sc
        self.nv = self.sc.nv
        self.ctx = ee.probe_context(self.sc, max_n_constraints=cap)
        self.ref = torch.zeros(3, dtype=torch.float64, device="cuda")
        self.xd, self.pd = _dev(self.sc.x), _dev(self.sc.prev if lagged else self.sc.x)
        if detect:
            self.nothing_detected()
            self.detect((0, len(self.sc.active)) if counts is None else counts)

    def detect(self, counts):
        self.nc = self.ctx.contact_detect(self.xd, self.pd)
        assert self.ctx.contact_counts() == counts and self.nc == sum(counts), (self.ctx.contact_counts(), counts)
        self.cons = self.ctx.constraints()
        assert np.array_equal(self.cons["idx"], self.sc.idx()[:self.nc])

    def close(self):
        self.ctx.close()

    def nothing_detected(self):
        """the carriers alone: F == 0 and a pure m / dt^2 diagonal, exactly, under spd 0 and 1"""
        for spd in (0, 1):
            _, _, _, g = self._assemble(self.sc.x, spd)
            assert not g.any() and np.array_equal(self.ctx.matrix_csr().toarray(), self.sc.mdt2 * np.eye(3 * self.nv)), spd

    def _assemble(self, x, spd):
        pos = _dev(x)
        g = torch.zeros(3 * self.nv, dtype=torch.float64, device="cuda")
        prev, vel = pos.clone(), torch.zeros_like(pos)
        self.ctx.assemble(pos, prev, vel, self.ref, spd=spd, grad=g)
        torch.cuda.synchronize()
        return pos, prev, vel, g.cpu().numpy()

    def assemble(self, x, spd):
        """what contact_numpy.check_assembly takes"""
        pos, prev, vel, g = self._assemble(x, spd)
        static = self.ctx.matrix_csr().toarray()
        d = np.diag(static).copy()
        assert np.array_equal(static, np.diag(d)) and np.array_equal(d, np.full(3 * self.nv, self.sc.mdt2)), "the static part is the mass term"
        op = self.ctx.operator_csr().toarray() - static
        return dict(blocks=self.ctx.contact_blocks(False), masked=self.ctx.contact_blocks(True), g=g, op=op, E=self.ctx.energy(pos, prev, vel, self.ref))

    def set_frozen(self, fz):
        self.ctx.set_frozen(np.zeros(3 * self.nv, np.int32) if fz is None else fz)


_CONS = {}


def _key(cons):
    k = hash(tuple(cons[q].tobytes() for q in ("idx", "w", "k", "mu", "dx0", "T", "n")))
    _CONS[k] = cons
    return k


@functools.lru_cache(maxsize=None)
def _expected(name, state, spd, key, lagged=True):
    return ee.expected(_CONS[key], ee.state_positions(name, state, lagged), spd, state=state)


def _frozen(sc, slot_pos):
    """one frozen dof in position `slot_pos` of every slot: component (slot + slot_pos) % 3"""
    fz = np.zeros(3 * sc.nv, np.int32)
    for s, vs in enumerate(sc.idx()):
        fz[3 * vs[slot_pos] + (s + slot_pos) % 3] = 1
    return fz


# ------------------------------------------------------------------------------------------------ records
def test_records_match_mpmath_and_repeat_bit_for_bit():
    """ctx.constraints() after contact_detect against the restatement at the detection state: idx and mu exact (the kind shows through mu), w[2] == 0 exactly,
    s, t, k, dx0, T, n within the bound, T orthogonal to n and its rows to each other within 8 u; the four probes at sin = 1e-2 (1 - 1e-6), s = -1e-6,
    t = 1 + 1e-6 and a gap of 1.5 eps are left out (16 slots of 20 probes, idx entry for entry); a second detection gives the same bits"""
    C = Ctx("geometry")
    assert C.sc.P == 20 and C.nc == 16
    R = EERatios()
    ee.check_records(C.sc, C.cons, R)
    assert C.ctx.contact_detect(C.xd, C.pd) == C.nc
    again = C.ctx.constraints()
    for q, v in C.cons.items():
        assert np.array_equal(v, again[q]), q
    C.close()
    R.check("records")


# ------------------------------------------------------------------------------------------------ assembly
@pytest.mark.parametrize("state", ee.ASSEMBLY_STATES)
def test_assembly_matches_mpmath(state):
    """16 slots (edges of 1 / 150 m and 1e-4 m and one against the other, sin 1 / 0.3 / 1e-2 (1 + 1e-6) at the detection, closest points mid-edge and 1e-3 and
    1e-6 from the ends, D > 0 and D < 0, |n.x| = 0.5 -+ 1e-6 and well to either side, the three kinds) at one evaluation state, under spd 0 and 1, free and
    with one frozen dof in each of the four positions of a slot in turn: unmasked and masked blocks per 3 x 3 sub-block, masked blocks exactly zero on
    frozen rows and columns, F per vertex, operator_csr() - matrix_csr() per vertex pair and nothing outside the slots' pairs, every block PSD under spd 1,
    the energy.  The operator difference carries the rounding of the float64 sum with the static diagonal m / dt^2 it is taken from: its pairs (v, v)
    take the bound of that term too (contact_numpy.check_assembly, static_diag)"""
    C = Ctx("geometry")
    key = _key(C.cons)
    x = ee.state_positions("geometry", state)
    R = EERatios()
    for pos in (None, 0, 1, 2, 3):
        fz = None if pos is None else _frozen(C.sc, pos)
        C.set_frozen(fz)
        for spd in (0, 1):
            cn.check_assembly(_expected("geometry", state, spd, key), C.assemble(x, spd), R, "%s spd%d frozen %s" % (state, spd, pos), fz, C.sc.mdt2)
    C.close()
    R.check(state)


def test_assembly_where_the_edges_are_exactly_parallel():
    """axis-aligned probes detected at sin = 1, the query edge then laid along the target edge: a x b == 0.0 bit for bit (asserted on the float64
    restatement, tests/test_ee_elements_numpy.py), so D / C is 0 / 0 inside the kernels and nowhere else.  The restatement's rule: the comparison with eps is
    false, the normal part is off, the friction part as usual.  Blocks, F, operator and energy under spd 0 and 1, free and frozen, must be finite and equal
    that value within the bound; the same context assembled once more at the rest state must give the rest-state values: nothing is left behind in LDS or
    the block buffers"""
    C = Ctx("parallel")
    key = _key(C.cons)
    state = "exactly parallel"
    x = ee.state_positions("parallel", state)
    R, R2 = EERatios(), EERatios()
    for pos in (None, 0, 3):
        fz = None if pos is None else _frozen(C.sc, pos)
        C.set_frozen(fz)
        for spd in (0, 1):
            got = C.assemble(x, spd)
            assert all(np.isfinite(got[q]).all() for q in ("blocks", "masked", "g", "op", "E")), (pos, spd)
            cn.check_assembly(_expected("parallel", state, spd, key), got, R, "%s spd%d frozen %s" % (state, spd, pos), fz, C.sc.mdt2)
            cn.check_assembly(_expected("parallel", "rest", spd, key), C.assemble(C.sc.x, spd), R2, "rest after parallel spd%d frozen %s" % (spd, pos), fz, C.sc.mdt2)
    C.close()
    R.check(state)
    R2.check("rest, after the parallel state")


# ------------------------------------------------------------------------------------------------ launch edges
@pytest.mark.parametrize("nc", [1, 15, 16, 17, 33, 63, 64, 65, 129])
def test_launch_edges_match_mpmath(nc):
    """nc_ee = 1, 15, 16, 17, 33: the 16-lane groups of k_contact_assemble_coop<., true> (an idle group recomputes slot nc - 1 inside the wave's shuffles);
    63, 64, 65, 129: the 64-wide k_ee_energy (and k_ee_backprop: test_reverse_step) and the scans; every slot checked; a cap equal to nc passes"""
    name = "nc%d" % nc
    C = Ctx(name, cap=nc)
    key = _key(C.cons)
    R = EERatios()
    for spd in (0, 1):
        cn.check_assembly(_expected(name, "bump", spd, key), C.assemble(ee.state_positions(name, "bump"), spd), R, "nc%d spd%d" % (nc, spd), None, C.sc.mdt2)
    C.close()
    R.check(name)


@pytest.mark.parametrize("n_vf,n_ee", [(5, 17), (64, 1)])
def test_slots_behind_vertex_triangle_slots(n_vf, n_ee):
    """vertex-triangle probes of contact_numpy in front of edge-edge probes in one context: the edge-edge launches start at slot n_vf (ee_args, c_G + 12 n_vf,
    Hfull + 144 n_vf).  Both ranges against their own restatements; with the key off the same context lists the vertex-triangle slots alone, with the same
    record bits, and its values meet the same references"""
    vname, ename = "nc%d" % n_vf, "nc%dup" % n_ee
    vt, es = cn.scene(vname), ee.scene(ename)
    C = Ctx(None, sc=ee.Merged(vt, es), counts=(n_vf, n_ee))
    cons = C.cons
    R = EERatios()
    flag, dr, pidx, pw = C.ctx.proj_export()
    cn.check_records(vt, {q: v[:n_vf] for q, v in cons.items()}, (pidx[0, vt.qv], pw[0, vt.qv], dr[0, vt.qv]), R)
    ee.check_records(es, {q: v[n_vf:] for q, v in cons.items()}, R, offset=vt.nv)
    x = np.concatenate([cn.state_positions(vname, "bump"), ee.state_positions(ename, "bump")])
    exps = {}
    for spd in (0, 1):
        exps[spd] = cn.Expected(cons, x, spd, model=[cn.VT] * n_vf + [ee.EE] * n_ee)
        cn.check_assembly(exps[spd], C.assemble(x, spd), R, "(%d, %d) spd%d" % (n_vf, n_ee, spd), None, C.sc.mdt2)
    C.ctx.set_param("contact_ee", 0)
    C.detect((n_vf, 0))
    R0 = EERatios()
    for q, v in C.cons.items():
        assert np.array_equal(v, cons[q][:n_vf]), q
    for spd in (0, 1):
        e0 = copy.copy(exps[spd])
        e0.slots, e0.cons = exps[spd].slots[:n_vf], C.cons
        cn.check_assembly(e0, C.assemble(x, spd), R0, "(%d, 0) spd%d" % (n_vf, spd), None, C.sc.mdt2)
    C.close()
    R.check("(n_vf, n_ee) = (%d, %d)" % (n_vf, n_ee))
    R0.check("the same vertex-triangle probes with the key off")


def test_a_row_of_more_than_64_entries():
    """70 query edges of 1e-3 m across one target edge of 5 cm: its two vertices have rows of 70 entries"""
    C = Ctx("crowd")
    assert len(C.cons["k"]) == 70 and (np.bincount(C.cons["idx"].ravel())[:2] == 70).all()
    key = _key(C.cons)
    R = EERatios()
    for spd in (0, 1):
        cn.check_assembly(_expected("crowd", "bump", spd, key), C.assemble(ee.state_positions("crowd", "bump"), spd), R, "crowd spd%d" % spd, None, C.sc.mdt2)
    C.close()
    R.check("crowd")


def test_a_cap_below_nc_is_an_error_and_leaves_nothing_behind():
    from thinshelllab_amd._lib import TslError
    C = Ctx("nc17", cap=16, detect=False)
    with pytest.raises(TslError, match="0 vertex-triangle \\+ 17 edge-edge active constraints exceed max_n_constraints = 16"):
        C.ctx.contact_detect(C.xd, C.pd)
    assert C.ctx.contact_counts() == (0, 0)
    C.close()
    C = Ctx("nc17", cap=17)
    assert C.nc == 17
    C.close()


# ------------------------------------------------------------------------------------------------ reverse step
@pytest.mark.parametrize("name,frozen_pos", [("rv16", None), ("rv16", 0), ("rv16", 3), ("rv63", None), ("rv64", 2), ("rv65", None), ("rv129", 1)])
def test_reverse_step_matches_mpmath(name, frozen_pos):
    """a three-state tape (x_0, x_1, x_2) and one adjoint_step at s = 2 with damping 1 (its detection runs at (x_1, x_1)): slots that stick, slip, keep their
    four vertices and one in four penetrated (ee_elements_numpy "reverse mix"), on 16, 63, 64, 65 and 129 probes with sin >= 0.3, both edge lengths and
    D of both signs, m / dt^2 = 2^22 (above the most negative eigenvalue of the unprojected operator: tests/test_ee_elements_numpy.py).  p is read back as
    -pos_grad[0] dt^2 / m on the free dofs (exact) and is zero on the frozen ones; with that p: pos_grad[1] = the gathered k_ee_backprop entries +
    2 m / dt^2 p, tmp_z_frozen on the frozen dofs.  The solver's accuracy plays no part"""
    C = Ctx(name)
    sc, nv = C.sc, C.nv
    fz = np.zeros(3 * nv, np.int32) if frozen_pos is None else _frozen(sc, frozen_pos)
    C.ctx.set_frozen(fz)
    free = fz == 0
    x2 = ee.state_positions(name, "reverse mix", lagged=False)
    tape = _dev(np.stack([sc.prev, sc.x, x2]))
    seed = 1e-3 * np.random.default_rng(9).normal(size=3 * nv) * free
    pg = torch.zeros((3, 3 * nv), dtype=torch.float64, device="cuda")
    pg[2] = _dev(seed)
    refb, ag = torch.zeros((3, 3), dtype=torch.float64, device="cuda"), torch.zeros((3, 3), dtype=torch.float64, device="cuda")
    tz = torch.zeros(3 * nv, dtype=torch.float64, device="cuda")
    stats = C.ctx.adjoint_step(2, 3, tape, pg, refb, ag, tz)
    torch.cuda.synchronize()
    assert np.array_equal(pg[2].cpu().numpy(), seed)
    assert C.ctx.contact_counts() == (0, len(sc.active))
    cons = C.ctx.constraints()      # the step detected at (x_1, x_1)
    assert np.array_equal(cons["idx"], sc.idx())
    pg0, pg1 = pg[0].cpu().numpy(), pg[1].cpu().numpy()
    assert not pg0[~free].any()
    p = -pg0 * cn.DT ** 2 / sc.mass
    assert np.isfinite(p).all(), stats
    assert np.array_equal(p * sc.mdt2, -pg0)
    exp = cn.Expected(cons, x2, 0, fz, p, model=ee.EE)
    rev = cn.expected_reverse(exp, p, np.zeros(len(cons["k"]), int), fz)
    R = EERatios()
    with mp.workdps(50):
        inertia = 2 * sc.mdt2 * p.reshape(nv, 3)                                    # exact in float64
        want = (rev["acc"][0] + inertia, rev["acc"][1])
        bnd = rev["accb"] + 32 * cn.U * cn._fn(inertia, 1)                          # sum of the two terms' bounds; the inertia term has e64 = 0
        R.add("pos_grad[1]", cn.worst_ratio(cn._fn(cn.diff(pg1.reshape(nv, 3), want), 1), bnd), 1.0)
        tzh = tz.cpu().numpy().reshape(nv, 3)
        assert not tzh[free.reshape(nv, 3)].any()
        if frozen_pos is not None:
            ez = np.abs(cn.diff(tzh, rev["zf"]))[~free.reshape(nv, 3)]
            R.add("tmp_z_frozen", cn.worst_ratio(ez, rev["zfb"][~free.reshape(nv, 3)]), 1.0)
    C.close()
    R.check("reverse step, %s, frozen %s" % (name, frozen_pos))


# ------------------------------------------------------------------------------------------------ the documented refusals
def test_gradients_that_edge_edge_slots_do_not_have_are_refused():
    """friction_grad, param_grads for k_contact and for a live mu key whose kind has edge-edge slots: each a TslError naming edge-edge, never a number"""
    from thinshelllab_amd._lib import TslError
    C = Ctx("geometry")
    assert set(C.sc.kinds()) == {0, 1, 2}
    x = _dev(C.sc.x)
    p = _dev(np.random.default_rng(5).normal(size=3 * C.nv))
    with pytest.raises(TslError, match="edge-edge"):
        C.ctx.friction_grad(x)
    for key in ("k_contact", "mu_cloth_elastic", "mu_cloth_cloth"):
        with pytest.raises(TslError, match="edge-edge"):
            C.ctx.param_grads(x, C.ref, [key], p=p)
    C.close()
