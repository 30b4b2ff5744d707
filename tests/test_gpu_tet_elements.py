"""The tetrahedron kernels alone (csrc/k_fem.hpp: k_tet_grad, tet_energy, k_tet_hess_coop; k_pg_tet of csrc/k_param.hpp) against the mpmath
restatement tests/tet_numpy.py, through crush and inversion.  Contexts hold elastic bodies only, built from tables: no cloth, no pairs,
gravity 0, prev_pos = pos, vel = 0, and a mass so small that m / dt^2 is lost in every block diagonal (the references add it all the same),
so that an element's 12 x 12 block reads straight out of ctx.matrix_csr().

Bound (tet_numpy.bound): |gpu - mp|_F <= 8 max(e64, 4 u |mp|_F) per element and quantity, e64 = the error of the float64 restatement against
mpmath, largest of the six relabelings of vertices 0..2; a projected block takes e64 of the unprojected block + 64 u |block|_F.  Sums over
elements (energy, per-key sums, the ring's shared vertices) take the sum of their elements' bounds.  Every test prints its largest
|gpu - mp| / bound per quantity."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tet_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu

U = tn.U
MASS, DT = 1e-30, 5e-3
MDT2 = MASS / DT ** 2


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda")


class Ctx:
    """a context of disjoint-tet bodies [(kind, [(rest, state), ...])] and the calls the tests make"""
    def __init__(self, bodies=None, raw=None, frozen=None):
        self.bodies, tabs, off = [], [], 0
        if raw is None:
            xs = []
            for kind, items in bodies:
                X, x, tets, B, W = tn.disjoint_mesh(items)
                tabs.append((tn.MATERIALS[kind], tets + off, B, W, off, len(x)))
                self.bodies.append((kind, items, off))
                xs.append(x); off += len(x)
            self.x = np.concatenate(xs)
        else:
            kind, x, tets, B, W = raw
            tabs.append((tn.MATERIALS[kind], tets, B, W, 0, len(x)))
            self.x = x
        self.tets = np.concatenate([t[1] for t in tabs])
        self.nv = len(self.x)
        self.ctx = tn.tet_context(tabs, self.nv, mass=MASS, dt=DT, frozen=frozen)
        self.ref = torch.zeros(3, dtype=torch.float64, device="cuda")

    def close(self):
        self.ctx.close()

    def assemble(self, spd, x=None):
        """(dense matrix, gradient) of one assembly; spd 0 / 1 / 2 as tsl_assemble takes it (2 = every element block projected)"""
        from thinshelllab_amd._lib import check
        from thinshelllab_amd.context import _ptr
        pos = _dev(self.x if x is None else x)
        g = torch.zeros(3 * self.nv, dtype=torch.float64, device="cuda")
        prev, vel = pos.clone(), torch.zeros_like(pos)   # (named: a temporary's memory is handed to the next allocation before the engine reads it)
        self.ctx.refresh_stream()
        check(self.ctx.L.tsl_assemble(self.ctx.h, _ptr(pos), _ptr(prev), _ptr(vel), _ptr(self.ref), int(spd), _ptr(g)), "tsl_assemble")
        torch.cuda.synchronize()
        return self.ctx.matrix_csr().toarray(), g.cpu().numpy()

    def energy(self):
        pos = _dev(self.x)
        return self.ctx.energy(pos, pos.clone(), torch.zeros_like(pos), self.ref)

    def force(self):
        out = torch.zeros(3 * self.nv, dtype=torch.float64, device="cuda")
        self.ctx.elastic_force(_dev(self.x), out)
        return out.cpu().numpy()

    def param_grads(self, keys, p):
        return self.ctx.param_grads(_dev(self.x), self.ref, keys, p=_dev(p))

    def refs(self):
        """element references in tet order"""
        return [tn.element_reference(r, s, kind) for kind, items, _ in self.bodies for r, s in items]


def _dofs(v):
    return (3 * np.asarray(v)[:, None] + np.arange(3)).ravel()


def _err(got, ref_mp):
    """|got - mp|_F with the difference taken in mp"""
    with mp.workdps(50):
        a = np.array([mp.mpf(float(v)) for v in np.asarray(got).ravel()], dtype=object)
        return float(tn.fro(a - np.asarray(ref_mp, dtype=object).ravel()))


def _mass12():
    return np.diag(np.full(12, mp.mpf(MDT2)))


class Ratios(dict):
    label = "tet elements"

    def add(self, q, err, bnd):
        self[q] = max(self.get(q, 0.0), err / bnd)

    def check(self, what):
        print("%s, %s: largest |gpu - mp| / bound: %s" % (self.label, what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (what, bad)


def _check_blocks(C, rs, spd, A, g, R, tag=""):
    """every element's 12 x 12 block and 12 gradient entries of a disjoint-tet mesh against mp, nothing outside the blocks, clamped blocks PSD"""
    mask = np.zeros_like(A, dtype=bool)
    for t, r in enumerate(rs):
        d = _dofs(C.tets[t])
        mask[np.ix_(d, d)] = True
        proj = tn.clamps(r["mat"], spd)
        with mp.workdps(50):
            want = (r["block_spd"] if proj else r["block"]) + _mass12()
        bnd = tn.block_bound(r, proj)
        blk = A[np.ix_(d, d)]
        R.add("block spd%d%s" % (spd, tag), _err(blk, want), bnd)
        if proj:   # within bnd of a PSD matrix in the Frobenius norm, hence in the 2-norm (Weyl)
            assert np.linalg.eigvalsh(0.5 * (blk[:9, :9] + blk[:9, :9].T)).min() >= -bnd, (t, spd)
        if g is not None:
            R.add("gradient", _err(g[d], r["grad"]), tn.bound(r["grad_e64"], r["grad_n"]))
    assert not A[~mask].any()


def _check_sums(C, rs, R, seed):
    """energy, elastic_force (with an external force) and the per-key sums of tsl_param_grad_keys of a disjoint-tet mesh"""
    with mp.workdps(50):
        E = sum(r["energy"] for r in rs)
        R.add("energy", abs(float(mp.mpf(C.energy()) - E)), float(8 * max(sum(r["energy_e64"] for r in rs), 4 * U * abs(E))))
        rng = np.random.default_rng(seed)
        gs = np.array([float(r["grad_n"]) for r in rs])
        fext = rng.normal(size=(C.nv, 3)) * np.repeat(gs, 4)[:, None] / 4
        C.ctx.set_ext_force(fext)
        f = C.force()
        C.ctx.set_ext_force(np.zeros((C.nv, 3)))
        zero = np.zeros((4, 3), dtype=object)
        for t, r in enumerate(rs):
            d = _dofs(C.tets[t])
            fe = np.array([mp.mpf(v) for v in fext[C.tets[t]].ravel()], dtype=object).reshape(4, 3)
            want = tn.elastic_force(r["grad"].reshape(4, 3), np.full(4, mp.mpf(MASS)), zero, fe)
            R.add("elastic_force", _err(f[d], want), tn.bound(r["grad_e64"], tn.fro(want)))
        p = rng.normal(size=3 * C.nv)
        t0 = 0
        for b, (kind, items, off) in enumerate(C.bodies):
            keys = ["elastic%d.mu" % b, "elastic%d.lam" % b]
            got = C.param_grads(keys, p)
            for key, q in zip(keys, ("dmu", "dlam")):
                want, e64 = mp.mpf(0), mp.mpf(0)
                for t in range(t0, t0 + len(items)):
                    pe = np.array([mp.mpf(v) for v in p[_dofs(C.tets[t])]], dtype=object)
                    want -= sum(pe * rs[t][q])
                    e64 += tn.fro(pe) * rs[t][q + "_e64"]
                R.add("key " + q[1:], abs(float(mp.mpf(got[key]) - want)), tn.bound(e64, abs(want)))
            t0 += len(items)


# ------------------------------------------------------------------------------------------------ disjoint tets
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", tn.SIZES)
def test_disjoint_tets_match_mpmath_in_every_spd_mode(n, kind):
    """one body of n tets with four vertices each, neighbours in different rest shapes and states (rest, moderate compression, stretch, x10, and
    nearly flat / exactly flat / inverted for kind 0, J on either side of 0.01 / inverted for kind 1): block, gradient, energy, force and
    per-key sums per element; tail groups of the last workgroup must leave tet n - 1 and everything else intact"""
    C = Ctx(tn.gpu_meshes()["n%d_kind%d" % (n, kind)])
    rs, R = C.refs(), Ratios()
    for spd in (0, 1, 2):
        A, g = C.assemble(spd)
        _check_blocks(C, rs, spd, A, g, R)
    _check_sums(C, rs, R, seed=n)
    C.close()
    R.check("n = %d, kind %d" % (n, kind))


def test_two_bodies_in_one_launch_mix_clamped_and_unclamped_groups_in_a_wave():
    """5 tets of kind 0, then 5 of kind 1, spd 1: the first wave holds four clamping groups, the second one clamping group and three that do
    not clamp (and two idle ones): the mixed `on` of spd_clamp9_par"""
    C = Ctx(tn.gpu_meshes()["two_bodies"])
    rs, R = C.refs(), Ratios()
    for spd in (1, 0, 2):
        A, g = C.assemble(spd)
        _check_blocks(C, rs, spd, A, g, R)
    _check_sums(C, rs, R, seed=7)
    C.close()
    R.check("two bodies")


# ------------------------------------------------------------------------------------------------ warm basis
def test_warm_started_clamp_meets_the_same_bound_after_large_jumps():
    """17 tets, tet t at state (a, g, a, e)[(k + t) % 4] in assembly k, spd 1: the basis stored at one state is useless at the next.  The warm
    answer ("tet_warm" 1, the default) meets the bound against mpmath that the cold one ("tet_warm" 0) meets; the two are not compared with
    each other."""
    meshes = tn.gpu_meshes()
    C = Ctx(meshes["warm0"])
    R = Ratios()
    for warm in (1, 0):
        C.ctx.set_param("tet_warm", warm)
        for k in range(4):
            kind, items = meshes["warm%d" % k][0]
            _, x, _, _, _ = tn.disjoint_mesh(items)
            A, _ = C.assemble(1, x)
            _check_blocks(C, [tn.element_reference(r, s, kind) for r, s in items], 1, A, None, R, " warm%d" % warm)
    C.close()
    R.check("warm sequence")


# ------------------------------------------------------------------------------------------------ ring: shared vertices, frozen rule
@pytest.mark.parametrize("kind", [0, 1])
def test_ring_of_24_tets_sums_to_the_mp_blocks_free_and_frozen(kind):
    """24 tets around a shared edge (valence 24 at the two axis vertices: the k_vertex_gather / k_cloth_gather lists): matrix and gradient
    against the sum of the mp element blocks, then with three vertices frozen against the frozen rule (rows / columns removed, diagonal
    m / dt^2, gradient entries zero, per-key sums over the free dofs)"""
    X, x, tets, B, W, rs = tn.ring_reference(kind)
    nv = len(x)
    p = np.random.default_rng(11).normal(size=3 * nv)
    for frozen_verts in ((), (0, 5, 17)):
        fz = np.zeros(3 * nv, np.int32)
        if frozen_verts:
            fz[_dofs(frozen_verts)] = 1
        C = Ctx(raw=(kind, x, tets, B, W), frozen=fz)
        R = Ratios()
        mdt2 = np.full(nv, mp.mpf(MDT2))
        with mp.workdps(50):
            for spd in (0, 1, 2):
                A, g = C.assemble(spd)
                want = np.diag(np.repeat(mdt2, 3)) + np.zeros((3 * nv, 3 * nv), dtype=object)
                wg = np.zeros(3 * nv, dtype=object) + mp.mpf(0)
                bA, bg = 0.0, 0.0
                for t, r in enumerate(rs):
                    d = _dofs(tets[t])
                    proj = tn.clamps(r["mat"], spd)
                    want[np.ix_(d, d)] += r["block_spd"] if proj else r["block"]
                    wg[d] += r["grad"]
                    bA += tn.block_bound(r, proj); bg += tn.bound(r["grad_e64"], r["grad_n"])
                want = tn.mask_matrix(want, fz, mdt2)
                wg[fz == 1] = mp.mpf(0)
                R.add("matrix spd%d" % spd, _err(A, want), bA)
                R.add("gradient", _err(g, wg), bg)
                assert not A[fz == 1][:, fz == 0].any() and not g[fz == 1].any()
            got = C.param_grads(["elastic0.mu", "elastic0.lam"], p)
            for key, q in (("elastic0.mu", "dmu"), ("elastic0.lam", "dlam")):
                want, e64 = mp.mpf(0), mp.mpf(0)
                for t, r in enumerate(rs):
                    d = _dofs(tets[t])
                    pe = np.array([mp.mpf(v) for v in p[d] * (fz[d] == 0)], dtype=object)
                    want -= sum(pe * r[q])
                    e64 += tn.fro(pe) * r[q + "_e64"]
                R.add("key " + q[1:], abs(float(mp.mpf(got[key]) - want)), tn.bound(e64, abs(want)))
            E = sum(r["energy"] for r in rs)
            R.add("energy", abs(float(mp.mpf(C.energy()) - E)), float(8 * max(sum(r["energy_e64"] for r in rs), 4 * U * abs(E))))
        C.close()
        R.check("ring, kind %d, %d frozen vertices" % (kind, len(frozen_verts)))
