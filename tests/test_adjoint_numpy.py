"""tests/adjoint_numpy.py, the reference of tests/test_gpu_adjoint_elements.py, pinned without the kernels: the x2a term and the a2ax direction against mp
differences of cloth_numpy, decisions_safe (the a2ax threshold included) and positive-definiteness at the chosen m / dt^2 for every state the GPU tests
use, the frozen patterns, the harness with float64 in the kernels' place (every ratio at most 1 / 8), seven wrong kernels that it must reject, each in
the quantity it corrupts and nowhere else, and the oracle's reverse step on a 3 x 2 rollout."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_numpy as an  # noqa: E402
import cloth_numpy as cn  # noqa: E402
import tet_numpy as tn  # noqa: E402
from cloth_numpy import MP  # noqa: E402


class Ratios(dict):
    label = "reverse step (float64 in the kernels' place)"

    def add(self, q, err, bnd):
        self[q] = max(self.get(q, 0.0), err / bnd)

    def show(self, what):
        print("%s, %s: largest |f64 - mp| / bound: %s" % (self.label, what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))


def _mpx(x):
    return np.array([mp.mpf(float(v)) for v in np.asarray(x).ravel()], dtype=object).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------------ the two hinge terms against mp differences
@pytest.mark.parametrize("key", ["3x2/dx150/bump", "3x2/dx1e-4/fold-170_refopp", "1x1/dx150/fold+90_refsame"])
@tn.with_mp
def test_x2a_term_is_minus_p_dot_the_derivative_of_the_bending_gradient_by_the_reference_angle(key):
    """-(p . d(theta)/dx) d_ref of a hinge = -p . d(bending gradient)/d(ref_angle of its slot), the gradient that of cloth_numpy.totals: it is linear in
    the reference angle, so a difference over 1e-3 rad at 50 digits is exact to 1e-45"""
    st = cn.STATES[key]()
    c, x, ra = st.cloths[0], _mpx(st.local(0)), st.ra[0]
    ev = cn.evaluate(MP, c, x, ra)
    p = np.random.default_rng(3).normal(size=(c.NV, 3))
    pm = _mpx(p)
    h_ = mp.mpf("1e-3")
    for h, (f, l) in enumerate(c.hinges):
        up, dn = np.array(ra, dtype=object) + mp.mpf(0), np.array(ra, dtype=object) + mp.mpf(0)
        up[f, l] += h_; dn[f, l] -= h_
        dG = (cn.totals(MP, c, x, up, "gradient")[2] - cn.totals(MP, c, x, dn, "gradient")[2]) / (2 * h_)
        want = -sum((pm * dG).ravel())
        got = an.x2a_term(MP, ev["g"][h], pm[c.hinge_verts(f, l)[0]], an.d_ref(MP, c))
        assert abs(got - want) <= mp.mpf("1e-40") * (abs(want) + tn.fro(dG)), (key, h)
        assert abs(want) > 0


@pytest.mark.parametrize("key", ["3x2/dx150/bump", "3x2/dx1e-4/bump", "1x1/dx150/fold-170_refopp"])
@tn.with_mp
def test_a2ax_direction_is_the_derivative_of_the_dihedral_angle(key):
    """the vector a2ax adds to the four vertices of a hinge is sgn d(theta)/dx, theta that of cloth_numpy.compute_angle: central differences with
    h = 1e-20 on coordinates of 1e-4 .. 1e-2 m, asserted at 1e-24 of the gradient"""
    st = cn.STATES[key]()
    c, x = st.cloths[0], _mpx(st.local(0))
    ev = cn.evaluate(MP, c, x, st.ra[0])
    hstep = mp.mpf("1e-20")
    for h, (f, l) in enumerate(c.hinges):
        hv, i2 = c.hinge_verts(f, l)[0], c.cf[f, l]

        def theta(y):
            X = [list(r) for r in y]
            return cn.compute_angle(MP, c, X, cn.normals(MP, c, X), f, i2, l)
        g = np.full((c.NV, 3), mp.mpf(0), dtype=object)
        for v in set(hv):
            for j in range(3):
                up, dn = x.copy(), x.copy()
                up[v, j] += hstep; dn[v, j] -= hstep
                g[v, j] = (theta(up) - theta(dn)) / (2 * hstep)
        want = np.full((c.NV, 3), mp.mpf(0), dtype=object)
        for a in range(4):
            want[hv[a]] += ev["g"][h, a]
        assert tn.fro(g - want) <= mp.mpf("1e-24") * tn.fro(want), (key, h)
        sgn = an.a2ax_sign(MP, ev["theta"][h], 0.0, c.k_angle, 2.0)
        assert sgn == (2 if abs(ev["theta"][h]) > c.k_angle else 2 * mp.mpf(0.1))


# ------------------------------------------------------------------------------------------------ the states of the GPU tests
_MIN_EIG = {}


@pytest.mark.parametrize("key", an.GPU_STATES)
def test_every_gpu_state_is_safe_and_positive_definite(key):
    """decisions_safe (every decision of cloth_numpy and the a2ax threshold, in mp and in every float64 evaluation) and the un-projected, un-masked
    operator positive definite with m / dt^2 = MDT2 on its diagonal"""
    ref = an.reference(key)
    assert an.decisions_safe(ref)
    op = an.cloth_operator(ref)
    lo = an.min_eigenvalue(op, 0.0)
    _MIN_EIG[key] = lo
    assert lo + an.MDT2 > 0 and an.min_eigenvalue(op, an.MDT2) > 0, (key, lo)


def test_mdt2_is_the_smallest_power_of_two_that_makes_every_operator_positive_definite():
    """MDT2 is a power of two, half of it leaves some operator of the GPU states indefinite, and the two ring bodies are positive definite with it"""
    assert np.log2(an.MDT2) == int(np.log2(an.MDT2)) and an.MASS == an.MDT2 * an.DT ** 2 and np.log2(an.MASS) == int(np.log2(an.MASS))
    for key in an.GPU_STATES:
        if key not in _MIN_EIG:
            _MIN_EIG[key] = an.min_eigenvalue(an.cloth_operator(an.reference(key)), 0.0)
    worst = min(_MIN_EIG, key=_MIN_EIG.get)
    print("most negative eigenvalue of an un-projected operator without the mass term: %.3e (%s)" % (_MIN_EIG[worst], worst))
    assert _MIN_EIG[worst] + an.MDT2 > 0 and _MIN_EIG[worst] + an.MDT2 / 2 < 0, (worst, _MIN_EIG[worst])
    for kind in (0, 1):
        assert an.min_eigenvalue(an.tet_operator(kind), an.MDT2) > 0, kind


@pytest.mark.parametrize("key", an.TRANSPOSE_STATES)
def test_stretched_and_compressed_states_separate_the_operator_from_its_transpose(key):
    """with the area term away from rest some block that couples a frozen dof to a free one differs from its transpose by more than 1e-3 of itself
    (frozen pattern A, "small" on 1 x 1): the only states where tmp_z_frozen read from block (c, p) instead of (p, c) shows"""
    op = an.cloth_operator(an.reference(key))
    nv = op.nv
    fz = an.frozen_pattern(nv, "A" if nv > 4 else "small").reshape(nv, 3).astype(bool)
    A = op.hl[0].reshape(nv, 3, nv, 3)
    worst = 0.0
    for v in np.nonzero(fz.any(axis=1))[0]:
        for u in np.nonzero(op.pattern[:, v])[0]:
            if not fz[u].all():
                blk, blkT = A[u][:, v][~fz[u]][:, fz[v]], A[v][:, u].T[~fz[u]][:, fz[v]]
                n = np.linalg.norm(blk)
                if n > 0:
                    worst = max(worst, np.linalg.norm(blk - blkT) / n)
    assert worst > 1e-3, (key, worst)


def test_frozen_patterns_cover_every_mask_and_both_kinds_of_neighbours():
    for key in ("3x2/dx150/compress", "8x8/dx150/compress_rot", "10x10/dx150/fold+90_ref0", "8x8+3x2/dx150/compress_rot"):
        op = an.cloth_operator(an.reference(key))
        pr = an.pattern_properties(an.frozen_pattern(op.nv, "A"), op.pattern)
        assert pr["values"] == set(range(1, 8)) and pr["both_partial"] and pr["whole_next_to_partial"], (key, pr)
        a, b = an.masks(an.frozen_pattern(op.nv, "A")), an.masks(an.frozen_pattern(op.nv, "B"))
        assert ((a > 0) | (b > 0)).all() and (a == 0).sum() < 64 and (b == 0).sum() < 64
    pr = an.pattern_properties(an.frozen_pattern(4, "small"), np.ones((4, 4), bool))
    assert pr["values"] == {3, 5, 7} and pr["both_partial"] and pr["whole_next_to_partial"]
    for kind in (0, 1):
        op = an.tet_operator(kind)
        pr = an.pattern_properties(an.frozen_pattern(op.nv, "A"), op.pattern)
        assert pr["values"] == set(range(1, 8)) and pr["both_partial"] and pr["whole_next_to_partial"]
    assert not an.frozen_pattern(9, "none").any()


# ------------------------------------------------------------------------------------------------ the harness
def _case(key, s=2, d=0.5, adj_clamp=1000.0, sw=1, pattern="A"):
    ref = an.reference(key)
    op = an.cloth_operator(ref)
    nv = op.nv
    fz = an.frozen_pattern(nv, pattern if nv > 4 else "small")
    inp = an.seeds(ref.st, nv, s, fz, adj_clamp, sw, d, seed=1)
    pg = an.f64_step(ref, op, inp, np.zeros((nv, 3)), k=0)["pg_s"]
    p = an.frozen_p(np.random.default_rng(5).normal(size=(nv, 3)) * 1e-3, pg, inp)
    return ref, op, inp, p, fz


EIGHTH = 0.125 * (1 + 1e-4)
HARNESS = [("3x2/dx150/compress_rot", 2, 0.5, 1000.0, 1), ("3x2/dx1e-4/stretch", 4, 1.0, 1.0, 0), ("plastic/+2", 1, 0.25, 1000.0, 1),
           ("plastic/-0.99", 2, 0.3, 1.0, 1), ("1x1/dx150/compress", 2, 0.0, 1000.0, 1), ("8x8/dx150/compress_rot", 3, 0.5, 1000.0, 1)]


@pytest.mark.parametrize("key,s,d,lim,sw", HARNESS)
def test_harness_passes_the_float64_restatement_at_an_eighth(key, s, d, lim, sw):
    """an F64 implementation of the whole step (three other evaluations of the Reference: other rounding) fed the same inputs and an exact p meets every
    bound at 1 / 8.  The stand-in's evaluations are among those e64 is taken over, so a vertex with one dominant term can sit at 1 / 8 exactly; its sums
    are extended, not exact (2^-11 u per addition, measured 1.2e-6 of a bound), hence EIGHTH = 1 / 8 (1 + 1e-4)"""
    ref, op, inp, p, fz = _case(key, s, d, lim, sw)
    exp = an.expected_reverse(ref, op, inp, p)
    R = Ratios()
    for k in (1, 4, 9):
        an.compare(exp, an.f64_step(ref, op, inp, p, k), R, frozen=fz)
    R.show(key)
    assert R and all(v <= EIGHTH for v in R.values()), R
    if key.startswith("plastic/+2"):
        assert len(set(exp["far"].values())) == 2, "both branches of a2ax"


WRONG = {   # variant -> the quantity it must corrupt
    "no_transpose": "tmp_z_frozen", "no_tenth": "pos_grad[s]", "compare": "pos_grad[s]", "a2ax_first": "pos_grad[s]", "d_for_1pd": "pos_grad[s-1]",
    "rm_skip": "tmp_z_frozen", "p_zero_frozen": "angleref_grad[s-1]"}


@pytest.mark.parametrize("key", ["3x2/dx150/compress_rot", "plastic/+2"])
@pytest.mark.parametrize("variant", an.VARIANTS)
def test_harness_rejects_wrong_kernels_each_where_it_must(variant, key):
    """the wrong kernels as variants of the float64 stand-in: tmp_z_frozen from block (c, p) instead of its transpose (no_transpose: 4e8 bounds on the
    turned compressed sheet, whose area term is far from rest; 5e3 on the plastic state's folds, where the area is at rest and only the second-order
    bending part is unsymmetric), the factor 0.1 dropped (no_tenth), the comparison taken the other way round (compare: at plastic/+2 every hinge sits 1e-2 .. 1 of k_angle
    inside its branch; `>=` for `>` differs on the threshold alone, where no state that passes decisions_safe can sit), a2ax before the clamp
    (a2ax_first), d where 1 + d belongs (d_for_1pd), a partly frozen neighbour skipped like a whole one (rm_skip: `rm == 7` read as `rm != 0`), p
    zeroed on the frozen dofs before x2a (p_zero_frozen).  Each gives a ratio above 1 in the quantity it corrupts and leaves every other at 1 / 8"""
    ref, op, inp, p, fz = _case(key)
    exp = an.expected_reverse(ref, op, inp, p)
    R = Ratios()
    try:
        an.compare(exp, an.f64_step(ref, op, inp, p, 1, variant), R, frozen=fz)
    except AssertionError as e:   # (a2ax_first also breaks the bit-equal vertices)
        assert variant == "a2ax_first" and "clip" in str(e), (variant, e)
        R["pos_grad[s]"] = np.inf
    R.show("%s, %s" % (key, variant))
    bad = WRONG[variant]
    assert R[bad] > 1.0, (variant, R)
    assert all(v <= EIGHTH for q, v in R.items() if q != bad), (variant, R)


# ------------------------------------------------------------------------------------------------ against the oracle
def test_oracle_reverse_step_agrees_with_the_restatement(oracle):
    """a 3 x 2 cloth with two frozen dofs, two steps under gravity (T = 3), one grad_transfer at s = 2 with seeds on every row: the oracle's pos_grad rows,
    angleref_grad rows and tmp_z_frozen against the restatement fed the oracle's own p (tmp_z_not_frozen), at 8 times the bound; and the oracle's p on
    the frozen dofs is pos_grad[s] / (m / dt^2), the rule of adjoint_numpy"""
    N, M, dx, T = 3, 2, 0.1 / 15, 3
    c = cn.ClothTables(N, M, dx)
    o = oracle.OracleScene(dt=cn.DT, plastic=0)
    ci = o.add_cloth(N, M, dx * N)
    o.cloth_init(ci, 0, 0, 0)
    o.finalize()
    rng = np.random.default_rng(2)
    fz = np.zeros(3 * c.NV, np.int32); fz[[2, 3 * 7 + 1]] = 1
    o.frozen[:] = fz
    o.pos[:] = o.pos + rng.normal(0, 2e-4, (c.NV, 3)); o.prev_pos[:] = o.pos; o.vel[:] = 0
    ra = rng.uniform(-0.3, 0.3, (c.NF, 3))
    o.arr("cloth0.ref_angle", (-1, 3))[:] = ra
    o.push_down_all()
    o.set_solver(1e-13)
    o.grad_new(T, 0)
    o.grad_copy_pos(0)
    for f in range(1, T):
        o.time_step(); o.grad_copy_pos(f)
    pb, rb = o.arr("grad.pos_buffer", (T, c.NV, 3)), o.arr("grad.ref_angle_buffer", (T, c.NF, 3))
    st = cn.make_state("oracle rollout", [(c, (pb[2].copy(), np.full(c.NF, -1), None), rb[1].copy(), None, (0.0, 0.0, 0.0))])
    ref = cn.Reference(st)
    assert an.decisions_safe(ref)
    op = an.cloth_operator(ref)
    mdt2 = (o.arr("mass") / o.dt ** 2).reshape(-1, 1)
    inp = an.seeds(st, c.NV, 2, fz, seed=4, mdt2=mdt2, p_row="none", quiet_corner=False)
    pg, ag = o.arr("grad.pos_grad", (T, c.NV, 3)), o.arr("grad.angleref_grad", (T, -1))
    pg[2], pg[1], pg[0] = inp.pg_s, inp.pg_prev, inp.pg_prev2
    ag[2], ag[1] = inp.ag_s, inp.ag_prev
    ag0 = ag[0].copy()
    o.grad_transfer(2)
    p = o.arr("tmp_z_not_frozen").reshape(-1, 3).copy()
    fzb = fz.reshape(-1, 3).astype(bool)
    want = (pg[2] / mdt2)[fzb]
    assert np.abs(p[fzb] - want).max() <= 1e-12 * np.abs(want).max(), "p on the frozen dofs: pos_grad[s] / (m / dt^2)"
    exp = an.expected_reverse(ref, op, inp, p)
    R = Ratios(); R.label = "reverse step (the oracle in the kernels' place)"
    an.compare(exp, dict(pg_s=pg[2], ag_s=ag[2], ag_prev=ag[1], tz=o.arr("tmp_z_frozen"), pg_prev=pg[1], pg_prev2=pg[0]), R, frozen=fz)
    R.show("3 x 2, T = 3")
    assert np.array_equal(ag[0], ag0)
    assert set(R) == {"pos_grad[s]", "angleref_grad[s-1]", "tmp_z_frozen", "pos_grad[s-1]", "pos_grad[s-2]"} and all(v <= 8.0 for v in R.values()), R
