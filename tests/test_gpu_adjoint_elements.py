"""The reverse step's own kernels alone (csrc/k_adjoint.hpp: k_clamp, k_adj_a2ax with the hinge range of k_vertex_gather, k_adj_x2a, k_zfrozen_gather +
k_scatter_perm, k_adj_prev; adjoint_pre / adjoint_post / adj_step of csrc/adjoint_api.hpp) against the mpmath restatement tests/adjoint_numpy.py.  Every
test is one adjoint_step (or a few) on a small context of cloths and / or one elastic body without pairs, handles, ties or colliders, dt = 2^-8 and
m / dt^2 = 2^29 (adjoint_numpy says why), on a tape of T = 5 rows whose every entry is seeded with noise; pos_grad lies inside a larger allocation
with guard rows before and after it.

How p is known without trusting the solver: the row that the inertia term is read from starts at zero (row s - 2 where it exists and d != 0, else row
s - 1), d is a power of two, so the row holds -d p m / dt^2 (or (1 + d) p m / dt^2) exactly and p on the free dofs is read back bit for bit; on the
frozen dofs p = pos_grad[s] (read back) / (m / dt^2), the rule adjoint_numpy states.  Every quantity is then checked as a function of that p: of the
solve only the flag and that p is finite are asserted.  The contexts use the sparse direct solve, which leaves the decoupled frozen rows exact.

Bound (tet_numpy.bound): 8 max(e64, 4 u |mp|) per hinge term and per vertex-pair block of the operator times |p|, sums take the sum of the bounds, exact
terms e64 = 0 (adjoint_numpy).  Every state passes adjoint_numpy.decisions_safe on the CPU (tests/test_adjoint_numpy.py); nothing is skipped or masked.
Bit-equal parts: angleref_grad[s] (clipped at 1000, or untouched with adj_clamp_angleref = 0 or without a cloth face), every slot of angleref_grad[s - 1]
that is no hinge, tmp_z_frozen on free dofs (exact zeros), pos_grad[s - 1] and [s - 2] on frozen dofs, pos_grad[s] == clip(seed) on the vertices all of
whose hinges carry a == 0 (vertex 0, the last vertex of the first cloth and the last vertex: `sgn * g` is +-0 whatever Kb and the geometry are; a 1 x 1
mesh has one hinge and no such vertex), every other row of the tape, pos_buffer, ref_buffer and the guard rows.  Every test prints its largest
|gpu - mp| / bound per quantity."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_numpy as an  # noqa: E402
import cloth_numpy as cn  # noqa: E402
import tet_numpy as tn  # noqa: E402
from test_gpu_tet_elements import Ratios, _dev  # noqa: E402

pytestmark = pytest.mark.gpu
T = 5
GUARD = 2


class AdjointRatios(Ratios):
    label = "reverse step"


def _context(cloths, nv, fz, bodies=()):
    ctx = an.reverse_context(cloths, nv, fz, bodies=bodies)
    ctx.set_param("direct", 1)
    return ctx


def _step(ctx, x, ra, inp, keep=False):
    """one adjoint_step at inp.s on a fresh noise-seeded tape; returns what adjoint_numpy.compare takes plus p (free dofs read back, frozen dofs by the
    rule) and the solve's statistics.  Asserts everything that must keep its bits"""
    nv, ns, s = len(x), len(inp.ag_s), inp.s
    rng = np.random.default_rng(77 + s)
    scale = np.abs(x).max()
    pos = rng.normal(size=(T, nv, 3)) * scale
    pos[s], pos[s - 1] = x, x + 1e-3 * scale * rng.normal(size=(nv, 3))
    refb = rng.normal(size=(T, ns))
    refb[s - 1] = ra
    big = rng.normal(size=(T + 2 * GUARD, 3 * nv))
    ag = rng.normal(size=(T, ns))
    big[GUARD + s], big[GUARD + s - 1] = inp.pg_s.ravel(), inp.pg_prev.ravel()
    if s > 1:
        big[GUARD + s - 2] = inp.pg_prev2.ravel()
    ag[s], ag[s - 1] = inp.ag_s, inp.ag_prev
    d_pos, d_ref, d_big, d_ag = _dev(pos.reshape(T, -1)), _dev(refb), _dev(big), _dev(ag)
    d_pg = d_big[GUARD:GUARD + T]
    assert d_pg.is_contiguous() and d_pg.data_ptr() == d_big.data_ptr() + GUARD * 3 * nv * 8
    tz = _dev(rng.normal(size=3 * nv))
    ctx.set_param("adj_clamp", inp.adj_clamp); ctx.set_param("adj_clamp_angleref", float(inp.clamp_angleref))
    stats = ctx.adjoint_step(s, T, d_pos, d_pg, d_ref, d_ag, tz, damping=inp.d)
    torch.cuda.synchronize()
    assert stats["flag"] in (0, 1), stats
    assert np.array_equal(d_pos.cpu().numpy(), pos.reshape(T, -1)) and np.array_equal(d_ref.cpu().numpy(), refb), "pos_buffer and ref_buffer are never written"
    gb, ga = d_big.cpu().numpy(), d_ag.cpu().numpy()
    rows = [r for r in range(T + 2 * GUARD) if r - GUARD not in (s, s - 1, s - 2)]
    assert np.array_equal(gb[rows], big[rows]), "guard rows and every other row of pos_grad keep their bits (nothing before the tape at s = 1)"
    arows = [r for r in range(T) if r not in (s, s - 1)]
    assert np.array_equal(ga[arows], ag[arows]), "every other row of angleref_grad keeps its bits"
    got = dict(pg_s=gb[GUARD + s].reshape(nv, 3), ag_s=ga[s], ag_prev=ga[s - 1], tz=tz.cpu().numpy().reshape(nv, 3), pg_prev=gb[GUARD + s - 1].reshape(nv, 3),
               pg_prev2=gb[GUARD + s - 2].reshape(nv, 3) if s > 1 else None)
    fz = inp.frozen
    assert np.array_equal(got["pg_prev"][fz], inp.pg_prev[fz]) and (s == 1 or np.array_equal(got["pg_prev2"][fz], inp.pg_prev2[fz])), "inertia on free dofs only"
    if s > 1 and not inp.pg_prev2.any() and inp.d != 0:
        p = -got["pg_prev2"] / (inp.d * inp.mdt2)
        assert np.array_equal(-p * inp.mdt2 * inp.d, got["pg_prev2"])
    else:
        assert not inp.pg_prev.any() and np.log2(1 + inp.d) == int(np.log2(1 + inp.d))
        p = got["pg_prev"] / ((1 + inp.d) * inp.mdt2)
        assert np.array_equal(p * inp.mdt2 * (1 + inp.d), got["pg_prev"])
        if s > 1 and inp.d == 0:
            assert np.array_equal(got["pg_prev2"], inp.pg_prev2), "d = 0: row s - 2 keeps its bits"
    assert np.isfinite(p).all() and np.isfinite(got["pg_s"]).all(), stats
    got["p"] = an.frozen_p(p, got["pg_s"], inp)
    got["stats"] = stats
    if keep:
        got["tape"] = (d_pos, d_ref)
    return got


# (s, d, adj_clamp, adj_clamp_angleref): the steps 1, 2 and 4 of a tape of five rows, the dampings whose products are exact, both clamps of pos_grad (1000
# and the 1.0 of the system-identification class), the angleref clip on and off; a state takes the combination of its place in the list
COMBOS = [(1, 1.0, 1000.0, 1), (2, 0.5, 1.0, 0), (4, 0.25, 1000.0, 1), (2, 0.0, 1000.0, 0), (4, 1.0, 1.0, 1), (1, 0.0, 1.0, 0)]


def _run_state(key, combo, patterns, R):
    ref = an.reference(key)
    st, op = ref.st, an.cloth_operator(ref)
    far = None
    for pat in patterns:
        fz = an.frozen_pattern(st.nv, pat)
        s, d, lim, sw = combo
        inp = an.seeds(st, st.nv, s, fz, lim, sw, d, seed=len(key))
        ctx = _context(st.cloths, st.nv, fz)
        got = _step(ctx, st.x, an.ref_row(st), inp)
        ctx.close()
        exp = an.expected_reverse(ref, op, inp, got["p"])
        an.compare(exp, got, R, frozen=fz)
        if pat == "none":
            assert not got["tz"].any(), "nothing frozen: tmp_z_frozen is all exact zeros"
        far = exp["far"]
    return far


@pytest.mark.parametrize("key", an.SMALL_STATES)
def test_small_meshes_match_mpmath(key):
    """1 x 1 (one hinge, fewer than three faces) and 3 x 2 (both cell parities), cells of 1 / 150 m and 1e-4 m: ripples just below and just above the
    series / acos switch, folds of +-90, +-170 degrees and +-(pi - 1e-3) with reference angles 0, the fold's own and its opposite (those of pi with 0
    and the opposite take the `> k_angle` branch of a2ax at k_angle = 3.14), stretch x 1.5, compression x 0.5 flat and turned (the turned ones are where
    the operator differs from its transpose).  Per-dof frozen pattern A (masks 7, 5, 3, 0 on the four vertices of 1 x 1), every third state also with
    nothing frozen; step, damping and clamps by the state's place in the list"""
    i = an.SMALL_STATES.index(key)
    R = AdjointRatios()
    _run_state(key, COMBOS[i % len(COMBOS)], ["small" if key.startswith("1x1") else "A"] + (["none"] if i % 3 == 0 else []), R)
    R.check(key)


@pytest.mark.parametrize("key", an.LARGE_STATES)
def test_launch_edges_slices_and_a_second_cloth_match_mpmath(key):
    """8 x 8 (81 vertices: two SELL-64 slices, the second partly filled; 128 faces), 10 x 10 (280 hinges: the 256-lane edge of k_adj_a2ax and k_adj_x2a,
    121 vertices), 8 x 8 with a 3 x 2 second cloth of its own dx, Kb, k_angle, v_offset and face_start (the offsets into the rows of angleref_grad and
    A.cid).  Frozen patterns A and B: every vertex has a frozen dof in one of the two, so every slice, the partly filled one too, holds frozen rows"""
    i = an.LARGE_STATES.index(key)
    R = AdjointRatios()
    _run_state(key, COMBOS[(i + 1) % len(COMBOS)], ["A", "B"] + (["none"] if i == 0 else []), R)
    R.check(key)


@pytest.mark.parametrize("key", cn.PLASTIC_KEYS)
def test_a2ax_at_its_threshold(key):
    """hinges at 0.5, 0.99, 1.01 and 2 times k_angle (0.5 rad, and 0.4 rad on the second cloth), both signs, beside flat hinges: above the threshold both
    branches of a2ax occur in one launch"""
    R = AdjointRatios()
    far = _run_state(key, COMBOS[cn.PLASTIC_KEYS.index(key) % len(COMBOS)], ["A"], R)
    assert (len(set(far.values())) == 2) == (abs(float(key.split("/")[1])) > 1), far
    R.check(key)


# ------------------------------------------------------------------------------------------------ steps, clamps, damping
@pytest.mark.parametrize("s", [1, 2, 4])
def test_rows_of_the_tape(s):
    """the row arithmetic of adj_step on T = 5: steps 1, 2 and 4 on fresh buffers write rows s, s - 1, s - 2 of pos_grad (nothing before the tape at
    s = 1: the guard rows keep their bits), rows s and s - 1 of angleref_grad, and nothing else (asserted in _step for every test; here at d = 1 and
    d = 0 for each step)"""
    key = "3x2/dx150/fold+90_refopp"
    R = AdjointRatios()
    for d in (1.0, 0.0):
        _run_state(key, (s, d, 1000.0, 1), ["A"], R)
    R.check("%s, s = %d" % (key, s))


@pytest.mark.parametrize("lim,sw", [(1000.0, 1), (1000.0, 0), (1.0, 1), (1.0, 0)])
def test_clamps(lim, sw):
    """adj_clamp 1000 and 1.0 with seeds inside, exactly at, one ulp inside / outside and beyond +-lim: pos_grad[s] - a2ax sum = clip(seed) within the a2ax
    bound, bit-equal on the vertices whose hinges carry a == 0 (module docstring); adj_clamp_angleref 1: angleref_grad[s] comes back clipped at 1000
    bit for bit (seeds at 1000, 2500 and -4000), 0: untouched"""
    key = "3x2/dx150/ripple1.5e-3"
    ref = an.reference(key)
    st = ref.st
    fz = an.frozen_pattern(st.nv, "A")
    inp = an.seeds(st, st.nv, 2, fz, lim, sw, 1.0, seed=3)
    assert (np.abs(inp.pg_s) > lim).any() and (np.abs(inp.pg_s) == lim).any() and (np.abs(inp.ag_s) > 1000).any() and (np.abs(inp.ag_s) == 1000).any()
    ctx = _context(st.cloths, st.nv, fz)
    got = _step(ctx, st.x, an.ref_row(st), inp)
    ctx.close()
    exp = an.expected_reverse(ref, an.cloth_operator(ref), inp, got["p"])
    assert exp["quiet"].sum() >= 2 and np.array_equal(got["pg_s"][exp["quiet"]], np.clip(inp.pg_s, -lim, lim)[exp["quiet"]])
    assert np.array_equal(got["ag_s"], np.clip(inp.ag_s, -1000, 1000) if sw else inp.ag_s)
    R = AdjointRatios()
    an.compare(exp, got, R, frozen=fz)
    R.check("%s, adj_clamp %g, adj_clamp_angleref %d" % (key, lim, sw))


def test_damping():
    """d = 1, 0.5, 0.25 (exact: p from row s - 2), d = 0 (row s - 2 keeps its bits, p from row s - 1) and the non-dyadic d = 0.3 with p from a twin run
    at d = 1 whose pos_grad[s] and tmp_z_frozen are bit-equal: its rows against mp at 4 u (|seed| + |term|): 1 + d, its product with p m / dt^2 and the
    sum with the seed are three roundings of at most u each"""
    key = "3x2/dx150/fold-90_refopp"
    ref = an.reference(key)
    st, op = ref.st, an.cloth_operator(ref)
    fz = an.frozen_pattern(st.nv, "A")
    R = AdjointRatios()
    for d in (1.0, 0.5, 0.25, 0.0):
        _run_state(key, (4, d, 1000.0, 1), ["A"], R)
    inp1 = an.seeds(st, st.nv, 4, fz, d=1.0, seed=8)
    inp3 = an.seeds(st, st.nv, 4, fz, d=0.3, seed=8, p_row="none")
    for q in ("pg_s", "ag_s", "ag_prev"):
        assert np.array_equal(getattr(inp1, q), getattr(inp3, q))
    ctx = _context(st.cloths, st.nv, fz)
    twin = _step(ctx, st.x, an.ref_row(st), inp1)
    ctx.close()
    # (the twin's p; _step reads a p of its own from rows that hold seeds here, so the run at 0.3 is made by hand)
    ctx = _context(st.cloths, st.nv, fz)
    got = _step_with_seeds(ctx, st, inp3)
    ctx.close()
    assert np.array_equal(got["pg_s"], twin["pg_s"]) and np.array_equal(got["tz"], twin["tz"]), "the twin runs agree bit for bit before the inertia term"
    exp = an.expected_reverse(ref, op, inp3, twin["p"])
    free = ~inp3.frozen
    xh = np.abs(twin["p"] * an.MDT2)
    for q, seed, fac in (("pg_prev", inp3.pg_prev, 1.3), ("pg_prev2", inp3.pg_prev2, 0.3)):
        name = {"pg_prev": "pos_grad[s-1] at d = 0.3 (4 u)", "pg_prev2": "pos_grad[s-2] at d = 0.3 (4 u)"}[q]
        err = np.abs(cn.diff(got[q], exp[q][0]))
        bnd = 4 * an.U * (np.abs(seed) + fac * xh)
        R.add(name, float((err[free] / bnd[free]).max()), 1.0)
        assert np.array_equal(got[q][~free], seed[~free])
    R.check(key)


def _step_with_seeds(ctx, st, inp):
    """adjoint_step with noise in every row (no row to read p from): the raw outputs"""
    nv, ns, s = st.nv, len(inp.ag_s), inp.s
    rng = np.random.default_rng(77 + s)   # (the tape of _step: same x_{s-1})
    scale = np.abs(st.x).max()
    pos = rng.normal(size=(T, nv, 3)) * scale
    pos[s], pos[s - 1] = st.x, st.x + 1e-3 * scale * rng.normal(size=(nv, 3))
    refb = np.zeros((T, ns)); refb[s - 1] = an.ref_row(st)
    pg, ag = np.zeros((T, 3 * nv)), np.zeros((T, ns))
    pg[s], pg[s - 1], pg[s - 2] = inp.pg_s.ravel(), inp.pg_prev.ravel(), inp.pg_prev2.ravel()
    ag[s], ag[s - 1] = inp.ag_s, inp.ag_prev
    d_pos, d_ref, d_pg, d_ag, tz = _dev(pos.reshape(T, -1)), _dev(refb), _dev(pg), _dev(ag), _dev(np.zeros(3 * nv))
    stats = ctx.adjoint_step(s, T, d_pos, d_pg, d_ref, d_ag, tz, damping=inp.d)
    torch.cuda.synchronize()
    assert stats["flag"] in (0, 1), stats
    g = d_pg.cpu().numpy()
    return dict(pg_s=g[s].reshape(nv, 3), pg_prev=g[s - 1].reshape(nv, 3), pg_prev2=g[s - 2].reshape(nv, 3), tz=tz.cpu().numpy().reshape(nv, 3))


# ------------------------------------------------------------------------------------------------ tetrahedra, and cloth and tetrahedra in one matrix
def _ring_body(kind, off=0):
    x, tets, B, W, _, _ = an.ring(kind)
    return x, (tn.MATERIALS[kind], tets + off, B, W, off, len(x))


@pytest.mark.parametrize("kind", [0, 1])
def test_ring_of_tetrahedra_matches_mpmath(kind):
    """one tet_numpy.ring_mesh body per material kind, no cloth, crushed (kind 0: to 1e-3 along one axis; kind 1: to J just below its clamp; both
    operators are symmetric, so the transposition shows in the mixed context's cloth part, not here), frozen patterns A and B and nothing frozen: tmp_z_frozen against minus the transposed free / frozen blocks of the
    summed mp element blocks times p; n_cface = 0, so the rows of angleref_grad are 3 doubles wide and keep their bits"""
    x, body = _ring_body(kind)
    nv = len(x)
    op = an.tet_operator(kind)
    R = AdjointRatios()
    for j, pat in enumerate(("A", "B", "none")):
        fz = an.frozen_pattern(nv, pat)
        inp = an.seeds(None, nv, (2, 4, 1)[j], fz, d=(0.5, 0.25, 1.0)[j], seed=kind)
        ctx = _context([], nv, fz, bodies=[body])
        got = _step(ctx, x, np.zeros(3), inp)
        ctx.close()
        assert np.array_equal(got["ag_s"], inp.ag_s) and np.array_equal(got["ag_prev"], inp.ag_prev)
        assert np.array_equal(got["pg_s"], np.clip(inp.pg_s, -1000, 1000)), "no hinge: pos_grad[s] is the clipped seed"
        an.compare(an.expected_reverse(None, op, inp, got["p"]), got, R, frozen=fz)
    R.check("ring, kind %d" % kind)


@pytest.mark.parametrize("kind", [0, 1])
def test_cloth_and_body_in_one_matrix(kind):
    """the turned compressed 8 x 8 cloth and a ring body without contact pairs: tmp_z_frozen sums the cloth blocks and the tet blocks of one SELL
    matrix, permuted by an order that mixes the two; frozen patterns A and B over all 107 vertices"""
    ref = an.reference("8x8/dx150/compress_rot")
    st = ref.st
    xr, body = _ring_body(kind, st.nv)
    nv = st.nv + len(xr)
    x = np.concatenate([st.x, xr])
    op = an.join(an.pad(an.cloth_operator(ref), nv), an.tet_operator(kind, nv, st.nv))
    R = AdjointRatios()
    for pat in ("A", "B"):
        fz = an.frozen_pattern(nv, pat)
        inp = an.seeds(st, nv, 2, fz, d=0.5, seed=5 + kind)
        ctx = _context(st.cloths, nv, fz, bodies=[body])
        got = _step(ctx, x, an.ref_row(st), inp)
        ctx.close()
        exp = an.expected_reverse(ref, op, inp, got["p"])
        an.compare(exp, got, R, frozen=fz)
        assert got["tz"][:st.nv].any() and got["tz"][st.nv:].any()
    R.check("8 x 8 cloth and ring of kind %d" % kind)


# ------------------------------------------------------------------------------------------------ the frozen rule, the repeat
def test_p_on_frozen_dofs_reaches_x2a_and_param_grads_reads_the_same_p():
    """after an adjoint_step, param_grads(x_s, ref, keys, p = None) reads the step's own p: bit-equal to param_grads(..., p = the restated p).  k_pg_hinge,
    k_pg_face and k_pg_tet sum over free dofs only (pg_dot_free), so this holds p on the free dofs and says nothing about the frozen ones; those are
    held by x2a alone: angleref_grad[s - 1] on the hinges with a frozen vertex matches the restatement with p = pos_grad[s] / (m / dt^2) there (compare)
    and is further than 1e6 bounds from the restatement with p = 0 there, so the match is not vacuous"""
    key = "3x2/dx150/fold+170_ref0"
    ref = an.reference(key)
    st, op = ref.st, an.cloth_operator(ref)
    fz = an.frozen_pattern(st.nv, "A")
    inp = an.seeds(st, st.nv, 2, fz, d=0.5, seed=6)
    ctx = _context(st.cloths, st.nv, fz)
    got = _step(ctx, st.x, an.ref_row(st), inp, keep=True)
    keys = ["cloth0.Kl", "cloth0.Ka", "cloth0.Kb"]
    xs, rr = _dev(st.x), _dev(an.ref_row(st))
    own = ctx.param_grads(xs, rr, keys, p=None)
    given = ctx.param_grads(xs, rr, keys, p=_dev(got["p"].ravel()))
    ctx.close()
    assert all(own[k] == given[k] and own[k] != 0 for k in keys), (own, given)
    exp = an.expected_reverse(ref, op, inp, got["p"])
    R = AdjointRatios()
    an.compare(exp, got, R, frozen=fz)
    zero = an.expected_reverse(ref, op, inp, np.where(inp.frozen, 0.0, got["p"]))
    t = exp["touched"]
    with_frozen = np.array([inp.frozen[hv].any() for _, _, _, hv in an.hinge_layout(st)])
    assert with_frozen.any()
    err = np.abs(cn.diff(got["ag_prev"], zero["ag_prev"][0]))[t]
    assert (err[with_frozen] > 1e6 * zero["ag_prev"][1][t][with_frozen]).all(), "p = 0 on frozen dofs is another value by far"
    R.check(key)


def test_ten_by_ten_repeats_bit_for_bit():
    """the 10 x 10 case on two fresh contexts: every output of the step, p included, is the same bits"""
    key = "10x10/dx150/fold+90_ref0"
    st = an.reference(key).st
    fz = an.frozen_pattern(st.nv, "A")
    inp = an.seeds(st, st.nv, 2, fz, d=0.5, seed=9)
    runs = []
    for _ in range(2):
        ctx = _context(st.cloths, st.nv, fz)
        runs.append(_step(ctx, st.x, an.ref_row(st), inp))
        ctx.close()
    for q in ("pg_s", "ag_s", "ag_prev", "tz", "pg_prev", "pg_prev2", "p"):
        assert np.array_equal(runs[0][q], runs[1][q]), q
