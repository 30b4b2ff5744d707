"""tests/tet_numpy.py, the reference of tests/test_gpu_tet_elements.py, pinned without the kernels: mp central differences of its own energy
and gradient, its two statements of the tactile material against each other, the quirk of the box material below its clamp, rotation
invariance, the oracle (oracle/pyoracle.py) on a crushed pad and box, and the size of the float64 errors that the GPU bounds are built from."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tet_numpy as tn  # noqa: E402
from tet_numpy import MP  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thinshelllab_amd", "data")
CASES = [(k, r, s) for k in (0, 1) for r in tn.REST for s in tn.STATES_OF_KIND[k]]
H = "1e-20"


def _mpx(x):
    return np.array([mp.mpf(float(v)) for v in np.asarray(x).ravel()], dtype=object).reshape(4, 3)


def _cd(fun, x):
    """central differences (h = 1e-20) of fun over the 12 coordinates, stacked on a new first axis"""
    h = mp.mpf(H)
    rows = []
    for i in range(12):
        xp_, xm_ = x.copy(), x.copy()
        xp_.flat[i] = xp_.flat[i] + h
        xm_.flat[i] = xm_.flat[i] - h
        rows.append((np.array(fun(xp_), dtype=object) - np.array(fun(xm_), dtype=object)) / (2 * h))
    return np.array(rows, dtype=object)


def _J(r):
    return tn._det(tn.deformation(MP, r["x"], r["B"])[0])


def _edge(rest):
    X = tn.REST[rest]
    return float(np.abs(X[:3] - X[3]).max())


@pytest.mark.parametrize("kind,rest,state", CASES)
@tn.with_mp
def test_gradient_and_block_are_differences_of_energy_and_gradient(kind, rest, state):
    """kind 0 everywhere (the polynomial form is smooth through J = 0), kind 1 wherever J > 0.01.  Step 1e-20 on coordinates of 1e-5 .. 1e-1 m at 50
    digits: truncation (h / edge)^2 <= 1e-30 and rounding 1e-50 edge / h <= 1e-31 relative, asserted at 1e-24 of the block's scale."""
    r = tn.element_reference(rest, state, kind)
    if kind == 1 and not _J(r) > mp.mpf("0.01"):
        return
    x, B, W, mat = _mpx(r["x"]), r["B"], r["W"], r["mat"]
    g_fd = _cd(lambda y: tn.energy(MP, y, B, W, mat), x)
    scale = r["block_n"] * _edge(rest)
    assert tn.fro(g_fd - r["grad"]) <= mp.mpf("1e-24") * scale
    K_fd = _cd(lambda y: tn.gradient(MP, y, B, W, mat), x)   # [variable][gradient entry]
    K = r["block"] if kind == 1 else r["block"].T            # kind 0 stores row = variable, kind 1 row = gradient entry
    assert tn.fro(K_fd.T - K) <= mp.mpf("1e-24") * r["block_n"]


@pytest.mark.parametrize("rest", list(tn.REST))
@pytest.mark.parametrize("state", tn.STATES_OF_KIND[0])
@tn.with_mp
def test_tactile_literal_and_polynomial_forms_agree(rest, state):
    r = tn.element_reference(rest, state, 0)
    if abs(_J(r)) < mp.mpf("1e-3"):
        return
    x, B, W, mat = r["x"], r["B"], r["W"], r["mat"]
    g = np.array(tn.gradient(MP, x, B, W, mat, "literal"), dtype=object)
    assert tn.fro(g - r["grad"]) <= mp.mpf("1e-40") * r["block_n"] * _edge(rest)
    K = np.array(tn.block12(MP, tn.block9(MP, x, B, W, mat, "literal")), dtype=object)
    assert tn.fro(K - r["block"]) <= mp.mpf("1e-40") * r["block_n"]


def test_the_states_meant_to_be_flat_or_beyond_the_clamp_are():
    with mp.workdps(50):
        for rest in tn.REST:
            assert _J(tn.element_reference(rest, "f", 0)) == 0
            assert abs(_J(tn.element_reference(rest, "e", 0)) - mp.mpf("1e-3")) < mp.mpf("1e-12")
            assert _J(tn.element_reference(rest, "g", 0)) < mp.mpf("-0.49")
            assert mp.mpf("0.01") < _J(tn.element_reference(rest, "h+", 1)) < mp.mpf("0.0102")
            assert mp.mpf("0.0098") < _J(tn.element_reference(rest, "h-", 1)) < mp.mpf("0.01")
            assert _J(tn.element_reference(rest, "i", 1)) < mp.mpf("-0.49")


@pytest.mark.parametrize("rest", list(tn.REST))
@pytest.mark.parametrize("state", ["h-", "i"])
@tn.with_mp
def test_box_block_below_the_clamp_is_the_differenced_gradient_plus_the_trace_term(rest, state):
    """log(max(J, 0.01)) is constant there, so the gradient's derivative has no lam tr(F^-1 dF) F^-T, which the reference keeps: the block
    exceeds the differenced gradient by exactly that term, W lam g g^T with g[(j, r)] = (F^-T B^T)[r][j] -- a symmetric rank-one matrix, so
    the block stays symmetric below the clamp as above it (the scatter convention of kind 1 cannot be told from its transpose by value)."""
    r = tn.element_reference(rest, state, 1)
    x, B, W, mat = r["x"], r["B"], r["W"], r["mat"]
    K_fd = _cd(lambda y: tn.gradient(MP, y, B, W, mat), _mpx(x)).T
    K_drop = np.array(tn.block12(MP, tn.block9(MP, x, B, W, mat, drop_trace_term=True)), dtype=object)
    assert tn.fro(K_fd - K_drop) <= mp.mpf("1e-24") * r["block_n"]
    F, Bm = tn.deformation(MP, x, B)
    G = tn._mul(tn._T(tn._inv(F)), tn._T(Bm))
    g = [G[c][j] for j in range(3) for c in range(3)]
    g += [-(g[c] + g[3 + c] + g[6 + c]) for c in range(3)]
    T = np.array([[mp.mpf(W) * mp.mpf(mat.lam) * g[a] * g[b] for b in range(12)] for a in range(12)], dtype=object)
    assert tn.fro(T) > mp.mpf("1e-2") * r["block_n"]   # (no small term)
    assert tn.fro(r["block"] - K_drop - T) <= mp.mpf("1e-40") * r["block_n"]
    assert tn.fro(r["block"] - r["block"].T) <= mp.mpf("1e-40") * r["block_n"]


@pytest.mark.parametrize("kind", [0, 1])
@tn.with_mp
def test_energy_is_invariant_under_rotation_and_the_gradient_rotates(kind):
    for state in ("c", "g" if kind == 0 else "i"):
        r = tn.element_reference("sliver", state, kind)
        B, W, mat = r["B"], r["W"], r["mat"]
        c, s = mp.cos(mp.mpf("0.9")), mp.sin(mp.mpf("0.9"))
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=object)
        Rx = np.array([[1, 0, 0], [0, c, s], [0, -s, c]], dtype=object)
        R = Rz.dot(Rx)
        xr = _mpx(r["x"]).dot(R.T)
        assert abs(tn.energy(MP, xr, B, W, mat) - r["energy"]) <= mp.mpf("1e-40") * r["energy_n"]
        g = np.array(tn.gradient(MP, xr, B, W, mat), dtype=object).reshape(4, 3)
        assert tn.fro(g - r["grad"].reshape(4, 3).dot(R.T)) <= mp.mpf("1e-40") * r["grad_n"]


@tn.with_mp
def test_projection_clamps_and_keeps_what_is_already_positive():
    r = tn.element_reference("corner", "g", 0)
    P9 = np.array([[float(r["block_spd"][i, j]) for j in range(9)] for i in range(9)])
    K9 = r["block_f"][:9, :9]
    w, V = np.linalg.eigh(0.5 * (K9 + K9.T))
    assert w.min() < 0 and np.abs((V * np.maximum(w, 0)) @ V.T - P9).max() <= 1e-12 * np.abs(K9).max()
    assert np.abs(r["block_spd_f"].sum(0)).max() <= 1e-12 * np.abs(K9).max()   # vertex 3 = minus the sums: rigid translations in the null space
    r = tn.element_reference("corner", "d", 1)
    assert r["min_eig"] > 0 and tn.fro(r["block_spd"] - r["block"]) <= mp.mpf("1e-40") * r["block_n"]


def test_frozen_rule():
    A = np.arange(36.0).reshape(6, 6) + 1
    M = tn.mask_matrix(A, [0, 1, 0, 0, 0, 1], [7.0, 9.0])
    assert M[1, 1] == 7.0 and M[5, 5] == 9.0 and M[0, 2] == A[0, 2]
    assert not M[1, [0, 2, 3, 4, 5]].any() and not M[[0, 2, 3, 4], 5].any()


@pytest.mark.parametrize("kind,rest,state", CASES)
def test_float64_errors_are_far_below_the_quantities_they_bound(kind, rest, state):
    """e64 < 1e-9 |mp|_F, so that bound() cannot swallow a real error.  At rest (state a) the gradient, and for kind 1 its parameter derivatives
    (F - F^-T, log J F^-T), vanish analytically and what is left of them is rounding of the inputs: there the yardstick is the size of the
    terms that cancel, |block|_F times the element's edge (over mu or lam for the derivatives).  The energy of a box element at rest is zero
    in the same way; it is asserted per mesh in test_mesh_energies_have_small_float64_errors, as the engine only returns the sum."""
    r = tn.element_reference(rest, state, kind)
    with mp.workdps(50):
        mat = r["mat"]
        cancel = r["block_n"] * _edge(rest)
        at_rest = state == "a"
        assert r["block_e64"] < mp.mpf("1e-9") * r["block_n"]
        assert r["grad_e64"] < mp.mpf("1e-9") * (cancel if at_rest else r["grad_n"])
        assert r["dmu_e64"] < mp.mpf("1e-9") * (cancel / mat.mu if at_rest and kind == 1 else r["dmu_n"])
        assert r["dlam_e64"] < mp.mpf("1e-9") * (cancel / mat.lam if at_rest and kind == 1 else r["dlam_n"])
        if not (at_rest and kind == 1):
            assert r["energy_e64"] < mp.mpf("1e-9") * r["energy_n"]


def test_mesh_energies_have_small_float64_errors():
    with mp.workdps(50):
        for name, bodies in tn.gpu_meshes().items():
            for kind, items in bodies:
                rs = [tn.element_reference(r, s, kind) for r, s in items]
                assert sum(r["energy_e64"] for r in rs) < mp.mpf("1e-9") * abs(sum(r["energy"] for r in rs)), (name, kind)


# ------------------------------------------------------------------------------------------------ against the oracle
def test_oracle_agrees_on_a_crushed_pad_and_box(oracle):
    """the tactile pad mesh and a box body under an affine map with J = 0.3 plus noise of 5 % of an edge: the oracle's F and H (converged
    eigen-clamp, set_spd_mode(1)) against the sum of the restatement's element gradients and blocks, to 1e-12 of each element block's norm"""
    nodes = oracle.read_node(os.path.join(DATA, "tactile.node")); tets = oracle.read_ele(os.path.join(DATA, "tactile.ele")); faces = oracle.read_face(os.path.join(DATA, "tactile.face"))
    oracle.set_spd_mode(1)
    try:
        o = oracle.OracleScene(gravity=(0.0, 0.0, 0.0))
        o.add_cloth(2, 2, 0.01)
        o.L.tslo_cloth_init_mesh(o.h, 0)
        et = o.add_tactile(1.0, nodes, tets, faces)
        eb = o.add_box(0.02, 3, 3, 3)
        o.elastic_init(et, 0, 0, 0, False)
        o.elastic_init(eb, 0.1, 0, 0, False)
        o.finalize()
        o.frozen[:] = 0
        rng = np.random.default_rng(5)
        A = tn.R1 @ np.diag([1.0, 0.6, 0.5]) @ tn.R2
        assert abs(np.linalg.det(A) - 0.3) < 1e-12
        nc = o.int("cloth0.NV")
        x = o.pos.copy()
        want_F = np.zeros(3 * len(x)); want_H = np.zeros((3 * len(x), 3 * len(x)))
        elements = []
        for e in (0, 1):
            off, tv = o.int("elastic%d.offset" % e), o.arr("elastic%d.F_vertices" % e, (-1, 4))
            Bs, Ws = o.arr("elastic%d.F_B" % e, (-1, 9)), o.arr("elastic%d.F_W" % e)
            mat = tn.Material(e, o.double("elastic%d.mu" % e), o.double("elastic%d.lam" % e), o.double("elastic%d.alpha" % e))
            nv = o.int("elastic%d.n_verts" % e)
            edge = np.abs(x[off + tv[0, 0]] - x[off + tv[0, 3]]).max()
            c = x[off:off + nv].mean(0)
            x[off:off + nv] = (x[off:off + nv] - c) @ A.T + c + rng.normal(scale=0.05 * edge, size=(nv, 3))
            elements += [(mat, off + tv[t], Bs[t], Ws[t]) for t in range(len(tv))]
        o.pos[:] = x; o.prev_pos[:] = x; o.vel[:] = 0
        o.push_down_all()
        o.newton_step_init(); o.compute_residual_and_Hessian(spd=True)
        got_F, got_H = o.arr("F").copy(), o.H_csr().toarray()
        mdt2 = o.arr("mass") / o.dt ** 2
        norms = np.zeros(len(elements))
        for k, (mat, v, B, W) in enumerate(elements):
            dofs = (3 * v[:, None] + np.arange(3)).ravel()
            K = np.array(tn.element_matrix(tn.F64, x[v], B, W, mat, 1), dtype=float)
            want_H[np.ix_(dofs, dofs)] += K
            want_F[dofs] += np.array(tn.gradient(tn.F64, x[v], B, W, mat), dtype=float)
            norms[k] = np.linalg.norm(K)
        want_H[np.arange(3 * nc, len(want_F)), np.arange(3 * nc, len(want_F))] += np.repeat(mdt2, 3)[3 * nc:]
        worst = 0.0
        for k, (mat, v, B, W) in enumerate(elements):
            dofs = (3 * v[:, None] + np.arange(3)).ravel()
            eh = np.linalg.norm(got_H[np.ix_(dofs, dofs)] - want_H[np.ix_(dofs, dofs)]) / norms[k]
            ef = np.linalg.norm(got_F[dofs] - want_F[dofs]) / (norms[k] * np.abs(x[v[:3]] - x[v[3]]).max())
            worst = max(worst, eh, ef)
        assert worst <= 1e-12, worst
    finally:
        oracle.set_spd_mode(0)
