"""Ties on the CPU: the NumPy restatement tests/tie_numpy.py against central differences of its own energy; csrc/tie_host.hpp
compiled into a stand-alone program under -fsanitize=address,undefined (tests/native/tie_ref.cpp) -- every refusal names its offender, the slot
records equal the restatement's, the partials of the k_tie key lie behind the table's --; and the factorisation plan of the product
(direct_sym.hpp / direct_plan.hpp through tests/native/ds_ref.cpp) with tie-shaped constraints k (c c^T) (x) I_3 against scipy's sparse LU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tie_numpy as tn
from test_direct_plan import cloth_cliques, dsref_lib

HERE = os.path.dirname(os.path.abspath(__file__))


def _grid_faces(N, M):
    f = []
    for i in range(N):
        for j in range(M):
            a = i * (M + 1) + j; b = a + 1; d = a + M + 1; c = d + 1
            f += [(a, b, c), (a, c, d)]
    return np.array(f)


def _random_list(rng, NV, faces_tab, n):
    faces = rng.integers(0, len(faces_tab), n)
    verts = np.array([rng.choice(np.setdiff1d(np.arange(NV), faces_tab[f])) for f in faces])
    bary = rng.dirichlet(np.ones(3), n)
    w = rng.uniform(0.2, 2.0, n)
    return verts, faces, bary, w


def test_restatement_matches_central_differences_of_its_own_energy():
    rng = np.random.default_rng(5)
    N, M = 4, 3
    NV = (N + 1) * (M + 1)
    tab = _grid_faces(N, M)
    verts, faces, bary, w = _random_list(rng, NV, tab, 14)
    bary[3] = (1.0, 0.0, 0.0); bary[4] = (0.0, 0.4, 0.6); w[5] = 0.0
    idx, b, w = tn.records(tab, verts, faces, bary, w)
    k = 2e5
    x = rng.standard_normal((NV, 3)) * 0.01
    g = tn.gradient(x, idx, b, w, k)
    H = tn.hessian(NV, idx, b, w, k)
    # the energy is quadratic: central differences are exact up to rounding at any step
    h = 1e-4
    gd = np.zeros(3 * NV)
    for d in range(3 * NV):
        e = np.zeros(3 * NV); e[d] = h
        gd[d] = (tn.energy(x + e.reshape(-1, 3), idx, b, w, k) - tn.energy(x - e.reshape(-1, 3), idx, b, w, k)) / (2 * h)
    assert np.abs(g.reshape(-1) - gd).max() <= 1e-9 * np.abs(g).max()
    Hd = np.zeros_like(H)
    for d in range(3 * NV):
        e = np.zeros(3 * NV); e[d] = h
        Hd[:, d] = (tn.gradient(x + e.reshape(-1, 3), idx, b, w, k) - tn.gradient(x - e.reshape(-1, 3), idx, b, w, k)).reshape(-1) / (2 * h)
    assert np.abs(H - Hd).max() <= 1e-9 * np.abs(H).max()
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() >= -1e-9 * np.abs(H).max()
    # force on the vertex, the parameter rows: d/dk and d/dw_i of -p . g over the free dofs
    assert np.allclose(tn.force(x, idx, b, w, k), -k * w[:, None] * tn.residuals(x, idx, b), rtol=0, atol=0)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[idx[0, 3]] = 1; frozen[idx[1, 0], 1] = 1
    free = frozen == 0
    rows = tn.pg_rows(x, p, frozen, idx, b)
    val = lambda k_, w_: -float(np.sum((p * tn.gradient(x, idx, b, w_, k_))[free]))
    dk = (val(k * 1.01, w) - val(k * 0.99, w)) / (0.02 * k)
    assert abs(dk - float(w @ rows)) <= 1e-10 * abs(dk)
    for i in (0, 1, 7):
        dw = np.zeros(len(w)); dw[i] = 0.01
        assert abs((val(k, w + dw) - val(k, w - dw)) / 0.02 - k * rows[i]) <= 1e-10 * abs(k * rows[i]) + 1e-12


def _nums(line):
    return np.array(line.split(":", 1)[1].split(), np.float64)


def test_host_module_under_sanitizers_records_refusals_and_the_key_place(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "tie_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "tie_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _nums(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    tab = got["faces"].astype(np.int64).reshape(-1, 3)
    idx, b, w = tn.records(tab, got["tie_verts"].astype(np.int64), got["tie_faces"].astype(np.int64), got["tie_bary"].reshape(-1, 3), got["tie_weights"])
    assert np.array_equal(got["idx"].astype(np.int64).reshape(-1, 4), idx) and np.array_equal(got["b"].reshape(-1, 3), b) and np.array_equal(got["w"], w)
    assert np.array_equal(got["w_default"], np.ones(len(w))) and len(got["idx_empty"]) == 0
    assert (idx[:, 3] == got["tie_verts"]).all() and all(len(set(row)) == 4 for row in idx.tolist())
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"face 144 of tie 2 out of range \[0, 144\)", r"face -1 of tie 2 out of range \[0, 144\)",
              r"vertex 90 of tie 2 \(face 5\) out of range \[0, 90\)", r"vertex -1 of tie 2 \(face 5\) out of range \[0, 90\)",
              r"vertex 12 of tie 2 is a corner of its own face 5",
              r"barycentric coordinate -0.1 of tie 2 \(face 5, vertex 88\) is not finite or outside \[0, 1\]",
              r"barycentric coordinate nan of tie 2 \(face 5, vertex 88\) is not finite or outside \[0, 1\]",
              r"barycentric coordinate 1.2 of tie 2 \(face 5, vertex 88\) is not finite or outside \[0, 1\]",
              r"barycentric coordinates \(0.3, 0.3, 0.3\) of tie 2 \(face 5, vertex 88\) sum to 0.9, not 1",
              r"weight -1 of tie 2 \(face 5, vertex 88\) is negative or not finite", r"weight inf of tie 2 \(face 5, vertex 88\) is negative or not finite",
              r"n = -2 is negative"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)
    # the k_tie partials: behind the table's total, two of them, whichever other keys are asked; the other keys' rows are where they are without it
    for name in ("place0", "place1", "place2"):
        row = got[name].astype(np.int64)
        total, off, cnt, total_tie = row[:4]
        assert off == total and cnt == 2 and total_tie == total + 2, (name, row)
        others = row[4:].reshape(-1, 2)
        assert all(o + c <= total for o, c in others)
    assert got["place0"][0] == 0 and got["place1"].astype(np.int64).tolist() == [8, 8, 2, 10, 0, 2]          # (cloth0.Kl: row 0 of 4 face rows x 2 workgroups)
    assert got["place_none"].astype(np.int64).tolist() == [7, 0, 7]
    assert got["table_knows_k_tie"][0] == 0


# ------------------------------------------------------------------------------------------------ the plan with tie-shaped constraints
def _tie_system(grids, rng):
    """grids: [(N, M)] cloth grids one after the other.  (NV, row_ptr, col, vals, A (lil), vertex offsets, triangles per grid)"""
    cliques, tris_of, offs = [], [], []
    off = 0
    for N, M in grids:
        tris, cl = cloth_cliques(N, M, off)
        cliques += cl; tris_of.append(tris); offs.append(off)
        off += (N + 1) * (M + 1)
    NV = off
    rows = [set([v]) for v in range(NV)]
    for c in cliques:
        for a in c:
            rows[a].update(c)
    rows = [sorted(r) for r in rows]
    row_ptr = np.zeros(NV + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32)
    A = sp.lil_matrix((3 * NV, 3 * NV))
    for c in cliques:
        d = np.concatenate([3 * v + np.arange(3) for v in c])
        X = rng.standard_normal((len(d), len(d)))
        A[np.ix_(d, d)] = A[np.ix_(d, d)].toarray() + X @ X.T / len(d)
    A = (A.tocsr() + 0.05 * sp.identity(3 * NV)).tolil()
    bsr = sp.bsr_matrix(A.tocsr(), blocksize=(3, 3)); bsr.sort_indices()
    look = {(r, bsr.indices[q]): bsr.data[q] for r in range(NV) for q in range(bsr.indptr[r], bsr.indptr[r + 1])}
    vals = np.zeros((len(col), 3, 3))
    for r in range(NV):
        for kk, cc in enumerate(rows[r]):
            vals[row_ptr[r] + kk] = look.get((r, cc), np.zeros((3, 3)))
    return NV, row_ptr, col, vals, A, offs, tris_of


def _face_with(tris, v):
    return next(t for t in tris if v in t)


def _seam(grids, offs, tris_of, rng):
    """row 0 of grid 1 onto faces of the last row of grid 0, one-hot: a full seam"""
    (N0, M0), (N1, M1) = grids
    W = M0 + 1
    cons, cs = [], []
    for j in range(W):
        target = offs[0] + N0 * W + j
        t = _face_with(tris_of[0], target)
        cons.append([t[0], t[1], t[2], offs[1] + j])
        cs.append([-(1.0 if v == target else 0.0) for v in t] + [1.0])
    return cons, cs


def _tube(grids, offs, tris_of, rng):
    (N, M), = grids
    W = M + 1
    cons, cs = [], []
    for j in range(W):
        target = N * W + j
        t = _face_with(tris_of[0], target)
        cons.append([t[0], t[1], t[2], j])
        cs.append([-(1.0 if v == target else 0.0) for v in t] + [1.0])
    return cons, cs


def _scattered(grids, offs, tris_of, rng, n=40):
    cons, cs = [], []
    nv1 = (grids[1][0] + 1) * (grids[1][1] + 1)
    for _ in range(n):
        t = tris_of[0][rng.integers(len(tris_of[0]))]
        b = rng.dirichlet(np.ones(3))
        cons.append([t[0], t[1], t[2], offs[1] + int(rng.integers(nv1))])
        cs.append(list(-b) + [1.0])
    return cons, cs


PLAN_CASES = [("seam", [(12, 12), (12, 12)], 8, _seam, 13), ("seam", [(32, 32), (32, 32)], 64, _seam, 33), ("tube", [(16, 12)], 8, _tube, 13),
              ("tube", [(32, 32)], 64, _tube, 33), ("scattered", [(20, 20), (20, 20)], 16, _scattered, 40)]


@pytest.fixture(scope="module")
def dsref():
    return dsref_lib()


@pytest.mark.parametrize("name,grids,leaf,make,n_ties", PLAN_CASES, ids=[f"{c[0]}-{c[1][0][0]}x{c[1][0][1]}" for c in PLAN_CASES])
def test_plan_with_tie_cliques_matches_sparse_lu(dsref, name, grids, leaf, make, n_ties):
    """the bounds of tests/test_direct_plan.py: 1e-8 in x, 1e-9 in the residual; rc = 0 says no constraint vertex lay outside its front"""
    rng = np.random.default_rng(100 * grids[0][0] + leaf)
    NV, row_ptr, col, vals, A, offs, tris_of = _tie_system(grids, rng)
    cons, cs = make(grids, offs, tris_of, rng)
    assert len(cons) == n_ties
    cons = np.array(cons, np.int32)
    kw = 50.0
    conH = np.stack([kw * np.kron(np.outer(c, c), np.eye(3)) for c in np.array(cs)])
    for e in range(len(cons)):
        d = np.concatenate([3 * v + np.arange(3) for v in cons[e]])
        A[np.ix_(d, d)] = A[np.ix_(d, d)].toarray() + conH[e]
    A = A.tocsc()
    g = np.array([[o, N, M] for o, (N, M) in zip(offs, grids)], np.int32).reshape(-1)
    blocks = np.zeros(2, np.int32)
    b = rng.standard_normal(3 * NV)
    x = np.zeros(3 * NV)
    stats = np.zeros(8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = dsref.dsref_solve(NV, P(row_ptr), P(col), P(vals), len(grids), P(g), 0, P(blocks), len(cons), P(cons), P(conH), leaf, P(b), P(x), P(stats))
    assert rc == 0
    xr = spla.splu(A).solve(b)
    err, res = np.linalg.norm(x - xr) / np.linalg.norm(xr), np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    print(f"{name} {grids} leaf {leaf}: {len(cons)} ties, |x - x_lu| / |x_lu| = {err:.2e}, residual {res:.2e}")
    assert stats[1] >= 2 and err <= 1e-8 and res <= 1e-9, (err, res, stats)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_sew_takes_the_lowest_face_the_checks_speak_the_library_s_words_and_the_tapes_have_tie_rows():
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_ties
    from thinshelllab_amd.task_scene.Scene_seam import Scene
    s = Scene(cloth_size=0.04, N=4, device="cpu")
    s.init_all()
    tab = s.faces.to_numpy()
    assert s.n_tie == 5 and s.k_tie == 2e5 and s.tot_NV == 50 and len(tab) == 64
    va, vb = s.seam_pairs()
    assert np.array_equal(s._tie_v, va) and np.array_equal(va, 25 + np.arange(5)) and np.array_equal(vb, 20 + np.arange(5))
    for i in range(5):
        f, b = s._tie_f[i], s._tie_b[i]
        assert sorted(b.tolist()) == [0.0, 0.0, 1.0] and tab[f][int(np.argmax(b))] == vb[i]
        assert f == min(q for q in range(len(tab)) if vb[i] in tab[q])
    # the seam starts closed; the tube's row N comes back onto row 0
    idx, b, w = tn.records(tab, s._tie_v, s._tie_f, s._tie_b)
    assert np.abs(tn.residuals(s.pos.to_numpy(), idx, b)).max() == 0.0
    t = Scene(cloth_size=0.04, N=4, tube=True, device="cpu")
    t.init_all()
    idx, b, w = tn.records(t.faces.to_numpy(), t._tie_v, t._tie_f, t._tie_b)
    assert t.tot_NV == 25 and t.n_tie == 5 and np.abs(tn.residuals(t.pos.to_numpy(), idx, b)).max() <= 1e-17
    for G in (Grad, GradSys):
        g = G(s, 4, 0)
        assert tuple(g.tie_grad.t.shape) == (4, 5) and g.param_keys == [] and g.grad_params == {}
    # the host checks: the messages of csrc/tie_host.hpp behind "set_ties: "
    good = [0.2, 0.3, 0.5]
    for args, pat in ((([30], [64], [good]), r"set_ties: face 64 of tie 0 out of range \[0, 64\)"),
                      (([50], [3], [good]), r"set_ties: vertex 50 of tie 0 \(face 3\) out of range \[0, 50\)"),
                      (([int(tab[3][1])], [3], [good]), rf"set_ties: vertex {int(tab[3][1])} of tie 0 is a corner of its own face 3"),
                      (([30], [3], [[0.3, 0.3, 0.3]]), r"set_ties: barycentric coordinates \(0.3, 0.3, 0.3\) of tie 0 \(face 3, vertex 30\) sum to 0.9, not 1"),
                      (([30], [3], [[1.2, 0.0, 0.0]]), r"set_ties: barycentric coordinate 1.2 of tie 0 \(face 3, vertex 30\) is not finite or outside \[0, 1\]"),
                      (([30], [3], [good], [-1.0]), r"set_ties: weight -1 of tie 0 \(face 3, vertex 30\) is negative or not finite")):
        with pytest.raises(ValueError, match=pat):
            validate_ties(s.tot_NV, tab, *args)
        with pytest.raises(ValueError, match=pat):
            s.set_ties(*args[:3], 10.0, *args[3:])
        assert s.n_tie == 5
    with pytest.raises(ValueError, match="k_tie must be finite and >= 0"):
        s.set_ties([30], [3], [good], -1.0)
    s.set_ties([], [], np.zeros((0, 3)), 0.0)
    assert s.n_tie == 0
