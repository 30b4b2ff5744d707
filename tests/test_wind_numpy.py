"""The wind on the CPU: the NumPy restatement tests/wind_numpy.py against central differences of its own energy and gradient, with
one mutation the differences must catch; csrc/wind_host.hpp and the gather lists of csrc/handle_host.hpp compiled into a stand-alone program under
-fsanitize=address,undefined (tests/native/wind_ref.cpp) -- every refusal names its offender, the lists of a 2 x 2-cell grid are the ones counted by
hand --; and the scene layer on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wind_numpy as wn

HERE = os.path.dirname(os.path.abspath(__file__))

DT = 5e-3
BOUND = 1e-6   # of the largest entry: the bound of the collider restatements' difference checks


def _grid(N):
    """(rest positions (NV, 3), faces (2 N N, 3)) of an N x N-cell grid of 5 mm cells, cells cut along alternating diagonals"""
    dx = 5e-3
    X = np.array([[i * dx, j * dx, 0.0] for i in range(N + 1) for j in range(N + 1)])
    F = []
    for i in range(N):
        for j in range(N):
            a = i * (N + 1) + j; b = a + 1; d = a + N + 1; c = d + 1
            F += [[c, b, a], [a, d, c]] if (i + j) % 2 == 0 else [[b, a, d], [d, c, b]]
    return X, np.array(F)


def _case(seed=7):
    """a 3 x 3-cell grid (16 vertices, 18 faces) bent out of its plane, moved by about dx / 10 over the step; 14 faces listed, out of order, two
    with weight 0; c_n != c_t; every component of W nonzero"""
    rng = np.random.default_rng(seed)
    X, F = _grid(3)
    xp = X + 5e-4 * rng.standard_normal(X.shape)
    x = xp + 5e-4 * rng.standard_normal(X.shape)
    ids = rng.permutation(len(F))[:14]
    w = rng.uniform(0.5, 2.0, len(ids)); w[[3, 9]] = 0.0
    W = np.array([0.31, -0.17, 0.23])
    return x, xp, F[ids], w, W, 9.0, 1.5


def _fd(f, z, h):
    """central differences of f (array-valued) in the entries of z: shape f.shape + z.shape"""
    z = np.asarray(z, np.float64)
    out = np.zeros(np.shape(f(z)) + z.shape)
    for idx in np.ndindex(*z.shape):
        e = np.zeros_like(z); e[idx] = h
        out[(Ellipsis,) + idx] = (np.asarray(f(z + e)) - np.asarray(f(z - e))) / (2 * h)
    return out


def test_restatement_matches_central_differences_in_x():
    """g against differences of E and H against differences of g, in x.  E is quadratic in x: central differences are exact up to rounding, which
    at step 1e-6 is 1e-16 E / h ~ 1e-9 of g; bound 1e-6 of the largest entry.  H is symmetric and positive semi-definite."""
    x, xp, F, w, W, cn, ct = _case()
    A = (F, w, W, cn, ct, DT)
    g = wn.gradient(x, xp, *A)
    gd = _fd(lambda z: wn.energy(z, xp, *A), x, 1e-6)
    print("g vs dE:", np.abs(g - gd).max() / np.abs(g).max())
    assert np.abs(g - gd).max() <= BOUND * np.abs(g).max()
    H = wn.hessian(x, xp, *A)
    Hd = _fd(lambda z: wn.gradient(z, xp, *A).reshape(-1), x, 1e-6).reshape(H.shape)
    print("H vs dg:", np.abs(H - Hd).max() / np.abs(H).max())
    assert np.abs(H - Hd).max() <= BOUND * np.abs(H).max()
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() >= -1e-12 * np.abs(H).max()
    # the force read-out is minus the sum of the gradient rows
    assert np.abs(wn.wind_force(x, xp, *A) + g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max()
    # unlisted vertices get nothing
    untouched = np.setdiff1d(np.arange(len(x)), F.reshape(-1))
    assert not g[untouched].any()


def test_prev_terms_and_read_out_match_differences_of_the_gradient():
    """-(dg/dx_prev)^T p and the five read-out columns against central differences of g contracted with p (free dofs).  g is smooth in x_prev with
    curvature scale |a| ~ dx^2 / 2: at step 1e-8 m (2e-6 of dx) the truncation error is ~ 4e-12 and the rounding error ~ 1e-16 / 1e-8 = 1e-8 of the
    value; g is linear in W, c_n, c_t (any step).  Bound 1e-6.  Mutation: without the derivative through the lagged area vector the x_prev rows miss
    by more than a hundred times the bound."""
    x, xp, F, w, W, cn, ct = _case()
    NV = len(x)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[int(F[0, 0])] = 1; frozen[int(F[1, 1]), 1] = 1; frozen[int(F[5, 2]), 2] = 1
    free = (frozen == 0).astype(np.float64)
    pf = (p * free).reshape(-1)
    grad = lambda xp_=xp, W_=W, cn_=cn, ct_=ct: wn.gradient(x, xp_, F, w, W_, cn_, ct_, DT).reshape(-1)
    J = _fd(lambda z: grad(xp_=z), xp, 1e-8).reshape(3 * NV, 3 * NV)
    want = (-(J.T @ pf)).reshape(-1, 3) * free
    got = wn.backprop_prev(x, xp, p, frozen, F, w, W, cn, ct, DT)
    print("prev terms:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    assert not got[frozen == 1].any()
    miss = np.abs(wn.backprop_prev(x, xp, p, frozen, F, w, W, cn, ct, DT, with_a=False) - want).max() / np.abs(want).max()
    print("without the derivative through a:", miss)
    assert miss > 100 * BOUND
    G = wn.wind_grad(x, xp, p, frozen, F, w, W, cn, ct, DT)
    Gd = np.zeros(5)
    Gd[0:3] = -(pf @ _fd(lambda z: grad(W_=z), W, 1e-3))
    Gd[3] = -(pf @ _fd(lambda z: grad(cn_=float(z)), np.float64(cn), 1e-2))
    Gd[4] = -(pf @ _fd(lambda z: grad(ct_=float(z)), np.float64(ct), 1e-2))
    for lo, hi, name in ((0, 3, "W"), (3, 4, "c_n"), (4, 5, "c_t")):
        err = np.abs(G[lo:hi] - Gd[lo:hi]).max() / np.abs(G[lo:hi]).max()
        print(f"wind_grad d/d{name}: {err:.3e}")
        assert err <= BOUND
    assert np.abs(G).min() > 0


def test_degenerate_face_and_limits():
    """A0 = 0 in x_prev: nothing anywhere, nothing NaN.  c_n = c_t = c: M = c A0 I.  W in the plane of a flat sheet at rest with c_t = 0: gradient 0."""
    x, xp, F, w, W, cn, ct = _case()
    xp2 = xp.copy(); xp2[F[4, 2]] = xp2[F[4, 1]]
    only = F[4:5], w[4:5]
    assert wn.energy(x, xp2, *only, W, cn, ct, DT) == 0.0 and not wn.gradient(x, xp2, *only, W, cn, ct, DT).any() and not wn.hessian(x, xp2, *only, W, cn, ct, DT).any()
    p = np.ones_like(x); fz = np.zeros(x.shape, np.int32)
    assert not wn.backprop_prev(x, xp2, p, fz, *only, W, cn, ct, DT).any() and not wn.wind_grad(x, xp2, p, fz, *only, W, cn, ct, DT).any()
    for q in (wn.gradient(x, xp2, F, w, W, cn, ct, DT), wn.backprop_prev(x, xp2, p, fz, F, w, W, cn, ct, DT)):
        assert np.isfinite(q).all()
    for f in wn.faces_of(F, np.ones(len(F)), x, xp, W, 3.0, 3.0, DT):
        assert np.abs(f.M - 3.0 * f.A0 * np.eye(3)).max() <= 1e-15 * 3.0 * f.A0
    X, Fall = _grid(3)
    assert not wn.gradient(X, X, Fall, np.ones(len(Fall)), [0.4, -0.3, 0.0], 5.0, 0.0, DT).any()


def _ints(line):
    return [int(t) for t in line.split(":", 1)[1].split()]


def test_host_module_under_sanitizers_lists_and_refusals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "wind_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "wind_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _ints(ln) for ln in lines if ":" in ln and not ln.startswith(("refused", "velocity"))}
    # the grid: faces 0 .. 7 of the 2 x 2 cells, vertex i * 3 + j; faces 6, 0, 3 are (4, 5, 8), (0, 1, 4), (1, 5, 4)
    assert got["NV"] == [9] and got["wind_faces"] == [6, 0, 3]
    assert got["cv"] == [4, 5, 8, 0, 1, 4, 1, 5, 4]
    # counted by hand.  Entries 3 i + a: vertex 0 <- (1, 0); 1 <- (1, 1), (2, 0); 4 <- (0, 0), (1, 2), (2, 2); 5 <- (0, 1), (2, 1); 8 <- (0, 2)
    assert got["vl_v"] == [0, 1, 4, 5, 8]
    assert got["vl_ptr"] == [0, 1, 3, 6, 8, 9]
    assert got["vl_ent"] == [3, 4, 6, 0, 5, 8, 1, 7, 2]
    # blocks: 3 x 9 entries; (4, 4) is shared by all three faces, (1, 1), (1, 4), (4, 1) by faces 0 and 3, (5, 5), (4, 5), (5, 4) by faces 6 and 3:
    # 27 - 2 - 3 - 3 = 19 blocks, ascending by (row, column)
    keys = [(0, 0), (0, 1), (0, 4), (1, 0), (1, 1), (1, 4), (1, 5), (4, 0), (4, 1), (4, 4), (4, 5), (4, 8), (5, 1), (5, 4), (5, 5), (5, 8), (8, 4), (8, 5), (8, 8)]
    sizes = [1, 1, 1, 1, 2, 2, 1, 1, 2, 3, 2, 1, 1, 2, 2, 1, 1, 1, 1]
    assert len(got["bl_addr"]) == 19 and got["bl_ptr"] == np.concatenate([[0], np.cumsum(sizes)]).tolist() and len(got["bl_ent"]) == 27
    look = np.array(got["lookup"]).reshape(9, 9)
    assert got["bl_addr"] == [int(look[a, b]) for a, b in keys] and min(got["bl_addr"]) >= 0 and len(set(got["bl_addr"])) == 19
    ent = {k: got["bl_ent"][got["bl_ptr"][q]:got["bl_ptr"][q + 1]] for q, k in enumerate(keys)}
    assert ent[(4, 4)] == [0, 17, 26] and ent[(1, 4)] == [14, 20] and ent[(4, 1)] == [16, 24] and ent[(5, 4)] == [3, 23] and ent[(8, 8)] == [8]
    # and the restated rule gives the same lists
    L = wn.gather_lists(got["cv"])
    assert L["vl_v"] == got["vl_v"] and L["vl_ptr"] == got["vl_ptr"] and L["vl_ent"] == got["vl_ent"]
    assert L["bl_key"] == keys and L["bl_ptr"] == got["bl_ptr"] and L["bl_ent"] == got["bl_ent"]
    # every face: 9 vertices with 24 entries; 9 diagonal blocks and two per edge (6 + 6 + 4 edges) with 72 entries
    assert got["all_counts"] == [9, 24, 41, 72]
    assert got["kept"] == [1] and [ln for ln in lines if ln.startswith("velocity")] == ["velocity: 3 0 -4"]
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"face 10 of entry 2 out of range \[0, 10\)", r"face -1 of entry 2 out of range \[0, 10\)",
              r"face 8 of entry 2 is a surface face of a body, not a cloth face \(cloth faces are \[0, 8\)\)",
              r"face 9 of entry 2 is a surface face of a body, not a cloth face \(cloth faces are \[0, 8\)\)",
              r"face 6 is listed twice \(entries 1 and 2\)", r"weight -0.25 of entry 2 \(face 5\) is negative or not finite",
              r"weight nan of entry 2 \(face 5\) is negative or not finite", r"weight inf of entry 2 \(face 5\) is negative or not finite",
              r"n = -2 is negative", r"null face list",
              r"component 1 of the wind velocity \(0, nan, 1\) is not finite", r"component 0 of the wind velocity \(-inf, 0, 1\) is not finite", r"null wind velocity"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_scene_flag_the_checks_speak_the_library_s_words_and_the_tapes_have_wind_rows():
    import torch
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_wind, validate_wind_velocity
    from thinshelllab_amd.task_scene.Scene_flag import Scene
    s = Scene(N=4, device="cpu")
    s.init_all()
    c = s.cloths[0]
    assert s.tot_NV == 25 and s.elastic_cnt == 0 and s.contact_pairs() == [] and s.n_wind == 32 and s.wind_cn > 0 and s.wind_ct > 0
    assert np.array_equal(s._wind_f, np.arange(32)) and np.array_equal(s._wind_f, c.faces()) and np.array_equal(s._wind_w, np.ones(32))
    assert int(s.frozen.to_numpy().sum()) == 6 and s.hung_vertices() == [0, 20] and s.free_edge() == [4, 9, 14, 19, 24]
    x = s.pos.to_numpy()
    assert not x[:, 1].any() and np.ptp(x[:, 0]) > 0 and x[s.free_edge(), 2].max() < x[s.hung_vertices(), 2].min()   # it hangs in the x-z plane
    for G in (Grad, GradSys):
        g = G(s, 4, 0)
        assert tuple(g.wind_velocity.t.shape) == (4, 3) and tuple(g.wind_grad.t.shape) == (4, 5)
        for f in range(4):
            s.set_wind_velocity([0.1 * f, 1.0, -0.2])
            g.copy_pos(s, f)
        assert np.array_equal(g.wind_velocity.t.numpy(), [[0.1 * f, 1.0, -0.2] for f in range(4)])
        g.wind_grad.t.copy_(torch.arange(20, dtype=torch.float64).reshape(4, 5))
        assert torch.equal(g.wind_velocity_grad(), g.wind_grad.t[:, 0:3])
        g.reset()
        assert not g.wind_grad.t.any() and not g.wind_velocity.t.any()
    assert "wind_velocity" in s._dirty or "wind" in s._dirty
    # the host checks: the messages of csrc/wind_host.hpp behind "set_wind: "
    keep_f, keep_W = s._wind_f.copy(), s._wind_W.copy()
    for args, kw, pat in (((1.0, 1.0), {"face_ids": [3, 5, 3]}, r"set_wind: face 3 is listed twice \(entries 0 and 2\)"),
                          ((1.0, 1.0), {"face_ids": [3, 32]}, r"set_wind: face 32 of entry 1 out of range \[0, 32\)"),
                          ((1.0, 1.0), {"face_ids": [-1]}, r"set_wind: face -1 of entry 0 out of range \[0, 32\)"),
                          ((1.0, 1.0), {"face_ids": [3, 5], "weights": [1.0, -2.0]}, r"set_wind: weight -2 of entry 1 \(face 5\) is negative or not finite"),
                          ((1.0, 1.0), {"face_ids": [3, 5], "weights": [np.nan, 1.0]}, r"set_wind: weight nan of entry 0 \(face 3\) is negative or not finite"),
                          ((1.0, 1.0), {"face_ids": [3, 5], "weights": [1.0]}, r"set_wind: 1 weights for 2 faces"),
                          ((-1.0, 1.0), {}, r"set_wind: wind_cn must be finite and >= 0 \(got -1\)"),
                          ((1.0, np.inf), {}, r"set_wind: wind_ct must be finite and >= 0 \(got inf\)")):
        with pytest.raises(ValueError, match=pat):
            validate_wind(32, 32, *args, **kw)
        with pytest.raises(ValueError, match=pat):
            s.set_wind(*args, **kw)
        assert np.array_equal(s._wind_f, keep_f)
    with pytest.raises(ValueError, match=r"set_wind: face 40 of entry 0 is a surface face of a body, not a cloth face \(cloth faces are \[0, 32\)\)"):
        validate_wind(32, 50, 1.0, 1.0, face_ids=[40])
    with pytest.raises(ValueError, match=r"set_wind_velocity: component 2 of the wind velocity \(0, 1, inf\) is not finite"):
        s.set_wind_velocity([0.0, 1.0, np.inf])
    with pytest.raises(ValueError, match=r"set_wind_velocity: 2 components, not 3"):
        validate_wind_velocity([0.0, 1.0])
    assert np.array_equal(s._wind_W, keep_W)
    s.set_wind(2.0, 0.5, face_ids=[7, 2], weights=[0.0, 3.0])
    assert s.n_wind == 2 and s._wind_f.tolist() == [7, 2] and s._wind_w.tolist() == [0.0, 3.0] and (s.wind_cn, s.wind_ct) == (2.0, 0.5)
    s.set_wind(0.0, 0.0, face_ids=[])
    assert s.n_wind == 0
