"""Half-space colliders on the CPU: the NumPy restatement tests/collider_numpy.py against central differences of its own energy and
gradient, through every branch; csrc/collider_host.hpp compiled into a stand-alone program under -fsanitize=address,undefined
(tests/native/collider_ref.cpp) -- every refusal names its offender, nine colliders are refused, a refused list leaves the old one in place --; and
the scene layer on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import collider_numpy as cn

HERE = os.path.dirname(os.path.abspath(__file__))

K, EPS, EH = 1.0e4, 2.0e-3, 1.0e-3


def _case():
    """14 vertices against a floor (mu 0.5), a plane tilted about x (mu 0.3) and a wall whose normal has |n.x| >= 0.5 (the other branch of the tangent
    pair; mu 0.8): vertices 0..11 walk through (d0 in / out) x (d in / out) x (slip 0, below eh, above eh) of the floor, vertex 12 lies deep inside
    everything with mask 0, vertex 13 sees the tilted plane only."""
    rng = np.random.default_rng(11)
    n = cn.unit([[0.0, 0.0, 1.0], [0.0, np.sin(0.3), np.cos(0.3)], [-0.8, 0.1, 0.6]])
    o = np.array([0.0, -1.0e-3, -2.0e-3])
    mu = np.array([0.5, 0.3, 0.8])
    xp, x = np.zeros((14, 3)), np.zeros((14, 3))
    q = 0
    for d0_in in (True, False):
        for d_in in (True, False):
            for slip in (0.0, 0.3 * EH, 3.0 * EH):
                xp[q] = [rng.uniform(-4e-3, 4e-3), rng.uniform(-4e-3, 4e-3), EPS + (-0.6e-3 if d0_in else 0.7e-3)]
                a = rng.uniform(0, 2 * np.pi)
                x[q] = [xp[q, 0] + slip * np.cos(a), xp[q, 1] + slip * np.sin(a), EPS + (-0.5e-3 if d_in else 0.4e-3)]
                q += 1
    xp[12] = [0.0, 0.0, -5e-3]; x[12] = [1e-3, 0.0, -6e-3]
    xp[13] = [1e-3, -2e-3, -1e-3]; x[13] = [1.5e-3, -2.2e-3, -1.2e-3]
    mask = cn.full_mask(14, 3)
    mask[12] = 0; mask[13] = 2
    return n, o, mu, mask, xp, x


def test_the_case_walks_through_every_branch():
    n, o, mu, mask, xp, x = _case()
    act, act0 = cn.active_sets(x, xp, n, o, mask, EPS)
    on = ((mask[:, None].astype(int) >> np.arange(3)) & 1).astype(bool)
    # d and d0 on either side of eps in every combination, on the floor
    for a in (True, False):
        for b in (True, False):
            assert ((act[:12, 0] == a) & (act0[:12, 0] == b)).sum() == 3
    # r = 0, r below and above eps_v dt, with friction on (d0 < eps, mu > 0)
    r = np.array([[np.linalg.norm(np.stack(cn.tangents(n[j])) @ (x[v] - xp[v])) for j in range(3)] for v in range(14)])
    fr = act0 & (mu[None, :] > 0)
    assert (fr & (r == 0.0)).any() and (fr & (r > 0) & (r < EH)).any() and (fr & (r > EH)).any()
    assert (fr[:, 2] & (r[:, 2] > 0)).any()                      # the wall's tangent pair (|n.x| >= 0.5) carries friction too
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any()   # two planes on one vertex
    assert mask[12] == 0 and (x[12] @ n.T - o < EPS).all() and not act[12].any()   # a masked-out vertex inside every plane
    assert on[13].tolist() == [False, True, False] and act[13, 1]
    # no pair within a difference step of a branch point
    d = x @ n.T - o; d0 = xp @ n.T - o
    assert np.abs(d - EPS)[on].min() > 1e-5 and np.abs(d0 - EPS)[on].min() > 1e-5 and np.abs(r - EH)[on & (r > 0)].min() > 1e-5


def test_restatement_matches_central_differences():
    """g against differences of E, H against differences of g; the bound of the project's other non-quadratic restatements, 1e-6 of the largest entry
    (tests/test_frame_numpy.py).  The steps: 1e-7 for E -> g (its third derivative is ~ lam / eh^2 = 5e6: 1e-8 of truncation against |g| ~ 10),
    1e-9 for g -> H (at r = 0 the gradient lam f1(r) T u is only once differentiable and the difference is off by h / (2 eh) of that entry)."""
    n, o, mu, mask, xp, x = _case()
    NV = len(x)
    args = (n, o, mu, mask, K, EPS, EH)
    g = cn.gradient(x, xp, *args)
    H = cn.hessian(x, xp, *args)
    gd = np.zeros(3 * NV)
    h = 1e-7
    for q in range(3 * NV):
        e = np.zeros(3 * NV); e[q] = h
        gd[q] = (cn.energy(x + e.reshape(-1, 3), xp, *args) - cn.energy(x - e.reshape(-1, 3), xp, *args)) / (2 * h)
    print("g vs dE:", np.abs(g.reshape(-1) - gd).max() / np.abs(g).max())
    assert np.abs(g.reshape(-1) - gd).max() <= 1e-6 * np.abs(g).max()
    Hd = np.zeros_like(H)
    h = 1e-9
    for q in range(3 * NV):
        e = np.zeros(3 * NV); e[q] = h
        Hd[:, q] = (cn.gradient(x + e.reshape(-1, 3), xp, *args) - cn.gradient(x - e.reshape(-1, 3), xp, *args)).reshape(-1) / (2 * h)
    print("H vs dg:", np.abs(H - Hd).max() / np.abs(H).max())
    assert np.abs(H - Hd).max() <= 1e-6 * np.abs(H).max()
    # symmetric, positive semi-definite, block diagonal, nothing on the masked-out vertex
    B = cn.blocks(x, xp, *args)
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max() and np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-9 * np.abs(H).max()
    assert np.array_equal(B[12], np.zeros((3, 3))) and np.array_equal(g[12], np.zeros(3))
    # the read-out: the forces on the planes sum to minus the gradient
    F = cn.force(x, xp, *args)
    assert np.abs(F.sum(axis=0) + g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max()


def test_prev_terms_and_collider_grad_match_differences_of_the_gradient():
    """the two x_prev terms (pos_grad[s-1] += -(dg / dx_prev)^T p) and both collider_grad columns (-p . dg/do_j, -p . dg/dmu_j over the free dofs)
    against central differences of g in x_prev, o and mu; step 1e-9 and bound 1e-6 as above (g is linear in mu: any step)"""
    n, o, mu, mask, xp, x = _case()
    NV = len(x)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[2] = 1; frozen[4, 1] = 1; frozen[13, 2] = 1
    free = (frozen == 0).astype(np.float64)
    grad = lambda xp_, o_, mu_: cn.gradient(x, xp_, n, o_, mu_, mask, K, EPS, EH)
    h = 1e-9
    J = np.zeros((3 * NV, 3 * NV))   # dg / dx_prev
    for q in range(3 * NV):
        e = np.zeros(3 * NV); e[q] = h
        J[:, q] = (grad(xp + e.reshape(-1, 3), o, mu) - grad(xp - e.reshape(-1, 3), o, mu)).reshape(-1) / (2 * h)
    want = (-(J.T @ (p * free).reshape(-1))).reshape(-1, 3) * free
    got = cn.backprop_prev(x, xp, p, frozen, n, o, mu, mask, K, EPS, EH)
    print("prev terms:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert np.array_equal(got[frozen == 1], np.zeros(int(frozen.sum()))) and np.array_equal(got[12], np.zeros(3))
    # the term through lam alone: a step of x_prev along n changes d0 only (T^T n = 0)
    v = 0
    e = np.zeros((NV, 3)); e[v] = n[0] * h
    dn = ((grad(xp + e, o, mu) - grad(xp - e, o, mu)) / (2 * h))[v]
    T = np.stack(cn.tangents(n[0]), axis=1)
    r = np.linalg.norm(T.T @ (x[v] - xp[v]))
    lam_term = -mu[0] * K * cn.f1(r, EH) * (T @ (T.T @ (x[v] - xp[v])))
    assert np.abs(dn - lam_term).max() <= 1e-6 * max(np.abs(lam_term).max(), 1.0)
    G = cn.collider_grad(x, xp, p, frozen, n, o, mu, mask, K, EPS, EH)
    for j in range(3):
        e = np.zeros(3); e[j] = h
        d_o = -float(np.sum(p * free * (grad(xp, o + e, mu) - grad(xp, o - e, mu)) / (2 * h)))
        e[j] = 0.01
        d_mu = -float(np.sum(p * free * (grad(xp, o, mu + e) - grad(xp, o, mu - e)) / 0.02))
        print(f"collider {j}: d/do {G[j, 0]:.9e} (differences {d_o:.9e}), d/dmu {G[j, 1]:.9e} (differences {d_mu:.9e})")
        assert abs(G[j, 0] - d_o) <= 1e-6 * np.abs(G[:, 0]).max() and abs(G[j, 1] - d_mu) <= 1e-9 * np.abs(G[:, 1]).max()
    assert np.abs(G).min() > 0


def _nums(line):
    return np.array(line.split(":", 1)[1].split(), np.float64)


def test_host_module_under_sanitizers_table_and_refusals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "collider_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "collider_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _nums(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    # the table: unit normals, offsets, mu, the tangent pair of the restatement; the scalars are left alone
    n = cn.unit(got["normals"].reshape(-1, 3))
    tab = got["table"].reshape(-1, 11)
    assert got["scalars"].tolist() == [3.0, 7.0, 0.5, 0.25] and len(tab) == 3
    assert np.abs(tab[:, :3] - n).max() <= 2e-16 and np.array_equal(tab[:, 3], got["offsets"]) and np.array_equal(tab[:, 4], got["mu"])
    for j in range(3):
        t1, t2 = cn.tangents(tab[j, :3])
        assert np.abs(tab[j, 5:8] - t1).max() <= 2e-16 and np.abs(tab[j, 8:11] - t2).max() <= 2e-16
        assert abs(t1 @ tab[j, :3]) <= 1e-15 and abs(t2 @ tab[j, :3]) <= 1e-15
    assert abs(n[1, 0]) < 0.5 <= abs(n[2, 0])   # both branches of the tangent pair
    moved = got["table_moved"].reshape(-1, 11)
    assert moved[:, 3].tolist() == [0.1, 0.2, 0.3] and np.array_equal(np.delete(moved, 3, axis=1), np.delete(tab, 3, axis=1))
    assert got["eight"][0] == 8 and got["empty"][0] == 0 and got["kept"][0] == 1
    assert got["mask_all"].tolist() == [7.0] * 20
    want = [5.0] * 20; want[7] = 0.0; want[9] = 2.0
    assert got["mask_given"].tolist() == want
    assert got["mask_ids"].astype(int).tolist() == cn.mask_from_ids(20, [[0, 19, 4], [], [4, 5]]).tolist()
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"normal \(0, 0, 0\) of collider 1 is zero or not finite", r"normal \(nan, 0, 1\) of collider 1 is zero or not finite",
              r"normal \(0, inf, 1\) of collider 1 is zero or not finite", r"offset nan of collider 1 is not finite", r"offset -inf of collider 1 is not finite",
              r"friction coefficient -0.5 of collider 1 is negative or not finite", r"friction coefficient nan of collider 1 is negative or not finite",
              r"friction coefficient inf of collider 1 is negative or not finite", r"9 colliders: at most 8", r"n = -1 is negative",
              r"offset nan of collider 1 is not finite", r"mask 0x08 of vertex 9 names a collider at or above 3",
              r"vertex 20 of collider 2 out of range \[0, 20\)", r"vertex -1 of collider 2 out of range \[0, 20\)"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_scene_floor_the_checks_speak_the_library_s_words_and_the_tapes_have_collider_rows():
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_colliders
    from thinshelllab_amd.task_scene.Scene_floor import Scene
    s = Scene(N=4, device="cpu")
    s.init_all()
    assert s.tot_NV == 25 and s.elastic_cnt == 0 and s.n_collider == 1 and s.k_collider > 0
    assert np.array_equal(s._col_n, [[0.0, 0.0, 1.0]]) and s._col_mask.tolist() == [1] * 25
    t = Scene(N=4, tilt=0.2, device="cpu")
    t.init_all()
    assert t.n_collider == 2 and np.abs(t._col_n[1] - [0.0, np.sin(0.2), np.cos(0.2)]).max() <= 1e-16
    for G in (Grad, GradSys):
        g = G(t, 4, 0)
        assert tuple(g.collider_offsets.t.shape) == (4, 2) and tuple(g.collider_grad.t.shape) == (4, 2, 2)
        t.set_collider_offsets([0.25, -0.5])
        g.copy_pos(t, 2)
        assert g.collider_offsets.t[2].tolist() == [0.25, -0.5] and g.collider_offsets.t[1].tolist() == [0.0, 0.0]
    # the host checks: the messages of csrc/collider_host.hpp behind "set_colliders: "
    up = [0.0, 0.0, 1.0]
    for args, kw, pat in ((([[0.0, 0.0, 0.0]], [0.0], [0.1]), {}, r"set_colliders: normal \(0, 0, 0\) of collider 0 is zero or not finite"),
                          (([up], [np.nan], [0.1]), {}, r"set_colliders: offset nan of collider 0 is not finite"),
                          (([up, up], [0.0, 0.0], [0.1, -1.0]), {}, r"set_colliders: friction coefficient -1 of collider 1 is negative or not finite"),
                          (([up] * 9, [0.0] * 9, [0.0] * 9), {}, r"set_colliders: 9 colliders: at most 8"),
                          (([up, up], [0.0, 0.0], [0.1, 0.1]), {"vertex_ids": [[0, 1], [3, 25]]}, r"set_colliders: vertex 25 of collider 1 out of range \[0, 25\)")):
        with pytest.raises(ValueError, match=pat):
            validate_colliders(s.tot_NV, *args, **kw)
        with pytest.raises(ValueError, match=pat):
            s.set_colliders(*args, 1e4, **kw)
        assert s.n_collider == 1 and np.array_equal(s._col_n, [[0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="k_collider must be finite and >= 0"):
        s.set_colliders([up], [0.0], [0.1], -1.0)
    with pytest.raises(ValueError, match=r"set_collider_offsets: offset inf of collider 0 is not finite"):
        s.set_collider_offsets([np.inf])
    with pytest.raises(ValueError, match=r"set_collider_offsets: 2 offsets for 1 colliders"):
        s.set_collider_offsets([0.0, 1.0])
    n, o, mu, mask = validate_colliders(25, [[0.0, 3.0, 4.0], up], [0.5, 1.0], [0.0, 2.0], vertex_ids=[None, [3, 4]])
    assert np.abs(n[0] - [0.0, 0.6, 0.8]).max() <= 1e-16 and mask.tolist() == [1, 1, 1, 3, 3] + [1] * 20
    s.set_colliders([], [], [], 0.0)
    assert s.n_collider == 0
