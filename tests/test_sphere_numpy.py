"""Sphere colliders on the CPU: the NumPy restatement tests/sphere_numpy.py against central differences of its own energy and
gradient, through every branch, with the sensitivity of every check to the terms a plane does not have; csrc/sphere_host.hpp compiled into a
stand-alone program under -fsanitize=address,undefined (tests/native/sphere_ref.cpp) -- every refusal names its offender, nine spheres are refused
and eight accepted, a refused list leaves the old one in place --; and the scene layer on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sphere_numpy as sn

HERE = os.path.dirname(os.path.abspath(__file__))

K, EPS, EH = 1.0e4, 2.0e-3, 1.0e-3
BOUND = 1e-6   # of the largest entry: the bound of the collider and frame restatements


def _case():
    """15 vertices against two balls (R 0.05, mu 0.5, and R 0.03, mu 0.3, both with c != cp).  Vertices 0..11 walk through (d0 in / out) x (d in / out)
    x (slip relative to the ball 0, below eh, above eh) of ball 0 near its top; ball 1's top lies in the same patch, so that some of them are in
    both shells.  Vertex 12 lies inside both balls' shells with mask 0, vertex 13 far outside, vertex 14 sees ball 1 only."""
    rng = np.random.default_rng(5)
    R = np.array([0.05, 0.03])
    mu = np.array([0.5, 0.3])
    c = np.array([[0.0, 0.0, -0.05], [5e-4, 0.0, -0.03 + 3e-4]])
    cp = c - np.array([[2e-4, 1e-4, 3e-4], [-1e-4, 2e-4, 1e-4]])
    xp, x = np.zeros((15, 3)), np.zeros((15, 3))
    q = 0
    for d0_in in (True, False):
        for d_in in (True, False):
            for slip in (0.0, 0.3 * EH, 3.0 * EH):
                th, ph = rng.uniform(0.0, 0.05), rng.uniform(0, 2 * np.pi)
                u0 = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
                xp[q] = cp[0] + (R[0] + EPS + (-0.6e-3 if d0_in else 0.7e-3)) * u0
                t = np.cross(u0, [1.0, 0.0, 0.0]); t /= np.linalg.norm(t)
                a = rng.uniform(0, 2 * np.pi)
                t = np.cos(a) * t + np.sin(a) * np.cross(u0, t)
                qq = xp[q] + (c[0] - cp[0]) + slip * t - c[0]
                x[q] = c[0] + (R[0] + EPS + (-0.5e-3 if d_in else 0.4e-3)) * qq / np.linalg.norm(qq)
                q += 1
    xp[12] = [0.0, 1e-4, 1e-3]; x[12] = [1e-4, 0.0, 0.8e-3]
    xp[13] = [0.0, 0.0, 0.05]; x[13] = [1e-3, 0.0, 0.051]
    xp[14] = cp[1] + (R[1] + EPS - 0.8e-3) * np.array([0.0, np.sin(0.02), np.cos(0.02)])
    x[14] = c[1] + (R[1] + EPS - 0.3e-3) * np.array([np.sin(0.03), np.sin(0.02), np.sqrt(1 - np.sin(0.03) ** 2 - np.sin(0.02) ** 2)])
    mask = sn.full_mask(15, 2)
    mask[12] = 0; mask[14] = 2
    return c, cp, R, mu, mask, xp, x


def _args():
    c, cp, R, mu, mask, xp, x = _case()
    return (c, cp, R, mu, mask, K, EPS, EH), xp, x


def _slip(x, xp, c, cp, j):
    return np.array([sn.Pair(x[v], xp[v], c[j], cp[j], 1.0, 0.0, K, EPS, EH).r for v in range(len(x))])


def test_the_case_walks_through_every_branch():
    c, cp, R, mu, mask, xp, x = _case()
    act, act0 = sn.active_sets(x, xp, c, cp, R, mask, EPS)
    on = ((mask[:, None].astype(int) >> np.arange(2)) & 1).astype(bool)
    for a in (True, False):   # d and d0 on either side of eps in every combination, on ball 0
        for b in (True, False):
            assert ((act[:12, 0] == a) & (act0[:12, 0] == b)).sum() == 3
    r = np.stack([_slip(x, xp, c, cp, 0), _slip(x, xp, c, cp, 1)], axis=1)
    fr = act0 & (mu[None, :] > 0)
    assert (fr & (r < 1e-9)).any() and (fr & (r > 1e-9) & (r < EH)).any() and (fr & (r > EH)).any()   # r = 0, below and above eps_v dt with friction on
    assert np.abs(c - cp).min() > 0                                       # both balls move
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any()   # two balls on one vertex
    d = np.linalg.norm(x[:, None] - c[None], axis=2) - R; d0 = np.linalg.norm(xp[:, None] - cp[None], axis=2) - R
    assert mask[12] == 0 and (d[12] < EPS).all() and not act[12].any()    # a masked-out vertex inside both shells
    assert on[13].all() and not act[13].any() and not act0[13].any()      # a vertex far outside
    assert on[14].tolist() == [False, True] and act[14, 1] and act0[14, 1]
    # no pair within a difference step of a branch point
    assert np.abs(d - EPS)[on].min() > 1e-5 and np.abs(d0 - EPS)[on].min() > 1e-5 and np.abs(r - EH)[on & (r > 1e-9)].min() > 1e-5


def _fd(f, z, h):
    """central differences of f (array-valued) in the entries of z: shape f.shape + z.shape"""
    z = np.asarray(z, np.float64)
    out = np.zeros(np.shape(f(z)) + z.shape)
    for idx in np.ndindex(*z.shape):
        e = np.zeros_like(z); e[idx] = h
        out[(Ellipsis,) + idx] = (np.asarray(f(z + e)) - np.asarray(f(z - e))) / (2 * h)
    return out


def test_restatement_matches_central_differences():
    """g against differences of E (step 1e-7), exact H against differences of g (step 1e-9: at r = 0 the gradient lam a w is only once differentiable and
    the difference is off by h / (2 eh) of that entry); bound 1e-6 of the largest entry.  The projected block is positive semi-definite, the exact one
    has a negative eigenvalue wherever d < eps.  Sensitivity: without the curvature part of H_n, or without (c - cp) in D, the same comparisons
    miss by more than ten times the bound."""
    A, xp, x = _args()
    NV = len(x)
    g = sn.gradient(x, xp, *A)
    H = sn.hessian(x, xp, *A)
    gd = _fd(lambda z: sn.energy(z, xp, *A), x, 1e-7)
    print("g vs dE:", np.abs(g - gd).max() / np.abs(g).max())
    assert np.abs(g - gd).max() <= BOUND * np.abs(g).max()
    Hd = _fd(lambda z: sn.gradient(z, xp, *A).reshape(-1), x, 1e-9).reshape(3 * NV, 3 * NV)
    print("H vs dg:", np.abs(H - Hd).max() / np.abs(H).max())
    assert np.abs(H - Hd).max() <= BOUND * np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    B, Bp = sn.blocks(x, xp, *A), sn.blocks(x, xp, *A, exact=False)
    assert np.array_equal(B[12], np.zeros((3, 3))) and np.array_equal(g[12], np.zeros(3)) and np.array_equal(B[13], np.zeros((3, 3)))
    # the projected block is PSD; the exact normal block has a negative eigenvalue wherever d < eps
    assert min(np.linalg.eigvalsh(0.5 * (b + b.T)).min() for b in Bp) >= -1e-12 * K
    n_act = 0
    for v, j, P in sn.pairs(x, xp, *A):
        if P.act:
            n_act += 1
            ev = np.linalg.eigvalsh(P.Hn(True))
            assert ev[0] < 0 and abs(ev[0] - ev[1]) <= 1e-9 * K and abs(ev[2] - K) <= 1e-9 * K, ev
            assert np.linalg.eigvalsh(P.Hn(False)).min() >= -1e-12 * K
    assert n_act >= 6
    # sensitivity
    miss_curv = np.abs(sn.hessian(x, xp, *A, curvature=False) - Hd).max() / np.abs(H).max()
    miss_dc = np.abs(sn.gradient(x, xp, *A, drop_centre_motion=True) - gd).max() / np.abs(g).max()
    print("without the curvature term:", miss_curv, " without (c - cp):", miss_dc)
    assert miss_curv > 10 * BOUND and miss_dc > 10 * BOUND
    # the read-out: the forces of the balls sum to minus the gradient
    F = sn.force(x, xp, *A)
    assert np.abs(F.sum(axis=0) + g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max()


def test_prev_terms_and_sphere_grad_match_differences_of_the_gradient():
    """the x_prev term (pos_grad[s-1] += -(dg / dx_prev)^T p) and the eight sphere_grad columns (-p . dg/d(c, cp, mu, R) over the free dofs) against
    central differences of g; step 1e-9 and bound 1e-6 as above (g is linear in mu: any step).  Sensitivity: without lam J_n P0 / rho0 in L the x_prev
    term misses by more than ten times the bound."""
    (c, cp, R, mu, mask, k, eps, eh), xp, x = _args()
    NV = len(x)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[2] = 1; frozen[4, 1] = 1; frozen[14, 2] = 1
    free = (frozen == 0).astype(np.float64)
    pf = (p * free).reshape(-1)
    grad = lambda xp_=xp, c_=c, cp_=cp, R_=R, mu_=mu: sn.gradient(x, xp_, c_, cp_, R_, mu_, mask, k, eps, eh).reshape(-1)
    h = 1e-9
    J = _fd(lambda z: grad(xp_=z), xp, h).reshape(3 * NV, 3 * NV)
    want = (-(J.T @ pf)).reshape(-1, 3) * free
    got = sn.backprop_prev(x, xp, p, frozen, c, cp, R, mu, mask, k, eps, eh)
    print("prev terms:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    assert np.array_equal(got[frozen == 1], np.zeros(int(frozen.sum()))) and np.array_equal(got[12], np.zeros(3))
    miss = np.abs(sn.backprop_prev(x, xp, p, frozen, c, cp, R, mu, mask, k, eps, eh, with_Jn=False) - want).max() / np.abs(want).max()
    print("without lam J_n P0 / rho0:", miss)
    assert miss > 10 * BOUND
    G = sn.sphere_grad(x, xp, p, frozen, c, cp, R, mu, mask, k, eps, eh)
    Gd = np.zeros_like(G)
    Gd[:, 0:3] = -(pf @ _fd(lambda z: grad(c_=z), c, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 3:6] = -(pf @ _fd(lambda z: grad(cp_=z), cp, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 6] = -(pf @ _fd(lambda z: grad(mu_=z), mu, 0.01))
    Gd[:, 7] = -(pf @ _fd(lambda z: grad(R_=z), R, h))
    for lo, hi, name in ((0, 3, "c"), (3, 6, "cp"), (6, 7, "mu"), (7, 8, "R")):
        err = np.abs(G[:, lo:hi] - Gd[:, lo:hi]).max() / np.abs(G[:, lo:hi]).max()
        print(f"sphere_grad d/d{name}: {err:.3e}")
        assert err <= BOUND
    assert np.abs(G).min() > 0
    # [3:6] is minus the sum of the x_prev rows over the sphere's vertices when a single ball acts
    one = mask & 1
    G1 = sn.sphere_grad(x, xp, p, frozen, c[:1], cp[:1], R[:1], mu[:1], one, k, eps, eh)
    b1 = sn.backprop_prev(x, xp, p * free, np.zeros_like(frozen), c[:1], cp[:1], R[:1], mu[:1], one, k, eps, eh)
    assert np.abs(G1[0, 3:6] + b1.sum(axis=0)).max() <= 1e-12 * np.abs(b1).max()


def test_degenerate_pairs_contribute_what_the_model_says():
    """rho < 1e-12: nothing; rho0 < 1e-12: the normal term alone"""
    (c, cp, R, mu, mask, k, eps, eh), xp, x = _args()
    x1 = np.array([c[0]]); xp1 = np.array([cp[0] + [0.0, 0.0, R[0]]])
    m1 = np.array([1], np.uint8)
    assert sn.energy(x1, xp1, c, cp, R, mu, m1, k, eps, eh) == 0.0 and not sn.blocks(x1, xp1, c, cp, R, mu, m1, k, eps, eh).any()
    x2 = np.array([c[0] + [0.0, 0.0, R[0]]]); xp2 = np.array([cp[0]])
    P = sn.Pair(x2[0], xp2[0], c[0], cp[0], R[0], mu[0], k, eps, eh)
    assert P.ok and not P.fric and P.lam == 0.0
    assert np.array_equal(sn.gradient(x2, xp2, c, cp, R, mu, m1, k, eps, eh)[0], k * (P.d - eps) * P.n)
    assert not sn.backprop_prev(x2, xp2, np.ones((1, 3)), np.zeros((1, 3)), c, cp, R, mu, m1, k, eps, eh).any()


def _nums(line):
    return np.array(line.split(":", 1)[1].split(), np.float64)


def test_host_module_under_sanitizers_table_and_refusals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "sphere_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "sphere_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _nums(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    # the table: centres, previous centres = centres, radii, mu; the scalars are left alone
    cen = got["centres"].reshape(-1, 3)
    tab = got["table"].reshape(-1, 8)
    assert got["scalars"].tolist() == [3.0, 7.0, 0.5, 0.25] and len(tab) == 3
    assert np.array_equal(tab[:, 0:3], cen) and np.array_equal(tab[:, 3:6], cen) and np.array_equal(tab[:, 6], got["radii"]) and np.array_equal(tab[:, 7], got["mu"])
    moved = got["table_moved"].reshape(-1, 8)
    assert np.array_equal(moved[:, 0:3], got["moved_c"].reshape(-1, 3)) and np.array_equal(moved[:, 3:6], got["moved_cp"].reshape(-1, 3))
    assert moved[1, 1] == 0.125 and moved[2, 5] == -0.75 and np.array_equal(moved[:, 6:], tab[:, 6:])
    rest = got["table_at_rest"].reshape(-1, 8)
    assert np.array_equal(rest[:, 0:3], moved[:, 0:3]) and np.array_equal(rest[:, 3:6], moved[:, 0:3]) and np.array_equal(rest[:, 6:], tab[:, 6:])
    assert got["eight"][0] == 8 and got["empty"][0] == 0 and got["kept"][0] == 1
    assert got["mask_all"].tolist() == [7.0] * 20 and got["mask_eight"].tolist() == [255.0] * 20
    want = [5.0] * 20; want[7] = 0.0; want[9] = 2.0
    assert got["mask_given"].tolist() == want
    assert got["mask_ids"].astype(int).tolist() == sn.mask_from_ids(20, [[0, 19, 4], [], [4, 5]]).tolist()
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"centre \(nan, 0, 1\) of sphere 1 is not finite", r"centre \(0, inf, 1\) of sphere 1 is not finite", r"centre \(0, 0, -inf\) of sphere 1 is not finite",
              r"radius 0 of sphere 1 is not finite and positive", r"radius -0.1 of sphere 1 is not finite and positive", r"radius nan of sphere 1 is not finite and positive",
              r"radius inf of sphere 1 is not finite and positive", r"friction coefficient -0.5 of sphere 1 is negative or not finite",
              r"friction coefficient nan of sphere 1 is negative or not finite", r"friction coefficient inf of sphere 1 is negative or not finite",
              r"9 spheres: at most 8", r"n = -1 is negative", r"centre \(0.01, nan, 0.03\) of sphere 1 is not finite",
              r"previous centre \(-3, 0.5, inf\) of sphere 2 is not finite", r"mask 0x08 of vertex 9 names a sphere at or above 3",
              r"vertex 20 of sphere 2 out of range \[0, 20\)", r"vertex -1 of sphere 2 out of range \[0, 20\)"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_scene_ball_the_checks_speak_the_library_s_words_and_the_tapes_have_sphere_rows():
    import torch
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_spheres
    from thinshelllab_amd.task_scene.Scene_ball import Scene
    s = Scene(N=4, device="cpu")
    s.init_all()
    assert s.tot_NV == 25 and s.elastic_cnt == 0 and s.n_sphere == 1 and s.k_sphere > 0 and s.contact_pairs() == []
    assert np.array_equal(s._sph_c, [[0.0, 0.0, -0.01]]) and np.array_equal(s._sph_cp, s._sph_c) and s._sph_mask.tolist() == [1] * 25
    assert int(s.frozen.to_numpy().sum()) == 12 and s.centre_vertex() == 12
    t = Scene(N=4, device="cpu")
    t.init_all()
    t.set_spheres([[0.0, 0.0, -0.01], [0.01, 0.0, -0.02]], [0.01, 0.02], [0.5, 0.0], 1e3)
    c0 = t._sph_c.copy()
    for G in (Grad, GradSys):
        t.set_sphere_centres(c0, prev_centres=c0)
        t._sph_cp_step = c0.copy()
        g = G(t, 4, 0)
        assert tuple(g.sphere_centres.t.shape) == (4, 2, 3) and tuple(g.sphere_centres_prev.t.shape) == (4, 2, 3) and tuple(g.sphere_grad.t.shape) == (4, 2, 8)
        g.copy_pos(t, 0)
        for f in range(1, 4):   # what a completed step does to the centres, without the step
            t.set_sphere_centres(c0 + 0.001 * f)
            t._spheres_step_done()
            g.copy_pos(t, f)
        assert np.array_equal(g.sphere_centres.t.numpy(), c0[None] + 0.001 * np.arange(4)[:, None, None])
        assert np.array_equal(g.sphere_centres_prev.t[1:].numpy(), g.sphere_centres.t[:-1].numpy()) and np.array_equal(g.sphere_centres_prev.t[0].numpy(), c0)
        # sphere_centre_grad: row s = sphere_grad[s, :, 0:3] + sphere_grad[s + 1, :, 3:6]
        g.sphere_grad.t.copy_(torch.arange(4 * 2 * 8, dtype=torch.float64).reshape(4, 2, 8))
        cg = g.sphere_centre_grad()
        sg = g.sphere_grad.t
        assert tuple(cg.shape) == (4, 2, 3) and torch.equal(cg[:3], sg[:3, :, 0:3] + sg[1:, :, 3:6]) and torch.equal(cg[3], sg[3, :, 0:3])
        g.sphere_centres_prev.t[2, 1, 0] += 1e-6   # a ball that was put somewhere else between two steps
        with pytest.raises(ValueError, match=r"sphere_centre_grad: the previous centres of step 2 are not the centres of step 1"):
            g.sphere_centre_grad()
        g.reset()
        assert not g.sphere_grad.t.any() and not g.sphere_centres.t.any()
    assert "sphere_centres" in t._dirty or "spheres" in t._dirty
    # the host checks: the messages of csrc/sphere_host.hpp behind "set_spheres: "
    o = [0.0, 0.0, -1.0]
    for args, kw, pat in ((([[np.nan, 0.0, 0.0]], [1.0], [0.1]), {}, r"set_spheres: centre \(nan, 0, 0\) of sphere 0 is not finite"),
                          (([o], [0.0], [0.1]), {}, r"set_spheres: radius 0 of sphere 0 is not finite and positive"),
                          (([o, o], [1.0, np.inf], [0.1, 0.1]), {}, r"set_spheres: radius inf of sphere 1 is not finite and positive"),
                          (([o, o], [1.0, 1.0], [0.1, -1.0]), {}, r"set_spheres: friction coefficient -1 of sphere 1 is negative or not finite"),
                          (([o] * 9, [1.0] * 9, [0.0] * 9), {}, r"set_spheres: 9 spheres: at most 8"),
                          (([o, o], [1.0, 1.0], [0.1, 0.1]), {"vertex_ids": [[0, 1], [3, 25]]}, r"set_spheres: vertex 25 of sphere 1 out of range \[0, 25\)")):
        with pytest.raises(ValueError, match=pat):
            validate_spheres(s.tot_NV, *args, **kw)
        with pytest.raises(ValueError, match=pat):
            s.set_spheres(*args, 1e4, **kw)
        assert s.n_sphere == 1 and np.array_equal(s._sph_c, [[0.0, 0.0, -0.01]])
    with pytest.raises(ValueError, match="k_sphere must be finite and >= 0"):
        s.set_spheres([o], [1.0], [0.1], -1.0)
    with pytest.raises(ValueError, match=r"set_sphere_centres: centre \(0, inf, 0\) of sphere 0 is not finite"):
        s.set_sphere_centres([[0.0, np.inf, 0.0]])
    with pytest.raises(ValueError, match=r"set_sphere_centres: previous centre \(nan, 0, 0\) of sphere 0 is not finite"):
        s.set_sphere_centres([o], prev_centres=[[np.nan, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"set_sphere_centres: 2 centres for 1 spheres"):
        s.set_sphere_centres([o, o])
    assert np.array_equal(s._sph_c, [[0.0, 0.0, -0.01]]) and np.array_equal(s._sph_cp, [[0.0, 0.0, -0.01]])
    c, r, mu, mask = validate_spheres(25, [o, o], [0.5, 1.0], [0.0, 2.0], vertex_ids=[None, [3, 4]])
    assert mask.tolist() == [1, 1, 1, 3, 3] + [1] * 20 and r.tolist() == [0.5, 1.0]
    s.set_spheres(np.ones((8, 3)), np.ones(8), np.zeros(8), 1.0)
    assert s.n_sphere == 8 and s._sph_mask.tolist() == [255] * 25
    s.set_spheres([], [], [], 0.0)
    assert s.n_sphere == 0
