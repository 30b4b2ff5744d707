"""Capsule colliders on the CPU: the NumPy restatement tests/capsule_numpy.py against central differences of its own energy and
gradient, through every branch (the two caps and the barrel for t and for t0, d and d0 on either side of eps, the three slip regimes), with the
sensitivity of every check to the terms a sphere does not have; csrc/capsule_host.hpp compiled into a stand-alone program under
-fsanitize=address,undefined (tests/native/capsule_ref.cpp) -- every refusal names its offender, nine capsules are refused and eight accepted, a
refused list or update leaves the old one in place --; and the scene layer on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import capsule_numpy as cn

HERE = os.path.dirname(os.path.abspath(__file__))

K, EPS, EH = 1.0e4, 2.0e-3, 1.0e-3
BOUND = 1e-6   # of the largest entry: the bound of the sphere, collider and frame restatements
AWAY = 1e-3    # no pair closer than this to s = 0, s = 1 (in s), d = eps, d0 = eps (in metres)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _place(a, b, ap, bp, R, s0, ang, d0_off, slip, slip_dir, d_off):
    """one vertex against the rod (a, b, ap, bp, R).  x_prev: at parameter s0 of the previous segment (s0 < 0 or > 1: over that cap, tilted beyond the end),
    at the angle `ang` about the axis from straight up, with gap d0 = eps + d0_off.  x: the rod's material point carried along, plus a slip of length
    `slip` in the tangent plane of n0 (slip_dir: angle in that plane from the axis direction), plus the multiple of n0 that makes d = eps + d_off."""
    e0 = bp - ap
    u0 = _unit(e0)
    side = _unit(np.cross(u0, [0.0, 0.0, 1.0]))
    up = np.cross(side, u0)
    rad = np.cos(ang) * up + np.sin(ang) * side
    t0 = min(max(s0, 0.0), 1.0)
    c0 = ap + t0 * e0
    out = (s0 - t0) * np.linalg.norm(e0)                   # how far beyond the end, along the axis
    n0 = _unit(rad * np.sqrt(max(0.0, 1.0 - (out / (R + EPS)) ** 2)) + u0 * out / (R + EPS)) if out else rad
    xp = c0 + (R + EPS + d0_off) * n0
    P = cn.Pair(xp, xp, ap, bp, ap, bp, R, 0.0, K, EPS, EH)
    n0, t0 = P.n, P.t                                      # (as the restatement sees them)
    dc = (1.0 - t0) * (a - ap) + t0 * (b - bp)
    t1 = _unit(u0 - n0 * (n0 @ u0))
    t2 = np.cross(n0, t1)
    base = xp + dc + slip * (np.cos(slip_dir) * t1 + np.sin(slip_dir) * t2)
    gap = lambda al: cn.Pair(base + al * n0, xp, a, b, ap, bp, R, 0.0, K, EPS, EH).d - (EPS + d_off)
    lo, hi = -5e-3, 6e-3
    assert gap(lo) < 0 < gap(hi), (gap(lo), gap(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gap(mid) < 0 else (lo, mid)
    return xp, base + 0.5 * (lo + hi) * n0


def _case():
    """23 vertices against two moving rods.  Rod 0 (R 5 mm, mu 0.5, 40 mm long along x, top at z = 0) translates, yaws and changes its length a little
    over the step; rod 1 (R 4 mm, mu 0.3, along y, its top 0.8 mm higher) crosses it under the middle, so that vertices near the middle of rod 0 lie in both
    shells; its mask names two of them.  Vertices 0..11: over the barrel of rod 0 before and after, (d0 in / out) x (d in / out) x (slip 0, below eh, above eh).  12..15: over
    cap a and over cap b before and after, slip below and above eh.  16..19: the region changes in the step (large slip along the axis): barrel ->
    cap a, barrel -> cap b, cap a -> barrel, cap b -> barrel.  20: inside both shells with mask 0; 21: far outside; 22: sees rod 1 only."""
    rng = np.random.default_rng(11)
    R = np.array([0.005, 0.004])
    mu = np.array([0.5, 0.3])
    a = np.array([[-0.02, 0.0, -0.005], [4e-4, -0.015, -0.004 + 8e-4]])
    b = np.array([[0.02, 0.0, -0.005], [6e-4, 0.015, -0.004 + 8e-4]])
    ap = a - np.array([[2e-4, 1e-4, 3e-4], [-1e-4, 2e-4, 1e-4]])
    bp = b - np.array([[1e-4, -2e-4, 2e-4], [2e-4, 1e-4, -1e-4]])
    rod0 = (a[0], b[0], ap[0], bp[0], R[0])
    xp, x = np.zeros((23, 3)), np.zeros((23, 3))
    IN0, OUT0, IN, OUT = -1.2e-3, 1.1e-3, -1.1e-3, 1.3e-3
    q = 0
    for d0_off in (IN0, OUT0):
        for d_off in (IN, OUT):
            for slip in (0.0, 0.3 * EH, 3.0 * EH):
                xp[q], x[q] = _place(*rod0, rng.uniform(0.42, 0.6), rng.uniform(-0.05, 0.05), d0_off, slip, rng.uniform(0, 2 * np.pi), d_off)
                q += 1
    for s0 in (-0.03, 1.03):       # over a cap before and after: the slip across the axis
        for slip in (0.3 * EH, 3.0 * EH):
            xp[q], x[q] = _place(*rod0, s0, rng.uniform(-0.05, 0.05), IN0, slip, 0.5 * np.pi, IN)
            q += 1
    for s0, along in ((0.03, np.pi), (0.97, 0.0), (-0.03, 0.0), (1.03, np.pi)):   # the region changes: 3 eh of slip along the axis is 0.075 in s
        xp[q], x[q] = _place(*rod0, s0, rng.uniform(-0.05, 0.05), IN0, 3.0 * EH, along, IN)
        q += 1
    xp[20] = [0.0, 1e-4, 1e-3]; x[20] = [1e-4, 0.0, 0.8e-3]
    xp[21] = [0.0, 0.0, 0.05]; x[21] = [1e-3, 0.0, 0.051]
    xp[22], x[22] = _place(a[1], b[1], ap[1], bp[1], R[1], 0.8, 0.02, IN0, 0.5 * EH, 1.0, IN)
    mask = np.ones(23, np.uint8)
    mask[[0, 2, 21]] = 3   # (rod 1 acts where its own gaps keep away from eps as well: on two vertices inside both of its shells, and on the far one)
    mask[20] = 0; mask[22] = 2
    return a, b, ap, bp, R, mu, mask, xp, x


def _args():
    a, b, ap, bp, R, mu, mask, xp, x = _case()
    return (a, b, ap, bp, R, mu, mask, K, EPS, EH), xp, x


def test_the_case_walks_through_every_branch_and_keeps_away_from_the_boundaries():
    A, xp, x = _args()
    a, b, ap, bp, R, mu, mask = A[:7]
    act, act0, reg, reg0 = cn.active_sets(x, xp, *A)
    P = {(v, j): p for v, j, p in cn.pairs(x, xp, *A)}
    for ia in (True, False):   # d and d0 on either side of eps in every combination, over the barrel of rod 0
        for ib in (True, False):
            assert ((act[:12, 0] == ia) & (act0[:12, 0] == ib)).sum() == 3
    assert (reg[:12, 0] == 0).all() and (reg0[:12, 0] == 0).all()
    # the regions of (t0, t) that one step can produce: the same one three times, and the four changes between the barrel and a cap; among them a
    # vertex whose t is clamped while its t0 is not
    got = {(int(reg0[v, 0]), int(reg[v, 0])) for v in range(20)}
    assert got == {(0, 0), (-1, -1), (1, 1), (0, -1), (0, 1), (-1, 0), (1, 0)}, got
    assert all(act[v, 0] and act0[v, 0] for v in range(12, 20))
    r = np.array([[P[v, j].r if (v, j) in P else np.nan for j in range(2)] for v in range(23)])
    fr = act0 & (mu[None, :] > 0)
    assert (fr & (r < 1e-9)).any() and (fr & (r > 1e-9) & (r < EH)).any() and (fr & (r > EH)).any()   # r = 0, below and above eps_v dt with friction on
    for j in range(2):                                                     # both rods move, turn and change length
        assert np.abs(a[j] - ap[j]).min() > 0 and np.abs(b[j] - bp[j]).min() > 0 and np.abs((b[j] - bp[j]) - (a[j] - ap[j])).min() > 0
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any()    # two rods on one vertex
    Pm = cn.Pair(x[20], xp[20], a[0], b[0], ap[0], bp[0], R[0], mu[0], K, EPS, EH), cn.Pair(x[20], xp[20], a[1], b[1], ap[1], bp[1], R[1], mu[1], K, EPS, EH)
    assert mask[20] == 0 and Pm[0].act and Pm[1].act and not act[20].any()  # a masked-out vertex inside both shells
    assert mask[21] == 3 and not act[21].any() and not act0[21].any()       # a vertex far outside
    assert mask[22] == 2 and act[22, 1] and act0[22, 1]
    # no masked pair within AWAY of a boundary: the Hessian jumps there, and a difference across one measures nothing
    for (v, j), p in P.items():
        assert min(abs(p.s), abs(p.s - 1.0), abs(p.s0), abs(p.s0 - 1.0)) > AWAY, (v, j, p.s, p.s0)
        assert abs(p.d - EPS) > AWAY and abs(p.d0 - EPS) > AWAY, (v, j, p.d, p.d0)
        assert p.r < 1e-9 or abs(p.r - EH) > 1e-5, (v, j, p.r)


def _fd(f, z, h):
    """central differences of f (array-valued) in the entries of z: shape f.shape + z.shape"""
    z = np.asarray(z, np.float64)
    out = np.zeros(np.shape(f(z)) + z.shape)
    for idx in np.ndindex(*z.shape):
        e = np.zeros_like(z); e[idx] = h
        out[(Ellipsis,) + idx] = (np.asarray(f(z + e)) - np.asarray(f(z - e))) / (2 * h)
    return out


def test_restatement_matches_central_differences():
    """g against differences of E (step 1e-7), exact H against differences of g (step 1e-9: at r = 0 the gradient lam a1 w is only once differentiable
    and the difference is off by h / (2 eh) of that entry); bound 1e-6 of the largest entry.  The projected block is positive semi-definite; the exact
    H_n has the eigenvalues (k, 0, k (d - eps) / rho) over the barrel and (k, k (d - eps) / rho twice) over a cap.  Sensitivity: without in u u^T in
    the curvature the same comparison misses by more than ten times the bound."""
    A, xp, x = _args()
    NV = len(x)
    g = cn.gradient(x, xp, *A)
    H = cn.hessian(x, xp, *A)
    gd = _fd(lambda z: cn.energy(z, xp, *A), x, 1e-7)
    print("g vs dE:", np.abs(g - gd).max() / np.abs(g).max())
    assert np.abs(g - gd).max() <= BOUND * np.abs(g).max()
    Hd = _fd(lambda z: cn.gradient(z, xp, *A).reshape(-1), x, 1e-9).reshape(3 * NV, 3 * NV)
    print("H vs dg:", np.abs(H - Hd).max() / np.abs(H).max())
    assert np.abs(H - Hd).max() <= BOUND * np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    B, Bp = cn.blocks(x, xp, *A), cn.blocks(x, xp, *A, exact=False)
    assert np.array_equal(B[20], np.zeros((3, 3))) and np.array_equal(g[20], np.zeros(3)) and np.array_equal(B[21], np.zeros((3, 3)))
    assert min(np.linalg.eigvalsh(0.5 * (b + b.T)).min() for b in Bp) >= -1e-12 * K
    assert np.abs((B - Bp) - cn.curvature_blocks(x, xp, *A)).max() <= 1e-12 * K
    n_barrel = n_cap = 0
    for v, j, P in cn.pairs(x, xp, *A):
        if P.act:
            ev = np.linalg.eigvalsh(P.Hn(True))
            cr = K * (P.d - EPS) / P.rho
            want = sorted([K, 0.0, cr]) if P.inn else sorted([K, cr, cr])
            assert cr < 0 and np.abs(ev - want).max() <= 1e-9 * K, (v, j, ev, want)
            assert np.linalg.eigvalsh(P.Hn(False)).min() >= -1e-12 * K
            n_barrel += P.inn; n_cap += not P.inn
    assert n_barrel >= 6 and n_cap >= 4
    miss = np.abs(cn.hessian(x, xp, *A, drop="uu") - Hd).max() / np.abs(H).max()
    print("without in u u^T:", miss)
    assert miss > 10 * BOUND
    # the read-out: the forces of the rods sum to minus the gradient; the torque of a single pair about the midpoint
    F = cn.force(x, xp, *A)
    assert np.abs(F[:, 0:3].sum(axis=0) + g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max()
    one = np.zeros(NV, np.uint8); one[3] = 1
    F1 = cn.force(x, xp, *A[:6], one, *A[7:])
    assert np.abs(F1[0, 3:6] - np.cross(x[3] - 0.5 * (A[0][0] + A[1][0]), F1[0, 0:3])).max() <= 1e-15 and np.abs(F1[0]).min() > 0


def test_prev_terms_and_capsule_grad_match_differences_of_the_gradient():
    """the x_prev term (pos_grad[s-1] += -(dg / dx_prev)^T p) and the six column groups of capsule_grad (-p . dg/d(a, b, ap, bp, mu, R) over the free
    dofs) against central differences of g; bound 1e-6 as above (g is linear in mu: any step).  The step is 1e-10: at r = 0 a central difference of lam a1 w is off by
    h / (2 eh) of its entry, and the columns add that error over the r = 0 vertices (measured: d/da off by 1.1e-6, 2.8e-7, 1.1e-7 at h = 1e-9, 2.5e-10,
    1e-10, linear in h as a kink of the difference is and an error of the formula is not); the rounding of g, 1e-15 / 2h against entries of 1e4, stays
    at 1e-9.  Sensitivity: each of phi' tau n^T,
    Delta dt0^T and the tau0 n0^T part of dn0/dap is deleted in turn and the miss printed; each is more than ten times the bound."""
    (a, b, ap, bp, R, mu, mask, k, eps, eh), xp, x = _args()
    NV = len(x)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[2] = 1; frozen[4, 1] = 1; frozen[17, 2] = 1
    free = (frozen == 0).astype(np.float64)
    pf = (p * free).reshape(-1)
    grad = lambda xp_=xp, a_=a, b_=b, ap_=ap, bp_=bp, R_=R, mu_=mu: cn.gradient(x, xp_, a_, b_, ap_, bp_, R_, mu_, mask, k, eps, eh).reshape(-1)
    h = 1e-10
    J = _fd(lambda z: grad(xp_=z), xp, h).reshape(3 * NV, 3 * NV)
    want = (-(J.T @ pf)).reshape(-1, 3) * free
    T = (a, b, ap, bp, R, mu, mask, k, eps, eh)
    got = cn.backprop_prev(x, xp, p, frozen, *T)
    print("prev terms:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    assert np.array_equal(got[frozen == 1], np.zeros(int(frozen.sum()))) and np.array_equal(got[20], np.zeros(3))
    G = cn.capsule_grad(x, xp, p, frozen, *T)
    Gd = np.zeros_like(G)
    Gd[:, 0:3] = -(pf @ _fd(lambda z: grad(a_=z), a, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 3:6] = -(pf @ _fd(lambda z: grad(b_=z), b, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 6:9] = -(pf @ _fd(lambda z: grad(ap_=z), ap, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 9:12] = -(pf @ _fd(lambda z: grad(bp_=z), bp, h).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 12] = -(pf @ _fd(lambda z: grad(mu_=z), mu, 0.01))
    Gd[:, 13] = -(pf @ _fd(lambda z: grad(R_=z), R, h))
    groups = ((0, 3, "a"), (3, 6, "b"), (6, 9, "ap"), (9, 12, "bp"), (12, 13, "mu"), (13, 14, "R"))
    for lo, hi, name in groups:
        err = np.abs(G[:, lo:hi] - Gd[:, lo:hi]).max() / np.abs(G[:, lo:hi]).max()
        print(f"capsule_grad d/d{name}: {err:.3e}")
        assert err <= BOUND
    assert np.abs(G).min() > 0
    # the three derivatives in x, a, b sum to zero, and so do those in x_prev, ap, bp, pair by pair (g depends on differences only)
    for v, j, P in cn.pairs(x, xp, *T):
        scale = max(np.abs(P.Hn()).max(), np.abs(P.lam * P.M()).max(), 1e-300)
        assert np.abs(P.Hn() + P.lam * P.M() + P.dg_da() + P.dg_db()).max() <= 1e-12 * scale
        assert np.abs(P.dg_dxp() + P.dg_dap() + P.dg_dbp()).max() <= 1e-9 * max(np.abs(P.dg_dxp()).max(), 1e-300)
    # sensitivity: the miss of the column groups (and of the x_prev term) with one term deleted
    for drop, cols in (("tau_n", (0, 6)), ("delta_dt0", (6, 12)), ("tau0_n0", (6, 12))):
        Gx = cn.capsule_grad(x, xp, p, frozen, *T, drop=drop)
        miss = max(np.abs(Gx[:, lo:hi] - Gd[:, lo:hi]).max() / np.abs(G[:, lo:hi]).max() for lo, hi, _ in groups if cols[0] <= lo < cols[1])
        print(f"without {drop}: capsule_grad misses by {miss:.3e}")
        assert miss > 10 * BOUND
    miss = np.abs(cn.backprop_prev(x, xp, p, frozen, *T, drop="delta_dt0") - want).max() / np.abs(want).max()
    print(f"without delta_dt0: the x_prev term misses by {miss:.3e}")
    assert miss > 10 * BOUND


def test_degenerate_pairs_contribute_what_the_model_says():
    """rho < 1e-12: nothing; rho0 < 1e-12: the normal term alone"""
    (a, b, ap, bp, R, mu, mask, k, eps, eh), xp, x = _args()
    T = (a, b, ap, bp, R, mu)
    m1 = np.array([1], np.uint8)
    mid, mid0 = 0.5 * (a[0] + b[0]), 0.5 * (ap[0] + bp[0])
    x1 = np.array([mid]); xp1 = np.array([mid0 + [0.0, 0.0, R[0]]])
    assert cn.energy(x1, xp1, *T, m1, k, eps, eh) == 0.0 and not cn.blocks(x1, xp1, *T, m1, k, eps, eh).any()
    x2 = np.array([mid + [0.0, 0.0, R[0]]]); xp2 = np.array([ap[0]])
    P = cn.Pair(x2[0], xp2[0], a[0], b[0], ap[0], bp[0], R[0], mu[0], k, eps, eh)
    assert P.ok and not P.fric and P.lam == 0.0
    assert np.array_equal(cn.gradient(x2, xp2, *T, m1, k, eps, eh)[0], k * (P.d - eps) * P.n)
    assert not cn.backprop_prev(x2, xp2, np.ones((1, 3)), np.zeros((1, 3)), *T, m1, k, eps, eh).any()
    assert not cn.capsule_grad(x2, xp2, np.ones((1, 3)), np.zeros((1, 3)), *T, m1, k, eps, eh)[0, 6:13].any()


def _nums(line):
    return np.array(line.split(":", 1)[1].split(), np.float64)


def test_host_module_under_sanitizers_table_and_refusals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "capsule_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "capsule_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _nums(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    # the table: a, b, previous endpoints = endpoints, radii, mu; the scalars are left alone
    A, B = got["a"].reshape(-1, 3), got["b"].reshape(-1, 3)
    tab = got["table"].reshape(-1, 14)
    assert got["scalars"].tolist() == [3.0, 7.0, 0.5, 0.25] and len(tab) == 3
    assert np.array_equal(tab[:, 0:3], A) and np.array_equal(tab[:, 3:6], B) and np.array_equal(tab[:, 6:9], A) and np.array_equal(tab[:, 9:12], B)
    assert np.array_equal(tab[:, 12], got["radii"]) and np.array_equal(tab[:, 13], got["mu"])
    moved = got["table_moved"].reshape(-1, 14)
    for lo, name in ((0, "moved_a"), (3, "moved_b"), (6, "moved_ap"), (9, "moved_bp")):
        assert np.array_equal(moved[:, lo:lo + 3], got[name].reshape(-1, 3))
    assert moved[1, 5] == 0.125 and moved[2, 9] == -0.75 and np.array_equal(moved[:, 12:], tab[:, 12:])
    rest = got["table_at_rest"].reshape(-1, 14)
    assert np.array_equal(rest[:, 0:6], moved[:, 0:6]) and np.array_equal(rest[:, 6:12], moved[:, 0:6]) and np.array_equal(rest[:, 12:], tab[:, 12:])
    assert got["eight"][0] == 8 and got["empty"][0] == 0 and got["kept"][0] == 1
    assert got["mask_all"].tolist() == [7.0] * 20 and got["mask_eight"].tolist() == [255.0] * 20
    want = [5.0] * 20; want[7] = 0.0; want[9] = 2.0
    assert got["mask_given"].tolist() == want
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"endpoint a \(nan, 0, 1\) of capsule 1 is not finite", r"endpoint b \(1, inf, 1\) of capsule 1 is not finite", r"endpoint a \(0, 0, -inf\) of capsule 1 is not finite",
              r"segment of capsule 1 is 0 m long: at least 1e-09 m", r"segment of capsule 1 is 5e-10 m long: at least 1e-09 m",
              r"radius 0 of capsule 1 is not finite and positive", r"radius -0.1 of capsule 1 is not finite and positive", r"radius nan of capsule 1 is not finite and positive",
              r"radius inf of capsule 1 is not finite and positive", r"friction coefficient -0.5 of capsule 1 is negative or not finite",
              r"friction coefficient nan of capsule 1 is negative or not finite", r"friction coefficient inf of capsule 1 is negative or not finite",
              r"9 capsules: at most 8", r"n = -1 is negative", r"endpoint a \(0.01, nan, 0.03\) of capsule 1 is not finite",
              r"segment of capsule 1 is 0 m long: at least 1e-09 m", r"previous endpoint b \(4, 0.5, inf\) of capsule 2 is not finite",
              r"previous segment of capsule 2 is 0 m long: at least 1e-09 m", r"previous endpoints a without previous endpoints b",
              r"previous endpoints b without previous endpoints a", r"mask 0x08 of vertex 9 names a capsule at or above 3"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_scene_rod_the_checks_speak_the_library_s_words_and_the_tapes_have_capsule_rows():
    import torch
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_capsules
    from thinshelllab_amd.task_scene.Scene_rod import Scene
    s = Scene(N=8, device="cpu")
    s.init_all()
    assert s.tot_NV == 81 and s.elastic_cnt == 0 and s.n_capsule == 1 and s.k_capsule > 0 and s.contact_pairs() == []
    e0 = np.array([[[-0.0135, 0.0, -0.005], [0.0135, 0.0, -0.005]]])
    assert np.allclose(s._cap_e, e0, rtol=0, atol=1e-15) and np.array_equal(s._cap_ep, s._cap_e) and s._cap_mask.tolist() == [1] * 81
    assert int(s.frozen.to_numpy().sum()) == 12 and s.centre_vertex() == 40
    # the rod is shorter than the sheet's side: the middle row has vertices over the barrel and, 0.3 of a spacing from each end, over both caps
    xs = s.pos.to_numpy()[np.abs(s.pos.to_numpy()[:, 1]) < 1e-12, 0]
    sx = (xs - s._cap_e[0, 0, 0]) / (s._cap_e[0, 1, 0] - s._cap_e[0, 0, 0])
    dx = 0.04 / 8
    assert ((sx > 0) & (sx < 1)).sum() == 5 and np.isclose(np.abs(xs[sx < 0]).min() - 0.0135, 0.3 * dx) and np.isclose(np.abs(xs[sx > 1]).min() - 0.0135, 0.3 * dx)
    t = Scene(N=4, device="cpu")
    t.init_all()
    t.set_capsules([[-0.01, 0.0, -0.01], [0.01, 0.0, -0.02]], [[0.01, 0.0, -0.01], [0.01, 0.01, -0.02]], [0.01, 0.02], [0.5, 0.0], 1e3)
    c0 = t._cap_e.copy()
    for G in (Grad, GradSys):
        t.set_capsule_ends(c0[:, 0], c0[:, 1], prev_a=c0[:, 0], prev_b=c0[:, 1])
        t._cap_ep_step = c0.copy()
        g = G(t, 4, 0)
        assert tuple(g.capsule_ends.t.shape) == (4, 2, 2, 3) and tuple(g.capsule_ends_prev.t.shape) == (4, 2, 2, 3) and tuple(g.capsule_grad.t.shape) == (4, 2, 14)
        g.copy_pos(t, 0)
        for f in range(1, 4):   # what a completed step does to the endpoints, without the step
            e = c0 + 0.001 * f
            t.set_capsule_ends(e[:, 0], e[:, 1])
            t._capsules_step_done()
            g.copy_pos(t, f)
        assert np.array_equal(g.capsule_ends.t.numpy(), c0[None] + 0.001 * np.arange(4)[:, None, None, None])
        assert np.array_equal(g.capsule_ends_prev.t[1:].numpy(), g.capsule_ends.t[:-1].numpy()) and np.array_equal(g.capsule_ends_prev.t[0].numpy(), c0)
        # capsule_end_grad: row s = capsule_grad[s, :, 0:6] + capsule_grad[s + 1, :, 6:12]
        g.capsule_grad.t.copy_(torch.arange(4 * 2 * 14, dtype=torch.float64).reshape(4, 2, 14))
        eg = g.capsule_end_grad()
        cg = g.capsule_grad.t
        assert tuple(eg.shape) == (4, 2, 2, 3) and torch.equal(eg[:3].reshape(3, 2, 6), cg[:3, :, 0:6] + cg[1:, :, 6:12]) and torch.equal(eg[3].reshape(2, 6), cg[3, :, 0:6])
        g.capsule_ends_prev.t[2, 1, 1, 0] += 1e-6   # a rod that was put somewhere else between two steps
        with pytest.raises(ValueError, match=r"capsule_end_grad: the previous endpoints of step 2 are not the endpoints of step 1"):
            g.capsule_end_grad()
        g.reset()
        assert not g.capsule_grad.t.any() and not g.capsule_ends.t.any()
    assert "capsule_ends" in t._dirty or "capsules" in t._dirty
    # the host checks: the messages of csrc/capsule_host.hpp behind "set_capsules: "
    o, o1 = [0.0, 0.0, -1.0], [1.0, 0.0, -1.0]
    keep = s._cap_e.copy()
    for args, kw, pat in ((([[np.nan, 0.0, 0.0]], [o1], [1.0], [0.1]), {}, r"set_capsules: endpoint a \(nan, 0, 0\) of capsule 0 is not finite"),
                          (([o], [[0.0, np.inf, 0.0]], [1.0], [0.1]), {}, r"set_capsules: endpoint b \(0, inf, 0\) of capsule 0 is not finite"),
                          (([o, o], [o1, [0.0, 5e-10, -1.0]], [1.0, 1.0], [0.1, 0.1]), {}, r"set_capsules: segment of capsule 1 is 5e-10 m long: at least 1e-09 m"),
                          (([o], [o1], [0.0], [0.1]), {}, r"set_capsules: radius 0 of capsule 0 is not finite and positive"),
                          (([o, o], [o1, o1], [1.0, np.inf], [0.1, 0.1]), {}, r"set_capsules: radius inf of capsule 1 is not finite and positive"),
                          (([o, o], [o1, o1], [1.0, 1.0], [0.1, -1.0]), {}, r"set_capsules: friction coefficient -1 of capsule 1 is negative or not finite"),
                          (([o] * 9, [o1] * 9, [1.0] * 9, [0.0] * 9), {}, r"set_capsules: 9 capsules: at most 8"),
                          (([o, o], [o1, o1], [1.0, 1.0], [0.1, 0.1]), {"vertex_ids": [[0, 1], [3, 81]]}, r"set_capsules: vertex 81 of capsule 1 out of range \[0, 81\)")):
        with pytest.raises(ValueError, match=pat):
            validate_capsules(s.tot_NV, *args, **kw)
        with pytest.raises(ValueError, match=pat):
            s.set_capsules(*args, 1e4, **kw)
        assert s.n_capsule == 1 and np.array_equal(s._cap_e, keep)
    with pytest.raises(ValueError, match="k_capsule must be finite and >= 0"):
        s.set_capsules([o], [o1], [1.0], [0.1], -1.0)
    with pytest.raises(ValueError, match=r"set_capsule_ends: endpoint a \(0, inf, 0\) of capsule 0 is not finite"):
        s.set_capsule_ends([[0.0, np.inf, 0.0]], [o1])
    with pytest.raises(ValueError, match=r"set_capsule_ends: segment of capsule 0 is 0 m long: at least 1e-09 m"):
        s.set_capsule_ends([o], [o])
    with pytest.raises(ValueError, match=r"set_capsule_ends: previous endpoint b \(nan, 0, 0\) of capsule 0 is not finite"):
        s.set_capsule_ends([o], [o1], prev_a=[o], prev_b=[[np.nan, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"set_capsule_ends: previous segment of capsule 0 is 0 m long: at least 1e-09 m"):
        s.set_capsule_ends([o], [o1], prev_a=[o1], prev_b=[o1])
    with pytest.raises(ValueError, match=r"set_capsule_ends: previous endpoints a without previous endpoints b"):
        s.set_capsule_ends([o], [o1], prev_a=[o])
    with pytest.raises(ValueError, match=r"set_capsule_ends: 2 endpoints a and 2 endpoints b for 1 capsules"):
        s.set_capsule_ends([o, o], [o1, o1])
    assert np.array_equal(s._cap_e, keep) and np.array_equal(s._cap_ep, keep)
    a, b, r, mu, mask = validate_capsules(25, [o, o], [o1, o1], [0.5, 1.0], [0.0, 2.0], vertex_ids=[None, [3, 4]])
    assert mask.tolist() == [1, 1, 1, 3, 3] + [1] * 20 and r.tolist() == [0.5, 1.0]
    s.set_capsules(np.zeros((8, 3)), np.ones((8, 3)), np.ones(8), np.zeros(8), 1.0)
    assert s.n_capsule == 8 and s._cap_mask.tolist() == [255] * 81
    s.set_capsules([], [], [], [], 0.0)
    assert s.n_capsule == 0
