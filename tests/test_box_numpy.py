"""Rounded-box colliders on the CPU: the NumPy restatement tests/box_numpy.py against central differences of its own energy and
gradient, through every branch (face, edge and corner for the closest point at x and at x_prev, a vertex that crosses an edge line in the step, d
and d0 on either side of eps, the three slip regimes, two boxes on one vertex, mask 0), with the sensitivity of every check to the terms a sphere
does not have; the two limits, a box with half extents (L/2, 0, 0) against tests/capsule_numpy.py and one with (0, 0, 0) against
tests/sphere_numpy.py; csrc/box_host.hpp compiled into a stand-alone program under -fsanitize=address,undefined (tests/native/box_ref.cpp) --
every refusal names its offender, nine boxes are refused and eight accepted, a refused list or update leaves the old one in place, the matrices
are the restatement's --; and the scene layer on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import box_numpy as bn
import capsule_numpy as cn
import sphere_numpy as sn

HERE = os.path.dirname(os.path.abspath(__file__))

K, EPS, EH = 1.0e4, 2.0e-3, 1.0e-3
BOUND = 1e-6   # of the largest entry: the bound of the capsule, sphere, collider and frame restatements
AWAY = 2e-5    # metres: no pair closer than this to a face plane of the core box (|y_i| = h_i), to d = eps or to d0 = eps

IN0, OUT0, IN, OUT = -1.2e-3, 1.1e-3, -1.1e-3, 1.3e-3


def _case():
    """31 vertices against two moving, turning boxes.  Box 0 (half extents 20 x 15 x 4 mm, r 5 mm, mu 0.5) translates by a few tenths of a millimetre
    and turns by a few milliradians over the step; box 1 (mu 0.3) is a smaller plate that lies askew inside box 0's top, its own top 0.8 mm higher, so
    that vertices over the middle of box 0 lie in both shells; its mask names three of them.  Vertices 0..11: over the top face of box 0 before and
    after, (d0 in / out) x (d in / out) x (slip 0, below eh, above eh).  12..15: over an edge, then over a corner, before and after, slip below and
    above eh.  16..21: the region changes in the step (3 eh of slip across a face plane of the core box): face -> edge, edge -> face, edge ->
    corner, corner -> edge, face -> edge with d0 outside (no friction, a normal term on the edge), edge -> face likewise.  22..25: the other faces:
    bottom, -x, +y, -y.  26: inside both shells with mask 0; 27: far outside; 28: sees box 1 only; 29: inside the core of box 1, deeper than r; 30: the +x face."""
    rng = np.random.default_rng(11)
    h = np.array([[0.02, 0.015, 0.004], [0.006, 0.004, 0.002]])
    r = np.array([0.005, 0.003])
    mu = np.array([0.5, 0.3])
    R = np.array([bn.quat_to_R([0.98, 0.05, -0.08, 0.12]), bn.quat_to_R([0.9, -0.1, 0.05, 0.4])])
    c = np.array([[0.001, -0.002, -0.009], [0.0, 0.0, 0.0]])
    c[1] = c[0] + R[0] @ np.array([0.0012, -0.0007, h[0, 2] + r[0] - h[1, 2] - r[1] + 8e-4])
    R[1] = R[0] @ bn.rot([0.0, 0.0, 0.3])
    cp = c - np.array([[2e-4, 1e-4, 3e-4], [-1e-4, 2e-4, 1e-4]])
    R0 = np.array([bn.rot([-6e-3, 4e-3, -8e-3]) @ R[0], bn.rot([5e-3, -7e-3, 3e-3]) @ R[1]])
    box0 = (c[0], R[0], cp[0], R0[0], h[0], r[0], K, EPS, EH)
    hx, hy, hz = h[0]
    xp, x = np.zeros((31, 3)), np.zeros((31, 3))
    q = 0
    for d0_off in (IN0, OUT0):
        for d_off in (IN, OUT):
            for slip in (0.0, 0.3 * EH, 3.0 * EH):
                y0 = [rng.uniform(-0.004, 0.004) + 0.009, rng.uniform(-0.005, 0.005), hz]
                xp[q], x[q] = bn.place(*box0, y0, [0, 0, 1], d0_off, slip, rng.uniform(0, 2 * np.pi), d_off)
                q += 1
    for slip in (0.3 * EH, 3.0 * EH):       # over the edge (+x, +z), the slip along it
        xp[q], x[q] = bn.place(*box0, [hx, rng.uniform(-0.005, 0.005), hz], [np.cos(0.7), 0, np.sin(0.7)], IN0, slip, 0.0, IN)
        q += 1
    for slip in (0.3 * EH, 1.5 * EH):       # over the corner (+x, -y, +z)
        xp[q], x[q] = bn.place(*box0, [hx, -hy, hz], [1.0, -0.9, 1.1], IN0, slip, rng.uniform(0, 2 * np.pi), IN)
        q += 1
    cross = (([hx - 1.5e-3, 0.003, hz], [0, 0, 1], IN0, 0.0),                  # face -> edge: 3 mm along +x
             ([hx, -0.004, hz], [0.26, 0, 0.966], IN0, 0.5 * np.pi),           # edge -> face: 3 mm along -x
             ([hx, hy - 1.5e-3, hz], [1, 0, 1], IN0, 0.0),                     # edge -> corner: 3 mm along +y
             ([hx, hy, hz], [1, 0.25, 1], IN0, np.pi),                         # corner -> edge: 3 mm along -y
             ([hx - 1.5e-3, -0.002, hz], [0, 0, 1], OUT0, 0.0),
             ([hx, 0.006, hz], [0.26, 0, 0.966], OUT0, 0.5 * np.pi))
    for y0, nl, d0_off, along in cross:
        xp[q], x[q] = bn.place(*box0, y0, nl, d0_off, 3.0 * EH, along, IN)
        q += 1
    for y0, nl in (([0.003, 0.002, -hz], [0, 0, -1]), ([-hx, 0.004, 0.001], [-1, 0, 0]), ([-0.006, hy, -0.002], [0, 1, 0]), ([0.011, -hy, 0.0015], [0, -1, 0])):
        xp[q], x[q] = bn.place(*box0, y0, nl, IN0, 0.6 * EH, rng.uniform(0, 2 * np.pi), IN)
        q += 1
    assert q == 26
    top = c[0] + R[0] @ np.array([0.001, 0.0005, hz + r[0]])
    xp[26] = top + [0.0, 1e-4, 1e-3]; x[26] = top + [1e-4, 0.0, 1.2e-3]
    xp[27] = c[0] + [0.0, 0.0, 0.08]; x[27] = c[0] + [1e-3, 0.0, 0.081]
    xp[28], x[28] = bn.place(c[1], R[1], cp[1], R0[1], h[1], r[1], K, EPS, EH, [0.004, -0.001, h[1, 2]], [0, 0, 1], IN0, 0.5 * EH, 1.0, IN)
    xp[29] = cp[1] + R0[1] @ np.array([0.001, 0.001, 0.0005]); x[29] = c[1] + R[1] @ np.array([0.0015, 0.001, 0.0004])
    xp[30], x[30] = bn.place(*box0, [hx, 0.007, -0.001], [1, 0, 0], IN0, 0.6 * EH, 2.0, IN)
    mask = np.ones(31, np.uint8)
    mask[[0, 2, 27]] = 3   # (box 1 acts where its own gaps keep away from eps as well: on vertices inside both shells, and on the far one)
    mask[26] = 0; mask[28] = 2; mask[29] = 2
    return c, R, cp, R0, h, r, mu, mask, xp, x


def _args():
    c, R, cp, R0, h, r, mu, mask, xp, x = _case()
    return (c, R, cp, R0, h, r, mu, mask, K, EPS, EH), xp, x


def branches(A, xp, x, nv_face=12):
    """the assertions on a case: shared with tests/test_gpu_boxes.py, whose pushed vertices must walk through the same branches"""
    c, R, cp, R0, h, r, mu, mask, k, eps, eh = A
    act, act0, reg, reg0 = bn.active_sets(x, xp, *A)
    P = {(v, j): p for v, j, p in bn.pairs(x, xp, *A)}
    for ia in (True, False):   # d and d0 on either side of eps in every combination, over a face of box 0
        for ib in (True, False):
            assert ((act[:nv_face, 0] == ia) & (act0[:nv_face, 0] == ib)).sum() == nv_face // 4
    assert (reg[:nv_face, 0] == 2).all() and (reg0[:nv_face, 0] == 2).all()
    # the regions (free axes at x_prev, at x) that one step can produce: face, edge and corner kept, and the changes across an edge line of the
    # core box in both directions -- free different from free0
    got = {(int(reg0[v, 0]), int(reg[v, 0])) for v in range(len(x)) if reg[v, 0] != 9}
    assert got >= {(2, 2), (1, 1), (0, 0), (2, 1), (1, 2), (1, 0), (0, 1)}, got
    fr = act0 & (mu[None, :] > 0)
    for kind in (2, 1, 0):     # face, edge and corner, each with a normal force and with friction
        assert (act[:, 0] & (reg[:, 0] == kind)).any() and (fr[:, 0] & (reg0[:, 0] == kind)).any(), kind
    assert any(p.act and not p.act0 and p.region()[0] != p.region()[1] for p in P.values())   # a normal term alone on a pair that changed its region
    rw = np.array([[P[v, j].r_w if (v, j) in P else np.nan for j in range(len(r))] for v in range(len(x))])
    assert (fr & (rw < 1e-9)).any() and (fr & (rw > 1e-9) & (rw < eh)).any() and (fr & (rw > eh)).any()   # r_w = 0, below and above eps_v dt with friction on
    for j in range(len(r)):    # every box moves and turns
        assert np.abs(c[j] - cp[j]).min() > 0 and np.abs(R[j] - R0[j]).max() > 1e-4
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any()    # two boxes on one vertex
    return act, act0, reg, reg0, P


def test_the_case_walks_through_every_branch_and_keeps_away_from_the_boundaries():
    A, xp, x = _args()
    c, R, cp, R0, h, r, mu, mask = A[:8]
    act, act0, reg, reg0, P = branches(A, xp, x)
    assert {(int(reg0[v, 0]), int(reg[v, 0])) for v in range(26)} == {(2, 2), (1, 1), (0, 0), (2, 1), (1, 2), (1, 0), (0, 1)}
    assert all(act[v, 0] and act0[v, 0] for v in range(12, 20)) and all(act[v, 0] and not act0[v, 0] for v in (20, 21))
    # every face of the core box of box 0 carries a vertex
    faces = {(int(np.flatnonzero(~p.free)[0]), float(np.sign(p.y[~p.free][0]))) for (v, j), p in P.items() if j == 0 and p.region()[0] == 2}
    assert len(faces) == 6, faces
    Pm = [bn.Pair(x[26], xp[26], c[j], R[j], cp[j], R0[j], h[j], r[j], mu[j], K, EPS, EH) for j in range(2)]
    assert mask[26] == 0 and Pm[0].act and Pm[1].act and not act[26].any()  # a masked-out vertex inside both shells
    assert mask[27] == 3 and not act[27].any() and not act0[27].any()       # a vertex far outside
    assert mask[28] == 2 and act[28, 1] and act0[28, 1]
    assert mask[29] == 2 and (29, 1) not in P                               # inside the core box: rho = 0, the pair contributes nothing
    # no masked pair within AWAY of a boundary: the Hessian jumps there, and a difference across one measures nothing
    for (v, j), p in P.items():
        assert np.abs(np.abs(p.y) - h[j]).min() > AWAY and np.abs(np.abs(p.y0) - h[j]).min() > AWAY, (v, j, p.y, p.y0)
        assert abs(p.d - EPS) > AWAY and abs(p.d0 - EPS) > AWAY, (v, j, p.d, p.d0)
        assert p.r_w < 1e-9 or abs(p.r_w - EH) > 1e-5, (v, j, p.r_w)


def _fd(f, z, h):
    """central differences of f (array-valued) in the entries of z: shape f.shape + z.shape"""
    z = np.asarray(z, np.float64)
    out = np.zeros(np.shape(f(z)) + z.shape)
    for idx in np.ndindex(*z.shape):
        e = np.zeros_like(z); e[idx] = h
        out[(Ellipsis,) + idx] = (np.asarray(f(z + e)) - np.asarray(f(z - e))) / (2 * h)
    return out


def test_restatement_matches_central_differences():
    """g against differences of E (step 1e-7), exact H against differences of g (step 1e-9: at r_w = 0 the gradient lam a1 w is only once
    differentiable and the difference is off by h / (2 eh) of that entry); bound 1e-6 of the largest entry, as the rods'.  The projected block is
    positive semi-definite; the exact H_n has the eigenvalues (k, 0, 0) on a face, (k, 0, k (d - eps) / rho) on an edge and (k, k (d - eps) / rho
    twice) at a corner.  Sensitivity: without sum free u u^T in the curvature the same comparison misses by more than ten times the bound."""
    A, xp, x = _args()
    NV = len(x)
    g = bn.gradient(x, xp, *A)
    H = bn.hessian(x, xp, *A)
    gd = _fd(lambda z: bn.energy(z, xp, *A), x, 1e-7)
    print("g vs dE:", np.abs(g - gd).max() / np.abs(g).max())
    assert np.abs(g - gd).max() <= BOUND * np.abs(g).max()
    Hd = _fd(lambda z: bn.gradient(z, xp, *A).reshape(-1), x, 1e-9).reshape(3 * NV, 3 * NV)
    print("H vs dg:", np.abs(H - Hd).max() / np.abs(H).max())
    assert np.abs(H - Hd).max() <= BOUND * np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    B, Bp = bn.blocks(x, xp, *A), bn.blocks(x, xp, *A, exact=False)
    for v in (26, 27, 29):
        assert np.array_equal(B[v], np.zeros((3, 3))) and np.array_equal(g[v], np.zeros(3))
    assert min(np.linalg.eigvalsh(0.5 * (b + b.T)).min() for b in Bp) >= -1e-12 * K
    assert np.abs((B - Bp) - bn.curvature_blocks(x, xp, *A)).max() <= 1e-12 * K
    count = {0: 0, 1: 0, 2: 0}
    for v, j, P in bn.pairs(x, xp, *A):
        if P.act:
            ev = np.linalg.eigvalsh(P.Hn(True))
            cr = K * (P.d - EPS) / P.rho
            nf = P.region()[0]
            want = sorted([K] + [0.0] * nf + [cr] * (2 - nf))
            assert cr < 0 and np.abs(ev - want).max() <= 1e-9 * K, (v, j, ev, want)
            assert np.linalg.eigvalsh(P.Hn(False)).min() >= -1e-12 * K
            count[nf] += 1
    assert count[2] >= 6 and count[1] >= 4 and count[0] >= 3, count
    miss = np.abs(bn.hessian(x, xp, *A, drop="free") - Hd).max() / np.abs(H).max()
    print("without sum free u u^T:", miss)
    assert miss > 10 * BOUND
    # the read-out: the forces of the boxes sum to minus the gradient; the torque of a single pair about the centre
    F = bn.force(x, xp, *A)
    assert np.abs(F[:, 0:3].sum(axis=0) + g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max()
    one = np.zeros(NV, np.uint8); one[3] = 1
    F1 = bn.force(x, xp, *A[:7], one, *A[8:])
    assert np.abs(F1[0, 3:6] - np.cross(x[3] - A[0][0], F1[0, 0:3])).max() <= 1e-15 and np.abs(F1[0]).min() > 0


def test_prev_terms_and_box_grad_match_differences_of_the_gradient():
    """the x_prev term (pos_grad[s-1] += -(dg / dx_prev)^T p) and the six column groups of box_grad (-p . dg/d(c, theta, cp, theta_p, mu, r) over the
    free dofs) against central differences of g; theta and theta_p are world-frame rotation vectors on the left of R and R0.  Bound 1e-6 as above
    (g is linear in mu: any step).  The step is 1e-10, as the rods': at r_w = 0 a central difference of lam a1 w is off by h / (2 eh) of its entry,
    and the columns add that error over the r_w = 0 vertices; the rounding of g, 1e-15 / 2h against entries of 1e4, stays at 1e-9.  A rotation
    vector takes the step 4e-9 rad, the second step size: it moves a point of box 0 (at most 25 mm from the centre) by the same 1e-10 m, where
    1e-10 rad would move it by 2.5e-12 m and leave the rounding of g forty times larger in the difference (measured: 1.2e-6).  Sensitivity: each of Delta, the turn of n0 with the previous pose and the (R b0) x .
    term of d/dtheta is deleted in turn and the miss printed; each is more than ten times the bound."""
    (c, R, cp, R0, h, r, mu, mask, k, eps, eh), xp, x = _args()
    NV, nb = len(x), len(r)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((NV, 3))
    frozen = np.zeros((NV, 3), np.int32); frozen[2] = 1; frozen[4, 1] = 1; frozen[17, 2] = 1
    free = (frozen == 0).astype(np.float64)
    pf = (p * free).reshape(-1)
    turned = lambda th, M: np.array([bn.rot(th[j]) @ M[j] for j in range(nb)])
    grad = lambda xp_=xp, c_=c, R_=R, cp_=cp, R0_=R0, r_=r, mu_=mu: bn.gradient(x, xp_, c_, R_, cp_, R0_, h, r_, mu_, mask, k, eps, eh).reshape(-1)
    hs, hr = 1e-10, 4e-9
    J = _fd(lambda z: grad(xp_=z), xp, hs).reshape(3 * NV, 3 * NV)
    want = (-(J.T @ pf)).reshape(-1, 3) * free
    T = (c, R, cp, R0, h, r, mu, mask, k, eps, eh)
    got = bn.backprop_prev(x, xp, p, frozen, *T)
    print("prev terms:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    assert np.array_equal(got[frozen == 1], np.zeros(int(frozen.sum()))) and np.array_equal(got[26], np.zeros(3))
    G = bn.box_grad(x, xp, p, frozen, *T)
    Gd = np.zeros_like(G)
    z3 = np.zeros((nb, 3))
    Gd[:, 0:3] = -(pf @ _fd(lambda z: grad(c_=z), c, hs).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 3:6] = -(pf @ _fd(lambda z: grad(R_=turned(z, R)), z3, hr).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 6:9] = -(pf @ _fd(lambda z: grad(cp_=z), cp, hs).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 9:12] = -(pf @ _fd(lambda z: grad(R0_=turned(z, R0)), z3, hr).reshape(3 * NV, -1)).reshape(-1, 3)
    Gd[:, 12] = -(pf @ _fd(lambda z: grad(mu_=z), mu, 0.01))
    Gd[:, 13] = -(pf @ _fd(lambda z: grad(r_=z), r, hs))
    groups = ((0, 3, "c"), (3, 6, "theta"), (6, 9, "cp"), (9, 12, "theta_p"), (12, 13, "mu"), (13, 14, "r"))
    for lo, hi, name in groups:
        err = np.abs(G[:, lo:hi] - Gd[:, lo:hi]).max() / np.abs(G[:, lo:hi]).max()
        print(f"box_grad d/d{name}: {err:.3e}")
        assert err <= BOUND
    assert np.abs(G).min() > 0
    # g depends on x - c and on x_prev - cp only: the derivatives in x and c sum to zero, and so do those in x_prev and cp, pair by pair
    for v, j, P in bn.pairs(x, xp, *T):
        assert np.array_equal(P.Hn() + P.lam * P.M(), -P.dg_dc()) and np.array_equal(P.dg_dxp(), -P.dg_dcp())
    # sensitivity: the miss of the column groups (and of the x_prev term) with one term deleted
    for drop, cols in (("delta", (6, 12)), ("spin_n0", (9, 12)), ("arm", (3, 6))):
        Gx = bn.box_grad(x, xp, p, frozen, *T, drop=drop)
        miss = max(np.abs(Gx[:, lo:hi] - Gd[:, lo:hi]).max() / np.abs(G[:, lo:hi]).max() for lo, hi, _ in groups if cols[0] <= lo < cols[1])
        print(f"without {drop}: box_grad misses by {miss:.3e}")
        assert miss > 10 * BOUND
    miss = np.abs(bn.backprop_prev(x, xp, p, frozen, *T, drop="delta") - want).max() / np.abs(want).max()
    print(f"without delta: the x_prev term misses by {miss:.3e}")
    assert miss > 10 * BOUND


def test_degenerate_pairs_contribute_what_the_model_says():
    """rho < 1e-12 (inside the core box): nothing; rho0 < 1e-12: the normal term alone; an axis with h_i = 0 is never free"""
    (c, R, cp, R0, h, r, mu, mask, k, eps, eh), xp, x = _args()
    T = (c, R, cp, R0, h, r, mu)
    m1 = np.array([1], np.uint8)
    inside, inside0 = c[0] + R[0] @ (0.5 * h[0]), cp[0] + R0[0] @ (0.5 * h[0])
    above = c[0] + R[0] @ np.array([0.0, 0.0, h[0, 2] + r[0]])
    x1 = np.array([inside]); xp1 = np.array([cp[0] + R0[0] @ np.array([0.0, 0.0, h[0, 2] + r[0]])])
    assert bn.energy(x1, xp1, *T, m1, k, eps, eh) == 0.0 and not bn.blocks(x1, xp1, *T, m1, k, eps, eh).any()
    assert not bn.box_grad(x1, xp1, np.ones((1, 3)), np.zeros((1, 3)), *T, m1, k, eps, eh).any()
    x2 = np.array([above]); xp2 = np.array([inside0])
    P = bn.Pair(x2[0], xp2[0], c[0], R[0], cp[0], R0[0], h[0], r[0], mu[0], k, eps, eh)
    assert P.ok and not P.fric and P.lam == 0.0 and P.region() == (2, 3)
    assert np.array_equal(bn.gradient(x2, xp2, *T, m1, k, eps, eh)[0], k * (P.d - eps) * P.n)
    assert not bn.backprop_prev(x2, xp2, np.ones((1, 3)), np.zeros((1, 3)), *T, m1, k, eps, eh).any()
    assert not bn.box_grad(x2, xp2, np.ones((1, 3)), np.zeros((1, 3)), *T, m1, k, eps, eh)[0, 6:13].any()
    flat = bn.Pair(np.array([0.001, 0.0, 0.004]), xp2[0], np.zeros(3), np.eye(3), cp[0], R0[0], np.array([0.02, 0.0, 0.0]), r[0], 0.0, k, eps, eh)
    assert flat.free.tolist() == [True, False, False] and flat.y[1] == 0.0 and flat.region()[0] == 1


# ------------------------------------------------------------------------------------------------ the two limits
def _limit_case(n_v=14):
    """vertices around a box that moves and turns, near enough to be in its shell, some outside; p and a frozen pattern"""
    rng = np.random.default_rng(5)
    L, rad, mu = 0.03, 0.005, 0.4
    R = bn.quat_to_R([0.9, 0.2, -0.3, 0.1])
    c = np.array([0.002, -0.001, 0.003])
    R0 = bn.rot([4e-3, -6e-3, 5e-3]) @ R
    cp = c - np.array([2e-4, -1e-4, 3e-4])
    s = rng.uniform(-0.75, 0.75, n_v) * L
    ang = rng.uniform(0, 2 * np.pi, n_v)
    dist = rad + EPS + rng.uniform(-1.5e-3, 1.0e-3, n_v)
    side = np.cos(ang)[:, None] * R0[:, 1] + np.sin(ang)[:, None] * R0[:, 2]
    xp = cp + s[:, None] * R0[:, 0] + dist[:, None] * side
    x = xp + (c - cp) + rng.uniform(-1, 1, (n_v, 3)) * np.array([1.2e-3, 1.2e-3, 4e-4])
    p = rng.standard_normal((n_v, 3))
    frozen = np.zeros((n_v, 3), np.int32); frozen[1] = 1; frozen[5, 2] = 1
    return L, rad, mu, c, R, cp, R0, xp, x, p, frozen


def test_a_box_with_half_extents_L2_0_0_is_the_rod():
    """energy, gradient, both Hessians, the x_prev term, force and torque equal capsule_numpy's for a = c - (L/2) u, b = c + (L/2) u; the pose gradients
    are the endpoint gradients: g_c = g_a + g_b, g_th = (L/2) u x (g_b - g_a), likewise for the previous pose; mu and r as they are.  The two
    restatements form the same numbers along different routes: 1e-9 of the largest entry (the lagged columns divide by rho0 and by e0 . e0)."""
    L, rad, mu, c, R, cp, R0, xp, x, p, frozen = _limit_case()
    m = np.ones(len(x), np.uint8)
    u, u0 = R[:, 0], R0[:, 0]
    a, b, ap, bp = c - 0.5 * L * u, c + 0.5 * L * u, cp - 0.5 * L * u0, cp + 0.5 * L * u0
    B = (c[None], R[None], cp[None], R0[None], np.array([[0.5 * L, 0.0, 0.0]]), np.array([rad]), np.array([mu]), m, K, EPS, EH)
    C = (a[None], b[None], ap[None], bp[None], np.array([rad]), np.array([mu]), m, K, EPS, EH)
    act, act0, reg, reg0 = bn.active_sets(x, xp, *B)
    assert act.any() and (~act).any() and act0.any() and (~act0).any() and set(reg[:, 0]) == {0, 1} and set(reg0[:, 0]) == {0, 1}
    close = lambda got, want, tol=1e-9: np.abs(np.asarray(got) - np.asarray(want)).max() <= tol * np.abs(want).max()
    assert abs(bn.energy(x, xp, *B) - cn.energy(x, xp, *C)) <= 1e-12 * cn.energy(x, xp, *C)
    assert close(bn.gradient(x, xp, *B), cn.gradient(x, xp, *C), 1e-12)
    assert close(bn.blocks(x, xp, *B), cn.blocks(x, xp, *C), 1e-12) and close(bn.blocks(x, xp, *B, exact=False), cn.blocks(x, xp, *C, exact=False), 1e-12)
    assert close(bn.backprop_prev(x, xp, p, frozen, *B), cn.backprop_prev(x, xp, p, frozen, *C))
    assert close(bn.force(x, xp, *B), cn.force(x, xp, *C), 1e-12)       # (the rod's midpoint is the box's centre)
    Gb, Gc = bn.box_grad(x, xp, p, frozen, *B)[0], cn.capsule_grad(x, xp, p, frozen, *C)[0]
    assert close(Gb[0:3], Gc[0:3] + Gc[3:6]) and close(Gb[3:6], 0.5 * L * np.cross(u, Gc[3:6] - Gc[0:3]))
    assert close(Gb[6:9], Gc[6:9] + Gc[9:12]) and close(Gb[9:12], 0.5 * L * np.cross(u0, Gc[9:12] - Gc[6:9]))
    assert close(Gb[12:14], Gc[12:14]) and np.abs(Gb).min() > 0


def test_a_box_with_half_extents_zero_is_the_ball():
    L, rad, mu, c, R, cp, R0, xp, x, p, frozen = _limit_case()
    rng = np.random.default_rng(8)
    nrm = rng.standard_normal((len(x), 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    xp = cp + nrm * (rad + EPS + rng.uniform(-1.5e-3, 1.0e-3, len(x)))[:, None]
    x = xp + (c - cp) + rng.uniform(-1, 1, (len(x), 3)) * 8e-4
    m = np.ones(len(x), np.uint8)
    B = (c[None], R[None], cp[None], R0[None], np.zeros((1, 3)), np.array([rad]), np.array([mu]), m, K, EPS, EH)
    S = (c[None], cp[None], np.array([rad]), np.array([mu]), m, K, EPS, EH)
    act, act0, reg, reg0 = bn.active_sets(x, xp, *B)
    assert act.any() and (~act).any() and act0.any() and (~act0).any() and set(reg[:, 0]) == {0} and set(reg0[:, 0]) == {0}
    close = lambda got, want, tol=1e-12: np.abs(np.asarray(got) - np.asarray(want)).max() <= tol * np.abs(want).max()
    assert abs(bn.energy(x, xp, *B) - sn.energy(x, xp, *S)) <= 1e-12 * sn.energy(x, xp, *S)
    assert close(bn.gradient(x, xp, *B), sn.gradient(x, xp, *S))
    assert close(bn.blocks(x, xp, *B), sn.blocks(x, xp, *S)) and close(bn.blocks(x, xp, *B, exact=False), sn.blocks(x, xp, *S, exact=False))
    assert close(bn.backprop_prev(x, xp, p, frozen, *B), sn.backprop_prev(x, xp, p, frozen, *S), 1e-9)
    assert close(bn.force(x, xp, *B)[:, 0:3], sn.force(x, xp, *S))
    Gb, Gs = bn.box_grad(x, xp, p, frozen, *B)[0], sn.sphere_grad(x, xp, p, frozen, *S)[0]
    assert close(Gb[0:3], Gs[0:3], 1e-9) and close(Gb[6:9], Gs[3:6], 1e-9) and close(Gb[12:14], Gs[6:8], 1e-9)
    # a ball does not feel its orientation, now or at the start of the step
    assert np.abs(Gb[3:6]).max() <= 1e-9 * np.abs(Gb[0:3]).max() * rad and np.abs(Gb[9:12]).max() <= 1e-9 * np.abs(Gb[6:9]).max() * rad


def _nums(line):
    return np.array(line.split(":", 1)[1].split(), np.float64)


def test_host_module_under_sanitizers_table_and_refusals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "box_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "box_ref.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _nums(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    # the table: c, R of the normalised quaternion, previous pose = pose, half extents, radii, mu; the scalars are left alone
    Cn, Q = got["centres"].reshape(-1, 3), got["quats"].reshape(-1, 4)
    tab = got["table"].reshape(-1, 29)
    assert got["scalars"].tolist() == [3.0, 7.0, 0.5, 0.25] and len(tab) == 3
    Rm = np.array([bn.quat_to_R(q).reshape(-1) for q in Q])
    assert np.array_equal(tab[:, 0:3], Cn) and np.array_equal(tab[:, 12:15], Cn) and np.array_equal(tab[:, 15:24], tab[:, 3:12])
    assert np.abs(tab[:, 3:12] - Rm).max() <= 4e-16   # (the same formula; a compiler may contract a product into a sum on one side)
    for j in range(3):
        M = tab[j, 3:12].reshape(3, 3)
        assert np.abs(M.T @ M - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(M) - 1.0) <= 1e-15
    assert np.array_equal(tab[:, 24:27], got["half"].reshape(-1, 3)) and np.array_equal(tab[:, 27], got["radii"]) and np.array_equal(tab[:, 28], got["mu"])
    moved = got["table_moved"].reshape(-1, 29)
    assert np.array_equal(moved[:, 0:3], got["moved_c"].reshape(-1, 3)) and np.array_equal(moved[:, 12:15], got["moved_cp"].reshape(-1, 3))
    assert np.abs(moved[:, 3:12] - np.array([bn.quat_to_R(q).reshape(-1) for q in got["moved_q"].reshape(-1, 4)])).max() <= 4e-16
    assert np.abs(moved[:, 15:24] - np.array([bn.quat_to_R(q).reshape(-1) for q in got["moved_qp"].reshape(-1, 4)])).max() <= 4e-16
    assert moved[1, 2] == 0.125 and moved[2, 14] == -0.75 and np.array_equal(moved[:, 24:], tab[:, 24:])
    assert not np.array_equal(moved[1, 3:12], tab[1, 3:12]) and not np.array_equal(moved[0, 15:24], tab[0, 15:24])
    rest = got["table_at_rest"].reshape(-1, 29)
    assert np.array_equal(rest[:, 0:12], moved[:, 0:12]) and np.array_equal(rest[:, 12:24], moved[:, 0:12]) and np.array_equal(rest[:, 24:], tab[:, 24:])
    assert got["eight"][0] == 8 and got["empty"][0] == 0 and got["kept"][0] == 1
    assert got["mask_all"].tolist() == [7.0] * 20
    want = [5.0] * 20; want[7] = 0.0; want[9] = 2.0
    assert got["mask_given"].tolist() == want
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"centre \(nan, 0, 1\) of box 1 is not finite", r"centre \(0, -inf, 1\) of box 1 is not finite",
              r"quaternion \(0, 0, 0, 0\) of box 1 is zero or not finite", r"quaternion \(1, nan, 0, 0\) of box 1 is zero or not finite",
              r"quaternion \(1, 0, inf, 0\) of box 1 is zero or not finite",
              r"half extents \(1, -0.5, 1\) of box 1 are negative or not finite", r"half extents \(1, 1, nan\) of box 1 are negative or not finite",
              r"half extents \(inf, 1, 1\) of box 1 are negative or not finite",
              r"radius 0 of box 1 is not finite and positive", r"radius -0.1 of box 1 is not finite and positive", r"radius nan of box 1 is not finite and positive",
              r"radius inf of box 1 is not finite and positive", r"friction coefficient -0.5 of box 1 is negative or not finite",
              r"friction coefficient nan of box 1 is negative or not finite", r"friction coefficient inf of box 1 is negative or not finite",
              r"9 boxes: at most 8", r"n = -1 is negative", r"null centres, null quaternions, null half extents, null radii or null friction coefficients",
              r"centre \(0.01, nan, 0.03\) of box 1 is not finite", r"quaternion \(0, 0, 0, 0\) of box 1 is zero or not finite",
              r"previous centre \(-3, 0.5, inf\) of box 2 is not finite", r"previous quaternion \(2, 0.2, nan, 0.6\) of box 0 is zero or not finite",
              r"previous centres without previous quaternions", r"previous quaternions without previous centres",
              r"mask 0x08 of vertex 9 names a box at or above 3"]
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)


# ------------------------------------------------------------------------------------------------ the scene layer on the host
def test_scene_table_the_checks_speak_the_library_s_words_and_the_tapes_have_box_rows():
    import torch
    from thinshelllab_amd.engine import frames
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.engine.BaseScene import validate_boxes
    from thinshelllab_amd.task_scene.Scene_table import Scene
    s = Scene(N=8, device="cpu")
    s.init_all()
    assert s.tot_NV == 81 and s.elastic_cnt == 0 and s.n_box == 1 and s.k_box > 0 and s.contact_pairs() == []
    assert np.array_equal(s._box_cp, s._box_c) and np.array_equal(s._box_qp, s._box_q) and s._box_mask.tolist() == [1] * 81
    assert int(s.frozen.to_numpy().sum()) == 6 and s.centre_vertex() == 40
    # the sheet against the plate: vertices over the face, over the long edge (0.3 of a spacing inside it: the middle column) and over two corners
    X = s.pos.to_numpy()
    c0, q0, h0, r0, mu0 = s.plate()
    A = (c0, np.array([bn.quat_to_R(q0[0])]), c0, np.array([bn.quat_to_R(q0[0])]), h0, r0, mu0, s._box_mask, s.k_box, s.eps_contact, s.eps_v * s.dt)
    act, act0, reg, reg0 = bn.active_sets(X, X, *A)
    assert {2, 1, 0} <= set(reg[:, 0].tolist()) and (reg[:, 0] == 2).sum() >= 20 and (reg[:, 0] == 1).sum() >= 9
    assert abs(X[s.hanging_vertex(), 0] - 0.02) < 1e-12 and abs(X[s.hanging_vertex(), 1]) < 1e-12
    t = Scene(N=4, device="cpu")
    t.init_all()
    t.set_boxes([[-0.01, 0.0, -0.01], [0.01, 0.0, -0.02]], [[2.0, 0.0, 0.0, 0.0], [1.0, 0.1, 0.0, 0.0]], [[0.01, 0.01, 0.001], [0.01, 0.0, 0.0]], [0.01, 0.02], [0.5, 0.0], 1e3)
    assert np.array_equal(t._box_q[0], [1.0, 0.0, 0.0, 0.0]) and abs(np.linalg.norm(t._box_q[1]) - 1.0) < 1e-15
    c0, q0 = t._box_c.copy(), t._box_q.copy()
    for G in (Grad, GradSys):
        t.set_box_poses(c0, q0, prev_centres=c0, prev_quats=q0)
        t._box_cp_step, t._box_qp_step = c0.copy(), q0.copy()
        g = G(t, 4, 0)
        assert tuple(g.box_poses.t.shape) == (4, 2, 7) and tuple(g.box_poses_prev.t.shape) == (4, 2, 7) and tuple(g.box_grad.t.shape) == (4, 2, 14)
        g.copy_pos(t, 0)
        for f in range(1, 4):   # what a completed step does to the poses, without the step
            t.move_boxes(np.full((2, 3), 0.001), np.array([[0.0, 0.0, 0.01], [0.02, 0.0, 0.0]]))
            t._boxes_step_done()
            g.copy_pos(t, f)
        P = g.box_poses.t.numpy()
        assert np.allclose(P[:, :, 0:3], c0[None] + 0.001 * np.arange(4)[:, None, None], rtol=0, atol=1e-15)
        want = frames.quat_mul(frames.quat_exp([0.0, 0.0, 0.03]), q0[0])
        assert np.abs(P[3, 0, 3:7] - want).max() <= 1e-15 and np.abs(np.linalg.norm(P[:, :, 3:7], axis=2) - 1.0).max() <= 1e-15
        assert np.array_equal(g.box_poses_prev.t[1:].numpy(), g.box_poses.t[:-1].numpy()) and np.array_equal(g.box_poses_prev.t[0, :, 0:3].numpy(), c0)
        # box_pose_grad: row s = box_grad[s, :, 0:6] + box_grad[s + 1, :, 6:12]
        g.box_grad.t.copy_(torch.arange(4 * 2 * 14, dtype=torch.float64).reshape(4, 2, 14))
        eg = g.box_pose_grad()
        cg = g.box_grad.t
        assert tuple(eg.shape) == (4, 2, 6) and torch.equal(eg[:3], cg[:3, :, 0:6] + cg[1:, :, 6:12]) and torch.equal(eg[3], cg[3, :, 0:6])
        g.box_poses_prev.t[2, 1, 4] += 1e-6   # a box that was turned between two steps
        with pytest.raises(ValueError, match=r"box_pose_grad: the previous poses of step 2 are not the poses of step 1"):
            g.box_pose_grad()
        g.reset()
        assert not g.box_grad.t.any() and not g.box_poses.t.any()
    assert "box_poses" in t._dirty or "boxes" in t._dirty
    # the host checks: the messages of csrc/box_host.hpp behind "set_boxes: "
    o, q1, hh = [0.0, 0.0, -1.0], [1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0]
    keep_c, keep_q = s._box_c.copy(), s._box_q.copy()
    for args, kw, pat in ((([[np.nan, 0.0, 0.0]], [q1], [hh], [1.0], [0.1]), {}, r"set_boxes: centre \(nan, 0, 0\) of box 0 is not finite"),
                          (([o], [[0.0, 0.0, 0.0, 0.0]], [hh], [1.0], [0.1]), {}, r"set_boxes: quaternion \(0, 0, 0, 0\) of box 0 is zero or not finite"),
                          (([o, o], [q1, [1.0, np.inf, 0.0, 0.0]], [hh, hh], [1.0, 1.0], [0.1, 0.1]), {}, r"set_boxes: quaternion \(1, inf, 0, 0\) of box 1 is zero or not finite"),
                          (([o, o], [q1, q1], [hh, [1.0, -0.5, 1.0]], [1.0, 1.0], [0.1, 0.1]), {}, r"set_boxes: half extents \(1, -0.5, 1\) of box 1 are negative or not finite"),
                          (([o], [q1], [hh], [0.0], [0.1]), {}, r"set_boxes: radius 0 of box 0 is not finite and positive"),
                          (([o, o], [q1, q1], [hh, hh], [1.0, np.inf], [0.1, 0.1]), {}, r"set_boxes: radius inf of box 1 is not finite and positive"),
                          (([o, o], [q1, q1], [hh, hh], [1.0, 1.0], [0.1, -1.0]), {}, r"set_boxes: friction coefficient -1 of box 1 is negative or not finite"),
                          (([o] * 9, [q1] * 9, [hh] * 9, [1.0] * 9, [0.0] * 9), {}, r"set_boxes: 9 boxes: at most 8"),
                          (([o, o], [q1, q1], [hh, hh], [1.0, 1.0], [0.1, 0.1]), {"vertex_ids": [[0, 1], [3, 81]]}, r"set_boxes: vertex 81 of box 1 out of range \[0, 81\)")):
        with pytest.raises(ValueError, match=pat):
            validate_boxes(s.tot_NV, *args, **kw)
        with pytest.raises(ValueError, match=pat):
            s.set_boxes(*args, 1e4, **kw)
        assert s.n_box == 1 and np.array_equal(s._box_c, keep_c) and np.array_equal(s._box_q, keep_q)
    with pytest.raises(ValueError, match="k_box must be finite and >= 0"):
        s.set_boxes([o], [q1], [hh], [1.0], [0.1], -1.0)
    with pytest.raises(ValueError, match=r"set_box_poses: centre \(0, inf, 0\) of box 0 is not finite"):
        s.set_box_poses([[0.0, np.inf, 0.0]], [q1])
    with pytest.raises(ValueError, match=r"set_box_poses: quaternion \(0, 0, 0, 0\) of box 0 is zero or not finite"):
        s.set_box_poses([o], [[0.0, 0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"set_box_poses: previous centre \(nan, 0, 0\) of box 0 is not finite"):
        s.set_box_poses([o], [q1], prev_centres=[[np.nan, 0.0, 0.0]], prev_quats=[q1])
    with pytest.raises(ValueError, match=r"set_box_poses: previous quaternion \(0, nan, 0, 0\) of box 0 is zero or not finite"):
        s.set_box_poses([o], [q1], prev_centres=[o], prev_quats=[[0.0, np.nan, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"set_box_poses: previous centres without previous quaternions"):
        s.set_box_poses([o], [q1], prev_centres=[o])
    with pytest.raises(ValueError, match=r"set_box_poses: 2 centres and 2 quaternions for 1 boxes"):
        s.set_box_poses([o, o], [q1, q1])
    with pytest.raises(ValueError, match=r"move_boxes: 2 translations and 1 rotation vectors for 1 boxes"):
        s.move_boxes([o, o], [o])
    assert np.array_equal(s._box_c, keep_c) and np.array_equal(s._box_cp, keep_c) and np.array_equal(s._box_q, keep_q)
    c, q, h, r, mu, mask = validate_boxes(25, [o, o], [q1, q1], [hh, hh], [0.5, 1.0], [0.0, 2.0], vertex_ids=[None, [3, 4]])
    assert mask.tolist() == [1, 1, 1, 3, 3] + [1] * 20 and r.tolist() == [0.5, 1.0]
    s.set_boxes(np.zeros((8, 3)), np.tile(q1, (8, 1)), np.ones((8, 3)), np.ones(8), np.zeros(8), 1.0)
    assert s.n_box == 8 and s._box_mask.tolist() == [255] * 81
    s.set_boxes([], [], [], [], [], 0.0)
    assert s.n_box == 0
