"""Sampled distance-field colliders (tsl_set_sdfs; csrc/k_sdf.hpp) through the C ABI.  The reference has no such term: it is checked
against the dense NumPy restatement (tests/sdf_numpy.py), the plane kernels where the field is a sampled plane, the sphere kernels where it is a
sampled ball (up to the smoothing of the spline), and whole-rollout differences.  The idiom is that of tests/test_gpu_boxes.py: a field quantity of
a state is the difference against the same state with k_sdf = 0 -- no field kernel runs there, and the rest is formed by the same launches in both
-- and K = 2e5 N/m, the size of the cloth's own diagonal entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_numpy as bn  # noqa: E402
import capsule_numpy as kn  # noqa: E402
import collider_numpy as cn  # noqa: E402
import handle_numpy as hn  # noqa: E402
import sdf_numpy as dn  # noqa: E402
import sphere_numpy as sn  # noqa: E402
import tie_numpy as tn  # noqa: E402
from thinshelllab_amd._lib import EXPORTS  # noqa: E402

assert "tsl_set_sdfs" in EXPORTS   # (without the feature the module does not import)

pytestmark = pytest.mark.gpu

K = 2.0e5
DX = 0.1 / 15
MU = np.array([0.5, 0.3])
QID = np.array([1.0, 0.0, 0.0, 0.0])
EZ = np.array([0.0, 0.0, 1.0])


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


class _State:
    """one state of a context: positions, start-of-step positions, zero velocity, rest angles; energy / gradient / operator of it as NumPy"""

    def __init__(self, ctx, x, xp, ref):
        self.ctx = ctx
        self.pos = _dev(x); self.prev = _dev(xp); self.vel = torch.zeros_like(self.pos)
        self.ref = ref

    def energy(self):
        return self.ctx.energy(self.pos, self.prev, self.vel, self.ref)

    def grad(self, spd=0):
        F = torch.zeros(self.pos.numel(), dtype=torch.float64, device="cuda")
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd, grad=F)
        return F.cpu().numpy().reshape(-1, 3)

    def operator(self, spd):
        """the full operator, dense: the static matrix plus the masked blocks of every constraint slot"""
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd)
        A = self.ctx.matrix_csr().toarray()
        if len(self.ctx.constraints()["idx"]):
            idx, blk = self.ctx.constraints()["idx"], self.ctx.contact_blocks(True)
            for c in range(len(blk)):
                d = np.concatenate([3 * v + np.arange(3) for v in idx[c]])
                A[np.ix_(d, d)] += blk[c]
        return A

    def part(self, fun, k=K, with_base=False, key="k_sdf"):
        """fun() with k_sdf = k minus fun() with k_sdf = 0 (with_base: and the latter)"""
        self.ctx.set_param(key, k)
        a = fun()
        self.ctx.set_param(key, 0.0)
        b = fun()
        self.ctx.set_param(key, k)
        return (a - b, b) if with_base else a - b


def _drape(N, pin=True, perturb=0.0, newton_cap=200):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=DX * N, N=N, M=N, pin_row=pin, perturb=perturb, newton_cap=newton_cap)
    s.init_all()
    return s


def _quat(theta, q=QID):
    from thinshelllab_amd.engine import frames
    return frames.quat_normalize(frames.quat_mul(frames.quat_exp(theta), q))


def _gap_draw(rng, eps):
    """a gap on either side of the shell, at least a quarter of it away from it: in (-0.5, 0.75) eps or in (1.25, 2.5) eps"""
    g = rng.uniform(-0.5, 2.0)
    return (g if g < 0.75 else g + 0.5) * eps


def noisy_ramp(dims, h, a, seed, noise=0.1):
    """samples of the ramp a . y about the middle of the valid region plus white noise of `noise` h, a tenth of the ramp's rise per cell: every
    sample distinct, the gradient never zero, a curvature everywhere"""
    a = np.asarray(a, np.float64) / np.linalg.norm(a)
    o = -0.5 * h * (np.array(dims) - 1.0)
    I, J, L = np.meshgrid(*(np.arange(n) for n in dims), indexing="ij")
    Y = o[None, None, None, :] + h * np.stack([I, J, L], axis=-1)
    return dn.Field(Y @ a + noise * h * np.random.default_rng(seed).standard_normal(dims), o, h)


def _newton(f, t=0.0, it=40):
    """t with f(t) = 0 for a function that rises at a rate near one"""
    for _ in range(it):
        t -= f(t)
    assert abs(f(t)) < 1e-15, f(t)
    return t


def placed(x0, sel, n_side, eps, eh, seed):
    """The vertices `sel` of a flat horizontal sheet (n_side cells of DX along x) against two moving, turning fields.
    Field 0: (22, 16, 6) samples at h = DX / 3, a ramp with noise whose level set phi = r + eps lies in the sheet, tilted against it by a hundredth; its
    valid region covers 7 x 5 vertices about the middle of the sheet, the outer ones in its boundary cells i = 1 and i = n - 3 of the axes 0 and 1; two
    vertices are carried into the boundary cells of axis 2 (one deep inside the solid, one far above it).  Each vertex gets gaps d0 and d on either
    side of the shell independently and a slip relative to the field's material point of 0, 0.3 or 3 eps_v dt; one is set on a cell face to within
    rounding.  Field 1: (4, 4, 4) -- one valid cell, which is the boundary cell i = 1 = n - 3 of every axis -- yawed by 0.4, two of its faces laid through
    the vertices A and B of one row: A is inside at x_prev and outside at x (friction alone), B the other way round (a normal term alone), the
    vertex M between them inside at both and also in field 0; a vertex far away sees both fields and is in neither grid.
    (fields, r, centres, quats, previous centres, previous quats, x_prev, x, mask, the vertices of field 0, (A, B, M, far))"""
    rng = np.random.default_rng(seed)
    x, xp = x0.copy(), x0.copy()
    xs, ys = np.unique(np.round(x0[sel, 0], 9)), np.unique(np.round(x0[sel, 1], 9))
    assert len(xs) == n_side + 1 and len(ys) == n_side + 1
    at = lambda i, j: int(sel[np.argmin(np.abs(x0[sel, 0] - xs[i]) + np.abs(x0[sel, 1] - ys[j]))])
    m = n_side // 2
    h = DX / 3.0
    r = np.array([5e-4, -2e-4])
    # field 0: tilted pose, the ramp's direction about the sheet's normal as the field sees it
    q = np.array([_quat([0.02, -0.03, 0.01]), _quat([0.05, 0.04, 0.4])])   # (field 0 nearly level: its valid region is three cells high)
    R = np.array([bn.quat_to_R(a) for a in q])
    a0 = R[0].T @ EZ + [0.01, -0.008, 0.0]
    F0 = noisy_ramp((22, 16, 6), h, a0, seed)
    a0 /= np.linalg.norm(a0)
    v_lo = at(m - 3, m - 2)
    y_lo = F0.o + h * np.array([1.5, 1.5, 0.0])
    y_lo[2] = (r[0] + eps - a0[0] * y_lo[0] - a0[1] * y_lo[1]) / a0[2]
    c = np.zeros((2, 3))
    c[0] = x0[v_lo] - R[0] @ y_lo
    # field 1: its cell's faces t_0 = 1 and t_0 = 2 through A and B
    A_, M_, B_ = at(m, m + 1), at(m + 1, m + 1), at(m + 2, m + 1)
    a1 = R[1].T @ EZ
    s_ab = float((R[1].T @ (x0[B_] - x0[A_]))[0])
    h1 = s_ab
    F1 = noisy_ramp((4, 4, 4), h1, a1, seed + 1)
    # (the cell is [-h1 / 2, h1 / 2)^3 in the field's frame: A at its face -h1 / 2, the level set phi = r + eps through the sheet's plane at M)
    c[1] = x0[A_] - R[1] @ np.array([-0.5 * h1, 0.3 * h1, 0.0])
    c[1] += EZ * (x0[M_, 2] - (c[1, 2] + (r[1] + eps)))
    cp = c - np.array([[0.4 * eh, 0.2 * eh, 0.6 * eh], [-0.2 * eh, 0.4 * eh, 0.2 * eh]])
    turn = np.array([[0.6, -0.8, 1.0], [-0.5, 0.7, 0.9]]) * (eh / 0.02)   # (a point 20 mm from the centre moves by about eps_v dt)
    qp = np.array([_quat(-turn[j], q[j]) for j in range(2)])
    R0 = np.array([bn.quat_to_R(a) for a in qp])
    F = [F0, F1]

    def put(v, j, g0, slip, ang, want):
        """vertex v against field j: x_prev over its place in the sheet with d0 = g0, x the material point carried along plus the slip plus d = want"""
        n_w = R0[j] @ (a0 if j == 0 else a1)
        t0 = _newton(lambda t: F[j].sample(R0[j].T @ (x0[v] + t * n_w - cp[j]))[0] - r[j] - g0)
        xp[v] = x0[v] + t0 * n_w
        y0 = R0[j].T @ (xp[v] - cp[j])
        n0 = R0[j] @ F[j].sample(y0)[1]; n0 /= np.linalg.norm(n0)
        t = np.array([np.cos(ang), np.sin(ang), 0.0]); t -= n0 * (n0 @ t); t /= np.linalg.norm(t)
        base = c[j] + R[j] @ y0 + slip * t
        al = _newton(lambda al: F[j].sample(R[j].T @ (base + al * n0 - c[j]))[0] - r[j] - want)
        x[v] = base + al * n0

    near = []
    for i in range(m - 3, m + 4):
        for jj in range(m - 2, m + 3):
            v = at(i, jj)
            near.append(v)
            put(v, 0, _gap_draw(rng, eps), rng.choice([0.0, 0.3 * eh, 3.0 * eh]), rng.uniform(0, 2 * np.pi), _gap_draw(rng, eps))
    # the first four of the list: one of each combination, whatever the draws gave the others
    for v, (g0, want, slip) in zip(near[:4], ((0.3 * eps, 0.2 * eps, 0.3 * eh), (0.4 * eps, 1.5 * eps, 3.0 * eh), (1.6 * eps, 0.5 * eps, 0.3 * eh), (1.7 * eps, 1.4 * eps, 0.0))):
        put(v, 0, g0, slip, 1.0, want)
    put(near[4], 0, 0.25 * eps, 0.0, 0.0, 0.3 * eps)           # (friction on, no slip: r_w = 0)
    # the boundary cells of axis 2: t_2 = 1.5 (deep inside the solid) and t_2 = 2.5 (far above the shell) at x and at x_prev
    for v, t2 in ((at(m - 1, m - 1), 1.5), (at(m + 1, m - 1), 2.5 + 1.0)):
        for arr, cc, RR in ((xp, cp[0], R0[0]), (x, c[0], R[0])):
            y = RR.T @ (x0[v] - cc)
            y[2] = F0.o[2] + h * t2
            arr[v] = cc + RR @ y
        x[v] += R[0] @ np.array([0.3 * eh, -0.2 * eh, 0.0])
    # on a cell face of axis 0 to within rounding, at x
    vf = at(m, m - 2)
    yf = R[0].T @ (x[vf] - c[0])
    yf[0] = F0.o[0] + h * np.round((yf[0] - F0.o[0]) / h)
    x[vf] = c[0] + R[0] @ yf
    # field 1
    put(M_, 1, 0.3 * eps, 0.3 * eh, 2.0, 0.25 * eps)
    z1 = lambda RR, cc, y, want: _newton(lambda t: F1.sample(y + t * EZ)[0] - r[1] - want)   # (along the local z: the other two coordinates stay)
    yA0 = np.array([-0.5 * h1 + 2e-5, 0.3 * h1, 0.0]); yA0 = yA0 + z1(R0[1], cp[1], yA0, 0.3 * eps) * EZ
    xp[A_] = cp[1] + R0[1] @ yA0
    x[A_] = c[1] + R[1] @ (yA0 + [-5e-5, 1e-5, 0.0])           # (3e-5 beyond the face: outside at x)
    yB = np.array([0.5 * h1 - 3e-5, float((R[1].T @ (x0[B_] - c[1]))[1]), 0.0]); yB = yB + z1(R[1], c[1], yB, 0.2 * eps) * EZ
    x[B_] = c[1] + R[1] @ yB
    xp[B_] = cp[1] + R0[1] @ (yB + [5e-5, 0.0, 1e-5])          # (2e-5 beyond the face: outside at x_prev)
    far = at(0, 0)
    mask = np.zeros(len(x0), np.uint8)
    mask[near] = 1
    mask[[near[7], near[20]]] = 0                               # (inside the grid, no field)
    mask[[A_, B_]] = 2
    mask[M_] = 3
    mask[far] = 3
    return F, r, c, q, cp, qp, xp, x, mask, np.array(near), (A_, B_, M_, far)


def _table(F, r, c, q, cp, qp, mask, eps, eh, mu=MU, k=K):
    """the arguments of the restatement behind (x, xp)"""
    return (F, c, np.array([bn.quat_to_R(a) for a in q]), cp, np.array([bn.quat_to_R(a) for a in qp]), r, mu, mask, k, eps, eh)


def branches(x, xp, A, special):
    """asserts that the state walks through every branch; returns the active set"""
    F, c, R, cp, R0, r, mu, mask, k, eps, eh = A
    A_, B_, M_, far = special
    val, val0, act, act0 = dn.active_sets(x, xp, *A)
    P = {(v, j): p for v, j, p in dn.pairs(x, xp, *A)}
    on = np.zeros(act.shape, bool)
    for v, j in P:
        on[v, j] = True
    fr = act0 & (mu[None, :] > 0)
    inside = on & val & val0
    for ia in (True, False):       # active with friction, active without, friction only, inactive: inside the grid at both points
        for ib in (True, False):
            assert (inside & (act == ia) & (act0 == ib)).any(), (ia, ib)
    rw = np.array([[P[v, j].r_w if (v, j) in P else np.nan for j in range(len(F))] for v in range(len(x))])
    assert (fr & (rw < 1e-9)).any() and (fr & (rw > 1e-9) & (rw < eh)).any() and (fr & (rw > eh)).any()
    # outside the valid region at x only, at x_prev only, at both
    assert not val[A_, 1] and val0[A_, 1] and P[A_, 1].lam > 0 and val[B_, 1] and act[B_, 1] and not val0[B_, 1]
    assert on[far].all() and not val[far].any() and not val0[far].any()
    assert act[M_].all() and fr[M_].all() and (mask == 0).any() and (on.sum(axis=1) == 1).any()       # two fields on one vertex
    # the boundary cells i = 1 and i = n - 3 of every axis of field 0, and the single cell of field 1
    cells = np.array([np.floor(F[0].coords(P[v, 0].y)) for v in range(len(x)) if (v, 0) in P and val[v, 0]])
    for a in range(3):
        assert (cells[:, a] == 1).any() and (cells[:, a] == F[0].dims[a] - 3).any(), a
    assert F[1].dims == (4, 4, 4) and len(set(F[0].dims)) == 3
    # a vertex on a cell face to within rounding; none nearer than 1e-9 h to the boundary of the valid region, where rounding would decide
    t_all = [(f.coords(pt), f) for (v, j), p in P.items() for pt, f in ((p.y, F[j]), (p.y0, F[j]))]
    assert any(np.abs(t - np.round(t)).min() < 1e-12 for t, f in t_all)
    for t, f in t_all:
        assert np.abs(np.concatenate([t - 1.0, t - (np.array(f.dims) - 2.0)])).min() > 1e-9, t
    for j in range(len(F)):
        assert np.abs(c[j] - cp[j]).min() > 0 and np.abs(R[j] - R0[j]).max() > 1e-4 and np.abs(R[j] - np.eye(3)).max() > 0.02
    # the premise of the 1e-12 bound: the rounding of the gathered sum against the smallest |d - eps| of an active pair
    gaps = min(min(abs(p.d - eps) if p.act else 1.0, abs(p.d0 - eps) if p.act0 else 1.0) for p in P.values())
    size = max(np.abs(f.s).max() for f in F)
    print("largest sample %.3e, smallest |d - eps| of an active pair %.3e m: e64 sample / |d - eps| = %.2e" % (size, gaps, 2.2e-16 * size / gaps))
    assert 2.2e-16 * size / gaps < 1e-12
    return act


def _frozen_pattern(fz0, touched):
    """on top of the scene's own frozen dofs: all dofs of one touched vertex, one dof of a second, two of a third"""
    fz = fz0.copy()
    v0, v1, v2 = touched[:3]
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


FORCE_GROUPS = ((0, 3), (3, 6))
GRAD_GROUPS = ((0, 3), (3, 6), (6, 9), (9, 12), (12, 13), (13, 14))


def _reverse_step(S, NV, n_ref, mass, dt, frozen):
    """One reverse step (step 2 of a tape of three states x_0 = x_1 = x_prev, x_2 = x) with a random right-hand side.  Returns (the adjoint solution p
    on its free dofs, the fields' share of pos_grad[1], sdf_grad of that solution).  k_adj_prev adds (1 + d) p m / dt^2 to pos_grad[1] and subtracts
    d p m / dt^2 from pos_grad[0] (d = 1, nothing else writes pos_grad[0], and with contact off only the fields write pos_grad[1] besides): p is
    read off pos_grad[0] with three roundings, and the fields' share is pos_grad[1] + 2 pos_grad[0] (the idiom of tests/test_gpu_wind.py)."""
    ctx = S.ctx
    pb = torch.stack([S.prev, S.prev, S.pos]).contiguous()
    pg = torch.zeros_like(pb)
    pg[2] = _dev(np.random.default_rng(6).normal(scale=1e-2, size=(NV, 3)))
    rb = torch.stack([S.ref[:n_ref].reshape(-1)] * 3).contiguous(); ag = torch.zeros_like(rb)
    tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
    st = ctx.adjoint_step(2, 3, pb, pg, rb, ag, tz, 1.0)
    assert st["flag"] != 3, st
    out = pg.cpu().numpy().reshape(3, NV, 3)
    free = frozen == 0
    p = np.where(free, -out[0] * (dt * dt) / mass[:, None], 0.0)
    assert not out[0][~free].any() and not out[1][~free].any()
    return p, out[1] + 2.0 * out[0], ctx.sdf_grad(S.pos, S.prev)


def _check_state(S, s, x, xp, A, fz_list, n_ref):
    """energy, gradient, operator in the spd modes 0, 1, 2 and with spd_literal, the read-outs and one reverse step of one state against the
    restatement.  Bound: 1e-12 of the largest field entry (of each column group for the read-outs), the boxes' bound."""
    ctx = S.ctx
    NV = len(x)
    mass = s.mass.to_numpy()
    assert ctx.sdf_count() == len(A[0])
    e_np, g_np = dn.energy(x, xp, *A), dn.gradient(x, xp, *A)
    H_ex, H_pr = dn.hessian(x, xp, *A, exact=True), dn.hessian(x, xp, *A, exact=False)
    B_np = dn.blocks(x, xp, *A)
    inside = np.zeros((3 * NV, 3 * NV), bool)
    for v in np.nonzero(np.abs(B_np).max(axis=(1, 2)) > 0)[0]:
        inside[3 * v:3 * v + 3, 3 * v:3 * v + 3] = True
    assert np.abs(H_ex - H_pr).max() > 1e-9 * np.abs(H_ex).max()          # (the curvature term is a thousand times over the bound)
    for frozen in fz_list:
        ctx.set_frozen(frozen.reshape(-1))
        fzb = frozen.astype(bool)
        free = (~fzb).ravel()
        e = S.part(S.energy)
        print("energy %.17g restatement %.17g rel %.2e" % (e, e_np, abs(e - e_np) / abs(e_np)))
        assert abs(e - e_np) <= 1e-12 * abs(e_np)
        g = S.part(S.grad)
        gm = g_np * ~fzb
        print("gradient err / max %.2e" % (np.abs(g - gm).max() / np.abs(gm).max()))
        assert np.abs(g - gm).max() <= 1e-12 * np.abs(gm).max() and (g[fzb] == 0).all()
        ff = np.outer(free, free)
        big = np.abs(H_ex * ff).max()
        got = {}
        for tag, spd, lit in (("spd 0", 0, 0), ("spd 1", 1, 0), ("spd 2", 2, 0), ("literal", 1, 1)):
            ctx.set_param("spd_literal", lit)
            D, Ab = S.part(lambda spd=spd: S.operator(spd), with_base=True)
            ctx.set_param("spd_literal", 0)
            Hm = (H_ex if spd == 0 else H_pr) * ff
            print("%s: operator err / largest field entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (tag, np.abs(D - Hm).max() / big, (D != D.T).sum(), (Ab != Ab.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * big
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (Ab == Ab.T)).any()
            got[tag] = (D, Ab)
        # spd 0 against spd 1: exactly the curvature term k (d - eps) R Hess phi R^T
        curv = H_ex - H_pr
        cb = dn.curvature_blocks(x, xp, *A)
        for v in range(NV):
            assert np.abs(curv[3 * v:3 * v + 3, 3 * v:3 * v + 3] - cb[v]).max() <= 1e-12 * big
        dc = (got["spd 0"][0] - got["spd 1"][0]) - curv * ff
        print("spd 0 - spd 1 against the curvature term: %.2e of the largest field entry (the term itself %.2e)" % (np.abs(dc).max() / big, np.abs(curv * ff).max() / big))
        assert np.abs(dc).max() <= 1e-12 * big
        for tag in ("spd 2", "literal"):   # the projected modes add the same numbers: the same bits wherever the rest of the operator has the same bits
            D1, A1 = got["spd 1"]; D2, A2 = got[tag]
            same = (A1 == A2) & inside
            assert (D1[same] == D2[same]).all() and np.abs(D1 - D2).max() <= 1e-12 * big
        # the read-outs (frozen dofs: not masked in the force, not counted in the gradients)
        fo, fo_np = ctx.sdf_force(S.pos, S.prev), dn.force(x, xp, *A)
        pn = np.random.default_rng(11).normal(size=(NV, 3))
        bg, bg_np = ctx.sdf_grad(S.pos, S.prev, _dev(pn.reshape(-1))), dn.sdf_grad(x, xp, pn, frozen, *A)
        assert fo.shape == fo_np.shape == (len(A[0]), 6) and bg.shape == bg_np.shape == (len(A[0]), 14)
        for lo, hi in FORCE_GROUPS:
            print("  sdf_force[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(fo - fo_np)[:, lo:hi].max() / np.abs(fo_np[:, lo:hi]).max()))
            assert np.abs(fo - fo_np)[:, lo:hi].max() <= 1e-12 * np.abs(fo_np[:, lo:hi]).max()
        for lo, hi in GRAD_GROUPS:
            print("  sdf_grad[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(bg - bg_np)[:, lo:hi].max() / np.abs(bg_np[:, lo:hi]).max()))
            assert np.abs(bg - bg_np)[:, lo:hi].max() <= 1e-12 * np.abs(bg_np[:, lo:hi]).max()
        assert np.abs(bg_np).min() > 0 and np.abs(fo_np).min() > 0


        # one reverse step: the fields' share of pos_grad[s-1], and the read-out of the step's own adjoint solution
        p, share, bg2 = _reverse_step(S, NV, n_ref, mass, s.dt, frozen)
        want = dn.backprop_prev(x, xp, p, frozen, *A)
        print("pos_grad[s-1] err / max %.2e (largest entry %.3e)" % (np.abs(share - want).max() / np.abs(want).max(), np.abs(want).max()))
        assert np.abs(share - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
        bg2_np = dn.sdf_grad(x, xp, p, frozen, *A)
        for lo, hi in GRAD_GROUPS:
            assert np.abs(bg2 - bg2_np)[:, lo:hi].max() <= 1e-12 * np.abs(bg2_np[:, lo:hi]).max()


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("N", [8, 20])
def test_bare_cloth_matches_the_restatement(N):
    """N = 8: the 9 x 9-vertex cloth on the single-stream path, two waves; N = 20: 441 vertices, two workgroups with a partial one, the placed vertices
    in both"""
    s = _drape(N)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    ctx.set_param("contact", 0)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    assert NV == (N + 1) ** 2 and ctx.contact_counts() == (0, 0)
    F, r, c, q, cp, qp, xp, x, mask, near, special = placed(s.pos.to_numpy(), np.arange(NV), N, eps, eh, seed=N)
    if N == 20:
        assert near.min() < 256 <= near.max()
    A = _table(F, r, c, q, cp, qp, mask, eps, eh)
    act = branches(x, xp, A, special)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    assert fz0.any()
    ctx.set_sdfs([f.s for f in F], [f.o for f in F], [f.h for f in F], c, q, r, MU, mask)
    ctx.set_sdf_poses(c, q, cp, qp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, s, x, xp, A, [fz0, _frozen_pattern(fz0, touched)], s.cloths[0].NF)
    # new poses alone: the table follows; without previous poses the fields are at rest
    ctx.set_frozen(fz0.reshape(-1))
    c2 = c + [[2e-5, 0.0, -4e-5], [0.0, 2e-5, 3e-5]]
    q2 = np.array([_quat([2e-4, -1e-4, 3e-4], q[0]), _quat([-1e-4, 2e-4, 1e-4], q[1])])
    e_old = dn.energy(x, xp, *A)
    for pc, pq, rc, rq in ((cp, qp, cp, qp), (None, None, c2, q2)):
        ctx.set_sdf_poses(c2, q2, pc, pq)
        e = S.part(S.energy)
        e_np = dn.energy(x, xp, *_table(F, r, c2, q2, rc, rq, mask, eps, eh))
        assert abs(e - e_np) <= 1e-12 * abs(e_np) and abs(e_np - e_old) > 1e-3 * abs(e_np)
    s._close_ctx()


def test_cloth_with_bodies_matches_the_restatement():
    """Scene_balancing with a 9 x 9-vertex cloth: bodies and contact pairs, so the assembly takes the three-stream schedule (assemble_enqueue_early)"""
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=DX * 8, cloth_N=8, cloth_M=8)
    s.init_all()
    ctx = s._ensure_ctx()
    ctx.set_param("tet_warm", 0)   # (two assemblies of one state differ in the last bits of the bodies' blocks otherwise; the differences ask for exact zeros)
    ctx.set_param("contact", 0)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    cl = s.cloths[0]
    assert cl.NV == 81 and ctx.n_body > 1
    NV = s.tot_NV
    cloth = np.arange(cl.offset, cl.offset + cl.NV)
    F, r, c, q, cp, qp, xp, x, mask, near, special = placed(s.pos.to_numpy(), cloth, 8, eps, eh, seed=5)   # (the bodies see no field)
    A = _table(F, r, c, q, cp, qp, mask, eps, eh)
    act = branches(x, xp, A, special)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_sdfs([f.s for f in F], [f.o for f in F], [f.h for f in F], c, q, r, MU, mask)
    ctx.set_sdf_poses(c, q, cp, qp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, s, x, xp, A, [fz0, _frozen_pattern(fz0, touched)], cl.NF)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ exact limits
def _jiggled(s, rng, amp):
    """the sheet's vertices moved by up to amp along z and a tenth of that sideways, at x and at x_prev independently"""
    x0 = s.pos.to_numpy()
    d = lambda: rng.uniform(-1.0, 1.0, x0.shape) * [0.1 * amp, 0.1 * amp, amp]
    return x0 + d(), x0 + d()


def _grid_about(fn, Y, h, margin):
    from thinshelllab_amd.engine import sdf
    return sdf.sample(fn, Y.min(axis=0) - margin, Y.max(axis=0) + margin, h)


def test_a_sampled_plane_in_a_rotated_pose_is_the_half_space():
    """phi = a . y sampled on a grid in a frame turned by 0.6 rad: the spline reproduces the plane, so energy, gradient, operator (spd 0 and 1) and
    the net force equal those of set_colliders with the normal R a and the offset n . c + r at the same stiffness, to 1e-12 of the largest entry,
    WITH friction (mu = 0.4) and without.  The field is at rest (the half-space has no lateral motion); the two kinds share no launch.
    The frame is turned, and the ramp tilted, about the world x axis, so that n_x = 0: the half-space measures the slip in the engine's tangent
    basis T (collider_host.hpp builds t1 and t2 from an un-normalised seed, as k_contact_pair builds c_T), which is orthonormal to |T^T T - I| =
    n_x^4 only, where the field projects with I - n0 n0^T; with n_x = 0 the friction parts of the two models coincide and the lagged-frame path of
    the field kernels has its exact limit.  A second pose, turned about an oblique axis (n_x = 0.03, |T^T T - I| = 8.1e-7), is printed beside it:
    there the 1e-12 is asserted for the normal part (mu = 0), and with friction the two models differ by the half-space's own figure (energy
    1.3e-8, operator 7e-7; the two NumPy restatements alike), asserted at ten times |T^T T - I| as computed from the half-space's restatement."""
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(23)
    x, xp = _jiggled(s, rng, 1.5 * eps)
    x0 = s.pos.to_numpy()
    S = _State(ctx, x, xp, s._ref_angle)

    def numbers(ks, kc):
        ctx.set_param("k_sdf", ks); ctx.set_param("k_collider", kc)
        return [np.array(S.energy()), S.grad(), S.operator(0), S.operator(1)]

    for tag, turn, tilt in (("about x", [0.6, 0.0, 0.0], [0.05, 0.0, 0.0]), ("oblique", [0.3, -0.2, 0.5], [0.05, -0.03, 0.0])):
        q = _quat(turn)[None]
        R = bn.quat_to_R(q[0])
        assert np.abs(R - np.eye(3)).max() > 0.4
        n = bn.rot(tilt) @ EZ
        a = R.T @ n
        c = np.array([x0.mean(axis=0) + [0.003, -0.002, -0.004]])
        r = np.array([3e-4])
        plane_z = float(x0[:, 2].mean()) - 0.3 * eps
        b = float(n @ np.array([x0[:, 0].mean(), x0[:, 1].mean(), plane_z]) - n @ c[0]) - r[0]   # phi(y) - r = n . x - (n . c + r + b): the solid's face 0.3 eps under the sheet
        grid, origin = _grid_about(lambda p: p @ a - b, (np.vstack([x, xp]) - c[0]) @ R, DX / 2, 2e-3)
        o = np.array([float(n @ c[0]) + r[0] + b])
        T = cn._terms(x[0], xp[0], cn.unit(n[None])[0], o[0], 0.4, K, eps, eh)[0]
        skew_T = float(np.abs(T.T @ T - np.eye(2)).max())
        print("%s: n = %s, the half-space's tangent basis: |T^T T - I| = %.2e" % (tag, n, skew_T))
        if tag == "about x":
            assert n[0] == 0.0 and skew_T <= 4e-16
            bounds = ((np.array([0.0]), 1e-12), (np.array([0.4]), 1e-12))
        else:
            assert 1e-12 < skew_T < 1e-5
            bounds = ((np.array([0.0]), 1e-12), (np.array([0.4]), 10.0 * skew_T))
        for mu, bound in bounds:
            ctx.set_sdfs([grid], [origin], [DX / 2], c, q, r, mu)
            ctx.set_colliders(n[None], o, mu)
            base, fld, pln = numbers(0.0, 0.0), numbers(K, 0.0), numbers(0.0, K)
            for name, z, f, p in zip(("energy", "gradient", "operator spd 0", "operator spd 1"), base, fld, pln):
                df, dp = f - z, p - z
                print("%s, mu = %g, %s: field against plane %.2e of the largest entry (bound %.1e)" % (tag, mu[0], name, np.abs(df - dp).max() / np.abs(dp).max(), bound))
                assert np.abs(dp).max() > 0 and np.abs(df - dp).max() <= bound * np.abs(dp).max()
            ctx.set_param("k_sdf", K); ctx.set_param("k_collider", K)
            ff, fp = ctx.sdf_force(S.pos, S.prev), ctx.collider_force(S.pos, S.prev)
            print("%s, mu = %g, force: field against plane %.2e of the largest entry" % (tag, mu[0], np.abs(ff[:, 0:3] - fp).max() / np.abs(fp).max()))
            assert np.abs(ff[:, 0:3] - fp).max() <= bound * np.abs(fp).max() and np.abs(fp).max() > 0
        # the state walks through the branches: inside the grid everywhere, gaps on both sides of the shell at both points, both friction regimes
        A = _table([dn.Field(grid, origin, DX / 2)], r, c, q, c, q, dn.full_mask(s.tot_NV, 1), eps, eh, np.array([0.4]))
        val, val0, act, act0 = dn.active_sets(x, xp, *A)
        assert val.all() and val0.all() and act.any() and (~act).any() and act0.any() and (~act0).any()
        rw = np.array([P.r_w for v, j, P in dn.pairs(x, xp, *A) if P.lam > 0])
        assert (rw < eh).any() and (rw > eh).any() and (act[:, 0] & act0[:, 0]).sum() >= 10
    s._close_ctx()


def test_the_offset_is_a_constant_taken_off_the_samples():
    """(grid, r) against (grid - r, 0): energy, gradient, operator and both read-outs agree to 1e-12 of the largest entry"""
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    F, r, c, q, cp, qp, xp, x, mask, near, special = placed(s.pos.to_numpy(), np.arange(NV), 8, eps, eh, seed=3)
    S = _State(ctx, x, xp, s._ref_angle)
    p = _dev(np.random.default_rng(2).normal(size=3 * NV))
    got = []
    for grids, rr in (([f.s for f in F], r), ([f.s - rj for f, rj in zip(F, r)], np.zeros(2))):
        ctx.set_sdfs(grids, [f.o for f in F], [f.h for f in F], c, q, rr, MU, mask)
        ctx.set_sdf_poses(c, q, cp, qp)
        got.append([np.array(S.part(S.energy)), S.part(S.grad), S.part(lambda: S.operator(0)), ctx.sdf_force(S.pos, S.prev), ctx.sdf_grad(S.pos, S.prev, p)])
    for a, b in zip(*got):
        assert np.abs(a).max() > 0 and np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    s._close_ctx()


def test_a_sampled_ball_against_the_sphere_kernels():
    """A ball of radius 30 mm sampled at h = 2 mm under the sheet against set_spheres: the spline smooths a curved field by about h^2 / 6 times its
    Laplacian, h^2 / (3 R) = 4.4e-5 m for the ball, so the gaps differ by about that and the gradients by about k times that.  The difference is
    printed (DESIGN.md 2.14 has it) and is not asserted beyond lying below ten times that figure: the margin is for the corner term of the
    smoothing, which nobody has measured on this kernel."""
    from thinshelllab_amd.engine import sdf
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps = s.eps_contact
    x0 = s.pos.to_numpy()
    Rb, h = 0.03, 0.002
    c = np.array([x0.mean(axis=0) - [0.0, 0.0, Rb - 0.5 * eps]])
    Y = x0 - c[0]
    near = np.flatnonzero(np.linalg.norm(Y, axis=1) < Rb + 4 * eps)
    assert len(near) >= 5
    grid, origin = sdf.sample(sdf.ball(Rb), Y[near].min(axis=0) - 3 * h, Y[near].max(axis=0) + 3 * h, h)
    mask = np.zeros(s.tot_NV, np.uint8); mask[near] = 1
    ctx.set_sdfs([grid], [origin], [h], c, [QID], [0.0], [0.0], mask)
    ctx.set_spheres(c, [Rb], [0.0], mask)
    S = _State(ctx, x0, x0, s._ref_angle)
    ctx.set_param("k_sphere", 0.0)
    g_f = S.part(S.grad)
    ctx.set_param("k_sdf", 0.0)
    g_s = S.part(S.grad, key="k_sphere")
    ctx.set_param("k_sphere", 0.0)
    shift = h * h / (3.0 * Rb)
    diff = np.abs(g_f - g_s).max()
    print("sampled ball against the sphere: largest gradient difference %.4e N = k x %.4e m; h^2 / (3 R) = %.4e m; largest gradient entry %.4e N"
          % (diff, diff / K, shift, np.abs(g_s).max()))
    assert np.abs(g_s).max() > 0 and diff < 10.0 * K * shift
    s._close_ctx()


def test_eight_fields_with_mask_bit_seven_in_use():
    s = _drape(8)
    ctx = s._ensure_ctx()
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    x0 = s.pos.to_numpy()
    mid = x0.mean(axis=0)
    F = [noisy_ramp((5 + (j % 3), 6, 4 + (j % 2)), 0.012, bn.rot([0.02 * j, -0.01 * j, 0.0]) @ EZ, 40 + j, noise=0.01) for j in range(8)]
    c8 = mid + np.arange(8)[:, None] * [0.0004, -0.0003, 0.0] - [0.0, 0.0, eps]
    q8 = np.array([_quat([0.0, 0.0, 0.02 * j]) for j in range(8)])
    cp8 = c8 - [2e-5, 1e-5, 1e-5]
    qp8 = np.array([_quat([1e-3, -2e-3, 1e-3], a) for a in q8])
    r8, mu8 = np.linspace(1e-4, 3e-4, 8), np.full(8, 0.1)   # (every solid reaches into the sheet's shell: every row of the read-outs is nonzero)
    mask = np.full(NV, 255, np.uint8); mask[::3] = 0x80; mask[1::3] = 0x7f
    ctx.set_sdfs([f.s for f in F], [f.o for f in F], [f.h for f in F], c8, q8, r8, mu8, mask)
    ctx.set_sdf_poses(c8, q8, cp8, qp8)
    ctx.set_param("k_sdf", K)
    xp = x0 - [1e-5, 2e-5, 0.0]
    pos, prev = _dev(x0), _dev(xp)
    f8 = ctx.sdf_force(pos, prev)
    pn = np.random.default_rng(1).normal(size=(NV, 3))
    g8 = ctx.sdf_grad(pos, prev, _dev(pn.reshape(-1)))
    A8 = _table(F, r8, c8, q8, cp8, qp8, mask, eps, eh, mu8)
    g8_np = dn.sdf_grad(x0, xp, pn, s.frozen.to_numpy().reshape(-1, 3), *A8)
    f8_np = dn.force(x0, xp, *A8)
    assert ctx.sdf_count() == 8 and g8.shape == (8, 14) and f8.shape == (8, 6) and np.abs(f8_np[7]).max() > 0 and np.abs(g8_np).min() > 0
    for lo, hi in GRAD_GROUPS:
        assert np.abs(g8 - g8_np)[:, lo:hi].max() <= 1e-12 * np.abs(g8_np[:, lo:hi]).max(), (lo, hi)
    for lo, hi in FORCE_GROUPS:
        assert np.abs(f8 - f8_np)[:, lo:hi].max() <= 1e-12 * np.abs(f8_np[:, lo:hi]).max(), (lo, hi)
    only7 = dn.force(x0, xp, *_table(F, r8, c8, q8, cp8, qp8, mask & 0x80, eps, eh, mu8))
    assert np.array_equal(only7[7], f8_np[7]) and not only7[:7].any()
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ all classes at once
def test_handles_ties_planes_a_ball_a_rod_a_box_and_a_field_in_one_scene():
    """Scene_seam (two 8 x 8 cloths, nine ties) with vertex handles, two planes, a ball, a rod, a box and two fields: the energy of all seven equals
    the sum of the restatements (the partials of every class lie where energy_async says), and the numbers of the other classes keep their bits
    with fields on"""
    from thinshelllab_amd.task_scene.Scene_seam import Scene
    s = Scene(cloth_size=DX * 8, N=8, k_tie=K, perturb=0.0, newton_cap=200)
    s.init_all()
    NV = s.tot_NV
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(21)
    hv = np.array([100, 5, 130, 77], np.int32); hw = np.array([1.0, 0.5, 2.0, 1.5])
    s.set_handles(hv, K, hw)
    ht = s.pos.to_numpy()[hv] + rng.normal(scale=1e-3, size=(4, 3))
    s.set_handle_targets(ht)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((NV, 3)))
    x0 = s.pos.to_numpy()
    first = np.arange(81)
    F, r, c, q, cp, qp, xp, x, fmask, near, special = placed(x0, first, 8, eps, eh, seed=9)
    x[81:] += rng.normal(scale=2e-4, size=(NV - 81, 3))   # (the second cloth moves too: the seam is stretched)
    n = cn.unit([[0.0, 0.0, 1.0], [0.0, np.sin(0.3), np.cos(0.3)]])
    o = np.array([float(x0[:, 2].mean()), float(n[1] @ x0.mean(axis=0)) + 0.5 * eps])
    mu_p = np.array([0.5, 0.3])
    pmask = cn.full_mask(NV, 2); pmask[::7] = 1; pmask[3] = 0
    mid = x0.mean(axis=0)
    sc = np.array([[mid[0] - 0.01, mid[1] + 0.005, mid[2] - 1.0]]); scp = sc - [[0.4 * eh, 0.2 * eh, 0.6 * eh]]
    sR, smu = np.array([1.0]), np.array([0.4])
    smask = sn.full_mask(NV, 1); smask[::5] = 0
    ka = np.array([[mid[0] - 0.02, mid[1], mid[2] - 0.5]]); kb = np.array([[mid[0] + 0.02, mid[1] + 0.01, mid[2] - 0.5]])
    kap, kbp = ka - [[0.3 * eh, 0.1 * eh, 0.5 * eh]], kb - [[0.2 * eh, -0.3 * eh, 0.4 * eh]]
    kR, kmu = np.array([0.5]), np.array([0.3])
    kmask = kn.full_mask(NV, 1); kmask[::4] = 0
    bc = np.array([[mid[0], mid[1], mid[2] - 0.012]]); bcp = bc - [[0.3 * eh, 0.2 * eh, 0.1 * eh]]
    bq = _quat([0.0, 0.01, 0.2])[None]; bqp = _quat([1e-3, 0.0, -1e-3], bq[0])[None]
    bh, brad, bmu = np.array([[0.015, 0.01, 0.002]]), np.array([0.01]), np.array([0.2])
    bmask = bn.full_mask(NV, 1); bmask[::6] = 0
    idx, bb, w = tn.records(s.faces.to_numpy(), s._tie_v, s._tie_f, s._tie_b)
    S = _State(ctx, x, xp, s._ref_angle)
    fz = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_colliders(n, o, mu_p, pmask); ctx.set_param("k_collider", K)
    ctx.set_spheres(sc, sR, smu, smask); ctx.set_sphere_centres(sc, scp); ctx.set_param("k_sphere", K)
    ctx.set_capsules(ka, kb, kR, kmu, kmask); ctx.set_capsule_ends(ka, kb, kap, kbp); ctx.set_param("k_capsule", K)
    ctx.set_boxes(bc, bq, bh, brad, bmu, bmask); ctx.set_box_poses(bc, bq, bcp, bqp); ctx.set_param("k_box", K)

    def numbers():
        p = _dev(np.random.default_rng(4).normal(size=3 * NV))
        return (ctx.handle_force(S.pos), ctx.handle_grad(p), ctx.tie_force(S.pos), ctx.tie_grad(S.pos, p), ctx.contact_blocks(False),
                ctx.collider_force(S.pos, S.prev), ctx.collider_grad(S.pos, S.prev, p), ctx.sphere_force(S.pos, S.prev), ctx.sphere_grad(S.pos, S.prev, p),
                ctx.capsule_force(S.pos, S.prev), ctx.capsule_grad(S.pos, S.prev, p), ctx.box_force(S.pos, S.prev), ctx.box_grad(S.pos, S.prev, p),
                ctx.param_grads(S.pos, S.ref, ["k_handle", "k_tie"], p=p))
    S.operator(1)
    before = numbers()
    e_six, g_six = S.energy(), S.grad()
    keys = ("k_handle", "k_tie", "k_collider", "k_sphere", "k_capsule", "k_box")
    for key in keys:
        ctx.set_param(key, 0.0)
    e_0 = S.energy()
    for key in keys:
        ctx.set_param(key, K)
    ctx.set_sdfs([f.s for f in F], [f.o for f in F], [f.h for f in F], c, q, r, MU, fmask); ctx.set_sdf_poses(c, q, cp, qp); ctx.set_param("k_sdf", K)
    S.operator(1)
    after = numbers()
    for a, d in zip(before[:13], after[:13]):
        assert np.array_equal(a, d)
    assert before[13] == after[13] and ctx.tie_count() == 9 and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 9
    e_all, g_all = S.energy(), S.grad()
    e_h, e_t, e_c = hn.energy(x, hv, hw, ht, K), tn.energy(x, idx, bb, w, K), cn.energy(x, xp, n, o, mu_p, pmask, K, eps, eh)
    e_s = sn.energy(x, xp, sc, scp, sR, smu, smask, K, eps, eh)
    e_k = kn.energy(x, xp, ka, kb, kap, kbp, kR, kmu, kmask, K, eps, eh)
    e_b = bn.energy(x, xp, bc, np.array([bn.quat_to_R(bq[0])]), bcp, np.array([bn.quat_to_R(bqp[0])]), bh, brad, bmu, bmask, K, eps, eh)
    A = _table(F, r, c, q, cp, qp, fmask, eps, eh)
    e_f = dn.energy(x, xp, *A)
    print("energy of the seven classes %.17g, restatements %.17g + %.17g + %.17g + %.17g + %.17g + %.17g + %.17g" % (e_all - e_0, e_h, e_t, e_c, e_s, e_k, e_b, e_f))
    tot = e_h + e_t + e_c + e_s + e_k + e_b + e_f
    assert min(e_h, e_t, e_c, e_s, e_k, e_b, e_f) > 1e-6 * tot          # (a class whose partials were lost or read twice would show a million times over the bound)
    assert abs((e_all - e_0) - ((((((e_h + e_t) + e_c) + e_s) + e_k) + e_b) + e_f)) <= 1e-12 * tot
    assert abs((e_all - e_six) - e_f) <= 1e-12 * tot
    gf = dn.gradient(x, xp, *A) * (fz == 0)
    assert np.abs((g_all - g_six) - gf).max() <= 1e-12 * max(np.abs(gf).max(), np.abs(g_all).max())
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ off means off
def _assemble_and_step(ctx, x, ref):
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=1, grad=F)
    H = ctx.operator_csr().toarray()
    e = ctx.energy(pos, prev, vel, ref)
    ctx.set_param("contact", 0.0)
    st = ctx.step(pos, prev, vel, ref)
    return F.cpu().numpy(), H, e, pos.cpu().numpy(), vel.cpu().numpy(), st["newton_iters"]


def _under(x0, eps, seed=31):
    """two small fields under the middle of a sheet, for the scene interface: (grids, origins, spacings, centres, quats, offsets, mu)"""
    mid = x0.mean(axis=0)
    F = [noisy_ramp((14, 12, 6), DX / 2, bn.rot([0.02, -0.03, 0.0]) @ EZ, seed, noise=0.02), noisy_ramp((4, 4, 4), 2 * DX, EZ, seed + 1, noise=0.01)]
    c = np.array([[mid[0], mid[1], mid[2] - 1e-4], [mid[0] + 0.02, mid[1], mid[2] - 2e-4]])
    return [f.s for f in F], [f.o for f in F], [f.h for f in F], c, [QID, _quat([0.0, 0.0, 0.5])], [0.0, 0.0], [0.5, 0.2]


@pytest.mark.parametrize("how", ["removed", "k_zero"])
def test_off_means_off(how):
    rng = np.random.default_rng(5)
    fresh = _drape(12, perturb=1e-4)
    x = fresh.pos.to_numpy()
    y = x + rng.normal(scale=1e-4, size=x.shape) * (fresh.frozen.to_numpy().reshape(-1, 3) == 0)
    ctx_f = fresh._ensure_ctx()
    ctx_f.set_param("direct", 1)
    want = _assemble_and_step(ctx_f, y, fresh._ref_angle)
    used = _drape(12, perturb=1e-4)
    used.set_sdfs(*_under(x, used.eps_contact), 2000.0)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    used.move_sdfs([[1e-5, 0.0, 1e-5], [1e-5, 1e-5, 1e-5]], [[0.0, 1e-3, 0.0], [1e-3, 0.0, 1e-3]])
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.sdf_count() == 2 and np.abs(used.sdf_force()).max() > 0
    assert not np.array_equal(_assemble_and_step(ctx_u, y, used._ref_angle)[0], want[0])
    if how == "removed":
        used.set_sdfs([], [], [], [], [], [], [], 0.0)
        assert used._ensure_ctx() is ctx_u and ctx_u.sdf_count() == 0
    else:
        ctx_u.set_param("k_sdf", 0.0)
        f = ctx_u.sdf_force(_dev(y), _dev(y))
        g = ctx_u.sdf_grad(_dev(y), _dev(y), _dev(rng.normal(size=y.size)))
        assert ctx_u.sdf_count() == 2 and f.shape == (2, 6) and not f.any() and g.shape == (2, 14) and not g.any()
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ whole rollouts
def _mould(N=8, **kw):
    from thinshelllab_amd.task_scene.Scene_mould import Scene
    s = Scene(N=N, **kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


STVK = (3.0e5, 2.0e5)
MOULD_PUSH, MOULD_K = 7.5e-4, 2.0e3
MOULD_ARM = 0.016   # metres: the ring's outer radius, the scale that makes a rotation step comparable to a translation step
# The ring's top lies 0.75 mm above the corners' plane.  The analytic gradient is the derivative of a step's ROOT, and the forward operator holds the
# Gauss-Newton part of the fields' block: what it leaves out is the normal force times the curvature of the ring's surface, which acts along the
# surface where only the sheet's own stiffness and inertia answer, and Newton converges linearly at their ratio.  With the ring 1.5 mm up that ratio
# is 0.43 (measured: max |p| / dt falls 4.3e-3, 1.0e-3, 3.3e-4, ... 9.8e-8 over 12 iterations), the engine's stop at 1e-7 leaves the state 4e-10 m off
# its root and the mu column, in which the loss is nearly linear, 8e-6 off where the rule asks for 2e-6.  At 0.75 mm the normal force is smaller, a
# step takes 7 iterations and ends 6e-11 m off its root: the scene is one whose steps the engine, as users run it, solves to their roots.
_RELAXED = {}


def _relaxed():
    """the rollout scene's start, computed once: the StVK sheet without bending (its matrix is the exact second derivative of its energy), all four
    corners frozen, pushed up by Scene_mould's ring whose top lies 0.75 mm above the corners' plane, after 40 steps (positions, velocities)"""
    if not _RELAXED:
        s = _mould(Kb=0.0, stvk=STVK, push=MOULD_PUSH, k_sdf=MOULD_K, pin="all")
        for f in range(1, 41):
            assert s.time_step(None, f)["unconverged"] == 0
        _RELAXED["x"], _RELAXED["v"] = s.pos.to_numpy().copy(), s.vel.to_numpy().copy()
        s._close_ctx()
    return _RELAXED["x"].copy(), _RELAXED["v"].copy()


def _mould_trajectory(T, c0, q0, eh):
    """(centres (T, 1, 3), quaternions (T, 1, 4)): the mould rises a little, translates along x by 0.4, 1.6 and 2.8 eps_v dt and along y by 0.3 eps_v dt
    per step, and tilts and yaws so that its rim moves a further 0.6 eps_v dt per step; the slip per step straddles eps_v dt"""
    from thinshelllab_amd.engine import frames
    c, q = np.tile(c0, (T, 1, 1)), np.tile(q0, (T, 1, 1))
    for f in range(1, T):
        c[f], q[f] = frames.compose(c[f - 1], q[f - 1], [[(0.4 + 1.2 * (f - 1)) * eh, 0.3 * eh, 2e-6]], [[0.0, -0.3 * eh / MOULD_ARM, 0.6 * eh / MOULD_ARM]])
    return c, q


# The two difference steps of every check, a decade apart, as fractions of the parameter's own scale: those of tests/test_gpu_boxes.py -- a point of
# the mould and the start positions against the slip scale eps_v dt = 5e-5 m (2 % and 0.2 %; a rotation vector takes them over the ring's radius),
# the offset against the shell eps = 4e-4 m (2.5 % and 0.25 %), mu against mu = 0.5 (20 % and 2 %).
FD_STEPS = {"c": (1e-6, 1e-7), "th": (1e-6 / MOULD_ARM, 1e-7 / MOULD_ARM), "mu": (1e-1, 1e-2), "r": (1e-5, 1e-6), "x": (1e-6, 1e-7)}


def _rollout_checks(steps=FD_STEPS):
    """([(name, analytic, (difference at the larger step, at the smaller step))], smallest and largest slip of an active pair in one step of the tape in
    units of eps_v dt)"""
    from thinshelllab_amd.engine import frames
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    x0, v0 = _relaxed()
    s = _mould(Kb=0.0, stvk=STVK, push=MOULD_PUSH, k_sdf=MOULD_K, pin="all")
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    grid, origin, h, c0, q0, r0, mu0 = s.mould()
    F = [dn.Field(grid, origin, h)]
    c_traj, q_traj = _mould_trajectory(T, c0, q0, eh)
    mask = s._sdf_mask.copy()
    free = (s.frozen.to_numpy().reshape(-1, 3) == 0)
    sets = []

    def tables(c, q, r, mu):
        return [_table(F, r, c[fr], q[fr], c[fr - 1], q[fr - 1], mask, eps, eh, mu, MOULD_K) for fr in range(1, T)]

    def rollout(c=c_traj, q=q_traj, mu=mu0, r=r0, x=x0, reverse=False):
        s.set_sdfs([grid], [origin], [h], c[0], q[0], r, mu, MOULD_K)
        # (row 0 of the tape is d(loss)/d(x_0) with the state before it held fixed: the start velocity moves with the start state)
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy(v0 + (x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        g.copy_pos(s, 0)
        for fr in range(1, T):
            s.set_sdf_poses(c[fr], q[fr])
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < 50
            if reverse:
                print("step %d: %d Newton iterations, last delta %.2e" % (fr, st["newton_iters"], st["last_delta"]))
            g.copy_pos(s, fr)
        xs = g.pos_buffer.t.cpu().numpy()
        sets.append([dn.active_sets(xs[fr], xs[fr - 1], *A) for fr, A in zip(range(1, T), tables(c, q, r, mu))])
        L = float((xs[T - 1] * wgt).sum())
        if not reverse:
            return L
        assert np.array_equal(g.sdf_poses.t.numpy()[:, :, 0:3], c) and np.array_equal(g.sdf_poses_prev.t.numpy()[1:], g.sdf_poses.t.numpy()[:-1])
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.last_stats["flag"] != 3 and g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.sdf_grad.t.numpy().copy(), g.sdf_pose_grad().numpy().copy(), g.pos_grad.t[0].cpu().numpy().copy(), xs

    _, bg, pg, pg0, xs = rollout(reverse=True)
    assert bg.shape == (T, 1, 14) and pg.shape == (T, 1, 6) and (bg[0] == 0).all() and np.abs(bg[1:]).min() > 0
    assert np.array_equal(pg[:-1], bg[:-1, :, 0:6] + bg[1:, :, 6:12])
    slip = np.zeros((T - 1, len(x0)))
    for fr, A in zip(range(1, T), tables(c_traj, q_traj, r0, mu0)):
        for v, j, P in dn.pairs(xs[fr], xs[fr - 1], *A):
            slip[fr - 1, v] = P.r_w
    act = np.array([a[2][:, 0] & a[3][:, 0] for a in sets[0]])
    assert all(a[0].all() and a[1].all() for a in sets[0])          # every vertex stays inside the grid
    print("active vertices per step: %s; slip per step of the active pairs: %.3e .. %.3e m, eps_v dt = %.1e m" % (act.sum(axis=1).tolist(), slip[act].min(), slip[act].max(), eh))
    d_c = rng.uniform(-1.0, 1.0, (T, 1, 3))
    d_th = rng.uniform(-1.0, 1.0, (T, 1, 3))
    d_mu = rng.uniform(0.5, 1.0, 1)
    d_r = rng.uniform(0.5, 1.0, 1)
    e = rng.normal(size=x0.shape) * free
    turned = lambda hh: np.array([frames.compose(c_traj[f], q_traj[f], np.zeros((1, 3)), hh * d_th[f])[1] for f in range(T)])
    fd = lambda f, hs: [(f(hh) - f(-hh)) / (2 * hh) for hh in hs]
    checks = [("sdf_pose_grad[:, :, 0:3] . delta_c", float((pg[:, :, 0:3] * d_c).sum()), fd(lambda hh: rollout(c=c_traj + hh * d_c), steps["c"])),
              ("sdf_pose_grad[:, :, 3:6] . delta_theta", float((pg[:, :, 3:6] * d_th).sum()), fd(lambda hh: rollout(q=turned(hh)), steps["th"])),
              ("sdf_grad[:, :, 12] . delta_mu", float((bg[:, :, 12].sum(axis=0) * d_mu).sum()), fd(lambda hh: rollout(mu=mu0 + hh * d_mu), steps["mu"])),
              ("sdf_grad[:, :, 13] . delta_r", float((bg[:, :, 13].sum(axis=0) * d_r).sum()), fd(lambda hh: rollout(r=r0 + hh * d_r), steps["r"])),
              ("pos_grad[0] . direction", float((pg0 * e).sum()), fd(lambda hh: rollout(x=x0 + hh * e), steps["x"]))]
    for i, a in enumerate(sets[1:]):
        for fr in range(T - 1):
            assert all(np.array_equal(a[fr][k], sets[0][fr][k]) for k in range(4)), "a vertex crossed the shell or the grid's border between the runs: a badly chosen input (perturbed run %d)" % i
    for name, got, d in checks:
        print("%s: analytic %.10e, differences %s" % (name, got, " / ".join("%.10e" % v for v in d)))
        print("    (the last two disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (abs(d[-2] - d[-1]) / abs(d[-1]), abs(got - d[-1]) / abs(d[-1]), 3 * abs(d[-2] - d[-1]) / abs(d[-1])))
    s._close_ctx()
    return checks, (slip[act].min() / eh, slip[act].max() / eh)


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state; Scene_mould with the
    StVK sheet without bending and four frozen corners, relaxed over the ring for 40 steps; the mould then rises by 2e-6 m per step, translates, tilts
    and yaws (_mould_trajectory).  sdf_pose_grad() contracted with a random centre-trajectory direction and with a random rotation-trajectory
    direction, the mu and r columns summed over the steps, and pos_grad[0] . e along a random free direction (the state before it held fixed), each
    against central differences at two steps a decade apart.  Rule: the two differences agree to 1e-2, and the analytic value lies within three
    times their disagreement.  No vertex may cross d = eps or d0 = eps between the runs; the field is C2, so there is no condition of the kind of
    the boxes' edge lines.  The measured figures are in DESIGN.md 2.14."""
    checks, (slip_min, slip_max) = _rollout_checks()
    assert slip_max > 1.0 > slip_min          # both friction regimes on the tape (in units of eps_v dt)
    for name, got, fd in checks:
        assert abs(fd[0] - fd[1]) < 1e-2 * abs(fd[1]), name
        assert abs(got - fd[1]) <= 3 * abs(fd[0] - fd[1]), name


# ------------------------------------------------------------------------------------------------ groups and plans
T_TAPE = 5


def _tape(s):
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    g = Grad(s, T_TAPE, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    return g


def test_group_members_equal_their_single_runs_and_two_runs_repeat():
    from thinshelllab_amd.scene_group import SceneGroup
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(81, 3))
    A, B = ((2e-5, 1e-5, 2e-6), (0.0, -1e-3, 2e-3)), ((-4e-5, 0.0, -1e-6), (1e-3, 1e-3, -2e-3))
    runs = {}
    for tag, (dp, dth) in (("a", A), ("b", A), ("c", B)):
        s = _mould(push=2e-4)
        g = _tape(s)
        for f in range(1, T_TAPE):
            s.move_sdfs([dp], [dth])
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
            g.copy_pos(s, f)
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
        for f in range(T_TAPE - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.sdf_grad.t.numpy().copy(), g.sdf_poses.t.numpy().copy())
        s._close_ctx()
    for a, d in zip(runs["a"], runs["b"]):
        assert np.array_equal(a, d)
    assert not np.array_equal(runs["a"][0], runs["c"][0]) and np.abs(runs["a"][2][1:, :, :12]).min() > 0 and (runs["a"][2][0] == 0).all()
    ms = [_mould(push=2e-4), _mould(push=2e-4)]
    G = SceneGroup(ms)
    gs = [_tape(m) for m in ms]
    for f in range(1, T_TAPE):
        for m, (dp, dth) in zip(ms, (A, B)):
            m.move_sdfs([dp], [dth])
        sts = G.time_step(None, f)
        assert all(r["unconverged"] == 0 for r in sts)
        for m, g in zip(ms, gs):
            g.copy_pos(m, f)
    for g in gs:
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
    for f in range(T_TAPE - 1, 0, -1):
        G.transfer_grad(f, gs, None)
    assert G.info()["merged_factorizations"] > 0
    G.close()
    for i, tag in ((0, "a"), (1, "c")):
        for a in range(2):
            assert np.array_equal((gs[i].pos_buffer.t, gs[i].pos_grad.t)[a].cpu().numpy(), runs[tag][a]), (i, a)
        assert np.array_equal(gs[i].sdf_grad.t.numpy(), runs[tag][2]) and np.array_equal(gs[i].sdf_poses.t.numpy(), runs[tag][3]), i
        assert np.array_equal(gs[i].sdf_poses_prev.t.numpy()[1:], runs[tag][3][:-1])
    for m in ms:
        m._close_ctx()


def test_fields_build_no_plan_and_no_slot():
    """the factorised path: the plan count after the first step does not change when fields are switched on, over the rollout or in the reverse sweep"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _mould(push=2e-4)
    grid, origin, h, c0, q0, r0, mu0 = s.mould()
    s.set_sdfs([], [], [], [], [], [], [], 0.0)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["factorizations"] > 0 and ctx.sdf_count() == 0
    plans = ctx.direct_info()["plans"]
    assert plans >= 1
    s.set_sdfs([grid], [origin], [h], c0, q0, r0, mu0, MOULD_K)
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.move_sdfs([[1e-5, -1e-5, 0.0]], [[0.0, 1e-3, 1e-3]])
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0 and st["nc"] == 0, st
        g.copy_pos(s, f)
        assert ctx.direct_info()["plans"] == plans and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 0
    assert s._ensure_ctx() is ctx and ctx.sdf_count() == 1 and np.abs(s.sdf_force()).max() > 0
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans and np.abs(g.sdf_grad.t.numpy()[1:]).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list_and_samples():
    s = _mould(push=2e-4)
    ctx = s._ensure_ctx()
    grid, origin, h, c0, q0, r0, mu0 = s.mould()
    ctx.set_sdfs([grid, grid], [origin, origin], [h, h], np.vstack([c0, c0 + [0.0, 0.0, -0.001]]), np.vstack([q0, q0]), [0.0, 0.0], [0.5, 0.1])
    pos = _dev(s.pos.to_numpy())
    before = ctx.sdf_force(pos, pos)
    assert before.shape == (2, 6) and np.abs(before).max() > 0
    o, q1 = [0.0, 0.0, -1.0], [1.0, 0.0, 0.0, 0.0]
    g4 = np.arange(64.0).reshape(4, 4, 4)
    bad_s = g4.copy(); bad_s[3, 0, 2] = np.inf
    two = lambda **kw: tuple(kw.get(key, dflt) for key, dflt in (("grids", [g4, g4]), ("origins", [o, o]), ("spacings", [0.01, 0.01]), ("centres", [o, o]), ("quats", [q1, q1]),
                                                               ("offsets", [0.0, 0.0]), ("mu", [0.1, 0.1])))
    cases = [(two(grids=[g4, np.zeros((4, 4, 3))]), r"dimension 3 of axis 2 of field 1 is below 4 or above 512"),
             (two(grids=[np.zeros((513, 4, 4)), g4]), r"dimension 513 of axis 0 of field 0 is below 4 or above 512"),
             (two(spacings=[0.01, 0.0]), r"spacing 0 of field 1 is not finite and positive"),
             (two(spacings=[0.01, np.nan]), r"spacing nan of field 1 is not finite and positive"),
             (two(origins=[o, [np.inf, 0.0, 0.0]]), r"origin \(inf, 0, 0\) of field 1 is not finite"),
             (two(offsets=[0.0, np.nan]), r"offset nan of field 1 is not finite"),
             (two(centres=[o, [0.0, np.nan, 0.0]]), r"centre \(0, nan, 0\) of field 1 is not finite"),
             (two(quats=[q1, [0.0, 0.0, 0.0, 0.0]]), r"quaternion \(0, 0, 0, 0\) of field 1 is zero or not finite"),
             (two(quats=[q1, [1.0, 0.0, np.inf, 0.0]]), r"quaternion \(1, 0, inf, 0\) of field 1 is zero or not finite"),
             (two(mu=[0.1, -0.5]), r"friction coefficient -0.5 of field 1 is negative or not finite"),
             (two(grids=[g4, bad_s]), r"sample \(3, 0, 2\) of field 1 is not finite \(inf\)"),
             (([g4] * 9, [o] * 9, [0.01] * 9, [o] * 9, [q1] * 9, [0.0] * 9, [0.1] * 9), r"9 fields: at most 8")]
    for args, pat in cases:
        with pytest.raises(Exception, match="tsl_set_sdfs: " + pat):
            ctx.set_sdfs(*args)
        with pytest.raises(ValueError, match="set_sdfs: " + pat):          # the scene's host check: the library's message
            s.set_sdfs(*args, 10.0)
        assert ctx.sdf_count() == 2 and np.array_equal(ctx.sdf_force(pos, pos), before)      # (the previous list AND its samples: the force is read from them)
    bad = np.full(s.tot_NV, 3, np.uint8); bad[17] = 4
    with pytest.raises(Exception, match=r"tsl_set_sdfs: mask 0x04 of vertex 17 names a field at or above 2"):
        ctx.set_sdfs(*two(), bad)
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: centre \(inf, 0, -1\) of field 0 is not finite"):
        ctx.set_sdf_poses([[np.inf, 0.0, -1.0], o], [q1, q1])
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: quaternion \(0, 0, 0, 0\) of field 1 is zero or not finite"):
        ctx.set_sdf_poses([o, o], [q1, [0.0, 0.0, 0.0, 0.0]])
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: previous centre \(0, 0, nan\) of field 1 is not finite"):
        ctx.set_sdf_poses([o, o], [q1, q1], [o, [0.0, 0.0, np.nan]], [q1, q1])
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: previous quaternion \(nan, 0, 0, 0\) of field 0 is zero or not finite"):
        ctx.set_sdf_poses([o, o], [q1, q1], [o, o], [[np.nan, 0.0, 0.0, 0.0], q1])
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: previous centres without previous quaternions"):
        ctx.set_sdf_poses([o, o], [q1, q1], [o, o], None)
    with pytest.raises(Exception, match=r"tsl_set_sdf_poses: previous quaternions without previous centres"):
        ctx.set_sdf_poses([o, o], [q1, q1], None, [q1, q1])
    assert ctx.sdf_count() == 2 and np.array_equal(ctx.sdf_force(pos, pos), before)
    with pytest.raises(Exception, match="k_sdf must be finite and >= 0"):
        ctx.set_param("k_sdf", -1.0)
    with pytest.raises(Exception, match="k_sdf must be finite and >= 0"):
        ctx.set_param("k_sdf", np.nan)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_mould import optimise
    losses, cen, quat = optimise(N=8, T=4, iters=4, log=print)
    assert len(losses) == 4 and losses[-1] < losses[0], losses
    assert cen.shape == (4, 1, 3) and quat.shape == (4, 1, 4) and (cen[1:] != cen[0]).any() and (quat[1:] != quat[0]).any()
