"""Plain restatement of the cloth multigrid preconditioner and of the PCG that runs through it (test infrastructure).

Written from the description in csrc/k_mg.hpp and from the mathematics; the stencil levels are dense matrices (at most ~3300 unknowns), level 0
and the transfers may be scipy sparse: bilinear
prolongation of a 3-vector field on an (N+1) x (M+1) vertex grid (vertex (i, j) has index i (M+1) + j), Galerkin operators
A_{l+1} = P^T A_l P, the radius-2 stencil-slot layout, damped block-Jacobi smoothing, a V(1,1) cycle and the engine's restarted PCG.
Every function takes the scalar type from `dt` (np.float64 or np.longdouble): the long-double run is the reference of a comparison, the
float64 run measures what float64 delivers for the same formulas in another order (e64 of tet_numpy.bound).

The cycle takes the arrays it reads -- single-precision copies included -- as INPUTS, so it can be run on the engine's exported copies
(a test of the cycle alone) or on arrays built here (a test of the restatement alone)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
LAST_SWEEPS = 8          # damped-Jacobi sweeps of a last level without a dense inverse (the first from a zero guess)
PI_STEPS = 12            # power-iteration steps behind every damping factor


# ------------------------------------------------------------------------------------------------ grids and transfers
def nodes(N, M):
    return (N + 1) * (M + 1)


def prolong_1d(N):
    """(N+1) x (N/2+1): an even fine index copies its coarse node, an odd one averages its two neighbours"""
    assert N % 2 == 0
    P = np.zeros((N + 1, N // 2 + 1))
    for i in range(N + 1):
        if i % 2 == 0:
            P[i, i // 2] = 1.0
        else:
            P[i, i // 2] = 0.5
            P[i, i // 2 + 1] = 0.5
    return P


def prolongation(N, M, block=True):
    """bilinear P from the (N/2+1) x (M/2+1) grid to the (N+1) x (M+1) grid; block: expanded with kron I3"""
    P = np.kron(prolong_1d(N), prolong_1d(M))
    return np.kron(P, np.eye(3)) if block else P


def prolongation_sp(N, M, dt=np.float64):
    """the block prolongation as a sparse matrix of scalar type dt"""
    import scipy.sparse as sp
    P = sp.csr_matrix(sp.kron(sp.kron(sp.csr_matrix(prolong_1d(N)), sp.csr_matrix(prolong_1d(M))), sp.identity(3)))
    return sp.csr_matrix((P.data.astype(dt), P.indices, P.indptr), shape=P.shape)


def galerkin(A, N, M, dt=LD):
    """P^T A P of a dense operator on the (N+1) x (M+1) grid (the weights are powers of two: only the additions round)"""
    P = prolongation(N, M).astype(dt)
    return P.T @ np.asarray(A, dtype=dt) @ P


# ------------------------------------------------------------------------------------------------ slot layouts
def _pairs(Nr, Mr, Nc, Mc, R, scale):
    """(slot, row nodes, column nodes) of a radius-R stencil: row node (I, J) of the (Nr+1) x (Mr+1) grid, column node (scale I + dI, scale J + dJ)
    of the (Nc+1) x (Mc+1) grid, slot (dI + R)(2R + 1) + dJ + R; neighbours outside the grid are left out"""
    I, J = np.meshgrid(np.arange(Nr + 1), np.arange(Mr + 1), indexing="ij")
    I = I.ravel(); J = J.ravel()
    for dI in range(-R, R + 1):
        for dJ in range(-R, R + 1):
            i2 = scale * I + dI; j2 = scale * J + dJ
            ok = (i2 >= 0) & (i2 <= Nc) & (j2 >= 0) & (j2 <= Mc)
            yield (dI + R) * (2 * R + 1) + dJ + R, (I * (Mr + 1) + J)[ok], (i2 * (Mc + 1) + j2)[ok]


def _to_dense(S, pairs, nr, ncol, dt):
    S = np.asarray(S).reshape(-1, 9, nr)
    D = np.zeros((3 * nr, 3 * ncol), dt)
    for s, rows, cols in pairs:
        for e in range(9):
            D[3 * rows + e // 3, 3 * cols + e % 3] = S[s, e, rows]
    return D


def _to_slots(D, pairs, nslots, nr, dtype):
    S = np.zeros((nslots, 9, nr), dtype)
    seen = np.zeros(D.shape, bool)
    for s, rows, cols in pairs:
        for e in range(9):
            S[s, e, rows] = D[3 * rows + e // 3, 3 * cols + e % 3]
            seen[3 * rows + e // 3, 3 * cols + e % 3] = True
    return S.ravel(), seen


def dense_from_slots(A, N, M, dt=np.float64):
    """25-slot operator A[(s 9 + e) n + row], s = (dI + 2) 5 + dJ + 2, as a dense 3n x 3n matrix"""
    n = nodes(N, M)
    return _to_dense(A, _pairs(N, M, N, M, 2, 1), n, n, dt)


def slots_from_dense(D, N, M, dtype=np.float64):
    """the inverse; also returns the largest |entry| of D outside the radius-2 stencil (must be 0 for a Galerkin operator of this hierarchy)"""
    n = nodes(N, M)
    S, seen = _to_slots(D, _pairs(N, M, N, M, 2, 1), 25, n, dtype)
    out = np.abs(np.where(seen, 0, D))
    return S, (float(out.max()) if out.size else 0.0)


def s_dense_from_slots(S, N, M, dt=np.float64):
    """49-slot S[(s 9 + e) nc + crow], s = (dI + 3) 7 + dJ + 3, column = fine node (2I + dI, 2J + dJ) of the (N+1) x (M+1) grid: dense 3nc x 3n"""
    return _to_dense(S, _pairs(N // 2, M // 2, N, M, 3, 2), nodes(N // 2, M // 2), nodes(N, M), dt)


def s_slots_from_dense(D, N, M, dtype=np.float32):
    S, seen = _to_slots(D, _pairs(N // 2, M // 2, N, M, 3, 2), 49, nodes(N // 2, M // 2), dtype)
    out = np.abs(np.where(seen, 0, D))
    return S, (float(out.max()) if out.size else 0.0)


# ------------------------------------------------------------------------------------------------ 3 x 3 blocks
def diag_blocks(A):
    n = A.shape[0] // 3
    return np.stack([A[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(n)])


def block_inverse(D, dt=np.float64):
    """cofactor inverse of (n, 3, 3) blocks: adj(D) / det(D), every entry one 2 x 2 minor over the determinant"""
    a = np.asarray(D, dtype=dt).reshape(-1, 9).T
    det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])
    r = np.stack([a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                  a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                  a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]) / det
    return r.T.reshape(-1, 3, 3)


def block_inverse_mp(D):
    """the same inverse in 50-digit arithmetic, (n, 3, 3) objects"""
    import mpmath as mp
    out = np.empty((len(D), 3, 3), dtype=object)
    with mp.workdps(50):
        for k, B in enumerate(np.asarray(D)):
            inv = mp.matrix([[mp.mpf(float(v)) for v in row] for row in B]) ** -1
            for i in range(3):
                for j in range(3):
                    out[k, i, j] = inv[i, j]
    return out


def block_apply(Dinv, v):
    """(n, 3, 3) blocks times a 3n vector"""
    return np.einsum("kij,kj->ki", Dinv, v.reshape(-1, 3)).ravel()


# ------------------------------------------------------------------------------------------------ damping factors
def pi_start(n, dt=np.float64, rows=None):
    """the deterministic pseudo-random start vector of the power iteration: per node the fractional parts of three scaled sines of its row p, minus
    1/2; rows: the row of every node where the level is stored in another order than the one given here (level 0), None: p = the node's index"""
    p = (np.arange(n) if rows is None else np.asarray(rows)).astype(dt)
    cols = []
    for f, o, sc in ((12.9898, 1.0, 43758.5453), (78.233, 2.0, 12345.678), (39.425, 3.0, 9876.543)):
        a = np.sin(dt(f) * p + dt(o)) * dt(sc)
        cols.append(a - np.floor(a) - dt(0.5))
    return np.stack(cols, 1).ravel()


def power_lambda(A, Dinv, dt=np.float64, steps=PI_STEPS, rows=None):
    """lambda_max(D^-1 A) estimate: `steps` un-normalised steps v <- D^-1 A v, the ratio of the last two norms"""
    if not hasattr(A, "indptr"):        # (a scipy sparse operator comes in the scalar type it is to be applied in)
        A = np.asarray(A, dtype=dt)
    Dinv = np.asarray(Dinv, dtype=dt)
    v = pi_start(A.shape[0] // 3, dt, rows)
    n2 = []
    for _ in range(steps):
        v = block_apply(Dinv, A @ v)
        n2.append(np.dot(v, v))
    return np.sqrt(n2[-1] / n2[-2])


def omega_of(lam, c_omega=1.5, omega_max=0.8):
    return min(omega_max, c_omega / lam) if (lam > 0 and np.isfinite(lam)) else omega_max


# ------------------------------------------------------------------------------------------------ the preconditioner
def build_hierarchy(A1, N1, M1, n_levels, last_kind, dt=np.float64, s_from_rounded=True, single=True):
    """the levels >= 1 of one cloth from its dense first stencil operator A1 on the (N1+1) x (M1+1) grid, every array formed here:
    per level A, A32 = float32(A), Dinv, omega, S32 = float32(P^T A32 Dinv) towards the next level, and on the last level its kind
    ("dense": Cinv = float32 of the symmetrised inverse, "one_workgroup" / "per_sweep": Jacobi sweeps); single = False keeps every copy in dt"""
    lv = []
    A, N, M = np.asarray(A1, dtype=dt), N1, M1
    for l in range(n_levels):
        last = l + 1 == n_levels
        Dinv = block_inverse(diag_blocks(A), dt)
        L = dict(N=N, M=M, A=A, Dinv=Dinv, kind=last_kind if last else "inner")
        if not (last and last_kind == "dense"):
            L["lam"] = power_lambda(A, Dinv, dt)
            L["omega"] = omega_of(L["lam"])
        if last:
            if last_kind == "dense":
                Ci = np.linalg.inv(np.asarray(A, dtype=np.float64))
                L["Cinv"] = (0.5 * (Ci + Ci.T)).astype(np.float32 if single else np.float64)
        else:
            L["A32"] = A.astype(np.float32) if single else A
            P = prolongation(N, M).astype(dt)
            src = L["A32"].astype(dt) if s_from_rounded else A
            Dd = np.zeros_like(A)
            for k in range(len(Dinv)):
                Dd[3 * k:3 * k + 3, 3 * k:3 * k + 3] = Dinv[k]
            L["S32"] = (P.T @ src @ Dd).astype(np.float32 if single else dt)
            A = P.T @ A @ P
            N //= 2; M //= 2
        lv.append(L)
    return lv


def _as(d, key, dt):
    """d[key] in scalar type dt (dense or scipy sparse), converted once and kept beside the original"""
    k = (key, np.dtype(dt).name)
    if k not in d:
        a = d[key]
        if hasattr(a, "indptr"):
            import scipy.sparse as sp
            a = sp.csr_matrix(a)
            d[k] = sp.csr_matrix((a.data.astype(dt), a.indices, a.indptr), shape=a.shape)
        else:
            d[k] = np.asarray(a, dtype=dt)
    return d[k]


def _P(d, N, M, dt):
    k = ("P", np.dtype(dt).name)
    if k not in d:
        d[k] = prolongation_sp(N, M, dt)
    return d[k]


def _stencil_cycle(lv, l, r, dt, mut):
    L = lv[l]
    Dinv = _as(L, "Dinv", dt)
    if L["kind"] == "dense":
        return _as(L, "Cinv", dt) @ r
    om = dt(L["omega"]) * (2 if mut == ("omega", l) else 1)
    x = om * block_apply(Dinv, r)
    if L["kind"] == "inner":
        P = _P(L, L["N"], L["M"], dt)
        rc = P.T @ r - om * (_as(L, "S32", dt) @ r)           # fused first sweep: P^T (r - A x) with x = omega Dinv r
        xc = np.zeros(rc.shape, dt) if mut == ("drop", l) else _stencil_cycle(lv, l + 1, rc, dt, mut)
        xt = x + P @ xc
        return xt + om * block_apply(Dinv, r - _as(L, "A32", dt) @ xt)
    A = _as(L, "A", dt)                                                     # a smoothed last level reads the double-precision operator
    prev = x
    for _ in range(1, LAST_SWEEPS):
        prev, x = x, x + om * block_apply(Dinv, r - A @ x)
    return prev if mut == ("pingpong", l) else x


def cycle(pc, r, dt=np.float64, mut=None):
    """z = M^-1 r, one V(1,1) cycle.  pc: H0 (level-0 operator as the smoother reads it, dense or scipy sparse), Dinv0 ((NV, 3, 3), zero on the rows of dense
    bodies), omega0, cloths: [dict(v_offset, N0, M0, levels)], bodies: [(dof indices, Binv dense)].  mut: a deliberate defect for the
    mutation checks -- ("restrict", 0) halves the weight of a boundary fine node onto its own coarse node, ("drop", l) skips the coarse
    correction below level l, ("omega", l) doubles a damping factor, ("pingpong", l) returns the last-but-one iterate of a smoothed last level"""
    r = np.asarray(r, dtype=dt)
    H0 = _as(pc, "H0", dt)
    D0 = _as(pc, "Dinv0", dt)
    om = dt(pc["omega0"])
    bodies = [(idx, np.asarray(B, dtype=dt)) for idx, B in pc.get("bodies", [])]
    z = om * block_apply(D0, r)
    for idx, B in bodies:
        z[idx] = B @ r[idx]
    t = H0 @ z
    for c in pc["cloths"]:
        n0 = nodes(c["N0"], c["M0"])
        dofs = 3 * c["v_offset"] + np.arange(3 * n0)
        P = _P(c, c["N0"], c["M0"], dt)
        R = P.T
        if mut == ("restrict", 0):
            R = R.tolil()
            for J in range(c["M0"] // 2 + 1):      # coarse row I = 0: fine node (0, 2J)
                for e in range(3):
                    R[3 * J + e, 3 * (2 * J) + e] = 0.5
            R = R.tocsr()
        x1 = _stencil_cycle(c["levels"], 0, R @ (r - t)[dofs], dt, mut)
        z[dofs] += P @ x1
    t = H0 @ z
    zn = z + om * block_apply(D0, r - t)
    for idx, B in bodies:
        zn[idx] = z[idx] + B @ (r - t)[idx]
    return zn


def cycle_matrix(pc, n, dt=np.float64, mut=None):
    return np.stack([cycle(pc, e, dt, mut) for e in np.eye(n, dtype=dt)], 1)


# ------------------------------------------------------------------------------------------------ PCG through it
def pcg(H, b, precond, cg_tol, scale=1.0, maxit=2000, max_restarts=20):
    """The engine's restarted PCG: the recurrence stops at |r_k| <= 0.5 tol |b| on the RECURRENCE residual, then the true residual b - H x
    decides (<= tol |b|: done; else a restart from it).  tol = scale * cg_tol.  Returns (x, updates of x performed, converged)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    nb = np.linalg.norm(b)
    tol = scale * cg_tol * nb
    it = 0
    for outer in range(max_restarts):
        r = b - H @ x
        if np.linalg.norm(r) <= tol:
            return x, it, True
        z = precond(r)
        rz = r @ z
        p = z.copy()
        while it < maxit:
            Ap = H @ p
            alpha = rz / (p @ Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            it += 1
            if np.linalg.norm(r) <= 0.5 * tol:
                break
            z = precond(r)
            rz, rz_old = r @ z, rz
            p = z + (rz / rz_old) * p
        if it >= maxit:
            break
    return x, it, bool(np.linalg.norm(b - H @ x) <= tol)


def pcg_window(H, b, precond, cg_tol, **kw):
    """(first count at a 4x looser threshold, count at the threshold, first count at a 4x tighter one)"""
    return tuple(pcg(H, b, precond, cg_tol, s, **kw)[1] for s in (4.0, 1.0, 0.25))


# ------------------------------------------------------------------------------------------------ operators for the tests
def oracle_drape(oracle, N, M, seed=0, amp=5e-5, spd=True, Kb=100.0, k_angle=3.14):
    """the drape of test_gpu_cloth._pair on the CPU oracle alone (same perturbation stream, last vertex row pinned): (H csr, residual F, frozen dofs)"""
    o = oracle.OracleScene(dt=5e-3, gravity=(0, 0, -9.8), newton_cap=50, plastic=0)
    ci = o.add_cloth(N, M, 0.1 / 15 * N)
    o.cloth_init(ci, 0, 0, 0)
    o.finalize()
    o.set_scalar("cloth0.Kb", Kb); o.set_scalar("cloth0.k_angle", k_angle)
    rng = np.random.default_rng(seed)
    x = o.pos.copy()
    x += rng.normal(0, amp, x.shape)
    o.pos[:] = x
    o.prev_pos[:] = x - rng.normal(0, 0.3 * amp, x.shape)
    o.vel[:] = rng.normal(0, 1e-2, x.shape)
    o.arr("cloth0.ref_angle", (-1, 3))[:] = rng.normal(0, 0.05, (2 * N * M, 3))
    fr = o.frozen.reshape(-1, 3)
    fr[N * (M + 1):(N + 1) * (M + 1)] = 1
    o.push_down_all()
    o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(spd)
    return o.H_csr(), o.arr("F").copy(), o.frozen.copy().ravel()


def restated_pc(H, N, M, n_levels, last_kind, dt=np.float64, s_from_rounded=True, single=True):
    """the whole preconditioner of a one-cloth scene formed here from its operator H (dense or sparse): what `cycle` takes"""
    Hd = np.asarray(H.todense()) if hasattr(H, "todense") else np.asarray(H)
    D0 = block_inverse(diag_blocks(Hd), dt)
    H32 = Hd.astype(np.float32).astype(np.float64) if single else Hd
    lam0 = power_lambda(H32, D0, dt)
    A1 = galerkin(Hd, N, M, dt)
    return dict(H0=H32, Dinv0=D0, omega0=omega_of(lam0), lam0=lam0,
                cloths=[dict(v_offset=0, N0=N, M0=M, levels=build_hierarchy(A1, N // 2, M // 2, n_levels, last_kind, dt, s_from_rounded, single))])


def transposed_in_one_slot(S32, N, M, dI=1, dJ=0):
    """the dense S of a level whose fine grid is (N+1) x (M+1) with the 3 x 3 blocks of ONE of its 49 slots transposed (a mutation check's defect)"""
    S, _ = s_slots_from_dense(np.asarray(S32), N, M, np.float32)
    nc = nodes(N // 2, M // 2)
    S = S.reshape(49, 9, nc).copy()
    s = (dI + 3) * 7 + dJ + 3
    S[s] = S[s].reshape(3, 3, nc).transpose(1, 0, 2).reshape(9, nc)
    return s_dense_from_slots(S.ravel(), N, M, np.float32)
