"""The multigrid preconditioner taken apart on the GPU: every array of a set-up (tsl_mg_export) and the cycle itself (tsl_mg_apply) against the
restatement in mg_numpy.py, quantity by quantity, and PCG through the cycle against the restated PCG's iteration window.

A solve that returns the spsolve answer says nothing about the preconditioner: PCG converges behind a wrong M^-1, only more slowly.  Here each
quantity is compared with its own reference formed from the engine's own exported inputs of that step, so that one level's error is not charged to
the next.  Bounds: Galerkin entries 81 u P^T |A| P (sums of at most 9 x 9 exactly weighted terms in any order); block inverses, power
iterations and cycles by tet_numpy.bound, 8 max(e64, 4 u |ref|) with e64 the float64 restatement against its 50-digit / long-double run; single-precision
copies exactly or to one float32 ulp; dense inverses by their residual against numpy.linalg.inv's, rounded the same way."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import berr
import mg_numpy as mg
from tet_numpy import bound

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53

# shape -> (N, M, {param: value}): what each exercises is in DESIGN.md 9j
CASES = {
    "8x8_dense75": (8, 8, dict(mg_dense_nodes=64)),
    "8x8_one_workgroup": (8, 8, dict(mg_coarse_exact=0)),
    "12x20": (12, 20, dict()),
    "32x16_dense45": (32, 16, dict(mg_dense_nodes=64)),
    "32x16_one_workgroup": (32, 16, dict(mg_coarse_exact=0)),
    "34x18_per_sweep": (34, 18, dict(mg_dense_nodes=100)),
    "50x26_per_sweep": (50, 26, dict(mg_dense_nodes=100)),     # 364 nodes smoothed: where the PCG window sees the wrong ping-pong buffer (test_mg_numpy.py)
    "64x64_dense243": (64, 64, dict(mg_dense_nodes=100)),      # 81 nodes: 8 tiles of 32, the last partly filled
    "64x64_dense867": (64, 64, dict(mg_dense_nodes=300)),      # 289 nodes: 28 tiles
}
SMALL = ("8x8_dense75", "8x8_one_workgroup", "12x20")     # every unit vector goes through the cycle
_cache = {}


class Ratios(dict):
    def add(self, q, err, bnd):
        err = np.asarray(err, dtype=np.float64); bnd = np.asarray(bnd, dtype=np.float64)
        ok = bnd > 0
        r = float(np.max(err[ok] / bnd[ok])) if ok.any() else 0.0
        if np.any(err[~ok] > 0):
            r = float("inf")
        self[q] = max(self.get(q, 0.0), r)

    def check(self, what):
        print("multigrid, %s: largest |gpu - ref| / bound: %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (what, bad)


def _ld(A):
    A = sp.csr_matrix(A)
    return sp.csr_matrix((A.data.astype(LD), A.indices, A.indptr), shape=A.shape)


class Case:
    """one context after an assembly, with every array of its preconditioner set-up on the host.  cloths: [(v_offset, N, M)] of the cloths that have a
    hierarchy, bodies: [(v_offset, n_verts)] of the dense bodies, both in the engine's order"""

    def __init__(self, name, ctx, b, cloths, bodies=(), keep=None):
        self.name, self.ctx, self.b, self.keep = name, ctx, b, keep
        self.info = ctx.mg_info()
        assert [(h["v_offset"], h["N0"], h["M0"]) for h in self.info["hierarchies"]] == list(cloths), self.info
        assert self.info["bodies"] == [3 * nv for _, nv in bodies], self.info
        self.Hs = ctx.matrix_csr()                                   # static part, what vals32 is the rounded copy of
        self.H = ctx.operator_csr() if len(ctx.constraints()["idx"]) else self.Hs
        self.NV = self.H.shape[0] // 3
        self.cdiag = sp.bsr_matrix(sp.block_diag(list(_diag0(self.H - self.Hs)))).tocsr() if self.H is not self.Hs else None
        H32 = self.Hs.copy()
        H32.data = H32.data.astype(np.float32).astype(np.float64)
        self.H32 = H32 if self.cdiag is None else sp.csr_matrix(H32 + (self.H - self.Hs))    # the smoother's level 0: rounded matrix + contact blocks
        self.Dinv0 = ctx.mg_export("Dinv", 0, -1).reshape(self.NV, 3, 3)
        self.omega0, self.lam0 = ctx.mg_export("omega", 0, -1)
        self.rowpos = ctx.mg_export("rowpos", 0, -1)
        assert sorted(self.rowpos) == list(range(self.NV))
        self.hier = []
        for h, H in enumerate(self.info["hierarchies"]):
            levels = []
            for l, L in enumerate(H["levels"]):
                n = mg.nodes(L["N"], L["M"])
                E = dict(N=L["N"], M=L["M"], kind=L["kind"], n=n)
                E["A_slots"] = ctx.mg_export("A", h, l)
                E["A"] = mg.dense_from_slots(E["A_slots"], L["N"], L["M"])
                E["Dinv"] = ctx.mg_export("Dinv", h, l).reshape(n, 3, 3)
                if L["kind"] == "dense":
                    E["Cinv"] = ctx.mg_export("Cinv", h, l, size=9 * n * n).reshape(3 * n, 3 * n)
                    E["bad"] = int(ctx.mg_export("bad", h, l)[0])
                else:
                    E["omega"], E["lam"] = ctx.mg_export("omega", h, l)
                if L["kind"] == "inner":
                    E["A32_slots"] = ctx.mg_export("A32", h, l)
                    E["S32_slots"] = ctx.mg_export("S32", h, l)
                    E["A32"] = sp.csr_matrix(mg.dense_from_slots(E["A32_slots"], L["N"], L["M"], np.float32))      # (sparse: the cycle applies them often)
                    E["S32"] = sp.csr_matrix(mg.s_dense_from_slots(E["S32_slots"], L["N"], L["M"], np.float32))
                levels.append(E)
            self.hier.append(dict(v_offset=H["v_offset"], N0=H["N0"], M0=H["M0"], levels=levels))
        self.bodies = []
        for k, (off, nv) in enumerate(bodies):
            n3 = 3 * nv
            ld = (n3 + 3) & ~3
            B = ctx.mg_export("Binv", k, 0, size=n3 * ld).reshape(n3, ld)
            assert not B[:, n3:].any()                                # the row padding multiplies zeros and must stay zero
            self.bodies.append(dict(dofs=3 * off + np.arange(n3), Binv=B[:, :n3].copy(), bad=int(ctx.mg_export("bad_body", k, 0)[0])))
        self.pc = dict(H0=self.H32, Dinv0=self.Dinv0, omega0=self.omega0, cloths=self.hier, bodies=[(B["dofs"], B["Binv"]) for B in self.bodies])
        self.N, self.M = cloths[0][1], cloths[0][2]
        self.levels = self.hier[0]["levels"]

    def fine_operator(self, h):
        """the cloth block of the matrix plus the contact diagonal: what the first Galerkin product of hierarchy h takes"""
        c = self.hier[h]
        d = 3 * c["v_offset"] + np.arange(3 * mg.nodes(c["N0"], c["M0"]))
        A = self.Hs if self.cdiag is None else sp.csr_matrix(self.Hs + self.cdiag)
        return sp.csr_matrix(A[d][:, d])

    def apply(self, R):
        """columns of R through tsl_mg_apply"""
        out = np.empty_like(R)
        for k in range(R.shape[1]):
            r = torch.as_tensor(np.ascontiguousarray(R[:, k]), device=self.b.device)
            out[:, k] = self.ctx.mg_apply(r).cpu().numpy()
        return out


def _drape(oracle, name):
    from test_gpu_cloth import _pair
    N, M, params = CASES[name]
    sys, _ = _pair(oracle, N, M, amp=5e-5)
    ctx = sys._ensure_ctx()
    for k, v in params.items():
        ctx.set_param(k, v)
    sys.compute_residual_and_Hessian(spd=True)
    fr = sys.frozen.to_numpy().reshape(-1, 3)
    assert fr[N * (M + 1):].all() and not fr[:N * (M + 1)].any()     # the pinned row keeps its masked rows in play
    return Case(name, ctx, sys.F.to_torch(), [(0, N, M)], keep=sys)


def _two_cloths(oracle, name):
    """a 16 x 16 and a 12 x 24 cloth in one context, two levels each: the second hierarchy starts at v_offset = 289 (rowpos, v_offset != 0)"""
    import cloth_numpy as cn
    from thinshelllab_amd.context import TslContext
    dx = 0.1 / 15
    cl = [cn.ClothTables(16, 16, dx, v_offset=0), cn.ClothTables(12, 24, dx, v_offset=17 * 17)]
    nv = cl[0].NV + cl[1].NV
    frozen = np.zeros((nv, 3), np.int32)
    x = np.zeros((nv, 3)); ra = []
    rng = np.random.default_rng(5)
    for k, c in enumerate(cl):
        i, j = cn.grid(c)
        x[c.v_offset:c.v_offset + c.NV] = np.stack([i * c.dx, j * c.dx, np.full(len(i), 0.05 * k)], 1)
        frozen[c.v_offset + c.N * (c.M + 1):c.v_offset + c.NV] = 1
        ra.append(rng.normal(0, 0.05, (c.NF, 3)).ravel())
        c.desc["mass"] = 40.0 * c.dx * c.dx
    x += rng.normal(0, 5e-5, x.shape)
    mass = np.concatenate([np.full(c.NV, c.desc["mass"]) for c in cl])
    ctx = TslContext(tot_NV=nv, dt=5e-3, mass=mass, gravity=np.tile([0.0, 0.0, -9.8], (nv, 1)), frozen=frozen.ravel(), cloths=[c.desc for c in cl])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
    pos, prev, vel, ref = dev(x), dev(x - rng.normal(0, 1.5e-5, x.shape)), dev(rng.normal(0, 1e-2, x.shape)), dev(np.concatenate(ra))
    g = torch.zeros(3 * nv, dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=True, grad=g)
    torch.cuda.synchronize()
    return Case(name, ctx, -g, [(0, 16, 16), (289, 12, 24)], keep=(pos, prev, vel, ref, g))


def _balancing(oracle, name):
    """the 16 x 8 balancing scene of test_gpu_scenes at a state with detected contacts: contact diagonal in the Galerkin product, dense body blocks"""
    from thinshelllab_amd.engine.geometry import projection_query
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=0.064, cloth_N=16, cloth_M=8)
    s.init_all()
    s.mu_cloth_elastic[None] = 5.0
    c = s.cloths[0]
    x = s.pos.to_numpy()
    x[c.offset:c.offset + c.NV, 2] += 2e-6 * np.sin(0.7 * np.arange(c.NV) + 0.3)
    s.pos.from_numpy(x); s.prev_pos.from_numpy(x)
    ctx = s._ensure_ctx()
    projection_query(s)
    s.compute_residual_and_Hessian(spd=True)
    assert len(ctx.constraints()["idx"]) > 0
    fr = s.frozen.to_numpy().reshape(-1, 3)
    bodies = [(e.offset, e.n_verts) for e in s.elastics if 2 <= e.n_verts <= 512 and not fr[e.offset:e.offset + e.n_verts].all()]
    return Case(name, ctx, s.F.to_torch(), [(c.offset, 16, 8)], bodies, keep=s)


BUILDERS = {"two_cloths": _two_cloths, "balancing_16x8": _balancing}
EXTRA = list(BUILDERS)


def _get(oracle, name):
    if name not in _cache:
        _cache[name] = BUILDERS.get(name, _drape)(oracle, name)
    return _cache[name]


@pytest.fixture
def case(oracle, request):
    return _get(oracle, request.param)


all_cases = pytest.mark.parametrize("case", list(CASES) + EXTRA, indirect=True)


def test_level_lists_are_the_ones_each_shape_is_here_for(oracle):
    want = {"8x8_dense75": [(4, 4, "dense")], "8x8_one_workgroup": [(4, 4, "inner"), (2, 2, "one_workgroup")],
            "12x20": [(6, 10, "inner"), (3, 5, "dense")], "32x16_dense45": [(16, 8, "inner"), (8, 4, "dense")],
            "32x16_one_workgroup": [(16, 8, "inner"), (8, 4, "inner"), (4, 2, "one_workgroup")], "34x18_per_sweep": [(17, 9, "per_sweep")], "50x26_per_sweep": [(25, 13, "per_sweep")],
            "64x64_dense243": [(32, 32, "inner"), (16, 16, "inner"), (8, 8, "dense")], "64x64_dense867": [(32, 32, "inner"), (16, 16, "dense")]}
    for name in CASES:
        got = [(L["N"], L["M"], L["kind"]) for L in _get(oracle, name).levels]
        assert got == want[name], (name, got)


def _galerkin(Af, N, M, Ac_slots, R, tag):
    """Ac_slots against P^T Af P formed in long double from the sparse fine operator Af on the (N+1) x (M+1) grid"""
    P = mg.prolongation_sp(N, M, LD)
    A = _ld(Af)
    ref = np.asarray((P.T @ A @ P).todense())
    aref = np.asarray((P.T @ abs(A) @ P).todense())
    bnd = 81 * U * aref
    ref_slots, outside = mg.slots_from_dense(ref, N // 2, M // 2, LD)
    assert outside == 0.0, (tag, outside)          # the coarse operator has radius 2: nothing of the reference is lost in the slot layout
    bnd_slots, _ = mg.slots_from_dense(bnd, N // 2, M // 2, LD)
    got = np.asarray(Ac_slots, dtype=LD)
    R.add(tag, np.abs(got - ref_slots).astype(np.float64), bnd_slots.astype(np.float64))
    # symmetry across slots: the coarse operator is as symmetric as its fine one
    Ad = mg.dense_from_slots(Ac_slots, N // 2, M // 2, LD)
    asym = np.asarray((P.T @ abs(A - A.T) @ P).todense())
    R.add(tag + "_sym", np.abs(Ad - Ad.T).astype(np.float64), (asym + 2 * bnd).astype(np.float64))


@all_cases
def test_galerkin_operators(case):
    R = Ratios()
    for h, c in enumerate(case.hier):
        lv = c["levels"]
        _galerkin(case.fine_operator(h), c["N0"], c["M0"], lv[0]["A_slots"], R, "A1")
        for l in range(len(lv) - 1):
            _galerkin(sp.csr_matrix(lv[l]["A"]), lv[l]["N"], lv[l]["M"], lv[l + 1]["A_slots"], R, "A%d" % (l + 2))
    R.check(case.name + " Galerkin")


def _mp_blocks(D):
    import mpmath as mp
    return np.array([mp.mpf(float(v)) for v in np.asarray(D).ravel()], dtype=object).reshape(np.shape(D))


def _dinv_check(D, got, R, tag):
    """(n, 3, 3) exported inverses against the 50-digit inverse of the blocks D, per block in the Frobenius norm"""
    import mpmath as mp
    with mp.workdps(50):
        ref = mg.block_inverse(_mp_blocks(D), object)
        f64 = mg.block_inverse(D, np.float64)
        e64 = np.array([float(mp.sqrt(sum((mp.mpf(float(a)) - b) ** 2 for a, b in zip(f.ravel(), r.ravel())))) for f, r in zip(f64, ref)])
        nrm = np.array([float(mp.sqrt(sum(b * b for b in r.ravel()))) for r in ref])
        err = np.array([float(mp.sqrt(sum((mp.mpf(float(a)) - b) ** 2 for a, b in zip(g.ravel(), r.ravel())))) for g, r in zip(got, ref)])
    R.add(tag, err, np.array([bound(e, n) for e, n in zip(e64, nrm)]))


@all_cases
def test_diagonal_inverses(case):
    R = Ratios()
    point = np.ones(case.NV, bool)
    for B in case.bodies:       # rows of dense bodies are served by their block: exactly zero
        point[B["dofs"][::3] // 3] = False
    assert not case.Dinv0[~point].any()
    _dinv_check(_diag0(case.H)[point], case.Dinv0[point], R, "Dinv0")
    for c in case.hier:
        for l, L in enumerate(c["levels"]):
            _dinv_check(mg.diag_blocks(L["A"]), L["Dinv"], R, "Dinv%d" % (l + 1))
    R.check(case.name + " diagonal inverses")


def _diag0(H):
    B = sp.bsr_matrix(H, blocksize=(3, 3))
    B.sort_indices()
    n = H.shape[0] // 3
    out = np.zeros((n, 3, 3))
    for i in range(n):
        for k in range(B.indptr[i], B.indptr[i + 1]):
            if B.indices[k] == i:
                out[i] = B.data[k]
    return out


def _lam_check(A, Dinv, om, lam, R, tag, eig=True, rows=None):
    assert om == min(0.8, 1.5 / lam), (tag, om, lam)           # bit for bit: one division and one minimum
    ref = mg.power_lambda(_ld(A) if sp.issparse(A) else A, Dinv, LD, rows=rows)
    f64 = mg.power_lambda(A, Dinv, np.float64, rows=rows)
    R.add(tag, abs(LD(lam) - ref), bound(float(abs(LD(f64) - ref)), float(ref)))
    if eig:   # what omega is for: the damped block-Jacobi iteration converges
        Dd = sp.block_diag(list(Dinv)).tocsr()
        T = Dd @ A
        n = T.shape[0]
        lmax = np.abs(np.linalg.eigvals(np.asarray(T.todense()) if sp.issparse(T) else T)).max() if n <= 2000 else \
            abs(sp.linalg.eigs(sp.csr_matrix(T), k=1, which="LM", return_eigenvectors=False, tol=1e-10)[0])
        assert om * lmax < 2.0, (tag, om, lmax)
        return float(om * lmax)
    return None


@all_cases
def test_damping_factors(case):
    import scipy.sparse.linalg  # noqa: F401
    R = Ratios()
    prod = {"omega0": _lam_check(case.H32, case.Dinv0, case.omega0, case.lam0, R, "lambda0", rows=case.rowpos)}
    for h, c in enumerate(case.hier):
        for l, L in enumerate(c["levels"]):
            if L["kind"] == "dense":
                assert "omega" not in L            # solved exactly: no smoother, skipped by construction
                continue
            prod["omega%d.%d" % (h, l + 1)] = _lam_check(L["A"], L["Dinv"], L["omega"], L["lam"], R, "lambda%d.%d" % (h, l + 1))
    print("multigrid, %s: omega * lambda_max(D^-1 A): %s" % (case.name, ", ".join("%s %.3f" % kv for kv in sorted(prod.items()))))
    R.check(case.name + " damping factors")


def _inverse_residual(X, A):
    """max |X A - I| accumulated in long double.  The rows that can hold the maximum are found in float64 first (its accumulation error, below
    1e-9 of the entries of |X||A|, is far below half the maximum of a float32 inverse's residual); only those are formed in long double."""
    n = len(A)
    R = np.abs(np.asarray(X, dtype=np.float64) @ A - np.eye(n)).max(1)
    rows = np.nonzero(R >= 0.5 * R.max())[0]
    assert 1e-9 * (np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(A)).max() < 0.25 * R.max()
    return float(np.abs(np.asarray(X, dtype=LD)[rows] @ A.astype(LD) - np.eye(n, dtype=LD)[rows]).max())


def dense_inverse_residuals(A, X):
    """(max |X A - I| of the exported inverse, the same of numpy.linalg.inv(A) symmetrised and rounded to float32)"""
    A = np.asarray(A, dtype=np.float64).copy()
    for i in np.nonzero(np.diag(A) == 0.0)[0]:
        A[i, i] = 1.0                           # empty rows are identity rows in the engine's dense matrix too
    Ci = np.linalg.inv(A)
    ref = (0.5 * (Ci + Ci.T)).astype(np.float32)
    return _inverse_residual(X, A), _inverse_residual(ref, A)


def _inverse_check(name, what, A, X, bad):
    assert bad == 0
    assert X.dtype == np.float32 and np.array_equal(X, X.T)                   # symmetric bit for bit
    got, ref = dense_inverse_residuals(A, X)
    print("multigrid, %s: %s n3 %d: max |X A - I| gpu %.3e, numpy.linalg.inv in float32 %.3e, ratio %.3f (allowed 4)" % (name, what, len(X), got, ref, got / ref))
    assert got <= 4 * ref, (got, ref)


@pytest.mark.parametrize("case", [k for k in CASES if "dense" in k or k == "12x20"] + EXTRA, indirect=True)
def test_coarse_and_body_inverses(case):
    for c in case.hier:
        L = c["levels"][-1]
        assert L["kind"] == "dense"
        _inverse_check(case.name, "Cinv", L["A"], L["Cinv"], L["bad"])
    for k, B in enumerate(case.bodies):
        d = B["dofs"]
        _inverse_check(case.name, "Binv%d" % k, case.H[d][:, d].toarray(), B["Binv"], B["bad"])


@pytest.mark.parametrize("case", [k for k in CASES if k not in ("8x8_dense75", "34x18_per_sweep", "50x26_per_sweep")] + ["two_cloths"], indirect=True)
def test_single_precision_copies(case):
    R = Ratios()
    for l, L in [(l, L) for c in case.hier for l, L in enumerate(c["levels"][:-1])]:
        assert L["A32_slots"].dtype == np.float32 and np.array_equal(L["A32_slots"], L["A_slots"].astype(np.float32)), l     # exactly the rounded operator
        P = mg.prolongation_sp(L["N"], L["M"], LD)
        Dd = _ld(sp.block_diag(list(L["Dinv"])))
        ref = np.asarray((P.T @ _ld(L["A32"]) @ Dd).todense())
        ref32, outside = mg.s_slots_from_dense(ref, L["N"], L["M"], LD)
        assert outside == 0.0
        ref32 = ref32.astype(np.float32)
        got = L["S32_slots"]
        assert got.dtype == np.float32
        # a double-precision sum that straddles a float32 rounding boundary may land on the neighbour: one ulp of the reference entry
        R.add("S32_%d" % (l + 1), np.abs(got.astype(np.float64) - ref32.astype(np.float64)), np.spacing(np.abs(ref32)).astype(np.float64))
        zero = ref32 == 0
        assert np.all(got[zero] == 0), l
    R.check(case.name + " single-precision copies")


def _vectors(case):
    n = 3 * case.NV
    if case.name in SMALL:
        return np.eye(n)
    rng = np.random.default_rng(11)
    V = [rng.normal(size=n) for _ in range(32)]
    verts = []
    for c in case.hier:     # corners, edges, the row next to the pinned one, pinned vertices of every cloth
        N, M = c["N0"], c["M0"]
        verts += [c["v_offset"] + v for v in (0, M, M // 2, (N // 2) * (M + 1), (N // 2) * (M + 1) + M, (N - 1) * (M + 1) + 1, N * (M + 1), N * (M + 1) + M // 2,
                                                 (N + 1) * (M + 1) - 1)]
    for B in case.bodies:   # first, a middle and the last vertex of every dense body
        verts += [int(B["dofs"][0]) // 3, int(B["dofs"][len(B["dofs"]) // 2]) // 3, int(B["dofs"][-1]) // 3]
    for v in verts:
        for d in range(3):
            e = np.zeros(n); e[3 * v + d] = 1.0
            V.append(e)
    return np.stack(V, 1)


@all_cases
def test_cycle(case):
    R = Ratios()
    V = _vectors(case)
    Z = case.apply(V)
    for k in range(V.shape[1]):
        ref = mg.cycle(case.pc, V[:, k], LD)
        f64 = mg.cycle(case.pc, V[:, k], np.float64)
        nrm = lambda v: float(np.sqrt(np.dot(v, v)))
        R.add("cycle", nrm(Z[:, k].astype(LD) - ref), bound(nrm(f64.astype(LD) - ref), nrm(ref)))
    assert np.array_equal(case.apply(V[:, :3]), Z[:, :3])       # a second application returns the same bits
    if case.name in SMALL:
        w = np.linalg.eigvalsh(0.5 * (Z + Z.T))
        asym = np.abs(Z - Z.T).max() / np.abs(Z).max()
        print("multigrid, %s: symmetrised cycle matrix: eigenvalues %.3e .. %.3e, |Z - Z^T| / |Z| %.2e" % (case.name, w.min(), w.max(), asym))
        assert w.min() > 0
    R.check(case.name + " cycle, %d vectors" % V.shape[1])


@all_cases
def test_pcg_through_the_cycle(case):
    ctx = case.ctx
    b = case.b.cpu().numpy()
    x, st = ctx.solve_with(0, case.b)
    x = x.cpu().numpy()
    cg_tol = 1e-10           # the engine's default
    lo, mid, hi = mg.pcg_window(case.H, b, lambda r: mg.cycle(case.pc, r), cg_tol)
    r = berr.residual(case.H, x, b)
    ev = 64 * U * (abs(_ld(case.H)) @ np.abs(x).astype(LD) + np.abs(b).astype(LD))
    nb = np.sqrt(np.dot(b.astype(LD), b.astype(LD)))
    rel = float(np.sqrt(np.dot(r, r)) / nb)
    print("multigrid, %s: PCG iterations gpu %d, restated %d, window [%d, %d]; true residual %.3e |b|" % (case.name, st["iters"], mid, lo, hi, rel))
    assert st["flag"] == 0 and st["method"] == 0
    assert rel <= cg_tol + float(np.sqrt(np.dot(ev, ev)) / nb)
    assert lo <= st["iters"] <= hi, (st["iters"], lo, mid, hi)
