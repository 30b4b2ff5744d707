"""The operator of the Krylov solvers alone: y = H x in the SELL-64 layout plus the matrix-free contact rows by every kernel that forms it (tsl_op_apply),
its tables, masks and diagonals as the next solve reads them (tsl_op_export), and the first iterations of a PCG run state by state (tsl_pcg_trace),
each against the restatement of tests/op_numpy.py evaluated in long double from the exported inputs of that very kernel.  DESIGN.md 9k.

A solve that meets cg_tol says nothing about a product that feeds no solve (the variants tsl_bench_spmv times), about an error that PCG absorbs at the
price of iterations (a wrong beta, a stale Ap in the recurrence A p_new = A z + beta A p_old), or about a preconditioner built from the values before
the last import.

Bounds are derived, none is measured (u = 2^-53, gamma(n) = n u / (1 - n u), n the operations on the longest path):
  product      |y - ref|_i <= gamma(3 slice_len + 12 entries_i + 8) (|H||x|)_i: a block column costs its row a multiplication and two additions (a
               masked repeat as many), a contact entry twelve (four 3-vectors), the joins of the waves, of the lanes of a contact row and of the two
               parts at most eight; kernels without contact rows are held against the static matrix alone
  dot, part    the rows' product bounds times |x_i|, plus gamma(3 NV + 16) sum |x_i y_i| for the summation in any order
  c_diag       (entries_i + 7) u sum |H|: entries_i - 1 additions in any order, lanes joined by a tree of six
  Dinv         tet_numpy.bound = 8 max(e64, 4 u |ref|_F) against the 50-digit inverse of the exported diagonal block plus c_diag (as 9j)
  one PCG step, everything from the exported state after n and after n + 1 iterations (one step: conditioning does not enter):
    rz, rr     gamma(n_part) sum |part| (the partials of the state after n, any order)
    beta       rz / rz_old: e_beta = gamma(n_part + 2) sum |part_rz| / |rz_old|
    p          e_beta |p_old| + gamma(2) (|z| + |beta p_old|)
    Ap         product bound of H z + e_beta |Ap_old| + gamma(2) (|H||z| + |beta Ap_old|)
    part_pAp   gamma(192) sum |p_i Ap_i| over the slice, from the exported p and Ap (the registers the kernel stored)
    alpha      rz / sum(part_pAp): e_alpha = gamma(n_slices + 2) |alpha| sum |part_pAp| / |pAp|
    x, r       e_alpha |p| + gamma(2) (|x| + |alpha p|), the same with Ap
    z          block Jacobi: gamma(3) |Dinv||r| (a multiplication and two additions); multigrid: the restated cycle under 9j's bound
    part_rr    gamma(768) sum r_i^2 over the 256 rows; part_rz the same with |r_i z_i| (block Jacobi), else its sum with gamma(3 NV + n_part)
Bit equality is asked only where it is the claim: masks, tables, a second call, a repeated run, the captured graph against eager launches."""
import numpy as np
import pytest
import torch

import cloth_numpy as cn
import mg_numpy as mg
import op_numpy as op
from scene_tables_numpy import expected_tables
from tet_numpy import bound

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = op.U
g = op.gamma
_cache = {}
NAMES = ["cloth_1x1", "drape_8x8", "drape_12x20_ties", "balancing_16x8"]
PCG_NAMES = ["drape_8x8", "drape_12x20_ties", "balancing_16x8"]


class Ratios(dict):
    def add(self, q, err, bnd):
        err = np.atleast_1d(np.asarray(err, dtype=np.float64)); bnd = np.atleast_1d(np.asarray(bnd, dtype=np.float64))
        ok = bnd > 0
        r = float(np.max(err[ok] / bnd[ok])) if ok.any() else 0.0
        if np.any(err[~ok] > 0) or not np.all(np.isfinite(err)):
            r = float("inf")
        self[q] = max(self.get(q, 0.0), r)

    def check(self, what):
        print("operator alone, %s: largest |gpu - ref| / bound: %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (what, bad)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")


class Case:
    """a context with an assembled operator; use("assembled" | "imported") switches the static values; every array in the solver's row order"""

    def __init__(self, name, ctx, args, frozen, mass, dt, assemble, keep, bodies=()):
        self.name, self.ctx, self.args, self.assemble, self.keep, self.bodies = name, ctx, args, assemble, keep, bodies
        self.NV = int(args["tot_NV"])
        self.frozen = np.asarray(frozen).reshape(self.NV, 3).astype(np.int64)
        self.mass, self.dt = np.asarray(mass, np.float64), float(dt)
        self.T = {k: ctx.op_export(k).astype(np.int64) for k in ("slice_off", "slice_len", "colidx", "perm", "rowpos", "diag_perm")}
        self.cons = ctx.constraints()["idx"].astype(np.int64)
        self.nc = len(self.cons)
        self.cr = op.contact_csr(self.cons, self.T["rowpos"], self.NV) if self.nc else (np.zeros(self.NV + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, 4), np.int64))
        self.cnt = np.diff(self.cr[0])
        self.state = "assembled"
        self.nnzb = len(ctx.matrix()[1])
        rng = np.random.default_rng(17)
        self.rhs = _dev(rng.normal(size=3 * self.NV))
        cv = int(self.T["rowpos"][self.cons[0, 3]]) if self.nc else self.NV // 2
        self.units = sorted({0, min(63, self.NV - 1), min(64, self.NV - 1), self.NV - 1, cv})
        self.X = op.seeded_vectors(self.NV, 23, self.units)
        self._ent = {}

    def use(self, state, force=False):
        if state == self.state and not force:
            return
        if state == "assembled":
            self.assemble()
        else:
            self.ctx.matrix_import(op.seeded_blocks(self.nnzb, 5))
        torch.cuda.synchronize()
        self.state = state
        self._ent.pop(state, None)

    def entries(self):
        """((rows, cols, blocks) of the static matrix, of the contact rows), long double, of the values in use"""
        if self.state not in self._ent:
            T = self.T
            st = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], self.ctx.op_export("vals"), self.NV, LD)[:3]
            ce = op.contact_entries(*self.cr, self.ctx.contact_blocks(True), LD) if self.nc else None
            self._ent[self.state] = (st, ce)
        return self._ent[self.state]

    def full(self):
        st, ce = self.entries()
        return st if ce is None else tuple(np.concatenate([a, b]) for a, b in zip(st, ce))

    def to_caller(self, v):
        out = np.empty(3 * self.NV); out.reshape(-1, 3)[self.T["perm"]] = np.asarray(v, np.float64).reshape(-1, 3)
        return out

    def to_solver(self, v):
        return np.asarray(v).reshape(-1, 3)[self.T["perm"]].ravel()


def _cloth_ctx(name, N, M, frozen_of, ties=False):
    from thinshelllab_amd.context import TslContext
    c = cn.ClothTables(N, M, 0.1 / 15)
    nv = c.NV
    c.desc["mass"] = 40.0 * c.dx * c.dx
    rng = np.random.default_rng(5)
    i, j = cn.grid(c)
    x = np.stack([i * c.dx, j * c.dx, np.zeros(nv)], 1) + rng.normal(0, 5e-5, (nv, 3))
    frozen = np.zeros((nv, 3), np.int32)
    args = dict(tot_NV=nv, cloths=[c.desc])
    T = expected_tables(**args)
    tie = op.corner_ties(T["perm"], T["rowpos"], c.f2v, nv) if ties else None
    frozen_of(frozen, T, tie)
    mass = np.full(nv, c.desc["mass"])
    ctx = TslContext(tot_NV=nv, dt=5e-3, mass=mass, gravity=np.tile([0.0, 0.0, -9.8], (nv, 1)), frozen=frozen.ravel(), cloths=[c.desc], faces=c.f2v.astype(np.int32),
                     max_n_constraints=64)
    ctx.set_param("direct", 0)
    ctx.set_param("mg", 0)
    if ties:
        ctx.set_ties(*tie)
        ctx.set_param("k_tie", 800.0)
    pos, prev, vel, ref = _dev(x), _dev(x - rng.normal(0, 1.5e-5, x.shape)), _dev(rng.normal(0, 1e-2, x.shape)), _dev(rng.normal(0, 0.05, (c.NF, 3)))
    grad = torch.zeros(3 * nv, dtype=torch.float64, device="cuda")
    assemble = lambda: ctx.assemble(pos, prev, vel, ref, spd=True, grad=grad)
    assemble()
    torch.cuda.synchronize()
    return Case(name, ctx, args, frozen, mass, 5e-3, assemble, (pos, prev, vel, ref, grad, c))


def _freeze_drape(frozen, T, tie):
    """row i = 0 pinned; one vertex z only, one x and y only, one fully -- the z-only one a tie vertex where there are ties"""
    nv = len(frozen)
    a = int(tie[0][7]) if tie is not None else nv // 2
    frozen[a, 2] = 1
    frozen[nv // 2 + 3, :2] = 1
    frozen[nv // 2 + 7] = 1


def _cloth_1x1(name):
    def fz(frozen, T, tie):
        frozen[2, 2] = 1
    try:
        return _cloth_ctx(name, 1, 1, fz)
    except Exception as e:       # the smallest cloth the context takes
        print("operator alone: a 1 x 1 cloth is refused (%s): 2 x 1 instead" % e)
        return _cloth_ctx(name, 2, 1, fz)


def _drape(name, N, M, ties):
    def fz(frozen, T, tie):
        frozen[:M + 1] = 1         # the row i = 0 pinned
        _freeze_drape(frozen, T, tie)
    return _cloth_ctx(name, N, M, fz, ties)


def _balancing(name):
    """the 16 x 8 balancing scene of 9j at a state with detected contacts, three more cloth vertices frozen (one of a contact z only)"""
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
    ctx.set_param("direct", 0)
    projection_query(s)
    s.compute_residual_and_Hessian(spd=True)
    idx = ctx.constraints()["idx"]
    assert len(idx) > 0
    in_cloth = [int(v) for v in idx.ravel() if c.offset <= v < c.offset + c.NV]
    fr = s.frozen.to_numpy().reshape(-1, 3).copy()
    free = [v for v in range(c.offset, c.offset + c.NV) if not fr[v].any() and v not in in_cloth]
    fr[in_cloth[0], 2] = 1
    fr[free[5], :2] = 1
    fr[free[40]] = 1
    s.frozen.from_numpy(fr.reshape(s.frozen.to_numpy().shape))
    ctx.set_frozen(fr.ravel())
    assemble = lambda: s.compute_residual_and_Hessian(spd=True)
    assemble()
    torch.cuda.synchronize()
    assert np.array_equal(ctx.constraints()["idx"], idx)
    args = dict(tot_NV=s.tot_NV, cloths=[cl._desc() for cl in s.cloths], elastics=[e._desc() for e in s.elastics])
    bodies = [(e.offset, e.n_verts) for e in s.elastics if 2 <= e.n_verts <= 512 and not fr[e.offset:e.offset + e.n_verts].all()]
    C = Case(name, ctx, args, fr, s.mass.to_numpy(), s.dt, assemble, s, bodies)
    C.cloth = (c.offset, 16, 8)
    return C


BUILD = {"cloth_1x1": _cloth_1x1, "drape_8x8": lambda n: _drape(n, 8, 8, False), "drape_12x20_ties": lambda n: _drape(n, 12, 20, True), "balancing_16x8": _balancing}


def _get(name):
    if name not in _cache:
        _cache[name] = BUILD[name](name)
    return _cache[name]


@pytest.fixture
def case(request):
    return _get(request.param)


every = pytest.mark.parametrize("case", NAMES, indirect=True)


# ------------------------------------------------------------------------------------------------ what each context is here for
def test_contexts_are_what_they_are_here_for():
    nks = set()
    for name in NAMES:
        C = _get(name)
        ln = C.T["slice_len"]
        nks |= {int((l - w + 3) // 4) for l in ln for w in range(4) if l - w > 0}
        print("operator alone, %s: NV %d, slice_len %s, constraints %d, longest contact row %d" % (name, C.NV, ln.tolist(), C.nc, C.cnt.max() if C.nc else 0))
    assert nks >= {1, 2, 3, 4, 5, 6}, nks
    assert _get("cloth_1x1").NV in (4, 6) and len(_get("cloth_1x1").T["slice_len"]) == 1
    assert _get("drape_8x8").T["slice_len"].tolist() == [13, 6] and _get("drape_8x8").NV == 81
    T = _get("drape_12x20_ties")
    assert T.T["slice_len"].tolist() == [13, 13, 9, 9, 6] and T.nc == 70
    last = T.cnt[256:]
    assert last.max() > 64 and np.any((last >= 1) & (last <= 63)) and np.any(last == 0)
    B = _get("balancing_16x8")
    assert B.NV == 1357 and len(B.T["slice_len"]) == 22 and B.T["slice_len"][0] == 24 and B.T["slice_len"][-1] == 6 and B.NV - 64 * 21 == 13
    assert B.nc > 0 and len(B.ctx.mg_info()["hierarchies"]) == 1 and len(B.ctx.mg_info()["bodies"]) > 0
    assert not _get("drape_8x8").ctx.mg_info()["hierarchies"]
    for name in NAMES[1:]:
        C = _get(name)
        part = C.frozen.sum(1)
        assert np.any(part == 1) and np.any(part == 2) and np.any(part == 3), name
        if C.nc:    # one of the partly frozen vertices belongs to a constraint
            assert any(0 < C.frozen[v].sum() < 3 for v in np.unique(C.cons)), name


@every
def test_tables_and_padded_slots(case):
    C = case
    E = expected_tables(**C.args)
    for k in ("slice_off", "slice_len", "colidx", "perm", "rowpos", "diag_perm"):
        assert np.array_equal(C.T[k], E[k]), k
    fz = C.ctx.op_export("fzmask")
    assert np.array_equal(fz, (C.frozen[C.T["perm"]] * np.array([1, 2, 4])).sum(1))
    assert np.array_equal(C.ctx.op_export("mdt2"), C.mass[C.T["perm"]] / (C.dt * C.dt))
    row_len = np.diff(E["row_ptr"])[E["perm"]]
    for state in ("assembled", "imported"):
        C.use(state)
        for what in ("vals", "vals_full") if state == "assembled" else ("vals",):
            rows, cols, B, k = op.sell_decode(C.T["slice_off"], C.T["slice_len"], C.T["colidx"], C.ctx.op_export(what), C.NV)
            real = op.real_slots(rows, cols, k, row_len)
            assert not B[~real].any(), (state, what)
            if state == "imported":
                assert np.all(B[real] != 0)
    # and nothing behind the last real row of the last slice either
    v = C.ctx.op_export("vals").reshape(-1, 9, 64)
    tail = C.NV - 64 * (len(C.T["slice_len"]) - 1)
    assert not v[int(C.T["slice_off"][-2]) // 64:, :, tail:].any()


@every
def test_masks_and_diagonals(case):
    C = case
    C.use("assembled", force=True)          # (an assembly from outside: every row of Dinv is formed, the dense bodies not yet in use)
    T = C.T
    ctx = C.ctx
    R = Ratios()
    full = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], ctx.op_export("vals_full"), C.NV)
    got = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], ctx.op_export("vals"), C.NV)
    ref = op.mask_blocks(full[0], full[1], full[2], ctx.op_export("fzmask"), ctx.op_export("mdt2"))
    assert np.array_equal(got[2], ref)
    D = op.diag_blocks(got[0], got[1], got[2], C.NV)
    cd = None
    if C.nc:
        Hm = ctx.contact_blocks(True)
        assert np.array_equal(Hm, op.mask_contact(ctx.contact_blocks(False), C.cons, C.frozen))
        assert np.array_equal(ctx.op_export("cr_ptr"), C.cr[0]) and np.array_equal(ctx.op_export("cr_ent"), C.cr[1])
        assert np.array_equal(ctx.op_export("cr_rows").reshape(-1, 4), C.cr[2])
        cd = ctx.op_export("c_diag").reshape(C.NV, 3, 3)
        cref, mag, cnt = op.contact_diag(C.cr[0], C.cr[1], Hm, C.NV, LD)
        R.add("c_diag", np.abs(cd.astype(LD) - cref), (cnt[:, None, None] + 7) * U * mag)
        assert not cd[cnt == 0].any()
    else:
        assert len(ctx.op_export("c_diag")) == 0 and len(ctx.op_export("cr_ptr")) == 0
    from test_gpu_mg_elements import _dinv_check
    Dinv = ctx.op_export("Dinv").reshape(C.NV, 3, 3)
    _dinv_check(D if cd is None else D + cd, Dinv, R, "Dinv")
    R.check(C.name + " masks and diagonals")


@every
def test_block_jacobi_inverse_follows_an_import(case):
    """tsl_matrix_import must leave nothing that was built from the values before it: the inverse the next solve reads is the one of the imported blocks"""
    C = case
    C.use("assembled", force=True)
    C.ctx.op_export("Dinv")
    C.use("imported", force=True)
    T = C.T
    got = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], C.ctx.op_export("vals"), C.NV)
    D = op.diag_blocks(got[0], got[1], got[2], C.NV)
    if C.nc:
        D = D + C.ctx.op_export("c_diag").reshape(C.NV, 3, 3)
    from test_gpu_mg_elements import _dinv_check
    R = Ratios()
    _dinv_check(D, C.ctx.op_export("Dinv").reshape(C.NV, 3, 3), R, "Dinv after import")
    R.check(C.name + " block-Jacobi inverse after an import")


# ------------------------------------------------------------------------------------------------ the product, kernel by kernel
ROWS_PER_PART = {1: 256, 2: 64, 3: 64, 4: 128, 5: 64, 6: 128, 7: 128, 9: 64}


@every
@pytest.mark.parametrize("state", ["assembled", "imported"])
def test_product_by_every_kernel(case, state):
    C = case
    C.use(state)
    st, ce = C.entries()
    full = C.full()
    R = Ratios()
    NV = C.NV
    zero = np.zeros(NV)
    for j in range(C.X.shape[1]):
        xs = C.X[:, j]
        x = _dev(C.to_caller(xs))
        refs = {}
        for contact in (False, True):
            ent = full if contact else st
            y = op.product(ent, xs, LD)
            refs[contact] = (y, op.product_bound(C.T["slice_len"], C.cnt if contact else zero, op.product(ent, xs, LD, absolute=True)))
        xl = xs.astype(LD).reshape(NV, 3)
        out = {}
        for kid in range(10):
            contact = kid in (0, 8, 9)
            yref, bnd = refs[contact]
            y, dot, part = C.ctx.op_apply(kid, x)
            ys = C.to_solver(y.cpu().numpy()).reshape(NV, 3)
            out[kid] = ys
            R.add("y, kernel %d" % kid, np.abs(ys.astype(LD) - yref), bnd)
            # x . y: the rows' bounds times |x_i| plus the summation of the products in any order
            rowdot = (xl * yref).sum(1)
            rowbnd = (np.abs(xs).reshape(NV, 3) * bnd).sum(1) + g(3 * NV + 16) * np.abs(xl * yref).sum(1).astype(np.float64)
            if kid == 0:
                R.add("dot, kernel 0", abs(LD(dot) - rowdot.sum()), rowbnd.sum())
            elif kid != 8:
                m = ROWS_PER_PART[kid]
                assert len(part) == (NV + m - 1) // m, (kid, len(part))
                R.add("partials, kernel %d" % kid, np.abs(part.astype(LD) - np.add.reduceat(rowdot, np.arange(0, NV, m))), np.add.reduceat(rowbnd, np.arange(0, NV, m)))
            if kid != 0:     # a second call returns the same bits (kernel 0 adds the contact part with f64 atomics)
                y2, _, part2 = C.ctx.op_apply(kid, x)
                assert torch.equal(y, y2) and np.array_equal(part, part2), kid
        if not C.nc:
            assert np.array_equal(out[2], out[8])
    R.check("%s, %s values, %d vectors" % (C.name, state, C.X.shape[1]))


# ------------------------------------------------------------------------------------------------ one PCG step
def _precond(C):
    """(z = M^-1 r restated in dt on flat solver-order vectors, is it the multigrid cycle)"""
    ctx = C.ctx
    if len(ctx.mg_info()["hierarchies"]):
        if "pc" not in C.__dict__:
            from test_gpu_mg_elements import Case as MgCase
            C.pc = MgCase(C.name, ctx, C.rhs, [C.cloth], C.bodies).pc
        return (lambda r, dt: C.to_solver(mg.cycle(C.pc, C.to_caller(r), dt))), True
    Dinv = ctx.op_export("Dinv").reshape(C.NV, 3, 3)
    return (lambda r, dt: mg.block_apply(Dinv.astype(dt), np.asarray(r, dtype=dt))), False


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", PCG_NAMES, indirect=True)
def test_one_pcg_step(case):
    C = case
    C.use("assembled", force=True)
    ctx = C.ctx
    NV = C.NV
    full = C.full()
    H = lambda v, absolute=False: op.product(full, v, LD, absolute=absolute).ravel()
    s1 = ctx.pcg_trace(C.rhs, 1)
    chunk = s1["chunk"]
    pre, is_mg = _precond(C)
    assert chunk == (4 if is_mg else 32)
    R = Ratios()
    # after iteration 0 the recurrence has not run: Ap is the product of p
    pb = op.product_bound(C.T["slice_len"], C.cnt, H(s1["p"], True).reshape(NV, 3)).ravel()
    R.add("Ap = H p after iteration 0", np.abs(s1["Ap"].astype(LD) - H(s1["p"])), pb)
    assert s1["iters"] == 1 and s1["flag"] == 0 and np.array_equal(s1["p"], ctx.pcg_trace(C.rhs, 1)["p"])
    L = lambda a: np.asarray(a, dtype=LD)
    for n in (1, 2, 3, chunk + 1):
        a, b = ctx.pcg_trace(C.rhs, n), ctx.pcg_trace(C.rhs, n + 1)
        assert _same(b, ctx.pcg_trace(C.rhs, n + 1)), n            # the run repeated gives the same bits
        assert a["flag"] == 0 and b["flag"] == 0 and a["iters"] == n and b["iters"] == n + 1
        par = n & 1
        rzh_a, rzh_b = [a["rzh0"], a["rzh1"]], [b["rzh0"], b["rzh1"]]
        np2, ns = a["n_part2"], a["n_part1"]
        assert len(a["part_rz"]) == np2 and len(a["part_pAp"]) == ns == len(C.T["slice_len"])
        # K1
        rz, rr = L(a["part_rz"]).sum(), L(a["part_rr"]).sum()
        R.add("rz", abs(LD(rzh_b[par]) - rz), g(np2) * np.abs(a["part_rz"]).sum())
        R.add("rr_last", abs(LD(b["rr_last"]) - rr), g(np2) * np.abs(a["part_rr"]).sum())
        assert b["rz_last"] == rzh_b[par] and rzh_b[par ^ 1] == rzh_a[par ^ 1] and np.array_equal(b["p_prev"], a["p"])
        rz_old = LD(rzh_a[par ^ 1])
        beta = rz / rz_old
        e_beta = float(g(np2 + 2) * np.abs(a["part_rz"]).sum() / abs(rz_old))
        p_ref = L(a["z"]) + beta * L(a["p"])
        R.add("p", np.abs(L(b["p"]) - p_ref), e_beta * np.abs(a["p"]) + g(2) * (np.abs(a["z"]) + np.abs(float(beta) * a["p"])))
        Hz, aHz = H(a["z"]), H(a["z"], True).astype(np.float64)
        Ap_ref = Hz + beta * L(a["Ap"])
        R.add("Ap", np.abs(L(b["Ap"]) - Ap_ref),
              op.product_bound(C.T["slice_len"], C.cnt, aHz.reshape(NV, 3)).ravel() + e_beta * np.abs(a["Ap"]) + g(2) * (aHz + np.abs(float(beta) * a["Ap"])))
        row = lambda v: np.asarray(v).reshape(NV, 3).sum(1)
        sl, bl = np.arange(0, NV, 64), np.arange(0, NV, 256)
        pAp_rows = row(L(b["p"]) * L(b["Ap"]))
        R.add("part_pAp", np.abs(L(b["part_pAp"]) - np.add.reduceat(pAp_rows, sl)), g(192) * np.add.reduceat(row(np.abs(b["p"] * b["Ap"])), sl))
        # K2
        pAp = L(b["part_pAp"]).sum()
        alpha = LD(rzh_b[par]) / pAp
        e_alpha = float(g(ns + 2) * abs(alpha) * np.abs(b["part_pAp"]).sum() / abs(pAp))
        al = abs(float(alpha))
        R.add("x", np.abs(L(b["x"]) - (L(a["x"]) + alpha * L(b["p"]))), e_alpha * np.abs(b["p"]) + g(2) * (np.abs(a["x"]) + al * np.abs(b["p"])))
        R.add("r", np.abs(L(b["r"]) - (L(a["r"]) - alpha * L(b["Ap"]))), e_alpha * np.abs(b["Ap"]) + g(2) * (np.abs(a["r"]) + al * np.abs(b["Ap"])))
        R.add("part_rr", np.abs(L(b["part_rr"]) - np.add.reduceat(row(L(b["r"]) ** 2), bl)), g(768) * np.add.reduceat(row(b["r"] ** 2), bl))
        if is_mg:
            ref, f64 = pre(b["r"], LD), pre(b["r"], np.float64)
            nrm = lambda v: float(np.sqrt(np.dot(v, v)))
            R.add("z (cycle)", nrm(L(b["z"]) - ref), bound(nrm(L(f64) - ref), nrm(ref)))
            R.add("sum part_rz", abs(L(b["part_rz"]).sum() - (L(b["r"]) * L(b["z"])).sum()), g(3 * NV + np2) * np.abs(b["r"] * b["z"]).sum())
        else:
            Dinv = ctx.op_export("Dinv").reshape(NV, 3, 3)
            R.add("z", np.abs(L(b["z"]) - pre(b["r"], LD)), g(3) * mg.block_apply(np.abs(Dinv), np.abs(b["r"])))
            R.add("part_rz", np.abs(L(b["part_rz"]) - np.add.reduceat(row(L(b["r"]) * L(b["z"])), bl)), g(768) * np.add.reduceat(row(np.abs(b["r"] * b["z"])), bl))
    R.check("%s, one PCG step behind 1, 2, 3 and %d iterations" % (C.name, chunk + 1))


@pytest.mark.parametrize("case", ["drape_8x8", "balancing_16x8"], indirect=True)
def test_captured_graph_against_eager_launches(case):
    C = case
    C.use("assembled", force=True)
    ctx = C.ctx
    chunk = ctx.pcg_trace(C.rhs, 1)["chunk"]
    full = C.full()
    for n in (1 + chunk, 1 + 2 * chunk):
        e, gr = ctx.pcg_trace(C.rhs, n, use_graph=False), ctx.pcg_trace(C.rhs, n, use_graph=True)
        assert e["iters"] == n or e["flag"] != 0
        assert _same(e, gr), n
    with pytest.raises(Exception, match="multiple of the chunk"):
        ctx.pcg_trace(C.rhs, chunk, use_graph=True)
    # drift of the recurrence A p_new = A z + beta A p_old behind 1 + 2 chunk iterations: recorded, not asserted (its growth has no bound derived here)
    Hp = op.product(full, e["p"], LD).ravel()
    aHp = op.product(full, e["p"], LD, absolute=True).ravel().astype(np.float64)
    ok = aHp > 0
    drift = float(np.max(np.abs(e["Ap"].astype(LD) - Hp).astype(np.float64)[ok] / (U * aHp[ok])))
    print("operator alone, %s: drift of Ap behind %d iterations: max |Ap - H p|_i / (u (|H||p|)_i) = %.2f (flag %d)" % (C.name, n, drift, e["flag"]))
