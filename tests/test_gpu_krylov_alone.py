"""Each Krylov solver of the iterative hierarchy alone (tsl_solve_with: no successor covers for it), asserting only what follows from a solver's
definition: a solver that reports convergence delivers the residual it promises, reports the residual it has, and says which solver it is; PCG on an
indefinite operator does not report convergence; GMRES without a restart terminates within the number of free unknowns.

Iteration counts of MINRES, GMRES and BiCGStab are printed next to scipy.sparse.linalg's for the same method behind the restated preconditioner
(mg_numpy.cycle on the exported arrays, or the block-Jacobi inverse); they are not compared, the stopping rules differ.  A solver that does not converge
within the cap where scipy's same method behind the same preconditioner does is a finding."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl
import torch

import berr
import mg_numpy as mg

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
CG_TOL = 1e-10          # the engine's default
NAMES = ("PCG", "MINRES", "GMRES", "BiCGStab")
_cache = {}


class System:
    """a context with an assembled operator, its right-hand side, and how to put the operator back after a switch of the preconditioner"""

    def __init__(self, name, ctx, b, reassemble, keep, indefinite):
        self.name, self.ctx, self.b, self.reassemble, self.keep, self.indefinite = name, ctx, b, reassemble, keep, indefinite
        self.H = ctx.operator_csr() if len(ctx.constraints()["idx"]) else ctx.matrix_csr()
        self.bh = b.cpu().numpy()
        fr = np.asarray(keep.frozen.to_numpy()).ravel()
        self.n_free = int((fr == 0).sum())
        self.has_mg = len(ctx.mg_info()["hierarchies"]) > 0
        self.mg_on = self.has_mg
        self._pre = {}

    def use_mg(self, on):
        if on != self.mg_on:
            self.ctx.set_param("mg", -1 if on else 0)
            self.reassemble()            # block-Jacobi inverse and body blocks of the preconditioner now in use
            self.mg_on = on

    def precond(self):
        """the restated preconditioner in use, as a function"""
        if self.mg_on not in self._pre:
            if self.mg_on:
                from test_gpu_mg_elements import Case
                info = self.ctx.mg_info()
                s = self.keep
                bodies = [(e.offset, e.n_verts) for e in getattr(s, "elastics", [])][:len(info["bodies"])]
                pc = Case(self.name, self.ctx, self.b, [(h["v_offset"], h["N0"], h["M0"]) for h in info["hierarchies"]], bodies).pc
                self._pre[True] = lambda r: mg.cycle(pc, r)
            else:
                Dinv = mg.block_inverse(mg.diag_blocks(self.H.toarray()))
                self._pre[False] = lambda r: mg.block_apply(Dinv, np.asarray(r, dtype=np.float64))
        return self._pre[self.mg_on]


def _drape(oracle, N, M, amp, spd):
    from test_gpu_cloth import _pair
    sys, _ = _pair(oracle, N, M, amp=amp)
    if spd:
        re = lambda: sys.compute_residual_and_Hessian(spd=True)
        re()
        b = sys.F.to_torch()
    else:
        re = lambda: sys.compute_Hessian(spd=False)
        re()
        b = torch.as_tensor(np.random.default_rng(3).normal(size=sys.tot_NV * 3), device=sys.device)
    return sys, b, re


def _balancing(oracle):
    from thinshelllab_amd.engine.geometry import projection_query
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=0.064, cloth_N=16, cloth_M=8)
    s.init_all()
    s.mu_cloth_elastic[None] = 5.0
    c = s.cloths[0]
    x = s.pos.to_numpy()
    x[c.offset:c.offset + c.NV, 2] += 2e-6 * np.sin(0.7 * np.arange(c.NV) + 0.3)
    s.pos.from_numpy(x); s.prev_pos.from_numpy(x)
    s._ensure_ctx()
    projection_query(s)
    re = lambda: s.compute_residual_and_Hessian(spd=True)
    re()
    return s, s.F.to_torch(), re


SYSTEMS = {
    "drape12x12_spd": lambda o: _drape(o, 12, 12, 5e-5, True) + (False,),
    "drape10x6_indefinite": lambda o: _drape(o, 10, 6, 2e-4, False) + (True,),
    "drape16x12_indefinite": lambda o: _drape(o, 16, 12, 2e-4, False) + (True,),
    "balancing_contacts": lambda o: _balancing(o) + (False,),
}


def _system(oracle, name):
    if name not in _cache:
        s, b, re, indef = SYSTEMS[name](oracle)
        _cache[name] = System(name, s._ctx, b, re, s, indef)
    return _cache[name]


def test_the_systems_are_what_they_are_here_for(oracle):
    for name in SYSTEMS:
        S = _system(oracle, name)
        Hd = S.H.toarray()
        w = np.linalg.eigvalsh(0.5 * (Hd + Hd.T))
        if S.indefinite:
            assert w.min() < 0 < w.max(), name                # eigenvalues of both signs
        else:
            assert w.min() > 0, name
    assert not _system(oracle, "drape10x6_indefinite").has_mg and _system(oracle, "drape16x12_indefinite").has_mg
    assert len(_system(oracle, "balancing_contacts").ctx.constraints()["idx"]) > 0      # matrix-free contact rows in every operator product


def _host_residual(S, x):
    """(|b - Hx| / |b|, its evaluation error 64 u |(|H||x| + |b|)| / |b|), long double"""
    r = berr.residual(S.H, x, S.bh)
    A = abs(sp.csr_matrix(S.H))
    ev = 64 * U * (sp.csr_matrix((A.data.astype(LD), A.indices, A.indptr), shape=A.shape) @ np.abs(x).astype(LD) + np.abs(S.bh).astype(LD))
    nb = np.sqrt(np.dot(S.bh.astype(LD), S.bh.astype(LD)))
    return float(np.sqrt(np.dot(r, r)) / nb), float(np.sqrt(np.dot(ev, ev)) / nb)


def _scipy(S, method, restart):
    """(converged to CG_TOL on the true residual, iterations) of scipy's solver of the same name behind the restated preconditioner"""
    n = S.H.shape[0]
    M = spl.LinearOperator((n, n), matvec=S.precond(), dtype=np.float64)
    cnt = [0]
    cb = lambda *_: cnt.__setitem__(0, cnt[0] + 1)
    H = sp.csr_matrix(S.H)
    if method == 1:
        try:
            x, _ = spl.minres(H, S.bh, M=M, rtol=CG_TOL, maxiter=20 * n, callback=cb)
        except ValueError:      # scipy's MINRES stops where r . M^-1 r < 0: the preconditioner of an indefinite matrix is not positive definite
            return False, -1
    elif method == 2:
        x, _ = spl.gmres(H, S.bh, M=M, rtol=CG_TOL, restart=restart, maxiter=max(1, 20 * n // restart), callback=cb, callback_type="pr_norm")
    else:
        x, _ = spl.bicgstab(H, S.bh, M=M, rtol=CG_TOL, maxiter=20 * n, callback=cb)
    rel, ev = _host_residual(S, x)
    return bool(np.all(np.isfinite(x)) and rel <= 100 * CG_TOL + ev), cnt[0]


# (system, method, multigrid on, gmres_m: 0 = the default): every solver on every system; PCG behind both preconditioners; GMRES restarted and not
RUNS = []
for _name in SYSTEMS:
    _has_mg = _name != "drape10x6_indefinite"
    for _mgon in ((True, False) if _has_mg else (False,)):
        RUNS.append((_name, 0, _mgon, 0))
    for _m in (1, 2, 3):
        RUNS.append((_name, _m, _has_mg, 0))
    RUNS.append((_name, 2, _has_mg, 100000))     # no restart within the cap of the basis (400 vectors): see the test


@pytest.mark.parametrize("name,method,mg_on,gmres_m", RUNS)
def test_solver_alone(oracle, name, method, mg_on, gmres_m):
    S = _system(oracle, name)
    S.use_mg(mg_on)
    ctx = S.ctx
    ctx.set_param("gmres_m", gmres_m if gmres_m else 300)
    try:
        x, st = ctx.solve_with(method, S.b)
    finally:
        ctx.set_param("gmres_m", 300)
    x = x.cpu().numpy()
    rel, ev = _host_residual(S, x) if np.all(np.isfinite(x)) else (float("inf"), 0.0)
    line = "krylov alone, %s, %s (mg %d%s): flag %d iters %d restarts %d attained %d, reported %.3e, true residual %.3e |b|" % (
        name, NAMES[method], mg_on, ", gmres_m %d" % gmres_m if gmres_m else "", st["flag"], st["iters"], st["restarts"], st["attained"], st["rel_residual"], rel)
    sc = None
    if method > 0:
        restart = min(400, S.H.shape[0]) if gmres_m else 300
        sc = _scipy(S, method, restart)
        line += "; scipy %s: %s after %d iterations" % (NAMES[method], "converged" if sc[0] else "not converged", sc[1])
    print(line)
    assert st["method"] == method
    if method == 0 and S.indefinite:
        # CG on an operator with eigenvalues of both signs must say so, not deliver something; the context must still solve afterwards
        assert st["flag"] == 3
        x2, st2 = ctx.solve(S.b)
        r2, e2 = _host_residual(S, x2.cpu().numpy())
        assert st2["flag"] == 1 and r2 <= 100 * CG_TOL + e2, (st2, r2)
        return
    assert st["flag"] in ((0,) if method == 0 else (1,)) + (3,)
    if st["flag"] == 3:
        # not converged alone within the cap: a finding exactly where scipy's same method behind the same preconditioner does converge
        assert sc is not None and not sc[0], "finding: %s" % line
        return
    assert rel <= (100 if st["attained"] == 1 else 1) * CG_TOL + ev, line
    assert abs(st["rel_residual"] - rel) <= ev, line
    if method == 2 and gmres_m and S.n_free <= 400:
        assert st["iters"] <= S.n_free, line       # no restart: finite termination within the number of free unknowns
