"""The restatement of the multigrid preconditioner (mg_numpy.py) pinned without the kernels: structure of the transfers, of the Galerkin operators
and of the slot layouts, the cycle as a symmetric positive definite operator, convergence of the two-grid iteration and of PCG through the cycle,
and the mutation checks that give the GPU tests their meaning -- each deliberate defect must leave the agreement bound of the cycle test and move the
PCG count out of the window of the PCG test, on inputs the GPU tests use (the oracle's assembled Hessian of the same perturbed drapes)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

import mg_numpy as mg
from tet_numpy import bound

LD = np.longdouble
CG_TOL = 1e-10

# the shapes of tests/test_gpu_mg_elements.py: (N, M, levels walked, kind of the last level)
SHAPES = {"8x8_dense75": (8, 8, 1, "dense"), "8x8_one_workgroup": (8, 8, 2, "one_workgroup"), "12x20": (12, 20, 2, "dense"),
          "32x16_dense45": (32, 16, 2, "dense"), "32x16_one_workgroup": (32, 16, 3, "one_workgroup"), "34x18_per_sweep": (34, 18, 1, "per_sweep"),
          "50x26_per_sweep": (50, 26, 1, "per_sweep")}
_cache = {}


def _case(oracle, name):
    if name not in _cache:
        N, M, nl, kind = SHAPES[name]
        H, F, frozen = mg.oracle_drape(oracle, N, M)
        assert frozen.reshape(-1, 3)[N * (M + 1):].all()
        pc = mg.restated_pc(H, N, M, nl, kind)
        Hd = H.toarray()
        _cache[name] = dict(N=N, M=M, H=H, Hd=Hd, F=F, pc=pc, window=mg.pcg_window(Hd, F, lambda r: mg.cycle(pc, r), CG_TOL))
    return _cache[name]


@pytest.mark.parametrize("N,M", [(8, 8), (12, 20), (6, 4)])
def test_prolongation(N, M):
    P = mg.prolongation(N, M, block=False)
    assert P.shape == (mg.nodes(N, M), mg.nodes(N // 2, M // 2))
    assert np.array_equal(P.sum(1), np.ones(len(P)))                                    # interpolation reproduces constants
    assert np.array_equal(mg.prolongation(N, M), np.kron(P, np.eye(3)))
    assert np.array_equal(mg.prolongation_sp(N, M).toarray(), mg.prolongation(N, M))
    G = P.T @ P
    d1 = lambda n: np.array([1.25] + [1.5] * (n // 2 - 1) + [1.25])                     # 1 + 1/4 per odd neighbour: one at an end, two inside
    assert np.array_equal(np.diag(G).reshape(N // 2 + 1, M // 2 + 1), np.outer(d1(N), d1(M)))      # corners 25/16, edges 15/8, interior 9/4
    G1 = mg.prolong_1d(N).T @ mg.prolong_1d(N)
    assert np.array_equal(np.diag(G1, 1), np.full(N // 2, 0.25)) and not np.triu(G1, 2).any()


@pytest.mark.parametrize("name", ["8x8_one_workgroup", "32x16_one_workgroup"])
def test_galerkin_operators_and_slot_layouts(oracle, name):
    c = _case(oracle, name)
    asym0 = np.abs(c["Hd"] - c["Hd"].T).max() / np.abs(c["Hd"]).max()
    Hs = 0.5 * (c["Hd"] + c["Hd"].T)
    A, N, M = mg.galerkin(Hs, c["N"], c["M"], np.float64), c["N"] // 2, c["M"] // 2
    for L in c["pc"]["cloths"][0]["levels"]:
        assert (L["N"], L["M"]) == (N, M)
        assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()                         # a symmetric operator keeps symmetric coarse operators
        B = L["A"]                                                                       # (the assembled one is as symmetric as the Hessian it came from)
        assert np.abs(B - B.T).max() <= 4 * asym0 * np.abs(B).max()
        S, outside = mg.slots_from_dense(B, N, M)
        assert outside == 0.0 and S.shape == (225 * mg.nodes(N, M),)                    # radius 2 on every level
        assert np.array_equal(mg.dense_from_slots(S, N, M), B)
        if "S32" in L:
            T, outside = mg.s_slots_from_dense(L["S32"], N, M)
            assert outside == 0.0 and T.shape == (441 * mg.nodes(N // 2, M // 2),)      # restriction radius 1 + stencil radius 2 on the fine grid
            assert np.array_equal(mg.s_dense_from_slots(T, N, M, np.float32), L["S32"])
            A, N, M = mg.galerkin(A, N, M, np.float64), N // 2, M // 2
    # a slot is where the kernels' index arithmetic says: row node (I, J), slot (dI + 2) 5 + dJ + 2, column node (I + dI, J + dJ)
    N, M = c["N"] // 2, c["M"] // 2
    S = np.zeros((25, 9, mg.nodes(N, M)))
    S[(1 + 2) * 5 + (-2 + 2), 3 * 0 + 2, 1 * (M + 1) + 2] = 7.0
    D = mg.dense_from_slots(S.ravel(), N, M)
    assert D[3 * (1 * (M + 1) + 2) + 0, 3 * (2 * (M + 1) + 0) + 2] == 7.0 and np.count_nonzero(D) == 1


def test_block_inverse_and_power_iteration(oracle):
    c = _case(oracle, "12x20")
    D = mg.diag_blocks(c["Hd"])
    Di = mg.block_inverse(D)
    assert np.abs(np.einsum("kij,kjl->kil", Di, D) - np.eye(3)).max() < 1e-12
    ref = mg.block_inverse_mp(D[:5])
    assert max(abs(float(ref[k, i, j]) - Di[k, i, j]) for k in range(5) for i in range(3) for j in range(3)) <= 1e-14 * np.abs(Di[:5]).max()
    lam = mg.power_lambda(c["pc"]["H0"], Di)
    T = np.zeros_like(c["Hd"])
    for k in range(len(Di)):
        T[3 * k:3 * k + 3] = Di[k] @ c["pc"]["H0"][3 * k:3 * k + 3]
    lmax = np.abs(np.linalg.eigvals(T)).max()
    assert 0.7 * lmax <= lam <= lmax * (1 + 1e-12)                                      # twelve steps from a rough start: a lower estimate
    assert mg.omega_of(lam) == min(0.8, 1.5 / lam) and mg.omega_of(lam) * lmax < 2
    assert mg.omega_of(float("nan")) == 0.8 and mg.omega_of(0.0) == 0.8


@pytest.mark.parametrize("name", ["8x8_dense75", "8x8_one_workgroup", "34x18_per_sweep"])
def test_cycle_matrix_is_symmetric_positive_definite(oracle, name):
    """with a symmetric operator and every array in double precision: the fused first sweep, the three kinds of last level and the post-sweep
    together are M^-1 = M^-T > 0 (what PCG needs)"""
    N, M, nl, kind = SHAPES[name]
    c = _case(oracle, name)
    Hs = 0.5 * (c["Hd"] + c["Hd"].T)
    pc = mg.restated_pc(Hs, N, M, nl, kind, single=False)
    Z = mg.cycle_matrix(pc, len(Hs))
    assert np.abs(Z - Z.T).max() <= 1e-11 * np.abs(Z).max()
    assert np.linalg.eigvalsh(0.5 * (Z + Z.T)).min() > 0


def test_two_grid_iteration_converges(oracle):
    c = _case(oracle, "8x8_dense75")         # level 0 smoothed, level 1 solved exactly: the two-grid method
    Z = mg.cycle_matrix(c["pc"], len(c["Hd"]))
    rho = np.abs(np.linalg.eigvals(np.eye(len(Z)) - Z @ c["Hd"])).max()
    print("two-grid error propagator of the 8 x 8 drape: spectral radius %.3f" % rho)
    assert rho < 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_pcg_through_the_cycle_reaches_spsolve(oracle, name):
    c = _case(oracle, name)
    x, it, ok = mg.pcg(c["Hd"], c["F"], lambda r: mg.cycle(c["pc"], r), CG_TOL)
    xs = spl.spsolve(c["H"].tocsc(), c["F"])
    lo, mid, hi = c["window"]
    print("restated PCG, %s: %d iterations, window [%d, %d]" % (name, mid, lo, hi))
    assert ok and it == mid and lo <= mid <= hi
    assert np.linalg.norm(x - xs) <= 1e-7 * np.linalg.norm(xs)


def _mutated(c, name, what):
    """(preconditioner arrays, mutation argument of the cycle) of one deliberate defect"""
    N, M, nl, kind = SHAPES[name]
    if what == "S_unrounded_transposed":
        pc = mg.restated_pc(c["H"], N, M, nl, kind, s_from_rounded=False)
        L = pc["cloths"][0]["levels"][0]
        L["S32"] = mg.transposed_in_one_slot(L["S32"], L["N"], L["M"])
        return pc, None
    return c["pc"], {"boundary_restriction_weight": ("restrict", 0), "coarse_level_dropped": ("drop", 0), "omega_doubled": ("omega", 0),
                     "other_pingpong_buffer": ("pingpong", nl - 1)}[what]


# every defect on an input of the GPU tests where BOTH checks see it (a case where one stayed inside was replaced: the damping factor of a level
# that is followed by an exact solve, and the last-but-one of eight sweeps on the smaller smoothed levels, cost one or two iterations only)
MUTATIONS = [("boundary_restriction_weight", "12x20"), ("coarse_level_dropped", "8x8_one_workgroup"), ("omega_doubled", "12x20"),
             ("S_unrounded_transposed", "32x16_dense45"), ("other_pingpong_buffer", "50x26_per_sweep")]


@pytest.mark.parametrize("what,name", MUTATIONS)
def test_mutation_leaves_the_cycle_bound_and_the_pcg_window(oracle, what, name):
    c = _case(oracle, name)
    pc, mut = _mutated(c, name, what)
    rng = np.random.default_rng(11)
    nrm = lambda v: float(np.sqrt(np.dot(v, v)))
    worst = 0.0
    for _ in range(4):
        r = rng.normal(size=len(c["F"]))
        ref = mg.cycle(c["pc"], r, LD)
        e64 = nrm(mg.cycle(c["pc"], r).astype(LD) - ref)
        worst = max(worst, nrm(mg.cycle(pc, r, mut=mut).astype(LD) - ref) / bound(e64, nrm(ref)))
    it = mg.pcg(c["Hd"], c["F"], lambda r: mg.cycle(pc, r, mut=mut), CG_TOL, maxit=4 * c["window"][2])[1]
    lo, mid, hi = c["window"]
    print("mutation %s on %s: |mutated - ref| / bound %.3g, PCG count %d against the window [%d, %d]" % (what, name, worst, it, lo, hi))
    assert worst > 1.0
    assert not lo <= it <= hi
