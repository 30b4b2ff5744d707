"""tests/contact_numpy.py pinned without the kernels: mp central differences of its energy against its gradient and of its gradient against its
unprojected block, rotations, the records against the construction, decisions_safe for every state a GPU test uses, and the harness of
tests/test_gpu_contact_elements.py run with the float64 restatement in the kernels' place and with three deliberately wrong kernels."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_numpy as cn  # noqa: E402
from cloth_numpy import rotations  # noqa: E402


class Ratios(dict):
    """(test_gpu_tet_elements.Ratios, which imports torch)"""
    label = "contact restatement (float64 in the kernels' place)"

    def add(self, q, err, bnd):
        self[q] = max(self.get(q, 0.0), err / bnd)

    def check(self, what):
        print("%s, %s: largest |f64 - mp| / bound: %s" % (self.label, what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (what, bad)


def _cons():
    return cn.records_as_data(cn.own_records("geometry"))


def _mpv(a):
    return np.array([mp.mpf(float(v)) for v in np.asarray(a).ravel()], dtype=object).reshape(np.shape(a))


# states away from every switch, and one on each side of each switch
DIFF_STATES = ["rest", "d=-0.5eps", "d=2eps", "r=0.3eh oblique", "r=10eh t2", "r=1e3eh oblique, d=-0.5eps", "bump", "sheared to a sliver",
               "d=eps(1-1e-6)", "d=eps(1+1e-6)", "r=eh(1-1e-6)", "r=eh(1+1e-6)", "r=1e-9(1-1e-3)", "r=1e-9(1+1e-3)"]
DIFF_SLOTS = (0, 5, 10, 15)    # both edge lengths, both shapes, both proj_dir, all three kinds


@pytest.mark.parametrize("state", DIFF_STATES)
def test_gradient_and_block_are_derivatives(state):
    """central differences in mp, h = 1e-20: energy -> gradient, gradient -> unprojected block, to 1e-18 (the truncation error is (h / l)^2 times a
    modest constant, l the smallest length of a state: 1e-9 where r = 1e-9, 1e-7 the altitude of the 1e-4 m sliver: 1e-22 at most).  Below the guard
    r = 1e-9 the block leaves out f2 u u^T / r on purpose: there the difference is that term"""
    cons = _cons()
    pos = cn.state_positions("geometry", state)
    with mp.workdps(50):
        h = mp.mpf("1e-20")
        for s in DIFF_SLOTS:
            rec, X = cn.slot_rec(cons, s), _mpv(pos[cons["idx"][s]])
            ev = cn.slot_eval(cn.MP, X, rec)
            g, H = np.array(ev["g"], dtype=object), np.array(ev["H"], dtype=object)
            dE, dG = np.zeros(12, dtype=object), np.zeros((12, 12), dtype=object)
            for k in range(12):
                Xp, Xm = X.copy(), X.copy()
                Xp[k // 3, k % 3] += h; Xm[k // 3, k % 3] -= h
                ep, em = cn.slot_eval(cn.MP, Xp, rec), cn.slot_eval(cn.MP, Xm, rec)
                dE[k] = (ep["E"] - em["E"]) / (2 * h)
                dG[k] = (np.array(ep["g"], dtype=object) - np.array(em["g"], dtype=object)) / (2 * h)
            assert cn.fro(dE - g) <= mp.mpf("1e-18") * max(cn.fro(g), mp.mpf("1e-30")), (state, s)
            miss = dG - H
            if float(ev["r"]) <= cn.R_GUARD and float(ev["r"]) > 1e-12:
                fr = cn.friction_part(cn.MP, cn._P(cn.MP, X), rec)
                T, u, r = cn._V(cn.MP, rec["T"]), fr["u"], fr["r"]
                f2 = cn.f2(cn.MP, r, mp.mpf(cn.EH))
                core = [[f2 * u[i] * u[j] / r for j in range(2)] for i in range(2)]
                k = mp.mpf(float(rec["k"]))
                h1 = [[k * (T[a] * (core[0][0] * T[b] + core[0][1] * T[3 + b]) + T[3 + a] * (core[1][0] * T[b] + core[1][1] * T[3 + b])) for b in range(3)] for a in range(3)]
                D = np.array([[fr["w1"][i1] * fr["w1"][i2] * h1[j1][j2] for i2 in range(4) for j2 in range(3)] for i1 in range(4) for j1 in range(3)], dtype=object)
                assert cn.fro(D) > mp.mpf("1e-6") * abs(k) * fr["f1"]      # (1e-5 of the friction block: the block is deliberately not the derivative there)
                miss = miss - D
            assert cn.fro(miss) <= mp.mpf("1e-18") * cn.fro(H), (state, s)
            assert cn.fro(H - H.T) <= mp.mpf("1e-40") * cn.fro(H), (state, s, "the unprojected block is symmetric")


def test_rotations_commute_with_the_evaluation():
    cons = _cons()
    pos = cn.state_positions("geometry", "bump")
    with mp.workdps(50):
        for s in DIFF_SLOTS:
            rec, X = cn.slot_rec(cons, s), pos[cons["idx"][s]]
            z = np.random.default_rng(s).normal(size=12)
            ev = cn.slot_eval(cn.MP, X, rec, spd=1); ev.update(cn.slot_reverse(cn.MP, X, rec, z))
            a = cn._arr(ev)
            for R in rotations()[1:]:
                er = cn.slot_eval(cn.MP, X @ R.T, cn._rot_rec(rec, R), spd=1)
                er.update(cn.slot_reverse(cn.MP, X @ R.T, cn._rot_rec(rec, R), (z.reshape(4, 3) @ R.T).ravel()))
                b = cn._back(cn._arr(er), _mpv(R))
                for q in ("E", "g", "H", "acc", "fg"):
                    assert cn.fro(np.asarray(a[q] - b[q], dtype=object)) <= mp.mpf("1e-40") * max(cn.fro(a[q]), mp.mpf("1e-30")), (s, q)


def test_records_follow_the_construction():
    """every probe meant to be active is, none else; idx and the swap; n.x on the side of 0.5 it was built on; T orthogonal to n, its rows orthogonal and of
    equal length sqrt(1 - (n . t1)^2); the launch-edge and crowd scenes have every probe active"""
    sc = cn.scene("geometry")
    recs = cn.own_records("geometry")
    assert [r["probe"] for r in recs] == sc.active and len(sc.active) == 16 and sc.P == 17
    assert np.array_equal(np.array([r["idx"] for r in recs]), sc.idx())
    with mp.workdps(50):
        rm = cn.scene_records(cn.MP, sc)
        seen = set()
        for r, p in zip(rm, (sc.probes[i] for i in sc.active)):
            nx = float(p.tag.split("nx")[1].split()[0])
            assert abs(float(r["n"][0]) - nx) < 1e-9 and abs(float(r["gap"]) - 0.5 * cn.EPS) < 1e-12
            n, t1, t2 = r["n"], r["T"][:3], r["T"][3:]
            c = n[0] ** 2 if abs(n[0]) < 0.5 else n[2] ** 2
            for v in (cn._dot(n, t1), cn._dot(n, t2), cn._dot(t1, t2), cn._dot(t1, t1) - (1 - c ** 2), cn._dot(t2, t2) - (1 - c ** 2)):
                assert abs(v) < mp.mpf("1e-45")
            seen.add((abs(nx) < 0.5, p.pdir, p.kind))
        assert {t[:2] for t in seen} == {(a, b) for a in (True, False) for b in (0, 1)} and {t[2] for t in seen} == {0, 1, 2}
    for name in ("crowd", "nc1", "nc17", "nc129"):
        s2 = cn.scene(name)
        assert len(cn.own_records(name)) == s2.P == len(s2.active)


ALL_STATES = [k for k in cn.STATES if k not in cn.UNLAGGED]
REVERSE_SCENES = ["rv16", "rw16", "rw63", "rw64", "rw65", "rw129"]


@pytest.mark.parametrize("name", REVERSE_SCENES)
def test_decisions_are_safe_for_the_reverse_step_states(name):
    """with the exception for r == 0.0 by construction: asserted bit for bit in float64 on the slots that keep their four vertices"""
    assert len(cn.exact_zero_slots(name, "reverse mix")) >= 2
    assert cn.decisions_safe(name, "reverse mix", lagged=False)


def test_decisions_are_safe_where_r_is_exactly_zero():
    """detection with prev == pos, evaluation at that pos: r == 0.0 on the eight slots with proj_dir == 1 (both edge lengths, both shapes, the three kinds)"""
    exact = cn.exact_zero_slots("geometry", "r == 0 exactly")
    sc = cn.scene("geometry")
    tags = [sc.probes[sc.active[s]].tag for s in exact]
    assert len(exact) == 8 and any("sliver" in t and "L0.0001" in t for t in tags) and {t[-1] for t in tags} == {"0", "1", "2"}
    assert cn.decisions_safe("geometry", "r == 0 exactly", lagged=False)


@pytest.mark.parametrize("state", ALL_STATES)
def test_decisions_are_safe_for_every_gpu_state(state):
    assert cn.decisions_safe("geometry", state)


@pytest.mark.parametrize("name", ["crowd"] + ["nc%d" % n for n in (1, 15, 16, 17, 33, 63, 64, 65, 129)])
def test_decisions_are_safe_for_the_launch_edge_scenes(name):
    assert cn.decisions_safe(name, "rest")
    assert cn.decisions_safe(name, "bump")


def _frozen(sc_name, slot_pos):
    """one frozen dof in position `slot_pos` of every slot: component (slot + slot_pos) % 3"""
    sc = cn.scene(sc_name)
    fz = np.zeros(3 * sc.nv, np.int32)
    for s, vs in enumerate(sc.idx()):
        fz[3 * vs[slot_pos] + (s + slot_pos) % 3] = 1
    return fz


def _harness(state, spd, frozen, lagged=True):
    pos = cn.state_positions("geometry", state, lagged)
    cons, got = cn.f64_kernels("geometry", pos, spd, frozen, lagged=lagged)
    R = Ratios()
    cn.check_assembly(cn.Expected(cons, pos, spd, frozen), got, R, "%s spd%d" % (state, spd), frozen)
    return R


def test_float64_records_pass_the_harness_and_a_missing_swap_does_not():
    sc = cn.scene("geometry")
    proj = cn.construction_proj(sc)
    R = Ratios()
    cn.check_records(sc, _cons(), proj, R)
    R.check("records")
    wrong = {q: v.copy() for q, v in _cons().items()}      # a kernel that swaps the vertices of a proj_dir == 0 slot and forgets their weights
    for s, i in enumerate(sc.active):
        if sc.probes[i].pdir == 0:
            wrong["w"][s] = wrong["w"][s][[0, 2, 1]]
    with pytest.raises(AssertionError, match="swap"):
        cn.check_records(sc, wrong, proj, Ratios())


@pytest.mark.parametrize("state", ALL_STATES + ["r == 0 exactly"])
def test_float64_restatement_passes_the_harness(state):
    """every ratio <= 1 (by construction of e64: a rotated float64 evaluation is one of the copies) under spd 0 and 1, free and with a frozen dof"""
    for spd in (0, 1):
        for frozen in (None, _frozen("geometry", (spd + len(state)) % 4)):
            _harness(state, spd, frozen, state not in cn.UNLAGGED).check("%s spd%d%s" % (state, spd, "" if frozen is None else " frozen"))


def _wrong_hab_sign(monkeypatch):
    """normal_part with the sign of nh . (e_j x e_k) flipped in the (a, b) and (b, a) blocks of the second derivative of C: H9 moves by
    k_contact (d - eps) (-D / C^2) (-2 nh . (e_j x e_k))"""
    right = cn.normal_part

    def wrong(xp, X, sc=cn.SC, dec=None):
        d, active, en, g9, H9 = right(xp, X, sc, dec)
        if active:
            a, b, p = cn._sub(X[1], X[0]), cn._sub(X[2], X[0]), cn._sub(X[3], X[0])
            cr = cn._cross(a, b)
            C = cn._norm(xp, cr)
            D, nh = cn._dot(cr, p), [v / C for v in cr]
            pe = xp.num(sc.k_contact) * (d - xp.num(sc.eps))
            E = [cn._unit(j, xp) for j in range(3)]
            for ja in range(3):
                for ka in range(3):
                    t = pe * (-D / C ** 2) * (-2 * cn._dot(nh, cn._cross(E[ja], E[ka])))
                    H9[ja][3 + ka] = H9[ja][3 + ka] + t
                    H9[3 + ka][ja] = H9[3 + ka][ja] + t
        return d, active, en, g9, H9
    monkeypatch.setattr(cn, "normal_part", wrong)


def _wrong_f2_side(monkeypatch):
    monkeypatch.setattr(cn, "f2", lambda xp, x, eh: -1 / x ** 2 if x <= eh else -1 / eh ** 2)


@pytest.mark.parametrize("wrong,state", [("hab_sign", "d=0.5eps"), ("hab_sign", "bump"), ("f2_side", "r=0.3eh oblique"), ("f2_side", "r=10eh t2")])
def test_wrong_kernels_are_rejected(wrong, state):
    """the sign of the cross term nh . (e_j x e_k) of the mixed second derivative of C flipped; f2 taken on the wrong side of eps_v dt (the missing weight
    swap: test_float64_records_pass_the_harness_and_a_missing_swap_does_not).  The mistakes are patched over the restatement for the wrong kernel's run
    only: the reference carries no switch for them"""
    pos = cn.state_positions("geometry", state)
    exp = cn.Expected(_cons(), pos, 0)                       # the reference, before anything is patched
    with pytest.MonkeyPatch.context() as m:
        {"hab_sign": _wrong_hab_sign, "f2_side": _wrong_f2_side}[wrong](m)
        _, got = cn.f64_kernels("geometry", pos, 0)
    R = Ratios()
    cn.check_assembly(exp, got, R, "%s at %s" % (wrong, state))
    with pytest.raises(AssertionError):
        R.check("%s at %s" % (wrong, state))
    bad = {k: v for k, v in R.items() if v > 1.0}
    assert any(k.startswith("block") for k in bad), bad


def test_reverse_and_key_sums_of_the_float64_restatement():
    """the reverse-step quantities and the per-key sums by the float64 restatement (summed in float64 in slot order) against the mp sums"""
    sc = cn.scene("geometry")
    cons = _cons()
    pos = cn.state_positions("geometry", "r=10eh t2")
    rng = np.random.default_rng(3)
    z = rng.normal(size=(sc.nv, 3))
    fz = _frozen("geometry", 3)
    z[fz.reshape(-1, 3) == 1] = 0.0
    exp = cn.Expected(cons, pos, 0, fz, z)
    rev = cn.expected_reverse(exp, z, sc.kinds(), fz)
    keys = cn.expected_keys(exp, z, sc.kinds(), fz)
    acc, fg, ks = np.zeros((sc.nv, 3)), 0.0, {k: 0.0 for k in cn.KEYS}
    free = (fz == 0).reshape(-1, 3)
    for s in range(len(cons["k"])):
        vs, rec = cons["idx"][s], cn.slot_rec(cons, s)
        r = cn.slot_reverse(cn.F64, pos[vs], rec, z[vs].ravel())
        ev = cn.slot_eval(cn.F64, pos[vs], rec)
        acc[vs] += np.array(r["acc"]).reshape(4, 3)
        pf = (z[vs] * free[vs]).ravel()
        if sc.kinds()[s] == 2:
            fg += float(np.dot(pf, np.array(r["fg"]))) / cn.MU_CC
        sn, sf = float(np.dot(pf, np.array(ev["gn1"]))), float(np.dot(pf, np.array(ev["gf1"])))
        ks["k_contact"] -= sn + sf * (rec["k"] / cn.K_CONTACT)
        if sc.kinds()[s] == 1:
            ks["mu_cloth_elastic"] -= sf * (rec["k"] / cn.MU_CE)
        if sc.kinds()[s] == 2:
            ks["mu_cloth_cloth"] -= sf * (rec["k"] / cn.MU_CC)
    R = Ratios()
    R.add("backprop", cn.worst_ratio(cn._fn(cn.diff(acc, rev["acc"]), 1), rev["accb"]), 1.0)
    with mp.workdps(50):
        cn.ratio(R, "friction_grad", abs(float(mp.mpf(fg) - rev["fg"])), rev["fgb"])
        for k, (want, bnd) in keys.items():
            cn.ratio(R, "key " + k, abs(float(mp.mpf(ks[k]) - want)), bnd)
    assert rev["zfb"][fz.reshape(-1, 3) == 1].min() > 0 and not rev["zfb"][fz.reshape(-1, 3) == 0].any()
    R.check("reverse step")


# ------------------------------------------------------------------------------------------------ against the oracle
def _oracle_probes(oracle, probes):
    """the probes as two loaded bodies of the oracle with mu = lam = 0: body 0 = a tetrahedron per target triangle (apex behind it, one surface triangle), body 1
    = the query vertices, each with three companions to make a tetrahedron; a pair per kind over the query vertices"""
    P = len(probes)

    def nodes(tris, qs):
        n0, comp = [], []
        for tri, q in zip(tris, qs):
            nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0]); nrm /= np.linalg.norm(nrm)
            side = 1.0 if np.dot(q - tri[0], nrm) > 0 else -1.0
            n0 += [tri[0], tri[1], tri[2], tri.mean(0) - side * 5e-3 * nrm]
            comp += [q + side * 1e-3 * nrm + 1e-3 * e for e in np.eye(3)]
        return np.array(n0), np.array(list(qs) + comp)

    n0, n1 = nodes([p.tri for p in probes], [p.q for p in probes])
    o = oracle.OracleScene(dt=cn.DT, k_contact=cn.K_CONTACT, eps_contact=cn.EPS, eps_v=cn.EPS_V, gravity=(0.0, 0.0, 0.0), mu_cloth_elastic=cn.MU_CE)
    t0 = np.arange(4 * P, dtype=np.int32).reshape(-1, 4)
    e0 = o.add_loaded(1000.0, n0, t0, t0[:, :3].copy())
    e1 = o.add_loaded(1000.0, n1, np.array([[i, P + 3 * i, P + 3 * i + 1, P + 3 * i + 2] for i in range(P)], np.int32), np.zeros((0, 3), np.int32))
    o.elastic_init(e0, 0, 0, 0); o.elastic_init(e1, 0, 0, 0)
    o.finalize()
    for e in (0, 1):
        o.set_scalar("elastic%d.mu" % e, 0.0); o.set_scalar("elastic%d.lam" % e, 0.0)
    o.set_scalar("mu_cloth_cloth", cn.MU_CC); o.set_scalar("grid_h", cn.GRID_H)
    off1 = o.int("elastic1.offset")
    kinds = [p.kind for p in probes]
    for kind, mu in ((0, (cn.MU_FIXED, 0.0)), (1, (None, cn.CE_FACTOR)), (2, ("cloth_cloth", 0.0))):
        ids = [i for i, k in enumerate(kinds) if k == kind]
        o.add_pair(0, off1 + ids[0], off1 + ids[-1] + 1, mu[0], mu[1])
    o.frozen[:] = 0
    p0, p1 = nodes([p.ptri for p in probes], [p.pq for p in probes])
    return o, np.concatenate([n0, n1]), np.concatenate([p0, p1]), off1 + np.arange(P)


def test_oracle_agrees_on_probes(oracle):
    """records, energy, F and the dense H of the oracle (oracle/tslo_contact.cpp), H unprojected and with the converged clamp (set_spd_mode(1)), against the float64
    restatement fed with the oracle's own projection, on the eight probes of 1 / 150 m (both shapes, both proj_dir, the four n.x, the three kinds): records and energy to 1e-12,
    the unprojected H per vertex-pair block to 1e-12 of that pair block of the slot + 8 u |x| |block| / altitude (the coordinates' rounding through the third
    derivative), the clamped H to 1e-12 of the slot's whole unprojected block (a clamp's rounding scales with what it removes: the penetrated sliver has an
    eigenvalue of -2e7 next to a projected block of 2e4), F per vertex to 1e-12 of the slot's gradient norm + 8 u |x| |block| (what the rounding of the
    coordinates, u |x|, does to a gradient through its block).  The probes of 1e-4 m are left to the mp comparisons: at
    0.1 m from the origin a coordinate carries 1e-17 m of rounding, 1e-13 of such an edge, and two float64 evaluations differ by 1e-11 there (e64 says so)"""
    class S:
        pass
    probes = sorted([p for p in cn.geometry_probes(16, 0) if "L0.00666667" in p.tag], key=lambda p: p.kind)
    assert len(probes) == 8
    mu_of = {0: cn.MU_FIXED, 1: cn.MU_CE * cn.CE_FACTOR, 2: cn.MU_CC}
    oracle.set_spd_mode(1)
    try:
        o, x, prev, qv = _oracle_probes(oracle, probes)
        assert np.array_equal(o.pos, x)
        o.prev_pos[:] = prev; o.vel[:] = 0; o.push_down_all()
        o.calc_vn(); o.projection_query(); o.contact_analysis()
        nc = o.nc
        assert nc == len(probes)
        nb = o.int("n_bodies")
        assert o.arr("proj_flag", (nb, -1))[0, qv].all() and set(o.arr("proj_dir", (nb, -1))[0, qv]) == {0, 1}
        pidx, pw, pdir = o.arr("proj_idx", (nb, -1, 3))[0, qv], o.arr("proj_w", (nb, -1, 3))[0, qv], o.arr("proj_dir", (nb, -1))[0, qv]
        got = dict(idx=o.arr("const_idx", (-1, 4))[:nc].copy(), w=o.arr("const_w", (-1, 3))[:nc].copy(), k=o.arr("const_k")[:nc].copy(), mu=o.arr("const_mu")[:nc].copy(),
                   dx0=o.arr("const_dx0", (-1, 3))[:nc].copy(), T=o.arr("const_T", (-1, 6))[:nc].copy(), n=o.arr("const_n", (-1, 3))[:nc].copy())
        recs = []
        for i, p in enumerate(probes):
            vs = list(pidx[i]) + [qv[i]]
            r = cn.slot_records(cn.F64, x[vs], prev[vs], pw[i], pdir[i], mu_of[p.kind])
            assert r["active"]
            r["idx"], r["probe"] = [vs[k] for k in r["order"]], i
            recs.append(r)
        want = cn.records_as_data(recs)
        assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["w"], want["w"]) and np.array_equal(got["mu"], want["mu"])
        for q in ("k", "dx0", "T", "n"):
            assert np.abs(got[q] - want[q]).max() <= 1e-12 * np.abs(want[q]).max(), q
        sc = S(); sc.x = x
        geo = cn._geom(sc, recs)
        mdt2 = np.repeat(o.arr("mass"), 3) / o.dt ** 2
        states = [x.copy(), cn._set_d(sc, x.copy(), geo, -0.5), cn._slip(sc, geo, 0.3, "oblique"), cn._slip(sc, geo, 10.0, "t2", dfac=2.0), cn._bump(sc, geo)]
        for st_i, xe in enumerate(states):
            o.pos[:] = xe; o.prev_pos[:] = xe; o.vel[:] = 0; o.push_down_all()
            o.newton_step_init()
            E = o.compute_energy()
            for spd in (0, 1):
                o.newton_step_init(); o.compute_residual_and_Hessian(spd=bool(spd))
                F, H = o.arr("F").copy().reshape(-1, 3), o.H_csr().toarray() - np.diag(mdt2)
                nv = len(x)
                wF, wH, sF, sH, wE = np.zeros((nv, 3)), np.zeros((nv, 3, nv, 3)), np.zeros(nv), np.zeros((nv, nv)), 0.0
                for s in range(nc):
                    vs = got["idx"][s]
                    a = cn._arr(cn.slot_eval(cn.F64, xe[vs], cn.slot_rec(got, s), spd=spd))
                    nH = np.linalg.norm(cn._arr(cn.slot_eval(cn.F64, xe[vs], cn.slot_rec(got, s), spd=0))["H"]) if spd else np.linalg.norm(a["H"])
                    wE += float(a["E"])
                    for i in range(4):
                        wF[vs[i]] += a["g"][i]; sF[vs[i]] = max(sF[vs[i]], np.linalg.norm(a["g"]) + 8 * cn.U * np.abs(xe[vs]).max() * nH / 1e-12)
                        for j in range(4):
                            wH[vs[i], :, vs[j], :] += a["H"][i, :, j, :]; sH[vs[i], vs[j]] = max(sH[vs[i], vs[j]], nH if spd else np.linalg.norm(a["H"][i, :, j, :]) + 8 * cn.U * np.abs(xe[vs]).max() * nH / geo[s]["alt"] / 1e-12)
                assert abs(E - wE) <= 1e-12 * abs(wE)
                eF = np.linalg.norm(F - wF, axis=1)
                eH = np.sqrt(((H.reshape(nv, 3, nv, 3) - wH) ** 2).sum(axis=(1, 3)))
                assert not eF[sF == 0].any() and not eH[sH == 0].any()
                assert (eF[sF > 0] / sF[sF > 0]).max() <= 1e-12, (st_i, spd, (eF[sF > 0] / sF[sF > 0]).max())
                assert (eH[sH > 0] / sH[sH > 0]).max() <= 1e-12, (st_i, spd, (eH[sH > 0] / sH[sH > 0]).max(), np.argwhere(eH > 1e-12 * sH))
    finally:
        oracle.set_spd_mode(0)
