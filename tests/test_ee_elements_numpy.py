"""tests/ee_elements_numpy.py pinned without the kernels: the probe scenes against ee_numpy.brute_force, mp central differences of its energy against its
gradient and of its gradient against its unprojected block, agreement with tests/ee_numpy.py, the lag term of the reverse step against the mp difference
through k, decisions_safe for every state a GPU test uses, and the harness of tests/test_gpu_ee_elements.py run with the float64 restatement in the
kernels' place (every ratio at most 1 / 8) and with four deliberately wrong kernels."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_numpy as cn  # noqa: E402
import ee_elements_numpy as ee  # noqa: E402
import ee_numpy as en  # noqa: E402

NCS = (1, 15, 16, 17, 33, 63, 64, 65, 129)
RVS = (16, 63, 64, 65, 129)


class Ratios(dict):
    label = "edge-edge restatement (float64 in the kernels' place)"
    limit = 0.125      # a rotated or the plain float64 evaluation is one of the copies e64 is taken from: 1 / 8 by construction of the bound

    def add(self, q, err, bnd):
        self[q] = max(self.get(q, 0.0), err / bnd)

    def check(self, what):
        print("%s, %s: largest |f64 - mp| / bound: %s" % (self.label, what, ", ".join("%s %.3f" % kv for kv in sorted(self.items()))))
        bad = {k: v for k, v in self.items() if not v <= self.limit}
        assert not bad, (what, bad)


def _mpv(a):
    return np.array([mp.mpf(float(v)) for v in np.asarray(a).ravel()], dtype=object).reshape(np.shape(a))


# ------------------------------------------------------------------------------------------------ the probe scenes
@pytest.mark.parametrize("name", ["geometry", "crowd", "parallel", "nc17up", "nc1up"] + ["nc%d" % n for n in NCS] + ["rv%d" % n for n in RVS])
def test_only_the_probed_pairs_qualify_and_vertex_triangle_sees_nothing(name):
    """ee_numpy.brute_force over all edges of all bodies lists the probes' own pairs, in slot order, and nothing else; every query-body vertex projects onto
    the rim of its target triangle, whose vertices carry the border flag"""
    sc = ee.scene(name)
    idx, st = ee.brute_force(sc)
    assert np.array_equal(idx, sc.idx()) and len(idx) == len(sc.active)
    assert ee.vertex_triangle_sees_nothing(sc)
    recs = ee.own_records(name)
    assert np.array_equal(np.array([r["idx"] for r in recs]), sc.idx())
    assert np.abs(np.array([[float(r["w"][0]), float(r["w"][1])] for r in recs]) - st).max() < 1e-9


def test_geometry_probes_cross_the_properties_and_four_are_left_out():
    sc = ee.scene("geometry")
    assert sc.P == 20 and len(sc.active) == 16
    act = [sc.probes[i] for i in sc.active]
    L = cn.LS
    assert {(p.La, p.Lb) for p in act} == {(L[0], L[0]), (L[1], L[1]), (L[0], L[1])}
    assert {p.swapped for p in act} == {True, False} and {p.kind for p in act} == {0, 1, 2}
    assert {(p.s, p.t) for p in act} == set(ee.STS)
    for want in ("sin1 ", "sin0.3 ", "sin0.01 ", "nx0.499999", "nx0.500001", "nx0.1 ", "nx-0.9"):
        assert any(want in p.tag for p in act), want
    with mp.workdps(50):
        for xp in (cn.MP, cn.F64):
            d = []
            recs = ee.scene_records(xp, sc, dec=d)
            assert [r["probe"] for r in recs] == sc.active
            dec = dict(d)
            out = [i for i in range(sc.P) if i not in sc.active]
            failed = sorted(next(n for n, v in dec[i] if (v < 0) != (n in ("gap",))) for i in out)    # the first decision on the refusing side
            assert failed == ["gap", "s>0", "sin", "t<1"], failed
            for i in out:
                last = dec[i][-1] if dec[i][-1][0] in ("sin", "gap") else [t for t in dec[i] if t[0] in ("s>0", "t<1") and t[1] < 0][0]
                assert 5e-7 <= abs(float(last[1])) and (abs(float(last[1])) < 3e-6 or last[0] == "gap"), (i, last)
        for r, p in zip(ee.scene_records(cn.MP, sc), act):
            nx = float(p.tag.split("nx")[1].split()[0])
            assert abs(float(r["n"][0]) - nx) < 1e-9 and abs(float(r["gap"]) - 0.5 * cn.EPS) < 1e-12 and r["swapped"] == p.swapped
            assert abs(float(r["w"][0]) - p.s) < 1e-9 and abs(float(r["w"][1]) - p.t) < 1e-9
            v = ee._sub(r["dx0"], [r["gap"] * c for c in r["n"]])
            assert float(cn.fro(np.array(v, dtype=object))) > 1e-6          # prev != pos: dx0 is not the gap vector alone


def test_states_do_what_their_names_say():
    sc = ee.scene("geometry")
    cons = ee.f64_records("geometry")

    def lines(state):
        pos = ee.state_positions("geometry", state)
        out = []
        for s in range(16):
            X = pos[cons["idx"][s]]
            a, b = X[1] - X[0], X[3] - X[2]
            sin = np.linalg.norm(np.cross(a, b)) / np.linalg.norm(a) / np.linalg.norm(b)
            st = en.qualifies(X[2], X[3], X[0], X[1], 1e9) if sin >= 1e-2 else None
            ev = ee.slot_eval(cn.F64, X, ee.slot_rec(cons, s))
            out.append((sin, float(ev["d"]), float(ev["r"]), st))
        return out
    for state, sin in (("turned to sin=1e-2", 1e-2), ("turned to sin=1e-3", 1e-3), ("turned to sin=1e-5", 1e-5)):
        for got, d, _, _ in lines(state):
            assert abs(got / sin - 1) < 1e-4 and abs(d / (0.5 * cn.EPS) - 1) < 1e-6, (state, got, d)
    for _, d, _, st in lines("slid off the ends"):
        assert st is None or not (0 < st[0] < 1) and not (0 < st[1] < 1)
        assert abs(d / (0.5 * cn.EPS) - 1) < 1e-6
    for state, rr in (("r=1e-9(1+1e-3)", cn.R_GUARD * (1 + 1e-3)), ("r=eh(1-1e-6)", cn.EH * (1 - 1e-6)), ("r=1e3eh t1", 1e3 * cn.EH)):
        for _, _, r, _ in lines(state):
            assert abs(r / rr - 1) < 1e-7, (state, r)
    for state, dd in (("d=eps(1+1e-6)", 1 + 1e-6), ("d=-3eps", -3.0), ("d=2eps", 2.0)):
        for _, d, _, _ in lines(state):
            assert abs(d / (dd * cn.EPS) - 1) < 1e-8, (state, d)


# ------------------------------------------------------------------------------------------------ derivatives
DIFF_STATES = ["rest", "d=-0.5eps", "d=2eps", "r=0.3eh oblique", "r=10eh t2", "r=1e3eh oblique, d=-0.5eps", "bump", "turned to sin=1e-3", "slid off the ends",
               "d=eps(1-1e-6)", "d=eps(1+1e-6)", "r=eh(1-1e-6)", "r=eh(1+1e-6)", "r=1e-9(1-1e-3)", "r=1e-9(1+1e-3)"]
DIFF_SLOTS = (1, 2, 7, 11, 15)     # both edge lengths and the mixed pair, the three sines, D of both signs, the three kinds, (s, t) at the ends


@pytest.mark.parametrize("state", DIFF_STATES)
def test_gradient_and_block_are_derivatives(state):
    """central differences in mp, h = 1e-20: energy -> gradient, gradient -> unprojected block, to 1e-18 of the block (the truncation error is (h / l)^2 times
    a modest constant, l the smallest length of a state: 1e-9 where r = 1e-9, 1e-7 = edge x sin at sin = 1e-3: 1e-22 at most).  Below the guard r = 1e-9 the
    block leaves out f2 u u^T / r on purpose: there the difference is that term"""
    cons = ee.f64_records("geometry")
    pos = ee.state_positions("geometry", state)
    with mp.workdps(50):
        h = mp.mpf("1e-20")
        for s in DIFF_SLOTS:
            rec, X = ee.slot_rec(cons, s), _mpv(pos[cons["idx"][s]])
            ev = ee.slot_eval(cn.MP, X, rec)
            g, H = np.array(ev["g"], dtype=object), np.array(ev["H"], dtype=object)
            dE, dG = np.zeros(12, dtype=object), np.zeros((12, 12), dtype=object)
            for k in range(12):
                Xp, Xm = X.copy(), X.copy()
                Xp[k // 3, k % 3] += h; Xm[k // 3, k % 3] -= h
                ep, em = ee.slot_eval(cn.MP, Xp, rec), ee.slot_eval(cn.MP, Xm, rec)
                dE[k] = (ep["E"] - em["E"]) / (2 * h)
                dG[k] = (np.array(ep["g"], dtype=object) - np.array(em["g"], dtype=object)) / (2 * h)
            assert cn.fro(dE - g) <= mp.mpf("1e-18") * max(cn.fro(g), mp.mpf("1e-30")), (state, s)
            miss = dG - H
            if float(ev["r"]) <= cn.R_GUARD:
                fr = ee.friction_part(cn.MP, cn._P(cn.MP, X), rec)
                T, u, r = cn._V(cn.MP, rec["T"]), fr["u"], fr["r"]
                f2 = cn.f2(cn.MP, r, mp.mpf(cn.EH))
                core = [[f2 * u[i] * u[j] / r for j in range(2)] for i in range(2)]
                k = mp.mpf(float(rec["k"]))
                h1 = [[k * (T[a] * (core[0][0] * T[b] + core[0][1] * T[3 + b]) + T[3 + a] * (core[1][0] * T[b] + core[1][1] * T[3 + b])) for b in range(3)] for a in range(3)]
                D = np.array([[fr["w1"][i1] * fr["w1"][i2] * h1[j1][j2] for i2 in range(4) for j2 in range(3)] for i1 in range(4) for j1 in range(3)], dtype=object)
                assert cn.fro(D) > mp.mpf("1e-6") * abs(k) * fr["f1"] * min(abs(w) for w in fr["w1"]) ** 2
                miss = miss - D
            assert cn.fro(miss) <= mp.mpf("1e-18") * cn.fro(H), (state, s)
            assert cn.fro(H - H.T) <= mp.mpf("1e-40") * cn.fro(H), (state, s, "the unprojected block is symmetric")


def test_block_sums_to_zero_over_the_vertices_and_rotations_commute():
    """M's columns sum to zero: a translation of all four vertices changes nothing, rows and columns of the block sum to zero per axis; rotated input, rotated
    records: the same answer turned"""
    cons = ee.f64_records("geometry")
    pos = ee.state_positions("geometry", "bump")
    with mp.workdps(50):
        for s in DIFF_SLOTS:
            rec, X = ee.slot_rec(cons, s), pos[cons["idx"][s]]
            z = np.random.default_rng(s).normal(size=12)
            ev = ee.slot_eval(cn.MP, X, rec, spd=1); ev.update(ee.EE.slot_reverse(cn.MP, X, rec, z))
            a = cn._arr(ev)
            assert cn.fro(a["H"].sum(axis=0)) <= mp.mpf("1e-40") * cn.fro(a["H"]) and cn.fro(a["g"].sum(axis=0)) <= mp.mpf("1e-40") * cn.fro(a["g"])
            for R in cn.rotations()[1:]:
                er = ee.slot_eval(cn.MP, X @ R.T, cn._rot_rec(rec, R), spd=1)
                er.update(ee.EE.slot_reverse(cn.MP, X @ R.T, cn._rot_rec(rec, R), (z.reshape(4, 3) @ R.T).ravel()))
                b = cn._back(cn._arr(er), _mpv(R))
                for q in ("E", "g", "H", "acc"):
                    assert cn.fro(np.asarray(a[q] - b[q], dtype=object)) <= mp.mpf("1e-38") * max(cn.fro(a[q]), mp.mpf("1e-30")), (s, q)


# ------------------------------------------------------------------------------------------------ against tests/ee_numpy.py
def test_agrees_with_ee_numpy_on_the_large_probes():
    """qualifies, record, energy_normal, energy_friction and the complex-step gradient of tests/ee_numpy.py on the probes of 1 / 150 m with sin >= 0.3, to
    1e-12 (relative to the quantity; the gradient to the slot's gradient norm)"""
    sc = ee.scene("geometry")
    n = 0
    for i, p in enumerate(sc.probes):
        if not (p.La == p.Lb == cn.LS[0] and ("sin1 " in p.tag or "sin0.3 " in p.tag)):
            continue
        vs = sc.cand(i)
        rec = ee.slot_records(cn.F64, sc.x[vs], sc.prev[vs], sc.mu_of_kind[p.kind])
        q = en.qualifies(sc.x[vs[0]], sc.x[vs[1]], sc.x[vs[2]], sc.x[vs[3]], cn.EPS)
        assert (rec is None) == (q is None) == (not p.active), p.tag
        if rec is None:
            continue
        n += 1
        s, t, D = q
        assert (D < 0) == rec["swapped"] == p.swapped
        s = 1 - s if D < 0 else s
        assert abs(s - rec["w"][0]) <= 1e-12 and abs(t - rec["w"][1]) <= 1e-12
        idx = [vs[o] for o in rec["order"]]
        r2 = en.record(sc.x, sc.prev, idx, (rec["w"][0], rec["w"][1]), cn.K_CONTACT, cn.EPS, sc.mu_of_kind[p.kind])
        for qn in ("dx0", "k", "n", "T"):
            assert np.abs(np.array(rec[qn], float) - r2[qn]).max() <= 1e-12 * np.abs(r2[qn]).max(), (p.tag, qn)
        data = {k: np.array(rec[k], float) for k in ("w", "dx0", "T", "n")}
        data["k"], data["mu"] = float(rec["k"]), float(rec["mu"])
        for state in ("rest", "d=-0.5eps", "r=0.3eh oblique", "r=10eh t2", "bump"):
            slot = [j for j, a in enumerate(sc.active) if a == i][0]
            X = ee.state_positions("geometry", state)[idx]
            assert np.array_equal(idx, ee.f64_records("geometry")["idx"][slot])
            ev = ee.slot_eval(cn.F64, X, data)
            fn = lambda Z: en.energy_normal(Z, cn.K_CONTACT, cn.EPS)
            ff = lambda Z: en.energy_friction(Z, data["w"], data["dx0"], data["T"], data["k"], cn.EH)
            assert abs(float(ev["En"]) - fn(X)) <= 1e-12 * abs(fn(X)) and abs(float(ev["Ef"]) - ff(X)) <= 1e-12 * abs(ff(X)), (p.tag, state)
            g = en.grad_cs(fn, X) + en.grad_cs(ff, X)
            assert np.abs(np.array(ev["g"], float) - g).max() <= 1e-12 * np.linalg.norm(g), (p.tag, state)
    assert n >= 5


# ------------------------------------------------------------------------------------------------ the lag term
def _lag_identity(slot_eval, slot_reverse, d_of, Xd, X, rec, z):
    """the lag entries against -d / d x_detect of z . (friction gradient at X with k = -mu k_contact (gap(x_detect) - eps)), the records otherwise kept: the
    friction gradient is k times gf1, so the derivative is (z . gf1) (-mu k_contact) d gap / d x_detect, the last factor by mp central differences of the
    distance at the detection positions"""
    with mp.workdps(50):
        h = mp.mpf("1e-20")
        ev = slot_eval(cn.MP, X, rec)
        zg = sum(mp.mpf(float(a)) * b for a, b in zip(z, ev["gf1"]))
        Xd = _mpv(Xd)
        dgap = []
        for k in range(12):
            Xp, Xm = Xd.copy(), Xd.copy()
            Xp[k // 3, k % 3] += h; Xm[k // 3, k % 3] -= h
            dgap.append((d_of(Xp) - d_of(Xm)) / (2 * h))
        want = np.array([-(zg * (-mp.mpf(float(rec["mu"])) * mp.mpf(cn.K_CONTACT)) * v) for v in dgap], dtype=object)
        lag = np.array(slot_reverse(cn.MP, X, rec, z), dtype=object)
        assert cn.fro(want) > 0
        # the records hold n and w rounded to float64 and, for the vertex-triangle slot, the projection's weights: 1e-9 of the term
        return float(cn.fro(lag - want) / cn.fro(want))


def test_lag_term_is_minus_the_derivative_through_k_for_both_slot_types():
    """d gap / d x_i = w1_i n at the detection (exact for the line distance at the closest points, and for the plane distance at the foot point): the lag term
    of the reverse step is MINUS the derivative of z . (friction gradient) with respect to the detection positions through k alone, with the same sign for
    this restatement and for contact_numpy.slot_reverse"""
    z = np.random.default_rng(8).normal(size=12)
    sc, cons = ee.scene("geometry"), ee.f64_records("geometry")
    pos = ee.state_positions("geometry", "r=0.3eh oblique")
    for s in (0, 1, 4, 10, 15):
        vs = cons["idx"][s]
        rel = _lag_identity(ee.slot_eval, lambda xp, X, rec, z: ee.slot_reverse(xp, X, rec, z)["acc_lag"],
                            lambda X: ee.normal_part(cn.MP, cn._P(cn.MP, X), cn.SC)[0], sc.x[vs], pos[vs], ee.slot_rec(cons, s), z)
        assert rel < 1e-9, ("edge-edge", s, rel)
    vsc, vcons = cn.scene("geometry"), cn.records_as_data(cn.own_records("geometry"))
    vpos = cn.state_positions("geometry", "r=0.3eh oblique")

    def vt_lag(xp, X, rec, z):
        X = cn._P(xp, X)
        fr = cn.friction_part(xp, X, rec, cn.SC, 0)
        full = cn.slot_reverse(xp, X, rec, z)["acc"]
        zz = cn._V(xp, z)
        blk = [sum(zz[3 * i1 + j1] * fr["w1"][i1] * fr["w1"][i2] * fr["h1"][j1][j2] for i1 in range(4) for j1 in range(3)) for i2 in range(4) for j2 in range(3)]
        return [a - b for a, b in zip(full, blk)]
    for s in (0, 5, 10):
        vs = vcons["idx"][s]
        rel = _lag_identity(cn.slot_eval, vt_lag, lambda X: cn.normal_part(cn.MP, cn._P(cn.MP, X), cn.SC)[0], vsc.x[vs], vpos[vs], cn.slot_rec(vcons, s), z)
        assert rel < 1e-9, ("vertex-triangle", s, rel)


def test_lag_term_is_the_same_for_both_signs_of_wp_and_changes_with_one():
    cons = ee.f64_records("geometry")
    pos = ee.state_positions("geometry", "r=0.3eh oblique")
    z = np.random.default_rng(8).normal(size=12)
    X, rec = pos[cons["idx"][3]], ee.slot_rec(cons, 3)
    a = np.array(ee.slot_reverse(cn.F64, X, rec, z)["acc_lag"])
    b = np.array(ee.slot_reverse(cn.F64, X, rec, z, wp_out=+1)["acc_lag"])
    assert np.abs(a).max() > 0 and np.array_equal(a, -b)


# ------------------------------------------------------------------------------------------------ decisions
@pytest.mark.parametrize("state", ee.ASSEMBLY_STATES)
def test_decisions_are_safe_for_every_gpu_state(state):
    assert ee.decisions_safe("geometry", state)


def test_decisions_are_safe_where_the_edges_are_exactly_parallel():
    """a x b == 0.0 bit for bit on the float64 restatement, in the state and in its six rotations; the rest state of the same scene"""
    assert ee.decisions_safe("parallel", "exactly parallel") and ee.decisions_safe("parallel", "rest")
    cons = ee.f64_records("parallel")
    pos = ee.state_positions("parallel", "exactly parallel")
    for s in range(6):
        ev = ee.slot_eval(cn.F64, pos[cons["idx"][s]], ee.slot_rec(cons, s))
        assert not ev["active"] and np.isnan(ev["d"]) and float(ev["En"]) == 0.0 and float(ev["Ef"]) > 0.0


@pytest.mark.parametrize("name", ["crowd", "nc17up", "nc1up"] + ["nc%d" % n for n in NCS])
def test_decisions_are_safe_for_the_launch_edge_scenes(name):
    assert ee.decisions_safe(name, "bump")


def test_decisions_are_safe_for_the_vertex_triangle_probes_of_the_offset_scenes():
    """(the edge-edge probes behind them, "nc17up" and "nc1up", stand 0.06 m above the lattice: with the launch-edge scenes)"""
    for name, up in (("nc5", "nc17up"), ("nc64", "nc1up")):
        assert cn.decisions_safe(name, "bump")
        m = ee.Merged(cn.scene(name), ee.scene(up))
        idx, _ = ee.brute_force(m)       # the merged tables list the edge-edge probes' own pairs and nothing else
        assert np.array_equal(idx, ee.scene(up).idx() + cn.scene(name).nv) and np.array_equal(m.idx()[cn.scene(name).P:], idx)


@pytest.mark.parametrize("n", RVS)
def test_decisions_are_safe_and_the_operator_is_definite_for_the_reverse_step(n):
    """m / dt^2 of the "rv" scenes is a power of two above the most negative eigenvalue of the summed mp unprojected operator at x_2, and the next smaller
    power of two is not"""
    name = "rv%d" % n
    assert ee.decisions_safe(name, "reverse mix", lagged=False)
    sc = ee.scene(name)
    cons = ee.f64_records(name, False)
    pos = ee.state_positions(name, "reverse mix", False)
    op = np.zeros((sc.nv, 3, sc.nv, 3))
    with mp.workdps(50):
        for s in range(len(cons["k"])) if n == 16 else ():
            vs = cons["idx"][s]
            H = np.array(ee.slot_eval(cn.MP, pos[vs], ee.slot_rec(cons, s))["H"], dtype=object).astype(float).reshape(4, 3, 4, 3)
            for i in range(4):
                for j in range(4):
                    op[vs[i], :, vs[j], :] += H[i, :, j, :]
    if n != 16:      # (the larger scenes repeat the probes of the first: float64 blocks, whose error the margin below covers many times over)
        op = ee.f64_kernels(name, pos, 0, lagged=False)[1]["op"]
    lo = np.linalg.eigvalsh(op.reshape(3 * sc.nv, 3 * sc.nv)).min()
    assert np.log2(sc.mdt2) == round(np.log2(sc.mdt2)) and -lo < sc.mdt2 / 1.25 and -lo > sc.mdt2 / 2, (lo, sc.mdt2)


# ------------------------------------------------------------------------------------------------ the harness with float64 in the kernels' place
def _frozen(name, slot_pos):
    sc = ee.scene(name)
    fz = np.zeros(3 * sc.nv, np.int32)
    for s, vs in enumerate(sc.idx()):
        fz[3 * vs[slot_pos] + (s + slot_pos) % 3] = 1
    return fz


def _harness(name, state, spd, frozen, lagged=True):
    pos = ee.state_positions(name, state, lagged)
    cons, got = ee.f64_kernels(name, pos, spd, frozen, lagged=lagged)
    R = Ratios()
    cn.check_assembly(ee.expected(cons, pos, spd, state=state), got, R, "%s spd%d" % (state, spd), frozen)
    return R


@pytest.mark.parametrize("state", ee.ASSEMBLY_STATES)
def test_float64_restatement_passes_the_harness(state):
    for spd in (0, 1):
        for frozen in (None, _frozen("geometry", (spd + len(state)) % 4)):
            _harness("geometry", state, spd, frozen).check("%s spd%d%s" % (state, spd, "" if frozen is None else " frozen"))


def test_float64_restatement_passes_the_harness_where_the_edges_are_exactly_parallel():
    for spd in (0, 1):
        for frozen in (None, _frozen("parallel", 2 + spd)):
            R = _harness("parallel", "exactly parallel", spd, frozen)
            R.check("exactly parallel spd%d" % spd)


def test_float64_records_pass_the_harness():
    R = Ratios()
    ee.check_records(ee.scene("geometry"), ee.f64_records("geometry"), R)
    R.check("records")
    assert set(R) == {"record " + q for q in ("s", "t", "k", "dx0", "n", "T")}


def _reverse_harness(name, frozen_pos, wrong=False):
    sc = ee.scene(name)
    cons = ee.f64_records(name, False)
    pos = ee.state_positions(name, "reverse mix", False)
    fz = np.zeros(3 * sc.nv, np.int32) if frozen_pos is None else _frozen(name, frozen_pos)
    z = np.random.default_rng(3).normal(size=(sc.nv, 3)) * (fz == 0).reshape(-1, 3)
    exp = cn.Expected(cons, pos, 0, fz, z, model=ee.EE)
    rev = cn.expected_reverse(exp, z, np.zeros(len(cons["k"]), int), fz)
    if wrong:
        with pytest.MonkeyPatch.context() as m:
            right = ee.slot_reverse
            m.setattr(ee, "slot_reverse", lambda *a, **k: right(*a, wp_out=+1, **k))
            acc, zf = ee.f64_reverse(name, pos, z, cons, fz)
    else:
        acc, zf = ee.f64_reverse(name, pos, z, cons, fz)
    R = Ratios()
    R.add("backprop", cn.worst_ratio(cn._fn(cn.diff(acc, rev["acc"]), 1), rev["accb"]), 1.0)
    on = fz.reshape(-1, 3) == 1
    if on.any():
        R.add("tmp_z_frozen", cn.worst_ratio(np.abs(cn.diff(zf, rev["zf"]))[on], rev["zfb"][on]), 1.0)
        assert rev["zfb"][on].min() > 0 and not rev["zfb"][~on].any()
    return R


@pytest.mark.parametrize("frozen_pos", [None, 0, 3])
def test_reverse_step_of_the_float64_restatement(frozen_pos):
    _reverse_harness("rv16", frozen_pos).check("reverse step, frozen %s" % frozen_pos)


# ------------------------------------------------------------------------------------------------ four wrong kernels
def _got_with(patch, state, spd=0):
    pos = ee.state_positions("geometry", state)
    cons = ee.f64_records("geometry")
    exp = ee.expected(cons, pos, spd, state=state)                  # the reference, before anything is patched
    with pytest.MonkeyPatch.context() as m:
        patch(m)
        _, got = ee.f64_kernels("geometry", pos, spd)
    R = Ratios()
    cn.check_assembly(exp, got, R, state)
    return R


@pytest.mark.parametrize("state", ["rest", "d=-0.5eps", "bump"])
def test_wrong_row_map_is_rejected(state):
    """the M row of vertex 2 with the wrong sign on q_1: (0, +1, 1)"""
    R = _got_with(lambda m: m.setattr(ee, "M", ((-1, 0, -1), (1, 0, 0), (0, 1, 1), (0, 1, 0))), state)
    with pytest.raises(AssertionError):
        R.check("wrong M at " + state)
    assert R["block spd0"] > 1e6 and R["F"] > 1e6, dict(R)


@pytest.mark.parametrize("state", ["rest", "r=10eh t2", "bump"])
def test_exchanged_friction_weights_are_rejected(state):
    """friction weights with s and t exchanged: w1 = (s - 1, -s, 1 - t, t)"""
    right = ee.weights

    def wrong(xp, w):
        s, t, _ = right(xp, w)
        return s, t, right(xp, [w[1], w[0]])[2]
    R = _got_with(lambda m: m.setattr(ee, "weights", wrong), state)
    with pytest.raises(AssertionError):
        R.check("exchanged weights at " + state)
    assert R["block spd0"] > 1e6 and R["F"] > 1e6, dict(R)


def test_missing_s_swap_is_caught_by_the_records_and_not_by_the_assembly():
    """s -> 1 - s left out of the swap: the records test names it; the assembly takes the exported records as data and passes, as it must"""
    sc = ee.scene("geometry")
    wrong = {q: v.copy() for q, v in ee.f64_records("geometry").items()}
    sw = [s for s, i in enumerate(sc.active) if sc.probes[i].swapped]
    assert len(sw) >= 4
    wrong["w"][sw, 0] = 1 - wrong["w"][sw, 0]
    with pytest.raises(AssertionError, match="s -> 1 - s left out"):
        ee.check_records(sc, wrong, Ratios())
    pos = ee.state_positions("geometry", "rest")
    _, got = ee.f64_kernels("geometry", pos, 0, cons=wrong)
    R = Ratios()
    cn.check_assembly(ee.expected(wrong, pos, 0), got, R, "missing swap")
    R.check("assembly with the records of a missing swap")


def test_wrong_sign_of_wp_is_caught_by_pos_grad_alone():
    """wp = +w1 on the entry the lag term writes: the backprop sum is off, tmp_z_frozen (blocks only) and the assembly are not"""
    R = _reverse_harness("rv16", 3, wrong=True)
    assert R["backprop"] > 1e6 and R["tmp_z_frozen"] <= 0.125, dict(R)
