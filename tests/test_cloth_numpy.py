"""tests/cloth_numpy.py, the reference of tests/test_gpu_cloth_elements.py, pinned without the kernels: mp central differences of its own energy
and gradients, rotations, the oracle (oracle/pyoracle.py) on flat and folded sheets, decisions_safe on every state the GPU tests use, the size of
the float64 errors the GPU bounds are built from, and the harness itself with the float64 restatement in the kernels' place."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloth_numpy as cn  # noqa: E402
import tet_numpy as tn  # noqa: E402
from cloth_numpy import MP  # noqa: E402

H = "1e-20"


def _mpx(x):
    return np.array([mp.mpf(float(v)) for v in np.asarray(x).ravel()], dtype=object).reshape(-1, 3)


def _cd(fun, x):
    """central differences (h = 1e-20) of fun over every coordinate of x, stacked on a new first axis"""
    h = mp.mpf(H)
    rows = []
    for i in range(x.size):
        xp_, xm_ = x.copy(), x.copy()
        xp_.flat[i] = xp_.flat[i] + h
        xm_.flat[i] = xm_.flat[i] - h
        rows.append((np.array(fun(xp_), dtype=object) - np.array(fun(xm_), dtype=object)) / (2 * h))
    return np.array(rows, dtype=object)


def _dense(c, ev, q):
    """face parts [f, l, j, m, k] summed into a dense (3 NV, 3 NV) object matrix"""
    A = np.full((c.NV, 3, c.NV, 3), mp.mpf(0), dtype=object)
    for f in range(c.NF):
        for l in range(3):
            for m in range(3):
                A[c.f2v[f, l], :, c.f2v[f, m], :] += ev[q][f, l, :, m, :]
    return A.reshape(3 * c.NV, 3 * c.NV)


# (no state with faces coplanar by construction off a coordinate plane: their true angle is the rounding of the inputs, 1e-16 rad of either sign, which
# the sign rule's dead zone of 1e-10 |e| reads as positive -- there the gradient 2 Kb |theta| d(theta) is not the derivative of Kb theta^2 when the true
# angle is negative, by 1e-16 of the terms: the rule's price, far below float64, but visible to a difference at 50 digits)
FD_STATES = ["1x1/dx150/bump", "1x1/dx150/fold-170_refopp", "1x1/dx1e-4/fold+pi_ref0", "1x1/dx150/fold-90_refsame", "2x1/dx1e-4/bump", "3x2/dx150/bump",
             "3x2/dx1e-4/compress"]


@pytest.mark.parametrize("key", FD_STATES)
@tn.with_mp
def test_gradients_and_blocks_are_differences_of_energy_and_gradient(key):
    """spring, area and hinge gradients are the derivatives of the restatement's own energies; the spring block and the area block are the
    derivatives of their gradients once the reference's two slips are taken out (literal=False: the sign of the off-diagonal of d2 len, and the
    doubled term of compute_area_dxy_p12), and differ from them with the slips in wherever a spring or the area is off its rest value.  Step 1e-20
    on coordinates of 1e-4 .. 1e-2 m at 50 digits: truncation and rounding below 1e-28 relative, asserted at 1e-24 of the block's scale."""
    st = cn.STATES[key]()
    c, x, ra = st.cloths[0], _mpx(st.local(0)), st.ra[0]
    g_fd = _cd(lambda y: cn.totals(MP, c, y, ra), x)                      # [coordinate][S, A, B]
    G = cn.totals(MP, c, x, ra, "gradient")
    ev = cn.evaluate(MP, c, x, ra, literal=False)
    lit = cn.evaluate(MP, c, x, ra)
    HS, HA = _dense(c, ev, "HS"), _dense(c, ev, "HA")
    scale = [tn.fro(HS) * c.dx, tn.fro(HA) * c.dx, tn.fro(lit["G"]) * c.dx]
    for t in range(3):
        assert tn.fro(g_fd[:, t] - G[t].ravel()) <= mp.mpf("1e-24") * scale[t], (key, "SAB"[t])
    K_fd = _cd(lambda y: cn.totals(MP, c, y, ra, "gradient")[:2].reshape(2, -1), x)   # [variable][S, A][gradient entry]
    assert tn.fro(K_fd[:, 0].T - HS) <= mp.mpf("1e-24") * tn.fro(HS)
    assert tn.fro(K_fd[:, 1].T - HA) <= mp.mpf("1e-24") * tn.fro(HA)
    if "bump" in key or "compress" in key:   # (springs and areas off rest: the literal blocks are not the derivatives)
        assert tn.fro(_dense(c, lit, "HS") - HS) > mp.mpf("1e-3") * tn.fro(HS)
        assert tn.fro(_dense(c, lit, "HA") - HA) > mp.mpf("1e-6") * tn.fro(HA)


@tn.with_mp
def test_rigid_rotations_leave_energy_and_angles_unchanged():
    c_, s_ = mp.cos(mp.mpf("0.9")), mp.sin(mp.mpf("0.9"))
    Rz = np.array([[c_, -s_, 0], [s_, c_, 0], [0, 0, 1]], dtype=object)
    Rx = np.array([[1, 0, 0], [0, c_, s_], [0, -s_, c_]], dtype=object)
    R = Rz.dot(Rx)
    for key in ("3x2/dx150/bump", "3x2/dx150/fold-170_refopp", "1x1/dx1e-4/fold+pi_ref0"):
        st = cn.STATES[key]()
        c, x, ra = st.cloths[0], _mpx(st.local(0)), st.ra[0]
        a, b = cn.evaluate(MP, c, x, ra), cn.evaluate(MP, c, x.dot(R.T), ra)
        # (the angle of two coplanar faces is the square root of the rounding of 1 - c, 1e-25 at 50 digits: theta and what is linear in it to 1e-24)
        for q, tol in (("eS", "1e-40"), ("eA", "1e-40"), ("eB", "1e-40"), ("theta", "1e-24"), ("newref", "1e-24")):
            assert tn.fro(a[q] - b[q]) <= mp.mpf(tol) * max(tn.fro(a[q]), 1), (key, q)
        for q, tol in (("gS", "1e-40"), ("gA", "1e-40"), ("gB", "1e-24")):
            assert tn.fro(a[q].dot(R.T) - b[q]) <= mp.mpf(tol) * max(tn.fro(a[q]), tn.fro(a["G"]) * c.dx), (key, q)


def test_signed_angles_of_the_built_states():
    """a fold built with the dihedral phi has theta = phi on the hinges of its line (the sign convention of the states is the reference's),
    a ripple +-theta alternating, and the reference angles of `same` cancel the bending gradient there"""
    for key, phi in (("3x2/dx150/fold+90_ref0", np.pi / 2), ("3x2/dx150/fold-170_ref0", -np.radians(170.0)), ("1x2/dx150/fold+pi_ref0", cn.PI_NEAR),
                     ("1x1/dx150/fold-90_refsame", -np.pi / 2)):
        st = cn.STATES[key]()
        c = st.cloths[0]
        ev = cn.evaluate(cn.F64, c, st.local(0), st.ra[0])
        on = np.abs(ev["theta"]) > 1e-3
        assert on.any() and np.allclose(ev["theta"][on], phi, rtol=0, atol=1e-9), (key, ev["theta"])
    st = cn.STATES["3x2/dx150/ripple1.5e-3"]()
    th = cn.evaluate(cn.F64, st.cloths[0], st.local(0), st.ra[0])["theta"]
    on = np.abs(th) > 1e-6
    assert sorted(set(np.round(th[on] / 1.5e-3, 6))) == [-1.0, 1.0]
    st = cn.STATES["3x2/dx150/fold+170_refsame"]()
    ev = cn.evaluate(cn.F64, st.cloths[0], st.local(0), st.ra[0])
    # (uncancelled it is theta = 3 times this yardstick; the coplanar hinges of the turned half leave 2e-8 rad of the series branch's rounding)
    assert np.abs(ev["gB"]).max() <= 1e-7 * np.abs(ev["G"]).max() * st.cloths[0].dx


def test_switch_sits_between_the_ripples():
    """c = 0.999999 is theta = 1.41421e-3: the ripples of 1.3e-3 take the series, those of 1.5e-3 acos"""
    for key, series in (("3x2/dx150/ripple1.0e-4", True), ("3x2/dx150/ripple1.3e-3", True), ("3x2/dx150/ripple1.5e-3", False)):
        d = [t for t in cn.decisions(cn.STATES[key](), cn.F64)[0] if t[0] == "switch" and abs(float(t[-1]) + 1) > 1e-3]
        assert d and all((float(t[-1]) < 0) == series for t in d), key


def test_update_ref_angle_moves_only_beyond_the_threshold():
    for key in cn.PLASTIC_KEYS:
        st = cn.STATES[key]()
        fac = float(key.split("/")[1])
        for i, c in enumerate(st.cloths):
            ev = cn.evaluate(cn.F64, c, st.local(i), st.ra[i])
            moved = ev["newref"] != 0
            assert moved.any() == (abs(fac) > 1), key
            if abs(fac) > 1:
                ka, th = c.k_angle, ev["theta"][moved]
                assert np.allclose(ev["newref"][moved], np.sign(th) * (np.abs(th) - ka), rtol=1e-12, atol=0)


@pytest.mark.parametrize("key", cn.GPU_KEYS + cn.PLASTIC_KEYS)
def test_every_gpu_state_has_safe_decisions(key):
    assert cn.decisions_safe(cn.STATES[key]())


def test_frozen_rule_and_pattern_of_expected():
    ref = cn.reference("1x1/dx150/bump")
    e = cn.expected(ref, "all", 0, (0, 2, 3), 5)
    A = e.A[0].reshape(4, 3, 4, 3)
    m = cn.MASS / cn.DT ** 2
    for v in (0, 2, 3):
        assert np.array_equal(A[v, :, v, :], m * np.eye(3)) and not A[v, :, [1], :].any() and not A[[1], :, v, :].any()
        assert not e.g[0][v].any()
    assert A[1, :, 1, :].any() and e.pattern.all()


ILL = ("pi", "sliver")   # theta within 1e-3 of pi (acos loses half the digits), slivers (1 / h)
E64_KEYS = [k for k in cn.GPU_KEYS if k.split("/")[0] in ("3x2", "1x1") or (k.split("/")[0] in ("2x1", "1x2") and "dx150" in k)]
COPLANAR_NOISE = 2 * np.sqrt(4 * 2.0 ** -53) / np.sqrt(2.0)   # 3e-8 rad: the series branch at 1 - c = four ulps


@pytest.mark.parametrize("key", E64_KEYS)
def test_float64_errors_are_far_below_the_quantities_they_bound(key):
    """e64 < 1e-9 of the quantity per element in every benign state, so that bound() cannot swallow a real error: face block parts, hinge block,
    and the gradients against the larger of their own norm and the terms that cancel in them (|block| dx).  In the ill-conditioned states
    (theta within 1e-3 of pi, slivers) the values are only finite, and printed.
    One more ill-conditioned case came out of the measurement and is the reference's own: two faces coplanar by construction but not parallel
    to a coordinate plane (a turned flat sheet, the tilted half of a fold, a tilted strip of a ripple) have c = 1 - (0 .. 2) ulp in float64, and
    the series branch takes the square root of that rounding: theta is 0 .. 2e-8 rad there instead of 0, in the oracle and in the kernels alike.
    What is linear in theta (the bending gradient, c_i of the second-order part) is then bounded by that angle and no better; with such a pair
    in the state gB and HB are asserted below 3e-8 (1 - c four ulps off), everything else below 1e-9 as elsewhere."""
    ref = cn.reference(key)
    ill = any(t in key for t in ILL)
    worst = {}
    noisy = False
    for i, c in enumerate(ref.st.cloths):
        hl = ref.hl[i]
        same = np.array([ref.st.pieces[i][f] >= 0 and ref.st.pieces[i][f] == ref.st.pieces[i][c.cf[f, l]] for f, l in c.hinges], bool)
        if same.any():
            noisy |= bool(max(np.abs(ev["theta"][same]).max() for ev in ref.f64[i]) > 0)
        for q, axes, yard in (("HS", (1, 2, 3, 4), None), ("HA", (1, 2, 3, 4), None), ("HB", (1, 2, 3, 4), "G"), ("G", (1, 2, 3, 4), None),
                              ("gS", (1, 2), "HS"), ("gA", (1, 2), "HA"), ("gB", (1, 2), "G")):
            if not len(hl[q][0]):
                continue
            e = ref.e64(i, lambda ev, part: cn._sel(ev, part, [q]), axes)
            n = np.sqrt((hl[q][0] ** 2).sum(axis=axes))
            if yard == "G" and q == "HB":     # the second-order bending part is a difference of terms of the size of the Gauss-Newton blocks
                n = np.maximum(n, np.sqrt((hl["G"][0] ** 2).sum(axis=(1, 2, 3, 4))).max())
            elif yard:
                n = np.maximum(n, np.sqrt((hl[yard][0] ** 2).sum(axis=(1, 2, 3, 4))).max() * c.dx)
            assert np.isfinite(e).all(), (key, q)
            on = n > 0
            if on.any():
                worst[q] = max(worst.get(q, 0.0), float((e[on] / n[on]).max()))
    print("cloth e64 / quantity, %s: %s" % (key, ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))
    if not ill:
        for q, v in worst.items():
            assert v < (COPLANAR_NOISE if noisy and q in ("gB", "HB") else 1e-9), (key, q, worst)


@pytest.mark.parametrize("key", ["3x2/dx150/fold+90_refopp", "3x2/dx1e-4/bump", "1x1/dx150/rest_rot", "3x2/dx150/sliver", "2x1/dx150/fold+pi_ref0"])
def test_harness_passes_the_float64_restatement_and_fails_a_wrong_term(key):
    """the float64 restatement in the kernels' place (another rotation, so other rounding) meets the bound of every quantity, 1 / 8 where e64
    is met; the same harness rejects the area block without the reference's slip and a hinge with its two inner gradients exchanged"""
    from test_gpu_tet_elements import Ratios
    ref = cn.reference(key)
    R = Ratios(); R.label = "cloth elements (float64 in the kernels' place)"
    for combo in cn.COMBOS:
        e = cn.expected(ref, combo, 0, (), 3)
        for k in (1, 4, 9):
            A, g, E = cn.f64_assembly(ref, combo, k)
            cn.check_assembly(e, A, g, R, "spd0 " + combo)
            cn.ratio(R, "energy", abs(float(mp.mpf(E) - e.E)), e.Eb)
    R.check(key)
    if "bump" in key:
        st = ref.st
        wrong = cn.evaluate(cn.F64, st.cloths[0], st.local(0), st.ra[0], literal=False)
        saved = ref.f64[0][0]
        try:
            ref.f64[0][0] = wrong
            A, g, E = cn.f64_assembly(ref, "Ka", 0)
        finally:
            ref.f64[0][0] = saved
        bad = Ratios()
        cn.check_assembly(cn.expected(ref, "Ka", 0, (), 3), A, g, bad, "spd0 Ka")
        assert max(bad.values()) > 1e3, bad
        swapped = dict(saved)   # d(theta)/dx of the two vertices on the hinge's edge exchanged
        swapped["gB"] = saved["gB"][:, [0, 2, 1, 3]]
        swapped["G"] = saved["G"][:, [0, 2, 1, 3]][:, :, :, [0, 2, 1, 3]]
        try:
            ref.f64[0][0] = swapped
            A, g, E = cn.f64_assembly(ref, "Kb", 0)
        finally:
            ref.f64[0][0] = saved
        bad = Ratios()
        cn.check_assembly(cn.expected(ref, "Kb", 0, (), 3), A, g, bad, "spd0 Kb")
        assert bad["block spd0 Kb"] > 1e3 and bad["gradient"] > 1e3, bad


# ------------------------------------------------------------------------------------------------ against the oracle
def _oracle_scene(oracle, N, M, dx, x, ra):
    o = oracle.OracleScene(dt=cn.DT, gravity=(0.0, 0.0, 0.0), plastic=0)
    ci = o.add_cloth(N, M, dx * N)
    o.cloth_init(ci, 0, 0, 0)
    o.finalize()
    o.frozen[:] = 0
    o.pos[:] = x; o.prev_pos[:] = x; o.vel[:] = 0
    o.arr("cloth0.ref_angle", (-1, 3))[:] = ra
    o.push_down_all()
    return o


@pytest.mark.parametrize("N,M", [(3, 2), (5, 4), (2, 7)])
def test_oracle_agrees_on_flat_and_folded_sheets(oracle, N, M):
    """F and the dense H of the oracle, unprojected and with the converged eigen-clamp of the spring blocks (set_spd_mode(1)), against the sums
    of the float64 restatement, per vertex-pair block to 1e-12 of the block norm (of the largest element block where blocks cancel): the
    flat sheet with 2e-4 m of noise of tests/test_gpu_cloth.py, and sheets folded by 90 and 170 degrees about a grid line with reference angles
    of +-0.3 rad on every slot"""
    dx = 0.1 / 15
    c = cn.ClothTables(N, M, dx)
    rng = np.random.default_rng(N * 10 + M)
    states = [("noise", cn.flat(c)[0] + rng.normal(0, 2e-4, (c.NV, 3)), rng.normal(0, 0.05, (c.NF, 3)))]
    ax, line = (0, 1) if N >= 3 else (1, 3)
    for deg in (90.0, -170.0):
        states.append(("fold %g" % deg, cn.fold(c, np.radians(deg), ax, line)[0], cn.random_ref(c, seed=int(abs(deg)))))
    oracle.set_spd_mode(1)
    try:
        for name, x, ra in states:
            o = _oracle_scene(oracle, N, M, dx, x, ra)
            assert np.array_equal(o.arr("cloth0.f2v", (-1, 3)), c.f2v) and np.array_equal(o.arr("cloth0.counter_face", (-1, 3)), c.cf)
            ev = cn.evaluate(cn.F64, c, x, ra)
            mdt2 = np.repeat(o.arr("mass") / o.dt ** 2, 3)
            for spd in (False, True):
                o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(spd)
                got_F, got_H = o.arr("F").copy().reshape(-1, 3), o.H_csr().toarray()
                K3 = ev["K3"] if not spd else np.array([[cn.clamp3(cn.F64, ev["K3"][f][s].tolist()) for s in range(3)] for f in range(c.NF)])
                HS = np.array([cn.scatter_springs(cn.F64, K3[f].tolist()) for f in range(c.NF)]).reshape(c.NF, 3, 3, 3, 3)
                T = HS + ev["HA"] + ev["HB"]
                want = np.zeros((c.NV, 3, c.NV, 3)); yard = np.zeros((c.NV, c.NV)); wF = np.zeros((c.NV, 3))
                for f in range(c.NF):
                    for l in range(3):
                        wF[c.f2v[f, l]] += ev["gS"][f, l] + ev["gA"][f, l]
                        for m in range(3):
                            want[c.f2v[f, l], :, c.f2v[f, m], :] += T[f, l, :, m, :]
                            yard[c.f2v[f, l], c.f2v[f, m]] = max(yard[c.f2v[f, l], c.f2v[f, m]], np.linalg.norm(T[f, l, :, m, :]))
                for h, (f, l) in enumerate(c.hinges):
                    hv = c.hinge_verts(f, l)[0]
                    for a in range(4):
                        wF[hv[a]] += ev["gB"][h, a]
                        for b in range(4):
                            want[hv[a], :, hv[b], :] += ev["G"][h, a, :, b, :]
                            yard[hv[a], hv[b]] = max(yard[hv[a], hv[b]], np.linalg.norm(ev["G"][h, a, :, b, :]))
                want = want.reshape(3 * c.NV, 3 * c.NV)
                want[np.arange(3 * c.NV), np.arange(3 * c.NV)] += mdt2
                err = np.sqrt(((got_H - want).reshape(c.NV, 3, c.NV, 3) ** 2).sum(axis=(1, 3)))
                nrm = np.maximum(np.sqrt((want.reshape(c.NV, 3, c.NV, 3) ** 2).sum(axis=(1, 3))), yard)
                assert not err[nrm == 0].any()
                assert (err[nrm > 0] / nrm[nrm > 0]).max() <= 1e-12, (name, spd, (err[nrm > 0] / nrm[nrm > 0]).max())
                gy = yard.max(axis=1) * dx
                assert (np.linalg.norm(got_F - wF, axis=1) / np.maximum(np.linalg.norm(wF, axis=1), gy)).max() <= 1e-12, (name, spd)
            E = ev["eS"].sum() + ev["eA"].sum() + ev["eB"].sum()
            assert abs(o.compute_energy() - E) <= 1e-12 * abs(E), name
    finally:
        oracle.set_spd_mode(0)
