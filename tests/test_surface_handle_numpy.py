"""Soft handles at barycentric points of faces on the CPU: the NumPy restatement (tests/surface_handle_numpy.py) against differences
of its own energy, the host checks of BaseScene.set_surface_handles, Cloth.locate, the tape's buffers for a face list, and the host module
csrc/handle_host.hpp compiled into a stand-alone program under AddressSanitizer and UBSan (tests/native/handle_ref.cpp), its gather lists -- of
a face list and of a vertex list -- compared with a NumPy construction of the same rule."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_handle_numpy as sn  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _random_case(seed=0, NV=11, NF=14, n=9):
    rng = np.random.default_rng(seed)
    tab = np.array([rng.choice(NV, 3, replace=False) for _ in range(NF)])
    f = rng.integers(0, NF, n)
    f[1] = f[0]                                   # two handles on one face
    b = rng.dirichlet(np.ones(3), n)
    b[2] = [1.0, 0.0, 0.0]; b[3] = [0.0, 0.4, 0.6]
    w = rng.uniform(0.25, 2.0, n); w[4] = 0.0
    x = rng.normal(size=(NV, 3))
    t = rng.normal(size=(n, 3))
    fz = np.zeros((NV, 3), np.int32)
    fv = tab[f]
    fz[fv[0, 0]] = 1; fz[fv[3, 1], 1] = 1; fz[fv[5, 2], 0] = 1; fz[fv[5, 2], 2] = 1
    return x, fv, b, w, t, fz


@pytest.mark.parametrize("frozen", [False, True])
def test_restatement_equals_differences_of_its_own_energy(frozen):
    x, fv, b, w, t, fz = _random_case()
    fz = fz if frozen else None
    k, h = 3.7, 1e-5
    free = sn._free(fz, len(x))
    g = sn.gradient(x, fv, b, w, t, k, fz)
    H = sn.matrix(len(x), fv, b, w, k, fz)
    fd = np.zeros_like(x)
    for v in range(len(x)):
        for c in range(3):
            xp = x.copy(); xp[v, c] += h
            xm = x.copy(); xm[v, c] -= h
            fd[v, c] = (sn.energy(xp, fv, b, w, t, k) - sn.energy(xm, fv, b, w, t, k)) / (2 * h)
    assert np.abs(g - fd * free).max() <= 1e-9 * np.abs(fd).max()    # (the energy is quadratic: central differences are exact up to rounding / h)
    Hfd = np.zeros_like(H)
    for v in range(len(x)):
        for c in range(3):
            xp = x.copy(); xp[v, c] += h
            xm = x.copy(); xm[v, c] -= h
            Hfd[:, 3 * v + c] = ((sn.gradient(xp, fv, b, w, t, k, fz) - sn.gradient(xm, fv, b, w, t, k, fz)) / (2 * h)).ravel()
    Hfd *= free.ravel()[None, :]
    assert np.abs(H - Hfd).max() <= 1e-9 * np.abs(H).max()
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() >= -1e-12 * np.abs(H).max()
    assert (H[~sn.touched(len(x), fv)] == 0).all()
    # target and stiffness derivatives against differences of the masked gradient
    p = np.random.default_rng(1).normal(size=x.size)
    tg = sn.target_grad(p, fv, b, w, k, fz)
    for i in range(len(t)):
        for c in range(3):
            tp = t.copy(); tp[i, c] += h
            tm = t.copy(); tm[i, c] -= h
            d = -float(p @ ((sn.gradient(x, fv, b, w, tp, k, fz) - sn.gradient(x, fv, b, w, tm, k, fz)) / (2 * h)).ravel())
            assert abs(tg[i, c] - d) <= 1e-9 * np.abs(tg).max()
    dk = -float(p @ ((sn.gradient(x, fv, b, w, t, k + h, fz) - sn.gradient(x, fv, b, w, t, k - h, fz)) / (2 * h)).ravel())
    assert abs(sn.k_deriv(x, p, fv, b, w, t, fz) - dk) <= 1e-9 * abs(dk)
    f = sn.force(x, fv, b, w, t, k)
    assert np.allclose(f, -k * w[:, None] * (sn.points(x, fv, b) - t), rtol=0, atol=0)


def test_validate_surface_handles_names_the_offender():
    from thinshelllab_amd.engine.BaseScene import validate_surface_handles as val
    ok_b = [[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]]
    f, b, w = val(10, [3, 9], ok_b, [1.0, 0.0])
    assert f.dtype == np.int32 and b.dtype == np.float64 and b.shape == (2, 3) and np.array_equal(f, [3, 9]) and np.array_equal(w, [1.0, 0.0])
    assert val(10, [3, 3, 3], [ok_b[0]] * 3)[2] is None          # any number of handles on a face
    f0, b0, _ = val(10, np.zeros(0, np.int32), np.zeros((0, 3)))
    assert f0.shape == (0,) and b0.shape == (0, 3)
    with pytest.raises(ValueError, match=r"face 10 of handle 1 out of range \[0, 10\)"):
        val(10, [3, 10], ok_b)
    with pytest.raises(ValueError, match=r"face -1 of handle 0 out of range"):
        val(10, [-1, 3], ok_b)
    for bad, txt in ((-0.1, "-0.1"), (np.nan, "nan"), (1.2, "1.2")):
        with pytest.raises(ValueError, match=rf"barycentric coordinate {txt} of handle 1 \(face 4\) is not finite or outside \[0, 1\]"):
            val(10, [3, 4], [ok_b[0], [bad, 0.5, 0.5]])
    with pytest.raises(ValueError, match=r"barycentric coordinates \(0.3, 0.3, 0.3\) of handle 0 \(face 3\) sum to 0.9, not 1"):
        val(10, [3], [[0.3, 0.3, 0.3]])
    with pytest.raises(ValueError, match=r"weight -1 of handle 1 \(face 4\) is negative or not finite"):
        val(10, [3, 4], ok_b, [1.0, -1.0])
    with pytest.raises(ValueError, match="shape"):
        val(10, [3, 4], [0.2, 0.3, 0.5])
    with pytest.raises(ValueError, match="flat list of integers"):
        val(10, [[3, 4]], ok_b)
    with pytest.raises(ValueError, match="1 weights for 2 handles"):
        val(10, [3, 4], ok_b, [1.0])
    assert val(10, [3], [[0.2, 0.3, 0.5 + 5e-10]])[1][0, 2] == 0.5 + 5e-10   # (within 1e-9 of 1: taken as given, not renormalised)


def _cloth(N, M, offset=0, offset_faces=0):
    from thinshelllab_amd.engine.model_fold_offset import Cloth
    c = Cloth(N, 5e-3, 0.01 * N, 0, 40.0, offset, False, M)
    c.init(0.02, -0.01, 0.3)
    c.offset_faces = offset_faces
    return c


def test_cloth_locate_on_a_5_by_7_grid():
    c = _cloth(5, 7, offset=11, offset_faces=4)
    X = c.pos.to_numpy()
    F = c.f2v.to_numpy()
    x00 = X[0]
    L = np.array([5 * c.dx, 7 * c.dx, 0.0])

    def point(u, v):
        f, b = c.locate(u, v)
        assert 4 <= f < 4 + c.NF and b.shape == (3,) and (b >= 0).all() and (b <= 1).all() and abs(b.sum() - 1) <= 1e-15, (u, v, f, b)
        return f, b, b @ X[F[f - 4]]

    # a grid of interior points reproduces the rest positions
    for u in np.linspace(0.03, 0.97, 23):
        for v in np.linspace(0.02, 0.99, 19):
            _, _, p = point(u, v)
            assert np.abs(p - (x00 + L * [u, v, 0.0])).max() <= 1e-15, (u, v)
    # the four corners: one coordinate 1 on the corner vertex, two zeros
    for (u, v), vid in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (0, 7, 5 * 8, 5 * 8 + 7)):
        f, b, p = point(u, v)
        assert sorted(b.tolist()) == [0.0, 0.0, 1.0] and F[f - 4][int(np.argmax(b))] == vid and np.array_equal(p, X[vid])
    # points on interior grid lines and on the cells' diagonals: one zero coordinate, on the corner opposite the edge
    for u, v in ((0.4, 0.5 / 7), (1.5 / 5, 3.0 / 7), (0.6, 6.25 / 7), (0.5 / 5, 0.5 / 7), (1.5 / 5, 0.5 / 7), (1.0, 0.5), (0.5, 1.0)):
        f, b, p = point(u, v)
        assert (b == 0).sum() == 1 or np.abs(b).min() <= 1e-15, (u, v, b)
        assert np.abs(p - (x00 + L * [u, v, 0.0])).max() <= 1e-15
    # an interior grid vertex: a valid face with two zeros
    f, b, p = point(2 / 5, 3 / 7)
    assert np.abs(np.sort(b) - [0, 0, 1]).max() <= 1e-15 and np.abs(p - X[2 * 8 + 3]).max() <= 1e-15
    with pytest.raises(ValueError, match="outside"):
        c.locate(1.01, 0.5)


def test_the_tape_has_handle_buffers_of_n_rows_for_a_face_list():
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.analytic_grad_system import Grad as GradSys
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=0.04, N=6, M=6, device="cpu")
    s.init_all()
    c = s.cloths[0]
    loc = [c.locate(u, v) for u, v in ((0.93, 0.07), (0.93, 0.07), (0.5, 0.5), (1.0, 1.0), (0.21, 0.77))]
    s.set_surface_handles([f for f, _ in loc], [b for _, b in loc], 2000.0, weights=[1, 2, 1, 0.5, 1])
    assert s.n_handle == 5 and s._handle_t.shape == (5, 3)
    p = s.handle_points()
    X = s.pos.to_numpy()
    assert np.abs(p[0, :2] - (X[0, :2] + [0.93 * 0.04, 0.07 * 0.04])).max() <= 1e-15 and np.array_equal(p[3], X[-1])   # (the drape's z is perturbed)
    s.set_handle_targets(p + 1e-3)
    s.set_handle_frames([0, 0, -1, 1, 1])           # grasp where they are: the targets of the framed rows stay the points
    assert s.n_frame == 2 and np.abs(s._handle_t[[0, 1, 3, 4]] - p[[0, 1, 3, 4]]).max() <= 1e-15 and np.array_equal(s._handle_t[2], p[2] + 1e-3)
    for G in (Grad, GradSys):
        g = G(s, 4, 0)
        assert tuple(g.handle_targets.t.shape) == (4, 5, 3) and tuple(g.handle_grad.t.shape) == (4, 5, 3)
        assert tuple(g.frame_pos.t.shape) == (4, 2, 3) and tuple(g.frame_grad.t.shape) == (4, 2, 6)
    # each setter replaces the other's list and drops the frames
    s.set_handles(c.corner_ids(), 100.0)
    assert s.n_handle == 4 and s._handle_f is None and s.n_frame == 0 and np.array_equal(s.handle_points(), X[c.corner_ids()])
    s.set_surface_handles([3], [[0.2, 0.3, 0.5]], 10.0)
    assert s.n_handle == 1 and len(s._handle_v) == 0
    s.set_surface_handles([], np.zeros((0, 3)), 0.0)
    assert s.n_handle == 0
    with pytest.raises(ValueError, match=r"face 72 of handle 0 out of range \[0, 72\)"):
        s.set_surface_handles([72], [[0.2, 0.3, 0.5]], 10.0)


def _ints(line):
    return np.array(line.split(":", 1)[1].split(), np.int64)


def test_host_module_under_sanitizers_builds_the_lists_of_the_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "handle_ref")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(HERE, "native", "handle_ref.cpp"), "-o", exe]
    # the sanitizers' runtimes inside the program where the tool chain has them as archives (the program then does not depend on the order in which
    # shared libraries are loaded into it); as shared libraries otherwise
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    got = {ln.split(":", 1)[0]: _ints(ln) for ln in lines if ":" in ln and not ln.startswith("refused")}
    NV = int(got["NV"][0])
    tab = got["faces"].reshape(-1, 3)
    address = sn.block_addresses(NV, tab)
    want = sn.gather_lists(NV, tab, got["handle_faces"], address)
    for k, v in want.items():
        assert np.array_equal(got[k], np.asarray(v, np.int64)), k
    # the vertex list: one corner per handle -- one entry per handled vertex and per diagonal block, at the pattern's diagonal address
    hv = got["handle_verts"]
    assert len(set(hv.tolist())) == len(hv) and (np.diff(hv) < 0).any() and hv.min() == 0 and hv.max() == NV - 1 and (hv < 64).any() and (hv >= 64).any()
    for k, v in sn.corner_lists(hv.reshape(-1, 1), address).items():
        assert np.array_equal(got["v_" + k], np.asarray(v, np.int64)), k
    order = np.argsort(hv)
    assert np.array_equal(got["v_vl_v"], hv[order]) and np.array_equal(got["v_vl_ent"], order) and np.array_equal(got["v_bl_ent"], order)
    assert np.array_equal(got["v_vl_ptr"], np.arange(len(hv) + 1)) and np.array_equal(got["v_bl_ptr"], np.arange(len(hv) + 1))
    assert np.array_equal(got["diag"], [address[(v, v)] for v in range(NV)]) and np.array_equal(got["v_bl_addr"], got["diag"][hv[order]])
    # properties the kernels rely on: every list is in range, every corner and every pair appears exactly once, the transposed block holds the same handles
    n = len(got["handle_faces"])
    assert sorted(got["vl_ent"].tolist()) == list(range(3 * n)) and sorted(got["bl_ent"].tolist()) == list(range(9 * n))
    assert (np.diff(got["vl_v"]) > 0).all() and got["vl_ptr"][0] == 0 and got["vl_ptr"][-1] == 3 * n and got["bl_ptr"][-1] == 9 * n
    assert len(set(got["bl_addr"].tolist())) == len(got["bl_addr"])
    assert max(len(range(a, b)) for a, b in zip(got["vl_ptr"][:-1], got["vl_ptr"][1:])) >= 4       # (face 17 carries three handles, one more meets it in a vertex)
    refused = [ln[len("refused: "):] for ln in lines if ln.startswith("refused")]
    expect = [r"face 144 of handle 2 out of range \[0, 144\)", r"face -1 of handle 2 out of range \[0, 144\)",
              r"barycentric coordinate -0.1 of handle 2 \(face 5\) is not finite or outside \[0, 1\]",
              r"barycentric coordinate nan of handle 2 \(face 5\) is not finite or outside \[0, 1\]",
              r"barycentric coordinate 1.2 of handle 2 \(face 5\) is not finite or outside \[0, 1\]",
              r"barycentric coordinates \(0.3, 0.3, 0.3\) of handle 2 \(face 5\) sum to 0.9, not 1",
              r"weight -1 of handle 2 \(face 5\) is negative or not finite", r"weight inf of handle 2 \(face 5\) is negative or not finite",
              r"vertices 2 and 89 of face 5 \(handle 1\) have no block in the matrix pattern",
              r"vertex 7 has more than one handle", r"vertex 90 out of range \[0, 90\)", r"weight -1 of vertex 3 is negative or not finite"]
    import re
    assert len(refused) == len(expect), refused
    for msg, pat in zip(refused, expect):
        assert re.fullmatch(pat, msg), (msg, pat)
