"""Generates tests/golden/handle_paths_{dense,sparse,vertex}.npz ON THE GPU:  python tests/golden/gen_handle_paths.py [out_dir]

What the library computed for soft handles while a vertex list and a face list still ran through kernels of their own (the commit before the corner
lists of csrc/k_handle.hpp): recorded once there, replayed by tests/test_gpu_handle_paths.py.  A face list is held to these bits; a vertex list to
1e-14 of the largest entry per quantity.
Only the public Python surface is used, so the script runs unchanged before and after.

Cases, all on the gravity-free perturbed drape cloth of the handle tests, frozen dofs on a handled vertex each (all three / one / two):
    dense   N = 12, 864 face handles (three per face, shuffled), 3 frames: 260 handles (a second pass of the 256-lane stride), 9, none; the rest free
    sparse  N = 12, the seven face handles of tests/test_gpu_surface_handles.py, no frames
    vertex  N = 16, 270 vertex handles in shuffled order, random weights, one weight 0 (two energy workgroups, the second with a partial wave), the
            frame layout of `dense`
Per case: energy, gradient and matrix (CSR values) at spd 0, 1, 2; handle_points, handle_force, handle_grad(p); the k_handle key; frame_wrench and
frame_grad(p); for the face lists the positions after 3 time steps with direct = 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

K = 2.0e5
CASES = ("dense", "sparse", "vertex")


def _sparse_lists(tab):
    """the seven handles of tests/test_gpu_surface_handles.py"""
    f1 = 120
    f2 = next(f for f in range(len(tab)) if f != f1 and tab[f1][0] in tab[f] and len(set(tab[f]) & set(tab[f1])) == 1)
    f = np.array([100, 50, 7, 200, 200, f1, f2], np.int32)
    b = np.array([[0.2, 0.5, 0.3], [0.0, 0.4, 0.6], [1.0, 0.0, 0.0], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8], [0.5, 0.25, 0.25], [0.3, 0.3, 0.4]])
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 0.75, 1.25])
    return f, b, w


def _frozen(NV, v0, v1, v2):
    assert len({int(v0), int(v1), int(v2)}) == 3
    fz = np.zeros((NV, 3), np.int32)
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


def build(name):
    """(scene, x, frozen): the scene with its handles, targets, frames and poses in place; x the perturbed state, frozen (NV, 3)"""
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    N = 16 if name == "vertex" else 12
    s = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, Kb=100.0, pin_row=False, perturb=0.0, newton_cap=200)
    s.init_all()
    s._ensure_ctx().set_gravity(np.zeros((s.tot_NV, 3)))
    rng = np.random.default_rng({"dense": 31, "sparse": 32, "vertex": 35}[name])
    dx = s.cloths[0].dx
    NV = s.tot_NV
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * dx, size=(NV, 3))
    if name == "vertex":
        assert NV == 289
        v = rng.permutation(NV)[:270].astype(np.int32)
        w = rng.uniform(0.25, 2.0, len(v))
        w[17] = 0.0
        pts = x[v]
        s.set_handles(v, K, w)
        fz = _frozen(NV, v[0], v[1], v[2])
    else:
        tab = s.faces.to_numpy()
        assert tab.shape == (288, 3) and NV == 169
        if name == "dense":
            f = rng.permutation(np.repeat(np.arange(288), 3)).astype(np.int32)
            b = rng.dirichlet(np.ones(3), len(f))
            w = rng.uniform(0.25, 2.0, len(f))
        else:
            f, b, w = _sparse_lists(tab)
        fv = tab[f]
        pts = (b[:, 0:1] * x[fv[:, 0]] + b[:, 1:2] * x[fv[:, 1]]) + b[:, 2:3] * x[fv[:, 2]]
        s.set_surface_handles(f, b, K, w)
        fz = _frozen(NV, fv[2, 0], fv[0, 1], fv[1, 2])
    n = len(w)
    s.set_handle_targets(pts + rng.normal(scale=0.5 * dx, size=(n, 3)))
    if name != "sparse":
        # grasped where the rest state has them, then the frames moved a little: the framed targets stay within reach of the cloth
        frame_of = -np.ones(n, np.int32)
        pick = rng.permutation(n)
        frame_of[pick[:260]] = 0
        frame_of[pick[260:269]] = 1
        s.set_handle_frames(frame_of, n_frames=3)
        s.set_frame_poses(rng.normal(scale=0.3 * dx, size=(3, 3)), np.array([1.0, 0.0, 0.0, 0.0]) + rng.normal(scale=0.02, size=(3, 4)))
    return s, x, fz


def record(name):
    """{quantity: array} of the case as the library in place computes it"""
    import torch
    s, x, fz = build(name)
    ctx = s._ensure_ctx()
    ctx.set_frozen(fz.reshape(-1))

    def dev(a):
        return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    pos = dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    ref = s._ref_angle
    p = dev(np.random.default_rng(11).normal(size=3 * s.tot_NV))
    out = {"energy": np.array(ctx.energy(pos, prev, vel, ref))}
    for spd in (0, 1, 2):
        F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
        ctx.assemble(pos, prev, vel, ref, spd=spd, grad=F)
        out["gradient_spd%d" % spd] = F.cpu().numpy()
        out["matrix_spd%d" % spd] = ctx.matrix_csr().data.copy()
    out["handle_points"] = ctx.handle_points(pos)
    out["handle_force"] = ctx.handle_force(pos)
    out["handle_grad"] = ctx.handle_grad(p)
    out["k_handle"] = np.array(ctx.param_grads(pos, ref, ["k_handle"], p=p)["k_handle"])
    out["frame_wrench"] = ctx.frame_wrench(pos)
    out["frame_grad"] = ctx.frame_grad(p)
    if name != "vertex":
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.fill(0.0)
        ctx.set_param("direct", 1)
        iters = [s.time_step(None, f)["newton_iters"] for f in (1, 2, 3)]
        out["newton_iters"] = np.array(iters)
        out["pos_after_3_steps"] = s.pos.to_numpy().copy()
    s._close_ctx()
    return out


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out_dir, exist_ok=True)
    for name in CASES:
        r = record(name)
        path = os.path.join(out_dir, "handle_paths_%s.npz" % name)
        np.savez_compressed(path, **r)
        print(name, {k: (v.shape, float(np.abs(v).max()) if v.size else 0.0) for k, v in r.items()}, os.path.getsize(path), "bytes", flush=True)
