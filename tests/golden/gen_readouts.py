"""Generates tests/golden/readouts_{drape,balancing}.npz ON THE GPU:  python tests/golden/gen_readouts.py [out_dir]

What the library computed for the energy, the read-outs of system identification and the reverse step while their kernels and entry points still
sat in csrc/tsl_hip.hip (the commit before k_scene.hpp, k_adjoint.hpp, adjoint_api.hpp and param_api.hpp): recorded once there, replayed bit for
bit by tests/test_gpu_readouts.py.  Only the public Python surface is used, so the script runs unchanged before and after.

Cases, the scenes of tests/test_gpu_param_grad.py's _task_scene:
    drape      12 x 12 cloth, 288 faces: two workgroups of the 256-lane face pass, so the offsets of the per-key partials are exercised
               (stepped and reversed through the sparse direct solve, whose bits repeat)
    balancing  cloth on a tactile body, live vertex-triangle contacts
Per case: the energy, the gradient of assemble at spd 0 and elastic_force at the scene's state; param_grads with a seeded p for every supported
key at once (shuffled), one key alone and a list of 33 keys with repeats (two launches of the final sum); then a tape of two more time steps and
two reverse steps from a seeded pos_grad: pos_grad, angleref_grad, and per reverse step tmp_z_frozen, param_grad, friction_grad and param_grads
with p = the step's adjoint solution."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("drape", "balancing")
T = 3


def supported_keys(s):
    """every key tsl_param_grad_keys differentiates on this scene (the StVK, handle and contact keys read exact zeros where the scene has none)"""
    keys = []
    for i in range(len(s.cloths)):
        keys += [f"cloth{i}.{f}" for f in ("Kl", "Ka", "Kb", "stvk_mu", "stvk_lam")]
    for i in range(len(s.elastics)):
        keys += [f"elastic{i}.{f}" for f in ("mu", "lam")]
    return keys + ["k_contact", "mu_cloth_elastic", "mu_cloth_cloth", "k_handle"]


def build(name):
    """the scene of the case at the state the read-outs are taken at"""
    if name == "drape":
        # _task_scene's drape with every solve on the sparse direct path: the iterative hierarchy a contact-free cloth takes by default does
        # not repeat its bits from one process to the next, and neither would anything recorded behind it
        from thinshelllab_amd.task_scene.Scene_drape import Scene
        s = Scene(cloth_size=0.1 / 15 * 12, N=12, M=12, Kb=100.0, k_angle=3.14, perturb=2e-3)
        s.init_all()
        s._ensure_ctx().set_param("direct", 1)
        for f in range(1, 3):
            s.time_step(None, f)
        return s
    from test_gpu_param_grad import _task_scene
    return _task_scene(name)


def record(name):
    """{quantity: array} of the case as the library in place computes it"""
    import torch
    from thinshelllab_amd.engine.geometry import projection_query
    s = build(name)
    ctx = s._ensure_ctx()
    contact = bool(s.elastics)
    fc = projection_query if contact else None
    pos, prev, vel, ref = s._state()
    NV = s.tot_NV
    out = {}

    def vec(d, keys):
        return np.array([d[k] for k in keys])

    # ---- the state after _task_scene's steps
    if contact:
        ctx.contact_detect(prev, prev)
        out["contact_counts"] = np.array(ctx.contact_counts())
    out["energy"] = np.array(ctx.energy(pos, prev, vel, ref))
    F = torch.zeros(pos.numel(), dtype=torch.float64, device=pos.device)
    ctx.assemble(pos, prev, vel, ref, spd=0, grad=F)
    out["gradient_spd0"] = F.cpu().numpy()
    out["elastic_force"] = ctx.elastic_force(pos, torch.full((NV, 3), 7.0, dtype=torch.float64, device=pos.device)).cpu().numpy()
    keys = supported_keys(s)
    shuffled = keys[:]
    random.Random(5).shuffle(shuffled)
    rng = np.random.default_rng(23)
    p = torch.tensor(rng.normal(size=3 * NV), device=pos.device)
    long = [keys[i] for i in rng.integers(0, len(keys), 33)]
    out["keys_all"] = vec(ctx.param_grads(pos, ref, shuffled, p=p), keys)
    out["keys_one"] = np.array(ctx.param_grads(pos, ref, [keys[2]], p=p)[keys[2]])
    out["keys_33"] = vec(ctx.param_grads(pos, ref, long, p=p), sorted(set(long)))      # (a dict: repeated keys collapse, all 33 are computed)
    # ---- a tape of T states and T - 1 reverse steps
    pb = torch.zeros((T, NV, 3), dtype=torch.float64, device=pos.device)
    rb = torch.zeros((T,) + tuple(ref.shape), dtype=torch.float64, device=pos.device)
    pb[0] = s.pos.t; rb[0] = s._ref_angle
    for f in range(1, T):
        s.time_step(fc, f)
        pb[f] = s.pos.t; rb[f] = s._ref_angle
    pg = torch.zeros_like(pb)
    pg[T - 1] = torch.tensor(rng.normal(scale=1e-2, size=(NV, 3)), device=pos.device)
    ag = torch.zeros_like(rb)
    tz = torch.zeros(3 * NV, dtype=torch.float64, device=pos.device)
    ctx.set_param("contact", 1.0 if contact else 0.0)
    for st in range(T - 1, 0, -1):
        ctx.adjoint_step(st, T, pb, pg, rb, ag, tz, 1.0)
        out["tmp_z_frozen_%d" % st] = tz.cpu().numpy()
        pg_ = ctx.param_grad(pb[st], rb[st - 1])
        out["param_grad_%d" % st] = np.array([pg_["kb"], pg_["mu"], pg_["lam"]])
        out["friction_grad_%d" % st] = np.array(ctx.friction_grad(pb[st]))
        out["keys_all_%d" % st] = vec(ctx.param_grads(pb[st], rb[st - 1], shuffled), keys)
        out["keys_33_%d" % st] = vec(ctx.param_grads(pb[st], rb[st - 1], long), sorted(set(long)))
    out["pos_grad"] = pg.cpu().numpy()
    out["angleref_grad"] = ag.cpu().numpy()
    s._close_ctx()
    return out


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out_dir, exist_ok=True)
    for name in CASES:
        r = record(name)
        path = os.path.join(out_dir, "readouts_%s.npz" % name)
        np.savez_compressed(path, **r)
        print(name, {k: (v.shape, float(np.abs(v).max()) if v.size else 0.0) for k, v in r.items()}, os.path.getsize(path), "bytes", flush=True)
