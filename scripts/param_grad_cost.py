"""Cost of tsl_param_grad_keys with every supported key against one tsl_adjoint_step on cfg3 (Scene_folding topology, 200 x 100 cloth,
40,000 triangles; bench.py's workload and drive).  Both are bracketed by hipEvent pairs (torch.cuda.Event) on the engine's stream; the
parameter call includes its read-back and synchronisation.  Usage: python scripts/param_grad_cost.py [--steps K] [--reps R]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import bench
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    from thinshelllab_amd.engine.geometry import projection_query
    args = argparse.Namespace(workload="cfg3", grid=200, idle=0)
    s = bench.build_scene(args, 0)
    K = a.steps
    g = Grad(s, K + 1, s.gripper.n_part); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, K + 1):
        s._bench_frame = f
        s.action(f, *bench._drive(s.gripper.n_part, s._bench_gs, 0, f, 0))
        s.time_step(projection_query, f)
        g.copy_pos(s, f)
    g.get_loss_slide(s)
    ctx = s._ensure_ctx()
    keys = [f"cloth{i}.{k}" for i in range(len(s.cloths)) for k in ("Kl", "Ka", "Kb")]
    keys += [f"elastic{i}.{k}" for i in range(len(s.elastics)) for k in ("mu", "lam")]
    keys += ["k_contact", "mu_cloth_elastic"]
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    adj_ms, pg_ms = [], []
    ctx.set_param("adj_clamp", 1.0); ctx.set_param("adj_clamp_angleref", 0.0)
    for st in range(K, 0, -1):
        e0, e1 = ev(), ev()
        e0.record()
        ctx.adjoint_step(st, K + 1, g.pos_buffer.t, g.pos_grad.t, g.ref_angle_buffer.t, g.angleref_grad.t, s.tmp_z_frozen.t, 1.0)
        e1.record(); torch.cuda.synchronize()
        adj_ms.append(e0.elapsed_time(e1))
        pos, ref = g.pos_buffer.t[st], g.ref_angle_buffer.t[st - 1]
        ctx.param_grads(pos, ref, keys)   # (first call of a step: allocations)
        for _ in range(a.reps):
            e0, e1 = ev(), ev()
            e0.record()
            ctx.param_grads(pos, ref, keys)
            e1.record(); torch.cuda.synchronize()
            pg_ms.append(e0.elapsed_time(e1))
        s.copy_pos_and_refangle(g, st)
    pg_ms.sort(); adj_ms.sort()
    pg = pg_ms[len(pg_ms) // 2]; adj = adj_ms[len(adj_ms) // 2]
    print(json.dumps(dict(workload="cfg3", triangles=sum(c.NF for c in s.cloths), keys=len(keys), nc=ctx.contact_counts(),
                          adjoint_step_ms_median=adj, adjoint_step_ms=adj_ms, param_grad_keys_ms_median=pg, param_grad_keys_ms_min=pg_ms[0],
                          ratio=pg / adj)))


if __name__ == "__main__":
    main()
