#!/usr/bin/env python
"""Headline benchmark: element-steps/s (fwd+adjoint) of the implicit thin-shell step on MI355X.

    python bench.py --gpus N --steps K --warmup W      (N > 1: re-executes itself under torch.distributed.run, one rank per GPU;
                                                        under an external launcher the ranks are taken from the environment)

Default workload = BASELINE.json configs[3] ("cfg4": cloth on ball + 4 tactile pads, 100k triangles, contact), the
configuration the metric is quoted on; --workload drape runs the contact-free pinned cloth of the same size.
One "step" = one implicit-Euler time step of the workload scene (gripper drive, contact detection, Newton loop with one sparse
factorisation + refined solve per iteration and the halving line search, velocity / plastic update: BaseScene.time_step) PLUS its
reverse-mode adjoint step (Grad.transfer_grad: contact re-detection, un-projected Hessian, one linear solve, back-propagation
kernels).  The timed region runs K forward steps onto the tape and then the K adjoint steps of the same rollout, all state
resident in HBM.  value = cloth triangles x K x n_gpus / wall seconds (max over ranks).  Ranks run independent scene rollouts
(trajectory-optimisation batch): no data-path collective, "scaling": "weak".
--dump-outputs DIR writes what the timed rollout computed (dump_outputs) as .npy files; the inputs depend on the arguments only, so
two builds run with the same arguments can be compared output for output.

A plain run sets up, warms up, times the K steps, dumps if asked and prints the line: the headline keys and `config` (the timed rollout's
own convergence accounting).  With --full the line also carries the legs that take runs of their own:
  roofline      -- the kernel class of the sparse direct solve that takes the most time per Newton iteration (named in the object):
                   algorithmic flops (or bytes) per launch / average launch duration between one HIP-event pair around back-to-back
                   replays of that class's launches on the run's last plan, against the f64 matrix-core peak (or 8 TB/s);
                   roofline.whole_step = SURVEY.md section 8d's whole-step figures from the measured counts;
  cpu_baseline  -- the fp64 CPU restatement (oracle/, "port": the reference itself needs taichi + cupy/CUDA and cannot run) timed on
                   this box's host cores: complete fwd+adjoint steps of the same scene with a coarser cloth next to the GPU on that
                   scene, and the cfg4-size extrapolation of a bounded sample (labelled as such).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F64_MFMA_PEAK_TF = 78.6   # v_mfma_f64_16x16x4_f64: half the f32 MFMA rate the guide lists (157.3 TF) = the f64 vector rate (AMD MI355X datasheet: 78.6 TF)
F64_MFMA_SUSTAINED_TF = 65.0   # what a GEMM K loop (LDS operand reads + v_mfma_f64_16x16x4_f64, 2 x 2 tiles per wave) sustains on this part: scripts/micro/mfma_lds.hip,
                               # profiles/r03_mfma_f64_sustained_peak.txt (65 TFLOP/s with the reads inside the loop, 67-72 with the operands in registers)

GS_CFG4 = 224 * 0.004 / 0.06  # similarity factor that keeps the native 4 mm cloth spacing of Scene_balancing at 224x224


def build_scene(args, rank, grid=None, cloth_size=None):
    dev = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
    grid = grid or args.grid
    if args.workload == "drape":
        from thinshelllab_amd.task_scene.Scene_drape import Scene
        s = Scene(cloth_size=args.cloth_size, N=grid, M=grid, Kb=100.0, k_angle=3.14, perturb=1e-4 * (1 + 0.01 * rank), device=dev, newton_cap=50)
        s.init_all()
        return s
    if args.workload == "cfg3":
        # SURVEY.md section 8d cfg3 (BASELINE configs[2]): folding topology with a 200 x 100 cloth (40,000 triangles, cloth_size 0.1 m), frozen table +
        # one tactile pad, plastic hinges; the N = 1 point of the cfg5 batch (8 such scenes over 8 GPUs)
        from thinshelllab_amd.task_scene.Scene_folding import Scene
        s = Scene(cloth_size=0.1, cloth_N=grid, cloth_M=grid // 2, device=dev)
        s.cloths[0].Kb[None] = 400.0      # trajopt_folding.py:50
        s.init_all()
        s.mu_cloth_elastic[None] = 5.0    # trajopt_folding.py:66
        s.prev_pos.copy_from(s.pos)
        s._bench_gs = 0.0
        s._bench_rank = rank
        return s
    # cfg4: balancing topology, cloth N = M = 224 with cloth_size = 0.12 m (dx = 5.4e-4 m) on the ball and the
    # four tactile pads at their native poses.  cfg4-scaled: the same scene enlarged by one similarity factor so that the cloth keeps
    # the native 4 mm spacing (the mesh-dependent stiffness of the reference model makes the literal refinement ~4x more expensive).
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    if args.workload == "cfg4":
        gs = 1.0
        s = Scene(cloth_size=cloth_size or 0.12 * grid / 224, cloth_N=grid, cloth_M=grid, device=dev)
    else:
        gs = grid * 0.004 / 0.06
        s = Scene(cloth_size=grid * 0.004, cloth_N=grid, cloth_M=grid, geom_scale=gs, device=dev)
    s.init_all()
    s.mu_cloth_elastic[None] = 5.0  # trajopt_balancing.py:42
    s.prev_pos.copy_from(s.pos)
    s._bench_gs = gs
    s._bench_rank = rank
    return s


def _drive(n_part, gs, rank, frame=1, idle=0):
    """gripper drive of global time step `frame` (1-based, warm-up included).  cfg4: SURVEY section 8d's trajectory -- `idle` steps
    of zero trajectory (--idle, default 0: every timed step is an active one), then +-z 1e-4 m per step on the two paired grippers,
    opposite signs (the balancing task tilts the cloth).  cfg4-scaled: both grippers rise and tilt a little every step.  The rank
    only changes the amplitude by 1 %, so the ranks run different but equally expensive rollouts."""
    import numpy as np
    a = 1.0 + 0.01 * rank
    dpos = np.zeros((n_part, 3)); drot = np.zeros((n_part, 3))
    if frame <= idle:
        return dpos, drot
    if gs == 0.0:    # cfg3: the pad moves -z 2e-4 m per step for ten steps, then +x 2e-4 m per step
        if frame <= 10:
            dpos[:, 2] = -2e-4 * a
        else:
            dpos[:, 0] = 2e-4 * a
    elif gs == 1.0:
        dpos[:, 2] = 1e-4 * a * np.where(np.arange(n_part) % 2 == 0, 1.0, -1.0)
    else:
        dpos[:, 2] = 5e-5 * gs * a
        drot[:, 1] = 2e-3 * a
    return dpos, drot


def run_rollout(scene, grad, K, args):
    """K forward steps onto the tape, loss seed on the last state, K adjoint steps."""
    contact = None
    if args.workload != "drape":
        from thinshelllab_amd.engine.geometry import projection_query as contact
    S = dict(newton=0, it_fwd=0, ls=0, it_adj=0, nc=0, fwd_fallback=0, fwd_unconverged=0, fwd_attained=0, factorizations=0, plans=0, max_res_fwd=0.0,
             adj_fallback=0, adj_unconverged=0, adj_attained=0, max_res_adj=0.0, max_be_adj=0.0, last_delta=[], methods={})
    grad.allow_unconverged = True   # counted and reported below instead of raising in the middle of the timed region
    grad.copy_pos(scene, 0)
    for f in range(1, K + 1):
        if contact is not None:
            scene._bench_frame = getattr(scene, "_bench_frame", 0) + 1
            scene.action(f, *_drive(scene.gripper.n_part, scene._bench_gs, scene._bench_rank, scene._bench_frame, args.idle))
        st = scene.time_step(contact, f)
        grad.copy_pos(scene, f)
        S["newton"] += st["newton_iters"]; S["it_fwd"] += st["cg_iters"]; S["ls"] += st["ls_evals"]; S["nc"] += st.get("nc", 0)
        S["fwd_fallback"] += st["fallback"]; S["fwd_unconverged"] += st["unconverged"]; S["fwd_attained"] += st["attained"]
        S["factorizations"] += st["factorizations"]; S["plans"] += st["plans"]
        S["max_res_fwd"] = max(S["max_res_fwd"], st["max_rel_residual"]); S["last_delta"].append(st["last_delta"])
    c = scene.cloths[0]
    grad.pos_grad.t.zero_(); grad.angleref_grad.t.zero_()
    if args.workload == "cfg3":
        grad.get_loss_fold(scene, 1.0, -1.0, rows=scene.fold_rows())   # analytic_grad_single.py:280-294, fold rows scaled with the grid
    elif contact is not None:
        grad.get_loss_balance(scene)  # analytic_grad_single.py:428-443: ball over the cloth centre, seeds on every tape step
    else:
        grad.pos_grad.t[K, c.offset:c.offset + c.NV, 2] = 1.0  # dL/dx_K: lift the cloth (sum of z)
    for s in range(K, 0, -1):
        grad.transfer_grad(s, scene, contact)
        ls = grad.last_stats
        S["it_adj"] += ls["iters"]; S["adj_fallback"] += int(ls["flag"] == 1); S["adj_unconverged"] += int(ls["flag"] == 3); S["adj_attained"] += ls["attained"]
        S["max_res_adj"] = max(S["max_res_adj"], ls["rel_residual"]); S["max_be_adj"] = max(S["max_be_adj"], ls["backward_error"])
        S["methods"][ls["method"]] = S["methods"].get(ls["method"], 0) + 1
    return S


def run_group_rollout(scenes, grads, group, K, args):
    """run_rollout for the members of a scene group: the K forward steps of ALL members in lock step (SceneGroup.time_step: one merged
    factorisation and first application per Newton iteration), then every member's loss seed and the reverse sweep in lock step as well
    (SceneGroup.transfer_grad: one merged factorisation per adjoint step)"""
    from thinshelllab_amd.engine.geometry import projection_query as contact
    stats = [dict(newton=0, it_fwd=0, ls=0, it_adj=0, nc=0, fwd_fallback=0, fwd_unconverged=0, fwd_attained=0, factorizations=0, plans=0, max_res_fwd=0.0,
                  adj_fallback=0, adj_unconverged=0, adj_attained=0, max_res_adj=0.0, max_be_adj=0.0, last_delta=[], methods={}) for _ in scenes]
    for sc, g in zip(scenes, grads):
        g.allow_unconverged = True
        g.copy_pos(sc, 0)
    for f in range(1, K + 1):
        for sc in scenes:
            sc._bench_frame = getattr(sc, "_bench_frame", 0) + 1
            sc.action(f, *_drive(sc.gripper.n_part, sc._bench_gs, sc._bench_rank, sc._bench_frame, args.idle))
        sts = group.time_step(contact, f)
        for sc, g, st, S in zip(scenes, grads, sts, stats):
            g.copy_pos(sc, f)
            S["newton"] += st["newton_iters"]; S["it_fwd"] += st["cg_iters"]; S["ls"] += st["ls_evals"]; S["nc"] += st.get("nc", 0)
            S["fwd_fallback"] += st["fallback"]; S["fwd_unconverged"] += st["unconverged"]; S["fwd_attained"] += st["attained"]
            S["factorizations"] += st["factorizations"]; S["plans"] += st["plans"]
            S["max_res_fwd"] = max(S["max_res_fwd"], st["max_rel_residual"]); S["last_delta"].append(st["last_delta"])
    for sc, g in zip(scenes, grads):
        g.pos_grad.t.zero_(); g.angleref_grad.t.zero_()
        if args.workload == "cfg3":
            g.get_loss_fold(sc, 1.0, -1.0, rows=sc.fold_rows())
        else:
            g.get_loss_balance(sc)
    for k in range(K, 0, -1):
        group.transfer_grad(k, grads, contact)
        for g, S in zip(grads, stats):
            ls = g.last_stats
            S["it_adj"] += ls["iters"]; S["adj_fallback"] += int(ls["flag"] == 1); S["adj_unconverged"] += int(ls["flag"] == 3); S["adj_attained"] += ls["attained"]
            S["max_res_adj"] = max(S["max_res_adj"], ls["rel_residual"]); S["max_be_adj"] = max(S["max_be_adj"], ls["backward_error"])
    return stats


def multi_scene(args, rank, S, K, W, single_value):
    """--scenes-per-gpu S: S independent scenes of the bench workload on ONE GPU as a scene group (thinshelllab_amd/scene_group.py,
    csrc/direct_group.hpp): one host thread steps them in lock step, the sparse direct solves of all members are ONE factorisation and ONE
    first application of the merged plan per Newton iteration, everything else runs per member on its own streams.  Each member's tape is
    bit-identical to its single-scene run (tests/test_gpu_group.py).  One scene leaves most of the chip idle during the latency-bound
    parts of its factorisation (roofline.whole_step); this is what a trajectory-optimisation batch larger than the GPU count does with it
    (BASELINE configs[4]).  Reported NEXT to the single-scene headline, never instead."""
    import torch
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.scene_group import SceneGroup
    if args.workload == "drape":
        return {"scenes_per_gpu": S, "value": None, "error": "scene groups need the sparse direct solve (contact workloads)"}
    scenes, grads = [], []
    for k in range(S):
        sc = build_scene(args, rank * S + k)   # (own drive amplitude per scene, like the ranks)
        ctx = sc._ensure_ctx()
        ctx.set_param("cg_tol", args.cg_tol)
        ctx.set_param("direct", 1)
        for kv in args.param:
            key, v = kv.split("=")
            ctx.set_param(key, float(v))
        g = Grad(sc, max(K, W) + 1, sc.gripper.n_part); g.init_mass(sc)
        scenes.append(sc); grads.append(g)
    try:
        group = SceneGroup(scenes)
        if W > 0:
            run_group_rollout(scenes, grads, group, W, args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = run_group_rollout(scenes, grads, group, K, args)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        info = group.info()
    except Exception as e:   # noqa: BLE001 -- reported in the line
        return {"scenes_per_gpu": S, "value": None, "error": repr(e)}
    T = scenes[0].cloths[0].NF
    val = T * K * S / elapsed
    cnt = [sc._ensure_ctx().direct_counters() for sc in scenes]
    out = {"scenes_per_gpu": S, "value": val, "unit": "element-steps/s on this GPU, all scenes together", "seconds": elapsed,
           "ms_per_step_per_scene": elapsed / (K * S) * 1e3, "ms_per_lock_step": elapsed / K * 1e3, "speedup_vs_single_scene": val / single_value if single_value else None,
           "solves_unconverged": sum(st["fwd_unconverged"] + st["adj_unconverged"] for st in stats),
           "newton_iters_per_step": [st["newton"] / K for st in stats],
           "applications_per_fwd_solve": [st["it_fwd"] / max(st["newton"], 1) for st in stats],
           "dataflow_launches_lost": sum(int(c["flow_aborts"]) for c in cnt),
           "group": info,
           "note": "S scenes as ONE scene group on one host thread: forward steps in lock step (merged factorisation + first application per Newton iteration), "
                   "loss seeds and reverse sweeps per member; every member's tape equals its single-scene run bit for bit (tests/test_gpu_group.py)"}
    group.close()
    return out


def _berr_counters(ctx):
    cc = ctx.direct_counters()
    return {"accepted": cc["berr_accepted"], "evaluated": cc["berr_seen"], "max_backward_error": cc["berr_max"], "max_rel_residual": cc["berr_rel_max"],
            "rule": "normwise |b - Hx| / (|H|_inf |x| + |b|) <= 1e-12 and |b - Hx| <= 50 cg_tol |b| (direct_refine; counters since context creation, warm-up included)"}


def _ripple(x, c):
    """deterministic sub-micron ripple on the cloth rows: the native poses put cloth vertices EXACTLY on the contact threshold, where
    the activation test is decided by round-off (tests/test_gpu_scenes.py::_pair does the same on both sides)"""
    import numpy as np
    x[c.offset:c.offset + c.NV, 2] += 2e-6 * np.sin(0.7 * np.arange(c.NV) + 0.3)
    return x


def cpu_baseline(args, scene, gpu_stats, K, rank):
    """(a) Complete fwd+adjoint steps of the oracle on the host cores next to the GPU on the SAME scene and rollout (the bench scene
    with a coarser cloth, same bodies, poses, drive, loss; the direct path is active on the GPU side) -- and the two results
    COMPARED: `parity` = max |dx| of the tape, relative errors of pos_grad / gripper_grad, Newton counts of both sides.  A parity
    failure (> 1e-4) voids the baseline leg, never the GPU number.
    (b) The bench-size figure (`value`): ONE complete Newton iteration of the oracle on the bench scene and state (energy, assembly,
    the linear solve by scipy's SuperLU as the reference calls spsolve, line search), timed, times the Newton iterations + adjoint solves the GPU run needed,
    plus the timed contact detections: measured per iteration, scaled -- a full oracle rollout at 100k triangles takes hours."""
    import numpy as np
    import torch
    from oracle import pyoracle as po
    from oracle.mirror import oracle_from_scene, rel_err
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    ncpu = os.cpu_count() or 1
    threads = min(ncpu, args.cpu_threads)
    po.set_threads(threads)
    out = {"unit": "element-steps/s", "cores": threads, "kind": "port"}
    if args.workload in ("cfg4", "cfg4-scaled"):
        G, Kc = args.cpu_grid, args.cpu_steps
        cs = 0.12 if args.workload == "cfg4" else None

        def fresh():
            s_ = build_scene(args, rank, grid=G, cloth_size=cs)
            x = _ripple(s_.pos.to_numpy(), s_.cloths[0])
            s_.pos.from_numpy(x); s_.prev_pos.from_numpy(x)
            return s_
        small = fresh()
        o = oracle_from_scene(po, small, check_init=False)
        o.set_solver(args.cg_tol); o.set_direct(1)   # the reference's solver is a sparse direct solve (spsolve): scipy's SuperLU here
        n_part = small.gripper.n_part
        o.grad_new(Kc + 1, n_part)
        o.stats(reset=True)
        tc0 = time.time()
        o.grad_copy_pos(0)
        for f in range(1, Kc + 1):
            o.action(*_drive(n_part, small._bench_gs, rank, f))
            o.time_step()
            o.grad_copy_pos(f)
        newton_o = o.stats()["newton"]
        pg = o.arr("grad.pos_grad", (Kc + 1, -1, 3))
        e = small.elastics[0]; tt = small.cloths[0].offset + (G + 1) // 2 * (G + 1) + (G + 1) // 2
        pb = o.arr("grad.pos_buffer", (Kc + 1, -1, 3))
        d = 2 * (pb[1:, e.offset:e.offset + e.n_verts, 0:2] - pb[1:, tt:tt + 1, 0:2])   # get_loss_balance (analytic_grad_single.py:428-443)
        pg[1:, e.offset:e.offset + e.n_verts, 0:2] = d; pg[1:, tt, 0:2] = -d[:, -1, :]
        for s_ in range(Kc, 0, -1):
            o.grad_transfer(s_)
        t_cpu = time.time() - tc0
        ostats = o.stats()
        # the same rollout on the GPU
        g2 = Grad(small, Kc + 1, n_part); g2.init_mass(small)
        sm_args = argparse.Namespace(**vars(args))
        run_rollout(small, g2, Kc, sm_args)   # warm-up (plans, allocations)
        small2 = fresh()
        g3 = Grad(small2, Kc + 1, n_part); g3.init_mass(small2)
        torch.cuda.synchronize(); tg0 = time.time()
        S2 = run_rollout(small2, g3, Kc, sm_args)
        torch.cuda.synchronize(); t_gpu = time.time() - tg0
        Ts = 2 * G * G
        gg_o = o.arr("grad.gripper_grad", (Kc + 1, n_part, 6)); gg_g = g3.gripper_grad.to_numpy()[:Kc + 1, :n_part]
        par = {"max_abs_dx": float(np.abs(g3.pos_buffer.to_numpy()[:Kc + 1] - pb).max()),
               "pos_grad_rel": max(rel_err(g3.pos_grad.to_numpy()[k], pg[k]) for k in range(Kc + 1)),
               "gripper_grad_rel": rel_err(gg_g, gg_o), "newton_gpu": int(S2["newton"]), "newton_oracle": int(newton_o),
               "what": f"oracle vs the HIP engine (multifrontal-LU path) on the {G}x{G} rollout timed here: tape positions, pos_grad of every tape step, gripper_grad"}
        par["ok"] = bool(par["max_abs_dx"] < 1e-6 and par["pos_grad_rel"] < 1e-4 and par["gripper_grad_rel"] < 1e-4)
        out["parity"] = par
        out["complete_steps_small_scene"] = {
            "value": Ts * Kc / t_cpu, "gpu_value_same_scene": Ts * Kc / t_gpu, "cores": threads,
            "sample": f"complete fwd+adjoint steps: the bench scene with a {G}x{G} cloth ({Ts} triangles, cloth_size 0.12 m; same bodies, drive and loss), "
                      f"{Kc} steps forward + {Kc} adjoint steps of the oracle on {threads} OpenMP threads of {ncpu} host cpus in {t_cpu:.1f} s "
                      f"(Newton / line-search / solver statistics {ostats}); the GPU engine ran the same rollout in {t_gpu:.2f} s"}
        out["value"] = Ts * Kc / t_cpu; out["gpu_value_same_scene"] = Ts * Kc / t_gpu
        out["sample"] = out["complete_steps_small_scene"]["sample"]
        del small, small2
    # (b) the bench size: one complete Newton iteration of the oracle, timed, scaled with the GPU run's counts
    try:
        torch.cuda.synchronize()
        o = oracle_from_scene(po, scene, check_init=False)
        o.set_solver(args.cg_tol); o.set_direct(1)
        if args.workload != "drape":
            o.calc_vn(); o.projection_query(); o.contact_analysis()
        sweep = {}
        for th in sorted({min(ncpu, t) for t in (16, 64, ncpu)}):   # the OpenMP part (energy + assembly); SuperLU itself is single-threaded
            po.set_threads(th)
            o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(True)
            t0 = time.time(); o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(True); sweep[th] = time.time() - t0
        best = min(sweep, key=sweep.get)
        po.set_threads(best)
        t_contact = 0.0
        if args.workload != "drape":
            t0 = time.time(); o.calc_vn(); o.projection_query(); o.contact_analysis(); t_contact = time.time() - t0
        # SuperLU with scipy's default column ordering (COLAMD).  MMD on A^T + A -- the operator is structurally symmetric -- was measured once and is 12x
        # SLOWER on this operator (590 s against 49 s per iteration in the build container: profiles/r05_cpu_superlu_orderings.txt), so it is not timed here
        o.stats(reset=True); po.direct_seconds[:] = [0.0, 0]
        t0 = time.time()
        o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(True); o.newton_step()
        t_newton = time.time() - t0
        st = o.stats()
        order = "COLAMD"
        n_it = gpu_stats["newton"] + K     # every adjoint step = one assembly + one solve
        t_total = 2 * K * t_contact + n_it * t_newton
        T = scene.cloths[0].NF
        out["bench_size"] = {
            "value": T * K / t_total, "cores": best, "per_newton_iteration_s": t_newton, "contact_detection_s": t_contact,
            "sparse_lu_s": po.direct_seconds[0], "sparse_lu_rel_residual": (po.direct_residuals[-1] if po.direct_residuals else None),
            "sparse_lu_ordering": "COLAMD (scipy's default; MMD_AT_PLUS_A measured 12x slower on this operator: profiles/r05_cpu_superlu_orderings.txt)",
            "solve_flag": st["flag"], "line_search_evals": st["ls"],
            "assembly_s_by_threads": {str(k): v for k, v in sweep.items()},
            "what": f"measured per iteration, scaled: ONE complete Newton iteration of the oracle on the bench scene and state (energy + assembly on {best} OpenMP threads of "
                    f"{ncpu} host cpus, best of the thread sweep: {sweep[best]:.3f} s; the linear solve by scipy's SuperLU like the reference's spsolve, single-threaded, column ordering {order}: "
                    f"{po.direct_seconds[0]:.1f} s; {st['ls']} line-search evaluations) = {t_newton:.1f} s, times the {n_it} Newton iterations + adjoint solves of the GPU run's "
                    f"{K} steps, plus 2 x {K} contact detections of {t_contact:.3f} s"}
        out["value"] = out["bench_size"]["value"]; out["cores"] = best
        out["sample"] = out["bench_size"]["what"] + (" || " + out["complete_steps_small_scene"]["sample"] if "complete_steps_small_scene" in out else "")
    except Exception as e:  # keep (a)
        out["bench_size"] = {"value": None, "what": f"failed: {e!r}"}
    # complete oracle steps AT BENCH SIZE exist too, as a constant: the fixture generator of tests/test_gpu_fullsize_oracle.py stepped the oracle on the bench scene in the
    # BUILD CONTAINER (8 cpus; a complete step at the Newton cap takes ~30 min there, too long for this leg) and recorded its wall times
    try:
        fx = os.path.join(ROOT, "tests", "golden", "oracle_cfg4.npz")
        if args.workload == "cfg4" and args.grid == 224 and os.path.exists(fx):
            G = np.load(fx)
            secs, stf = G["seconds"], G["stats"]
            t_all = float(secs[:, 0].sum() + G["adjoint_seconds"][0])
            out["complete_steps_bench_size_build_container"] = {
                "value": float(G["triangles"]) * len(secs) / t_all, "unit": "element-steps/s", "cores": int(G["threads"]),
                "seconds_per_step": [float(x) for x in secs[:, 0]], "superlu_seconds_per_step": [float(x) for x in secs[:, 1]], "newton_per_step": [int(x) for x in stf[:, 1]],
                "contacts_per_step": [int(x) for x in stf[:, 0]], "reverse_step_seconds": float(G["adjoint_seconds"][0]),
                "what": f"MEASURED complete oracle steps at bench size ({len(secs)} forward steps from the initial state + the reverse step of the last), timed in the build container by "
                        "tests/golden/gen_oracle_fullsize.py when it wrote the parity fixture: a constant read from tests/golden/oracle_cfg4.npz, NOT timed on this box; the HIP engine "
                        "reproduces that rollout in tests/test_gpu_fullsize_oracle.py"}
    except Exception as e:   # noqa: BLE001
        out["complete_steps_bench_size_build_container"] = {"value": None, "what": f"failed: {e!r}"}
    if "parity" in out and not out["parity"]["ok"]:
        out["value"] = None
        out["sample"] = "PARITY FAILED (oracle vs HIP engine on the rollout timed for this baseline): " + json.dumps(out["parity"]) + " || " + out.get("sample", "")
    return out


def roofline(ctx, scene, elapsed, K, stats, args):
    """dominant kernel class of the sparse direct solve, measured live with HIP events (tsl_bench_direct), + section 8d's whole-step model"""
    names = {0: "k_ds_gj_step (+ k_ds_pivot0 / k_ds_gj_finish: blocked Gauss-Jordan inversion W = F11^-1 of every front of a batch, one launch per 32 pivots, f64 MFMA tiles)",
             3: "k_ds_inv_small (the same inversion of the leaf levels and small fronts: all block steps inside one launch, the pivot block in LDS)",
             5: "k_ds_gj_flow (the same inversion of the batches of the upper tree levels as ONE persistent launch per batch: a workgroup keeps a super-tile of 2 x 2 tiles in registers over all block steps, steps ordered by point-to-point flags; bytes = the pivot blocks read and written once)",
             1: "k_ds_gemm[schur] (Schur complement S = sum_children ext(S_child) - F21 G of every front of a batch: K = pp GEMM on v_mfma_f64_16x16x4_f64, the children's stored S gathered in the epilogue, S stored once -- no atomics, no cleared F22)",
             6: "k_ds_extend_panels (the panels F11 / F12 / F21 of every front of a level take their share of the children's Schur complements: the other half of the gather-form extend-add)",
             2: "k_ds_gemm[g] (G = W F12 of every front of a batch: K = pp GEMM on v_mfma_f64_16x16x4_f64)",
             4: "k_ds_gemv (level sweeps of one application of the factors: W, F21 upwards, G downwards)"}
    cls = {}
    for k in names:
        try:
            cls[k] = ctx.bench_direct(k, 10)
            if k == 5:   # the replays invert their own output again and again: tiles that trip the inversion's guards there take the guarded form as well (none do in the run itself)
                cls[k]["tiles_guarded_in_replays"] = int(ctx.direct_counters().get("tiles_guarded", 0))
        except Exception as e:
            print(f"roofline: tsl_bench_direct({k}) failed: {e!r}", file=sys.stderr)
            return None, None
    info = ctx.direct_info()
    per_fact = {k: v["us_per_launch"] * v["launches"] for k, v in cls.items()}
    apply_per_iter = max(1.0, (stats["it_fwd"] + stats["it_adj"]) / max(stats["newton"] + K, 1))
    share = dict(per_fact); share[4] = per_fact[4] * apply_per_iter     # applications per factorisation
    # The dominant class: by the IN-SITU totals of the committed rocprofv3 kernel trace of the driver's command where there is one (sibling batches on
    # parallel streams, real cache state: the dataflow chains 1510 ms against 1419 ms of the Schur GEMMs in profile set r05f; 1404 against 1452 in r05e), else by this run's
    # replays (which serialise sibling batches: chains 1086 us, Schur GEMMs 1005 us per factorisation).  Every class is listed either way.
    pats = {0: ("k_ds_gj_step", "k_ds_pivot0", "k_ds_gj_finish"), 1: ("k_ds_gemm<1", "k_ds_gemm_x<1"), 2: ("k_ds_gemm<0", "k_ds_gemm_x<0", "k_ds_gemm_g32"), 3: ("k_ds_inv_small",),
            4: ("k_ds_gemv",), 5: ("k_ds_gj_flow",), 6: ("k_ds_extend_panels",)}
    insitu = None
    try:
        path = os.path.join(ROOT, "profiles", f"latest_{args.workload.replace('-', '_')}_kernel_stats.json")
        if os.path.exists(path) and args.grid == 224:
            with open(path) as fh:
                ks_ = json.load(fh)
            insitu = {k: sum(x["total_ns"] for nm, x in ks_["kernels"].items() if any(q in nm for q in pats[k])) for k in pats}
    except (OSError, KeyError, ValueError):
        insitu = None
    order = sorted(insitu, key=insitu.get, reverse=True) if insitu and max(insitu.values()) > 0 else sorted(share, key=share.get, reverse=True)
    # a class that did not run in THIS run (no launches in the replays: e.g. the dataflow kernel after the context lost its dataflow path to an aborted launch) cannot lead the line
    order = [k for k in order if cls[k]["launches"] > 0 and cls[k]["us_per_launch"] > 0] or [max(share, key=share.get)]
    dom = order[0]

    def class_roof(k):
        """the roofline record of kernel class k: the matrix-core roof for the classes that are flops (GEMMs and the three inversion paths), the HBM roof for the
        sweeps and the panel gather; replay figures of THIS run, traffic and in-situ launch average as constants of the committed profile set"""
        v = cls[k]
        flop_class = k in (0, 1, 2, 3, 5)
        if flop_class:
            ach = v["flops_per_launch"] / (v["us_per_launch"] * 1e-6) / 1e12
            r = {"bound": "mfma", "achieved": ach, "peak": F64_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": ach / F64_MFMA_PEAK_TF, "traffic": None}
        else:
            ach = v["bytes_per_launch"] / (v["us_per_launch"] * 1e-6) / 1e9
            r = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None}
        # HBM bytes per launch: NOT measured by this run -- the figure of the latest committed rocprofv3 --pmc passes for this kernel
        # (scripts/gpu_profile_parts.sh + install_profiles.py), labelled with the profile set and the commit it was taken on
        r["traffic_source"] = None
        try:
            key = {0: "k_ds_gj_step", 1: "k_ds_gemm1", 2: "k_ds_gemm0", 3: "k_ds_inv_small", 4: "k_ds_gemv", 5: "k_ds_gj_flow", 6: "k_ds_extend_panels"}[k]
            path = os.path.join(ROOT, "profiles", f"latest_{args.workload.replace('-', '_')}_pmc_{key}.json")
            if os.path.exists(path) and args.grid == 224:
                with open(path) as fh:
                    j = json.load(fh)
                r["traffic"] = j["traffic_bytes_per_launch"]
                r["traffic_source"] = (f"committed rocprofv3 --pmc passes (FETCH_SIZE x2 + WRITE_SIZE, separate passes) of profile set {j.get('tag', '?')} taken on commit "
                                       f"{j.get('commit', '?')}: a constant read from profiles/, not a measurement of this run")
        except (OSError, KeyError, ValueError):
            pass
        # the same class IN SITU: average duration of its launches in the committed rocprofv3 kernel trace of the driver's command (sibling batches on parallel
        # streams, the real cache state) -- a constant read from profiles/, labelled with its set and commit, next to this run's own replays
        r["avg_launch_us_replay"] = v["us_per_launch"]
        r["avg_launch_us_rocprof"] = None
        try:
            pat = pats[k]
            path = os.path.join(ROOT, "profiles", f"latest_{args.workload.replace('-', '_')}_kernel_stats.json")
            if os.path.exists(path) and args.grid == 224:
                with open(path) as fh:
                    ks = json.load(fh)
                sel = [x for nm, x in ks["kernels"].items() if any(q in nm for q in pat)]
                calls = sum(x["calls"] for x in sel); tot_ns = sum(x["total_ns"] for x in sel)
                if calls:
                    us = tot_ns / calls * 1e-3
                    r["avg_launch_us_rocprof"] = us
                    # per FACTORISATION where the trace says how many it holds (the look-ahead issues the Schur / G launches of the upper levels in two parts and the sweeps
                    # of a first application on two streams: in-situ launch averages no longer compare with this run's whole-batch replays, totals per factorisation do)
                    nf_tr = ks.get("factorisations")
                    us_cmp = (tot_ns * 1e-3 / nf_tr / max(v["launches"], 1)) if nf_tr else us   # in-situ time of the class per factorisation, per replay launch
                    r["in_situ_us_per_factorisation"] = (tot_ns * 1e-3 / nf_tr) if nf_tr else None
                    if flop_class:
                        r["frac_in_situ"] = v["flops_per_launch"] / (us_cmp * 1e-6) / 1e12 / F64_MFMA_PEAK_TF
                    else:
                        r["frac_in_situ"] = v["bytes_per_launch"] / (us_cmp * 1e-6) / 1e9 / HBM_PEAK_GBS
                    r["rocprof_source"] = (f"kernel trace of profile set {ks.get('tag', '?')} (commit {ks.get('commit', '?')}; {ks.get('command', '')}): {calls} launches of {' + '.join(pat)}; "
                                           "a constant read from profiles/, not a measurement of this run")
        except (OSError, KeyError, ValueError):
            pass
        # the GEMM classes against BOTH roofs (the Schur launches gather the children's Schur complements and store their own in the epilogue)
        if k in (1, 2):
            r["hbm_side"] = {"algorithmic_GBs": v["bytes_per_launch"] / (v["us_per_launch"] * 1e-6) / 1e9,
                              "algorithmic_frac_of_peak": v["bytes_per_launch"] / (v["us_per_launch"] * 1e-6) / 1e9 / HBM_PEAK_GBS,
                              "counted_GBs": (r["traffic"] / (v["us_per_launch"] * 1e-6) / 1e9) if r["traffic"] else None,
                              "counted_frac_of_peak": (r["traffic"] / (v["us_per_launch"] * 1e-6) / 1e9 / HBM_PEAK_GBS) if r["traffic"] else None,
                              "note": "same launches priced against the 8 TB/s HBM roof: algorithmic bytes from the plan, counted bytes from the committed --pmc passes (traffic_source)"}
        return r

    rf = class_roof(dom)
    v = cls[dom]
    # the class next in GPU time with the same record (the dataflow inversions and the Schur GEMMs are within a few per cent of each other in the committed
    # traces: 1510 against 1419 ms in set r05f, 1404 against 1452 in r05e): whichever leads, both are in the line
    if len(order) > 1:
        ru = class_roof(order[1])
        ru.update({"kernel": names[order[1]], "flops_per_launch": cls[order[1]]["flops_per_launch"], "bytes_per_launch": cls[order[1]]["bytes_per_launch"],
                   "launches_per_factorization": cls[order[1]]["launches"]})
        rf["runner_up"] = ru
    tot = sum(share.values())
    rf.update({"kernel": names[dom], "flops_per_launch": v["flops_per_launch"], "bytes_per_launch": v["bytes_per_launch"], "avg_launch_us": v["us_per_launch"],
               "launches_per_factorization": v["launches"], "share_of_direct_solve_time": share[dom] / tot,
               "dominant_by": ("in-situ totals of the committed kernel trace (profiles/latest_*_kernel_stats.json): "
                               + ", ".join(f"{names[k].split(' ')[0]} {insitu[k] * 1e-6:.0f} ms" for k in sorted(insitu, key=insitu.get, reverse=True)[:3])) if insitu and max(insitu.values()) > 0
                              else "this run's replays (classes_us_per_newton_iteration)",
               "classes_us_per_newton_iteration": {names[k].split(" ")[0]: share[k] for k in share},
               "classes": {names[k].split(" ")[0]: {"avg_launch_us": cls[k]["us_per_launch"], "launches_per_factorization": cls[k]["launches"], **({"tiles_guarded_in_replays": cls[k]["tiles_guarded_in_replays"]} if "tiles_guarded_in_replays" in cls[k] else {}),
                                                    "flops_per_launch": cls[k]["flops_per_launch"], "bytes_per_launch": cls[k]["bytes_per_launch"],
                                                    "TFLOPs": cls[k]["flops_per_launch"] / max(cls[k]["us_per_launch"], 1e-9) / 1e6,
                                                    "GBs": cls[k]["bytes_per_launch"] / max(cls[k]["us_per_launch"], 1e-9) / 1e3} for k in cls},
               "timing": "avg_launch_us = one HIP-event pair on the library's stream around 10 back-to-back replays of every launch of this kernel class of one "
                         "factorisation (one application for k_ds_gemv) on the run's last plan, divided by the launches (includes the gaps between dependent "
                         "launches; compare the rocprofv3 kernel-trace averages under profiles/)",
               "plan": {k: info[k] for k in ("supernodes", "levels", "batches", "flops_per_factorization", "front_bytes")},
               "mfma_f64_sustained_TFLOPs": {"value": F64_MFMA_SUSTAINED_TF,
                                             "source": "committed micro-benchmark scripts/micro/mfma_lds.hip (profiles/r03_mfma_f64_sustained_peak.txt): the K loop of a GEMM tile alone, LDS operand reads + "
                                                       "v_mfma_f64_16x16x4_f64; a constant, not measured by this run.  The GEMM classes against it: "
                                                       + ", ".join(f"{names[k].split(' ')[0]} {cls[k]['flops_per_launch'] / max(cls[k]['us_per_launch'], 1e-9) / 1e6 / F64_MFMA_SUSTAINED_TF:.2f}" for k in (1, 2))}})
    # bytes_model(measured counts) / wall / 8e12 with the per-triangle figures of the assembled-matrix algorithm (fp64)
    T = scene.cloths[0].NF
    B_cg, B_asm, B_E = 686.0, 600.0, 128.0
    n_asm = stats["newton"] + K
    bytes_model = T * (n_asm * B_asm + (stats["it_fwd"] + stats["it_adj"]) * B_cg + (stats["newton"] + stats["ls"]) * B_E + K * 150.0)
    flops_fact = info["flops_per_factorization"] * stats["factorizations_total"]
    step = {"bytes_model": bytes_model, "achieved_GBs": bytes_model / elapsed / 1e9, "frac_of_hbm_peak": bytes_model / elapsed / 8e12,
            "note": "section 8d prices a step as assemblies + PCG iterations + energy evaluations; the solves are now one sparse factorisation + ~1 refinement iteration "
                    "each (the reference's own algorithm: a direct sparse solve per Newton iteration), so the model's iteration term is nearly empty and the "
                    "factorisation flops are the whole-step yardstick instead",
            "factorization_flops": flops_fact, "factorization_TFLOPs_over_wall": flops_fact / elapsed / 1e12, "frac_of_f64_mfma_peak": flops_fact / elapsed / 1e12 / F64_MFMA_PEAK_TF}
    # FLAT keys (a driver that drops nested objects still keeps these): the north_star's whole-step yardsticks and the runner-up class; `frac` is the IN-SITU
    # figure where the committed kernel trace gives one (what the launches take inside the driver's command), the replay figure of this run stays beside it
    rf["frac_replay"] = rf["frac"]; rf["achieved_replay"] = rf["achieved"]
    if rf.get("frac_in_situ") is not None:
        rf["frac"] = rf["frac_in_situ"]; rf["achieved"] = rf["frac_in_situ"] * rf["peak"]
        rf["frac_is"] = "in situ: algorithmic flops (bytes) per launch / average launch duration of the committed rocprofv3 kernel trace (rocprof_source); frac_replay = this run's HIP-event replays"
    else:
        rf["frac_is"] = "replay: this run's HIP-event pair around back-to-back replays (no committed kernel trace for this workload)"
    rf["hbm_frac_whole_step"] = step["frac_of_hbm_peak"]
    rf["mfma_frac_whole_step"] = step["frac_of_f64_mfma_peak"]
    rf["factorization_TFLOPs_over_wall"] = step["factorization_TFLOPs_over_wall"]
    if "runner_up" in rf:
        ru = rf["runner_up"]
        rf["runner_up_kernel"] = ru["kernel"].split(" ")[0]
        rf["runner_up_frac_replay"] = ru["frac"]
        rf["runner_up_frac_in_situ"] = ru.get("frac_in_situ")
        alg = ru["bytes_per_launch"]
        rf["runner_up_traffic_ratio"] = (ru["traffic"] / alg) if ru.get("traffic") and alg else None
    alg = rf["bytes_per_launch"]
    rf["traffic_ratio"] = (rf["traffic"] / alg) if rf.get("traffic") and alg else None
    return rf, step


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, grad, K):
    """--dump-outputs: what the timed rollout handed its caller, as DIR/<name>.npy in float64 -- the state after the last forward step
    (the tape's x_K: the reverse sweep leaves the scene itself at x_1), the parameter-side gradients of the reverse sweep's last step
    (pos_grad / angleref_grad of tape step 0) and the gripper gradients of the K steps.  An array larger than its share of the 64 MB
    budget is replaced by a fixed sample of its leading-axis rows (default_rng(0), sorted), the same for every run with the same arguments."""
    import numpy as np
    arrays = {
        "pos_final": grad.pos_buffer.t[K],
        "pos_grad_0": grad.pos_grad.t[0],
        "angleref_grad_0": grad.angleref_grad.t[0].reshape(-1, 3),
        "gripper_grad": grad.gripper_grad.t[1:K + 1],
    }
    share = (DUMP_BUDGET_BYTES - 4096 * len(arrays)) // len(arrays)    # room for the .npy headers
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy().astype(np.float64, copy=False)
        if a.nbytes > share:
            rows = max(1, share // max(1, a[0].nbytes))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], size=rows, replace=False))]
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))
        written[name] = list(a.shape)
    return written


def timed_region(batch, run, sync=None):
    """The timed region of the contract: barrier + device synchronisation on BOTH sides of `run()` (K steps of this rank's rollout), wall seconds = the MAX over
    the ranks.  Returns (what run returned, seconds).  Rank logic only -- tests/test_host_logic.py drives it with two gloo ranks and a stand-in rollout."""
    sync = sync or (lambda: None)
    batch.barrier()
    sync()
    t0 = time.perf_counter()
    res = run()
    sync()
    batch.barrier()
    elapsed = time.perf_counter() - t0
    return res, batch.max_over_ranks(elapsed)


def headline(T, K, W, world, elapsed):
    """the contract's keys: value = units of ALL ranks (T triangles x K steps x world) / the max-over-ranks seconds; weak scaling (one scene per GPU)"""
    return {"metric": "element-steps/s (fwd+adjoint), 100k-tri cloth; 1/2/4/8-GPU scaling",
            "value": T * K * world / elapsed, "unit": "element-steps/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic"}


def emit(out, rank):
    """rank 0 prints the ONE JSON line"""
    if rank == 0:
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--idle", type=int, default=0, help="cfg4: leading steps with the zero trajectory (SURVEY section 8d: 10 of T = 50); default 0, every step active")
    ap.add_argument("--workload", choices=["cfg4", "cfg4-scaled", "cfg3", "drape"], default="cfg4",
                    help="cfg4: cloth on ball + 4 tactile pads with contact, cloth_size 0.12 m (the configuration the metric is quoted on); "
                         "cfg4-scaled: same scene enlarged so that the cloth keeps its native 4 mm spacing; cfg3: folding scene with a 200 x 100 cloth "
                         "(40,000 triangles; --grid sets N, M = N / 2): one scene of the cfg5 batch; drape: contact-free pinned cloth")
    ap.add_argument("--grid", type=int, default=224, help="cloth grid N = M (224 -> 100,352 triangles)")
    ap.add_argument("--cloth-size", type=float, default=0.1 / 15 * 224, help="edge length of the square cloth in m (default keeps the reference dx = 0.1/15)")
    ap.add_argument("--cg-tol", type=float, default=1e-10)
    ap.add_argument("--full", action="store_true", help="after the headline measurement, also the legs that take runs of their own: roofline (kernel-class "
                                                         "replays) and cpu_baseline (oracle steps on the host; --no-cpu-baseline leaves it out)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave cpu_baseline out")
    ap.add_argument("--param", action="append", default=[], metavar="KEY=VALUE", help="extra tsl_set_param settings (solver experiments)")
    ap.add_argument("--scenes-per-gpu", type=int, default=0, help="after the single-scene measurement: the same workload as S independent scenes on this GPU stepped in lock step as one scene group "
                                                                     "(merged factorisations), reported as multi_scene next to the headline value")
    ap.add_argument("--multi-only", type=int, default=0, help=argparse.SUPPRESS)      # child process of --scenes-per-gpu
    ap.add_argument("--single-value", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-grid", type=int, default=71, help="cloth grid of the complete oracle steps of cpu_baseline")
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed rollout computed (rank 0) as DIR/<name>.npy in float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.workload == "cfg3" and args.grid == 224:
        args.grid = 200

    if args.multi_only > 1:
        import torch  # noqa: F401
        print(json.dumps(multi_scene(args, 0, args.multi_only, args.steps, args.warmup, args.single_value)), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one rank per GPU of this node over RCCL: re-execute under torch.distributed.run (the driver's own launcher sets WORLD_SIZE)
        port = 29500 + os.getpid() % 2000
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path in thinshelllab_amd)")
    from thinshelllab_amd.batch import Batch
    batch = Batch()  # one process per GPU (RANK / LOCAL_RANK / WORLD_SIZE from torch.distributed.run); backend nccl == RCCL
    world, rank = batch.world, batch.rank
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but the process group has {world} ranks")
    torch.cuda.set_device(batch.local_rank)

    from thinshelllab_amd.engine.analytic_grad_single import Grad
    scene = build_scene(args, rank)
    K, W = args.steps, args.warmup
    ctx = scene._ensure_ctx()
    ctx.set_param("cg_tol", args.cg_tol)
    for kv in args.param:
        k, v = kv.split("=")
        ctx.set_param(k, float(v))
    n_part = scene.gripper.n_part if args.workload != "drape" else 0
    grad = Grad(scene, max(K, W) + 1, n_part)
    grad.init_mass(scene)
    if W > 0:
        run_rollout(scene, grad, W, args)

    info0 = ctx.direct_info()
    stats, elapsed = timed_region(batch, lambda: run_rollout(scene, grad, K, args), torch.cuda.synchronize)
    info1 = ctx.direct_info()
    stats["factorizations_total"] = info1["factorizations"] - info0["factorizations"]
    dumped = dump_outputs(args.dump_outputs, grad, K) if args.dump_outputs and rank == 0 else None

    T = scene.cloths[0].NF
    n_solves_fwd = max(stats["newton"], 1)
    out = headline(T, K, W, world, elapsed)
    value = out["value"]
    out.update({
        "config": {"workload": (f"cfg4 (SURVEY.md section 8d): Scene_balancing topology, {args.grid}x{args.grid} cloth ({T} triangles, cloth_size "
                                f"{0.12 * args.grid / 224:.3f} m, dx {0.12 / 224:.2e} m) on the ball + 4 tactile pads at their native poses, paired grippers driven "
                                f"+-1e-4 m in z every step" + (f" after {args.idle} idle steps" if args.idle else "") + ", loss get_loss_balance; "
                                if args.workload == "cfg4" else
                                f"cfg3 (SURVEY.md section 8d): Scene_folding topology with a {args.grid}x{args.grid // 2} cloth ({T} triangles, cloth_size 0.1 m), frozen table + one "
                                f"tactile pad driven -z 2e-4 m per step for ten steps then +x, plastic hinges, loss get_loss_fold(1, -1); "
                                if args.workload == "cfg3" else
                                f"cfg4-scaled: Scene_balancing (cloth on ball + 4 tactile pads, paired grippers driven every step) with a {args.grid}x{args.grid} cloth "
                                f"({T} triangles) and the whole scene enlarged x{args.grid * 0.004 / 0.06:.2f} so that the cloth keeps its native 4 mm spacing; "
                                if args.workload == "cfg4-scaled" else
                                f"drape: {args.grid}x{args.grid} square cloth ({T} triangles, dx={args.cloth_size / args.grid:.3e} m), one pinned row, no contact; ") +
                               "per step: implicit-Euler Newton time step (contact detection, friction; per Newton iteration one multifrontal LU of the "
                               "operator, its first application accepted when backward stable, else refined to cg_tol) + adjoint transfer_grad; one independent scene per GPU",
                   "triangles": T, "tot_NV": scene.tot_NV, "cg_tol": args.cg_tol, "active_contacts_per_step": stats["nc"] / K,
                   "newton_iters_per_step": stats["newton"] / K, "line_search_evals_per_step": stats["ls"] / K,
                   "newton_last_delta_per_step": [float(f"{d:.3g}") for d in stats["last_delta"]],
                   "refinement_iters_per_fwd_solve": stats["it_fwd"] / n_solves_fwd, "refinement_iters_per_adjoint_solve": stats["it_adj"] / K,
                   "pcg_iters_per_fwd_solve": stats["it_fwd"] / n_solves_fwd, "pcg_iters_per_adjoint_solve": stats["it_adj"] / K,
                   "factorizations": stats["factorizations_total"], "symbolic_plans": info1["plans"] - info0["plans"], "plan_host_seconds": info1["plan_seconds"] - info0["plan_seconds"],
                   "solves_unconverged": stats["fwd_unconverged"] + stats["adj_unconverged"],
                   "solver_fallbacks": {"forward": stats["fwd_fallback"], "adjoint": stats["adj_fallback"]},
                   "solves_accepted_at_attainable_accuracy": {"forward": stats["fwd_attained"], "adjoint": stats["adj_attained"]},
                   "first_passes_accepted_on_backward_error": _berr_counters(ctx),
                   "dataflow_launches": {"launched": int(ctx.direct_counters()["flow_launches"]), "lost": int(ctx.direct_counters()["flow_aborts"]),
                                         "note": "k_ds_gj_flow launches since context creation; lost = launches that ran into their poll limit (the solve then refactorises on the launch-per-block-step path and the context keeps that path: slower, same bits)"},
                   "max_rel_residual_fwd": stats["max_res_fwd"], "max_rel_residual_adjoint": stats["max_res_adj"], "max_backward_error_adjoint": stats["max_be_adj"],
                   "adjoint_solve_methods": {str(k): v for k, v in stats["methods"].items()}},
    })
    if dumped is not None:
        out["dumped_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
    if args.full:
        rf, step = roofline(ctx, scene, elapsed, K, stats, args)
        if rf is not None:
            rf["whole_step"] = step   # SURVEY section 8d's bytes model and the factorisation-flops figure of the WHOLE step, inside the object the driver keeps
            out["roofline"] = rf
    if args.scenes_per_gpu > 1 and rank == 0 and world == 1:
        # the multi-scene leg runs in a child process of its own (a fresh HIP context: this process keeps its scene, plans and arenas for the baseline leg below)
        try:
            ctx.set_param("direct_flow_token", 0)   # the child's scene group takes the device's dataflow token while this process waits
            env = dict(os.environ)   # (more hardware queues than the runtime's default were measured SLOWER for a group: 461 against 430 ms per lock step at S = 2, 1168 against 855 at S = 4)
            cmd = [sys.executable, os.path.abspath(__file__), "--multi-only", str(args.scenes_per_gpu), "--single-value", repr(value / world), "--steps", str(K), "--warmup", str(W),
                   "--workload", args.workload, "--grid", str(args.grid), "--idle", str(args.idle), "--cg-tol", repr(args.cg_tol)] + [x for kv in args.param for x in ("--param", kv)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1800)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            out["multi_scene"] = json.loads(line[-1]) if line else {"scenes_per_gpu": args.scenes_per_gpu, "value": None, "error": (r.stderr or "no output")[-400:]}
        except Exception as e:   # noqa: BLE001 -- never fail the headline on the extra measurement
            out["multi_scene"] = {"scenes_per_gpu": args.scenes_per_gpu, "value": None, "error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(args, scene, stats, K, rank)
        except Exception as e:  # the oracle is optional test infrastructure; never fail the GPU number on it
            out["cpu_baseline"] = {"value": None, "unit": "element-steps/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e!r}"}
    emit(out, rank)
    batch.close()


if __name__ == "__main__":
    main()
