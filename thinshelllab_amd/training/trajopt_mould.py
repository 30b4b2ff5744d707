"""Trajectory optimisation of a mould (no counterpart in the reference, whose moulds are meshed bodies): a ``Scene_mould`` cloth, its corners frozen,
lies over a ring given as a sampled distance field (``BaseScene.set_sdfs``); the mould's pose at every step -- its centre and a world-frame rotation
vector on top of its orientation, so that lifting and tilting are both free -- are the optimisation variables, the loss is the squared distance at
the end of the rollout of a vertex that lies on the ring to a target above and beside where it starts.
Forward rollout with the poses on the tape, reverse sweep of ``analytic_grad_single.Grad`` (``sdf_pose_grad()[s, 0]`` = d(loss)/d(centre, rotation
vector of step s)), Adam on (centre, arm * rotation vector), the rotation applied with ``frames.compose``.  A usage example of the field interface,
not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=8, T=4, iters=4, k=2000.0, lift=(1e-5, 0.0, 4e-5), step_len=4e-6, arm=0.02, device="cuda:0", log=print):
    """returns (losses per iteration, centres (T, 1, 3), quaternions (T, 1, 4)).  Adam with beta = (0.9, 0.999) and the step step_len in metres of the
    centre (a rotation of step_len / arm; arm: the length in metres that makes a rotation comparable to a translation)."""
    from ..engine import frames
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_mould import Scene

    sys = Scene(N=N, k_sdf=k, push=2e-4, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    grid, origin, h, c0, q0, r, mu = sys.mould()
    # the vertex of the sheet's middle row that lies nearest over the ring's crest
    row = np.flatnonzero(np.abs(x0[:, 1] - x0[sys.centre_vertex(), 1]) < 1e-12)
    tip = int(row[np.argmin(np.abs(x0[row, 0] - sys._mould["major"]))])
    target = torch.as_tensor(x0[tip] + np.asarray(lift, dtype=np.float64))
    cen, quat = np.repeat(c0[None], T, axis=0), np.repeat(q0[None], T, axis=0)
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    m1, m2, losses = np.zeros((T, 1, 6)), np.zeros((T, 1, 6)), []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_sdf_poses(cen[0], quat[0], cen[0], quat[0])   # (the mould at rest in its first pose)
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_sdf_poses(cen[f], quat[f])
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        err = grad.pos_buffer.t[T - 1, tip].cpu() - target
        loss = float((err * err).sum())
        grad.pos_grad.t[T - 1, tip] = (2.0 * err).to(grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.sdf_pose_grad().numpy().copy()
        g[0] = 0.0   # (the mould starts where it lies)
        g[:, :, 3:6] /= arm   # (the gradient in (centre, arm * rotation vector))
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  |error| {float(err.norm()):.3e} m  max |d loss / d pose| {float(np.abs(g).max()):.3e}  force and torque of the mould {sys.sdf_force()[0]}")
        m1 = 0.9 * m1 + 0.1 * g
        m2 = 0.999 * m2 + 0.001 * g * g
        step = step_len * (m1 / (1.0 - 0.9 ** (it + 1))) / (np.sqrt(m2 / (1.0 - 0.999 ** (it + 1))) + 1e-300)
        step[0] = 0.0
        for f in range(T):
            cen[f], quat[f] = frames.compose(cen[f], quat[f], -step[f, :, 0:3], -step[f, :, 3:6] / arm)
    return losses, cen, quat


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--step_len', float, 4e-6)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, step_len=args.step_len)


if __name__ == "__main__":
    main()
