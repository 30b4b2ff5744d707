"""Trajectory optimisation of a plate (no counterpart in the reference, whose table tops are meshed bodies): a ``Scene_table`` cloth, two corners
frozen, lies half on a rounded-box collider (``BaseScene.set_boxes``) and hangs over its edge; the plate's pose at every step -- its centre and a
world-frame rotation vector on top of its orientation, so that lifting and tilting are both free -- are the optimisation variables, the loss is
the squared distance of the cloth's centre vertex, which lies over the plate's edge, at the end of the rollout to a target above and beside where
it starts.
Forward rollout with the poses on the tape, reverse sweep of ``analytic_grad_single.Grad`` (``box_pose_grad()[s, 0]`` = d(loss)/d(centre,
rotation vector of step s)), plain gradient descent, the rotation applied with ``frames.compose``.  A usage example of the box interface, not a
benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=8, T=4, iters=3, k=2000.0, lift=(1e-5, 0.0, 4e-5), step_len=4e-6, arm=0.02, device="cuda:0", log=print):
    """returns (losses per iteration, centres (T, 1, 3), quaternions (T, 1, 4)).  The learning rate is fixed by the first gradient: its largest entry
    moves the centre by step_len, or turns the plate by step_len / arm (arm: the length in metres that makes a rotation comparable to a
    translation)."""
    from ..engine import frames
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_table import Scene

    sys = Scene(N=N, k_box=k, push=2e-4, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    tip = sys.centre_vertex()
    target = torch.as_tensor(x0[tip] + np.asarray(lift, dtype=np.float64))
    c0, q0, h, r, mu = sys.plate()
    cen, quat = np.repeat(c0[None], T, axis=0), np.repeat(q0[None], T, axis=0)
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    lr, losses = None, []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_boxes(cen[0], quat[0], h, r, mu, k)   # (the plate at rest in its first pose)
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_box_poses(cen[f], quat[f])
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        err = grad.pos_buffer.t[T - 1, tip].cpu() - target
        loss = float((err * err).sum())
        grad.pos_grad.t[T - 1, tip] = (2.0 * err).to(grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.box_pose_grad().numpy().copy()
        g[0] = 0.0   # (the plate starts where it lies)
        g[:, :, 3:6] /= arm * arm   # (descent in (centre, arm * rotation vector))
        if lr is None:
            lr = step_len / max(float(np.abs(g[:, :, 0:3]).max()), float(np.abs(g[:, :, 3:6]).max()) * arm, 1e-300)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  |error| {float(err.norm()):.3e} m  max |d loss / d pose| {float(np.abs(g).max()):.3e}  force and torque of the plate {sys.box_force()[0]}")
        for f in range(T):
            cen[f], quat[f] = frames.compose(cen[f], quat[f], -lr * g[f, :, 0:3], -lr * g[f, :, 3:6])
    return losses, cen, quat


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--step_len', float, 4e-6)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, step_len=args.step_len)


if __name__ == "__main__":
    main()
