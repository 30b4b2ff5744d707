"""Trajectory optimisation of a pusher (no counterpart in the reference, whose pushers are meshed bodies): a ``Scene_ball`` cloth, its corners
frozen, lies over a sphere collider (``BaseScene.set_spheres``); the ball's centre at every step is the optimisation variable, the loss is the
squared distance of the cloth's centre vertex at the end of the rollout to a target above and beside where it starts.  Forward rollout with the
centres on the tape, reverse sweep of ``analytic_grad_single.Grad`` (``sphere_centre_grad()[s, 0]`` = d(loss)/d(centre of step s)), plain gradient
descent.  A usage example of the sphere interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=8, T=4, iters=3, k=2000.0, lift=(1e-5, 0.0, 4e-5), step_len=4e-6, device="cuda:0", log=print):
    """returns (losses per iteration, centres (T, 1, 3)).  The learning rate is fixed by the first gradient: its largest entry moves a centre by step_len."""
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_ball import Scene

    sys = Scene(N=N, k_sphere=k, push=2e-4, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    mid = sys.centre_vertex()
    target = torch.as_tensor(x0[mid] + np.asarray(lift, dtype=np.float64))
    c0 = sys.ball()[0]
    centres = torch.as_tensor(c0).repeat(T, 1, 1).clone()
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    lr, losses = None, []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_spheres(centres[0].numpy(), *sys.ball()[1:], k)   # (the ball at rest at the first centre)
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_sphere_centres(centres[f].numpy())
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        err = grad.pos_buffer.t[T - 1, mid].cpu() - target
        loss = float((err * err).sum())
        grad.pos_grad.t[T - 1, mid] = (2.0 * err).to(grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.sphere_centre_grad()
        g[0] = 0.0   # (the ball starts where it lies)
        if lr is None:
            lr = step_len / max(float(g.abs().max()), 1e-300)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  |error| {float(err.norm()):.3e} m  max |d loss / d centre| {float(g.abs().max()):.3e}  force of the ball {sys.sphere_force()[0]} N")
        centres -= lr * g
    return losses, centres


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--step_len', float, 4e-6)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, step_len=args.step_len)


if __name__ == "__main__":
    main()
