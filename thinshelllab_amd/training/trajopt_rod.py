"""Trajectory optimisation of a rod (no counterpart in the reference, whose rods are meshed bodies): a ``Scene_rod`` cloth, its corners frozen, lies
over a capsule collider (``BaseScene.set_capsules``); the rod's two endpoints at every step are the optimisation variables -- they are
independent, so translation and yaw are both free --, the loss is the squared distance of the cloth's centre vertex at the end of the rollout
to a target above and beside where it starts.  Forward rollout with the endpoints on the tape, reverse sweep of ``analytic_grad_single.Grad``
(``capsule_end_grad()[s, 0]`` = d(loss)/d(endpoints a, b of step s)), plain gradient descent.  A usage example of the capsule interface, not a
benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=8, T=4, iters=3, k=2000.0, lift=(1e-5, 0.0, 4e-5), step_len=4e-6, device="cuda:0", log=print):
    """returns (losses per iteration, endpoints (T, 1, 2, 3)).  The learning rate is fixed by the first gradient: its largest entry moves an endpoint by step_len."""
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_rod import Scene

    sys = Scene(N=N, k_capsule=k, push=2e-4, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    mid = sys.centre_vertex()
    target = torch.as_tensor(x0[mid] + np.asarray(lift, dtype=np.float64))
    a0, b0, R, mu = sys.rod()
    ends = torch.as_tensor(np.stack([a0, b0], axis=1)).repeat(T, 1, 1, 1).clone()
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    lr, losses = None, []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_capsules(ends[0, :, 0].numpy(), ends[0, :, 1].numpy(), R, mu, k)   # (the rod at rest at its first endpoints)
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_capsule_ends(ends[f, :, 0].numpy(), ends[f, :, 1].numpy())
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        err = grad.pos_buffer.t[T - 1, mid].cpu() - target
        loss = float((err * err).sum())
        grad.pos_grad.t[T - 1, mid] = (2.0 * err).to(grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.capsule_end_grad()
        g[0] = 0.0   # (the rod starts where it lies)
        if lr is None:
            lr = step_len / max(float(g.abs().max()), 1e-300)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  |error| {float(err.norm()):.3e} m  max |d loss / d endpoint| {float(g.abs().max()):.3e}  force and torque of the rod {sys.capsule_force()[0]}")
        ends -= lr * g
    return losses, ends


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--step_len', float, 4e-6)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, step_len=args.step_len)


if __name__ == "__main__":
    main()
