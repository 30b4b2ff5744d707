"""Trajectory optimisation of a fan (no counterpart in the reference, which has no load from the medium): a ``Scene_flag`` cloth hangs from two
corners in a wind (``BaseScene.set_wind``); the wind velocity at every step is the optimisation variable, the loss is the squared distance of the
centroid of the flag's free edge at the end of the rollout to a target beside where it starts.  Forward rollout with the wind velocities on the
tape, reverse sweep of ``analytic_grad_single.Grad`` (``wind_velocity_grad()[s]`` = d(loss)/d(wind velocity of step s)), Adam.  A usage example
of the wind interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=16, T=6, iters=5, shift=(2e-4, 6e-4, 1e-4), lr=0.2, device="cuda:0", log=print):
    """returns (losses per iteration, wind velocities (T, 3)).  Adam with step `lr` m / s on the velocities of steps 1 .. T - 1."""
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_flag import Scene

    sys = Scene(N=N, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    edge = sys.free_edge()
    target = torch.as_tensor(x0[edge].mean(axis=0) + np.asarray(shift, dtype=np.float64))
    W = np.tile(sys._wind["W"], (T, 1))
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    m1, m2, losses = np.zeros_like(W), np.zeros_like(W), []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_wind_velocity(W[0])
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_wind_velocity(W[f])
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        err = grad.pos_buffer.t[T - 1, edge].mean(dim=0).cpu() - target
        loss = float((err * err).sum())
        grad.pos_grad.t[T - 1, edge] = (2.0 * err / len(edge)).to(grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.wind_velocity_grad().numpy()
        g[0] = 0.0   # (no step uses the velocity of row 0)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  |error| {float(err.norm()):.3e} m  max |d loss / d W| {np.abs(g).max():.3e}  force of the wind {sys.wind_force()} N")
        m1 = 0.9 * m1 + 0.1 * g
        m2 = 0.999 * m2 + 0.001 * g * g
        W = W - lr * (m1 / (1 - 0.9 ** (it + 1))) / (np.sqrt(m2 / (1 - 0.999 ** (it + 1))) + 1e-30)
    return losses, W


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 16), ('--tot_step', int, 6), ('--iter', int, 10), ('--lr', float, 0.2)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, lr=args.lr)


if __name__ == "__main__":
    main()
