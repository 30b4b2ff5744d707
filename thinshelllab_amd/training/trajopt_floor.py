"""Trajectory optimisation of a rising plate (no counterpart in the reference, whose supports are frozen bodies): a ``Scene_floor`` cloth rests on
the collider floor (``BaseScene.set_colliders``), the floor's offset at every step is the optimisation variable, the loss is the squared distance
of the cloth's mean height at the end of the rollout to a target above its resting height.  Forward rollout with the offsets on the tape, reverse
sweep of ``analytic_grad_single.Grad`` (``collider_grad[s, 0, 0]`` = d(loss)/d(offset of step s)), plain gradient descent.  A usage example of the collider interface, not a benchmark."""
from argparse import ArgumentParser

import torch


def optimise(N=8, T=4, iters=3, k=2000.0, lift=2e-5, step_len=4e-6, device="cuda:0", log=print):
    """returns (losses per iteration, offsets (T,)).  The learning rate is fixed by the first gradient: its largest entry moves an offset by step_len."""
    from ..engine.analytic_grad_single import Grad
    from ..task_scene.Scene_floor import Scene

    sys = Scene(N=N, k_collider=k, device=device)
    sys.init_all()
    x0 = sys.pos.to_numpy()
    target = float(x0[:, 2].mean()) + lift
    offsets = torch.zeros((T, 1), dtype=torch.float64)
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    lr, losses = None, []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_collider_offsets(offsets[0].numpy())
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_collider_offsets(offsets[f].numpy())
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        z = grad.pos_buffer.t[T - 1, :, 2]
        err = float(z.mean().item()) - target
        loss = err * err
        grad.pos_grad.t[T - 1, :, 2] = 2.0 * err / z.numel()
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.collider_grad.t[:, :, 0]
        if lr is None:
            lr = step_len / max(float(g.abs().max()), 1e-300)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  mean height error {err:.3e} m  max |d loss / d offset| {float(g.abs().max()):.3e}  force on the plate {sys.collider_force()[0, 2]:.3e} N")
        offsets -= lr * g
    return losses, offsets


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--lift', float, 2e-5), ('--step_len', float, 4e-6)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, lift=args.lift, step_len=args.step_len)


if __name__ == "__main__":
    main()
