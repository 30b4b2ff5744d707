"""Trajectory optimisation of a bare cloth through soft handles (no counterpart in the reference, whose drivers move a cloth through gripper
bodies): a ``Scene_drape`` cloth hangs from two handles on the corners of its last grid row (``BaseScene.set_handles``), the handle targets of
every step are the optimisation variable, the loss is the squared distance of the opposite edge to a line at the end of the rollout (the edge's
own line moved towards the held side: the sheet has to be dragged there; what gravity does to the free edge meanwhile stays in the loss).  Forward
rollout with the targets on the tape, reverse sweep of ``analytic_grad_single.Grad`` (``handle_grad`` = d(loss)/d(targets)), plain gradient
descent with ``optimizer.optim.SGD_single``.  A usage example of the handle interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def edge_line_loss(x, edge, q, u):
    """sum over the edge vertices of the squared distance to the line q + s u (|u| = 1) and its gradient with respect to their positions"""
    r = x[edge] - q
    perp = r - (r @ u)[:, None] * u
    return float((perp * perp).sum()), 2.0 * perp


def optimise(N=8, T=4, iters=3, k=2000.0, shift=1e-3, step_len=2e-4, device="cuda:0", log=print):
    """returns (losses per iteration, targets (T, 2, 3)).  The learning rate is fixed by the first gradient: its largest entry moves a target by step_len."""
    from ..engine.analytic_grad_single import Grad
    from ..optimizer.optim import SGD_single
    from ..task_scene.Scene_drape import Scene

    sys = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, pin_row=False, perturb=0.0, device=device)
    sys.init_all()
    c = sys.cloths[0]
    x0 = sys.pos.to_numpy()
    held = c.corner_ids()[2:]                                  # the corners of grid row i = N
    edge = np.arange(c.offset, c.offset + c.M + 1)             # the opposite edge: grid row i = 0
    u = x0[edge[-1]] - x0[edge[0]]
    u /= np.linalg.norm(u)
    n = x0[held].mean(0) - x0[edge].mean(0)
    q = x0[edge[0]] + shift * n / np.linalg.norm(n)            # the goal: the edge's own line, moved in the plane towards the held corners
    sys.set_handles(held, k)
    targets = torch.tensor(np.repeat(x0[held][None], T, axis=0))
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    opt, losses = None, []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_handle_targets(targets[0])
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.set_handle_targets(targets[f])
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        loss, dl = edge_line_loss(grad.pos_buffer.t[T - 1].cpu().numpy(), edge, q, u)
        grad.pos_grad.t[T - 1, torch.as_tensor(edge)] = torch.as_tensor(dl, device=grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = grad.handle_grad.t
        if opt is None:
            opt = SGD_single(tuple(targets.shape), step_len / max(float(g.abs().max()), 1e-300), 0, 0, 0)
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  max |d loss / d target| {float(g.abs().max()):.3e}  handle force {np.abs(sys.handle_force()).max():.3e} N")
        opt.step(targets, g)
    return losses, targets


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--shift', float, 1e-3), ('--step_len', float, 2e-4)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, shift=args.shift, step_len=args.step_len)


if __name__ == "__main__":
    main()
