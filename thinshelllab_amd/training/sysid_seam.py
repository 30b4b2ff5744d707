"""System identification of a seam's stiffness (no counterpart in the reference): ``Scene_seam`` -- a cloth sewn to the free edge of a pinned one,
hanging from it under gravity -- is rolled out for T steps at a true ``k_tie`` and the trajectory is recorded; gradient descent on ``log k_tie``
from a wrong start then lowers the squared distance of the rollout to the record.  The gradient comes from the reverse sweep of
``analytic_grad_system.Grad`` through ``param_keys = ["k_tie"]``.  A usage example of the tie interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch


def optimise(N=8, T=4, iters=3, k_true=2000.0, k_start=500.0, max_step=0.4, stvk=(3.0e5, 2.0e5), device="cuda:0", log=print):
    """returns (losses per iteration, k_tie per iteration).  A step moves log k_tie by at most max_step: the first by exactly that, the later ones
    in proportion to their gradient."""
    from ..engine.analytic_grad_system import Grad
    from ..task_scene.Scene_seam import Scene

    sys = Scene(N=N, k_tie=k_true, Kb=0.0, perturb=0.0, stvk=stvk, device=device)
    sys.init_all()
    sys._ensure_ctx().set_param("direct", 1)
    x0 = sys.pos.to_numpy()
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    grad.count_kb_grad = False
    grad.param_keys = ["k_tie"]

    def forward(k):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        sys._ensure_ctx().set_param("k_tie", k)
        grad.reset()
        grad.copy_pos(sys, 0)
        for f in range(1, T):
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        return grad.pos_buffer.t.clone()

    record = forward(k_true)
    theta, lr = float(np.log(k_start)), None
    losses, ks = [], []
    for it in range(iters):
        k = float(np.exp(theta))
        diff = forward(k) - record
        loss = 0.5 * float((diff * diff).sum())
        grad.pos_grad.t[1:] = diff[1:]
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = k * grad.grad_params["k_tie"]          # d loss / d log k_tie
        if lr is None:
            lr = max_step / abs(g)
        losses.append(loss); ks.append(k)
        log(f"iter {it}: k_tie {k:.6e}  loss {loss:.6e}  d loss / d log k_tie {g:.3e}  largest tie residual {np.abs(sys.tie_residuals()).max():.3e} m")
        theta -= float(np.clip(lr * g, -max_step, max_step))
    return losses, ks


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k_true', float, 2000.0), ('--k_start', float, 500.0)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k_true=args.k_true, k_start=args.k_start)


if __name__ == "__main__":
    main()
