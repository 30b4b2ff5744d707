"""Trajectory optimisation of a bare cloth gripped at points of its surface (no counterpart in the reference): the driver of ``trajopt_frames.py``
with the clamp replaced by two grip patches of three points each, placed by ``Cloth.locate`` at parametric coordinates inside faces near the two
corners of the held edge (0.07 and 0.93 of the width) -- the same material points at every resolution N -- and tied to one rigid frame through
``BaseScene.set_surface_handles`` and ``BaseScene.set_handle_frames``.  The optimisation variable is the frame's step (delta_pos, delta_theta) of
every time step; the reverse sweep of ``analytic_grad_single.Grad`` returns ``frame_grad``.  The loss is the in-plane goal of ``trajopt_handles``
(the squared distance of the opposite edge to its own line moved towards the grip), which the membrane transmits within the horizon.  Adam
(``optimizer.optim.Adam_single``) on the steps.  A usage example of the surface-handle interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch

from .trajopt_frames import step_gradient
from .trajopt_handles import edge_line_loss

# (u, v) of the grip points: u along grid index i (1 = the held edge), v along the width; three points per patch, none on a vertex or an edge
GRIP_POINTS = ((0.97, 0.07), (0.93, 0.05), (0.94, 0.11), (0.97, 0.93), (0.93, 0.95), (0.94, 0.89))

def optimise(N=8, T=4, iters=3, k=2000.0, shift=1e-3, lr=1e-4, stvk=(3.0e5, 2.0e5), device="cuda:0", log=print):
    """returns (losses per iteration, steps (T, 1, 6): delta_pos in m and delta_theta in rad of every time step; row 0 is not used).  Adam moves a
    position step by about lr metres per iteration, and a rotation step by the angle that moves the far end of the held edge as much."""
    from ..engine.analytic_grad_single import Grad
    from ..optimizer.optim import Adam_single
    from ..task_scene.Scene_drape import Scene

    sys = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, Kb=0.0, pin_row=False, perturb=0.0, device=device)
    c = sys.cloths[0]
    c.stvk_mu[None], c.stvk_lam[None] = stvk   # the StVK membrane: its matrix is the exact second derivative, so the reverse sweep is exact too
    c.membrane[None] = 1.0
    sys.init_all()
    x0 = sys.pos.to_numpy()
    held = np.arange(c.offset + c.N * (c.M + 1), c.offset + (c.N + 1) * (c.M + 1))   # the held edge: grid row i = N
    edge = np.arange(c.offset, c.offset + c.M + 1)                                   # the opposite edge: grid row i = 0
    u = x0[edge[-1]] - x0[edge[0]]
    width = float(np.linalg.norm(u))
    u /= width
    n = x0[held].mean(0) - x0[edge].mean(0)
    q = x0[edge[0]] + shift * n / np.linalg.norm(n)            # the goal: the edge's own line, moved in the plane towards the clamp
    grip = [c.locate(a, b) for a, b in GRIP_POINTS]                      # (global face id, barycentric coordinates) of every grip point
    sys.set_surface_handles([f for f, _ in grip], [b for _, b in grip], k)
    sys.set_handle_frames(np.zeros(len(grip), np.int32), n_frames=1)
    pose0 = (x0[held].mean(0)[None], np.array([[1.0, 0.0, 0.0, 0.0]]))   # the frame at the middle of the held edge, axes along the world's
    sys.set_frame_poses(*pose0)
    sys.set_handle_frames(np.zeros(len(grip), np.int32))                 # grasp the points where they are: r_i = R^T (p_i - c)
    rot_unit = 1.0 / width                                               # rad per unit of the rotation variables
    steps = torch.zeros((T, 1, 6), dtype=torch.float64)                  # (delta_pos, delta_theta / rot_unit)
    grad = Grad(sys, T, 0)
    grad.init_mass(sys)
    opt, losses = Adam_single((T, 1, 6), lr, 0.9, 0.999, 1e-30), []
    for it in range(iters):
        sys.pos.from_numpy(x0); sys.prev_pos.from_numpy(x0); sys.vel.fill(0.0)
        grad.reset()
        sys.set_frame_poses(*pose0)
        grad.copy_pos(sys, 0)
        d = steps.numpy() * np.array([1.0, 1.0, 1.0, rot_unit, rot_unit, rot_unit])
        for f in range(1, T):
            sys.move_frames(d[f, :, :3], d[f, :, 3:])
            sys.time_step(None, f)
            grad.copy_pos(sys, f)
        loss, dl = edge_line_loss(grad.pos_buffer.t[T - 1].cpu().numpy(), edge, q, u)
        wrench = sys.frame_wrench()[0]
        grad.pos_grad.t[T - 1, torch.as_tensor(edge)] = torch.as_tensor(dl, device=grad.pos_grad.t.device)
        for f in range(T - 1, 0, -1):
            grad.transfer_grad(f, sys, None)
        g = step_gradient(grad.frame_grad.t.numpy(), d[:, :, 3:])
        g[:, :, 3:] *= rot_unit
        losses.append(loss)
        log(f"iter {it}: loss {loss:.6e}  max |d loss / d step| {np.abs(g).max():.3e}  grip force {np.linalg.norm(wrench[:3]):.3e} N  "
            f"moment {np.linalg.norm(wrench[3:]):.3e} N m")
        opt.step(steps, torch.as_tensor(g))
    return losses, steps.numpy() * np.array([1.0, 1.0, 1.0, rot_unit, rot_unit, rot_unit])


def main(argv=None):
    parser = ArgumentParser()
    for flag, typ, default in (('--N', int, 8), ('--tot_step', int, 4), ('--iter', int, 10), ('--k', float, 2000.0), ('--shift', float, 1e-3), ('--lr', float, 1e-4)):
        parser.add_argument(flag, type=typ, default=default)
    args = parser.parse_args(argv)
    return optimise(N=args.N, T=args.tot_step, iters=args.iter, k=args.k, shift=args.shift, lr=args.lr)


if __name__ == "__main__":
    main()
