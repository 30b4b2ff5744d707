"""Trajectory optimisation of a bare cloth through a rigid frame (no counterpart in the reference, whose drivers move a cloth through gripper
bodies): the sheet of ``trajopt_handles.py``, as an StVK membrane without bending stiffness, with one whole edge (grid row i = N) clamped on a single frame (``BaseScene.set_handle_frames``).
The optimisation variable is the frame's step (delta_pos, delta_theta) of every time step, applied through ``BaseScene.move_frames`` -- 6 numbers in
per step; the reverse sweep of ``analytic_grad_single.Grad`` returns ``frame_grad``, 6 numbers out per step: d(loss)/d(position) and
d(loss)/d(world rotation vector applied on the left) of the pose of that step.  The loss is the in-plane goal of ``trajopt_handles``: the squared
distance of the opposite edge to its own line moved towards the clamp.  Adam (``optimizer.optim.Adam_single``) on the steps.  A usage example of the
frame interface, not a benchmark."""
from argparse import ArgumentParser

import numpy as np
import torch

from .trajopt_handles import edge_line_loss


def _hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def left_jacobian(theta):
    """J with exp([theta + d]x) = exp([J d]x) exp([theta]x) to first order in d"""
    phi = float(np.linalg.norm(theta))
    K = _hat(theta)
    if phi < 1e-4:
        return np.eye(3) + 0.5 * K + K @ K / 6.0
    return np.eye(3) + (1.0 - np.cos(phi)) / phi ** 2 * K + (phi - np.sin(phi)) / phi ** 3 * (K @ K)


def step_gradient(frame_grad, delta_theta):
    """d(loss)/d(steps) (T, n_frame, 6) from d(loss)/d(poses) = frame_grad (T, n_frame, 6): the pose of step s is the product of the steps f <= s, so
    a position step f reaches every pose s >= f as it is, and a rotation step f reaches pose s as the world rotation A J d, A the product of the
    rotation steps f + 1 .. s and J the left Jacobian of step f"""
    from ..engine.frames import quat_exp
    from ..engine.gripper_single import quat_to_rotmat
    T, nf = frame_grad.shape[:2]
    out = np.zeros_like(frame_grad)
    for j in range(nf):
        for f in range(1, T):
            A = np.eye(3)
            acc = np.zeros(3)
            for s in range(f, T):
                if s > f:
                    A = quat_to_rotmat(quat_exp(delta_theta[s, j])) @ A
                out[f, j, :3] += frame_grad[s, j, :3]
                acc += A.T @ frame_grad[s, j, 3:]
            out[f, j, 3:] = left_jacobian(delta_theta[f, j]).T @ acc
    return out


def optimise(N=8, T=4, iters=3, k=2000.0, shift=1e-3, lr=1e-4, stvk=(3.0e5, 2.0e5), device="cuda:0", log=print):
    """returns (losses per iteration, steps (T, 1, 6): delta_pos in m and delta_theta in rad of every time step; row 0 is not used).  Adam moves a
    position step by about lr metres per iteration, and a rotation step by the angle that moves the far end of the clamp as much."""
    from ..engine.analytic_grad_single import Grad
    from ..optimizer.optim import Adam_single
    from ..task_scene.Scene_drape import Scene

    sys = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, Kb=0.0, pin_row=False, perturb=0.0, device=device)
    c = sys.cloths[0]
    c.stvk_mu[None], c.stvk_lam[None] = stvk   # the StVK membrane: its matrix is the exact second derivative, so the reverse sweep is exact too
    c.membrane[None] = 1.0
    sys.init_all()
    x0 = sys.pos.to_numpy()
    held = np.arange(c.offset + c.N * (c.M + 1), c.offset + (c.N + 1) * (c.M + 1))   # the clamp: grid row i = N, M + 1 vertices on one frame
    edge = np.arange(c.offset, c.offset + c.M + 1)                                   # the opposite edge: grid row i = 0
    u = x0[edge[-1]] - x0[edge[0]]
    width = float(np.linalg.norm(u))
    u /= width
    n = x0[held].mean(0) - x0[edge].mean(0)
    q = x0[edge[0]] + shift * n / np.linalg.norm(n)            # the goal: the edge's own line, moved in the plane towards the clamp
    sys.set_handles(held, k)
    sys.set_handle_frames(np.zeros(len(held), np.int32), n_frames=1)
    pose0 = (x0[held].mean(0)[None], np.array([[1.0, 0.0, 0.0, 0.0]]))   # the frame at the middle of the clamp, axes along the world's
    sys.set_frame_poses(*pose0)
    sys.set_handle_frames(np.zeros(len(held), np.int32))                 # grasp the edge where it is: r_i = R^T (x_i - c)
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
        log(f"iter {it}: loss {loss:.6e}  max |d loss / d step| {np.abs(g).max():.3e}  clamp force {np.linalg.norm(wrench[:3]):.3e} N  "
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
