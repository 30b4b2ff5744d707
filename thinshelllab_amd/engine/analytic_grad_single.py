"""Trajectory adjoint: host-side counterpart of ``Grad``
(/root/reference/code/engine/analytic_grad_single.py).

The tape (``pos_buffer``, ``ref_angle_buffer``) and the gradient buffers live in HBM; one reverse step
(``transfer_grad``, :217-257) is a single ``tsl_adjoint_step`` call -- contact re-detection, the un-projected
Hessian, one linear solve, the frozen-dof coupling and the three back-propagation kernels -- followed by the
(tiny) gripper reduction on the host (``get_gripper_grad``, :118-139).
"""
import numpy as np
import torch

from .field import Field


# ---- soft handles on the tape (BaseScene.set_handles; shared with analytic_grad_system.Grad and SceneGroup.transfer_grad)
def handle_tape_init(grad, sys, T):
    """handle_targets / handle_grad (T, n, 3) when the scene has handles, frame_pos / frame_quat / frame_grad (T, n_frame, 3 / 4 / 6) when it has
    frames; nothing otherwise"""
    grad.n_handle = getattr(sys, "n_handle", 0)
    if grad.n_handle:
        grad.handle_targets = Field(torch.zeros((T, grad.n_handle, 3), dtype=torch.float64))
        grad.handle_grad = Field(torch.zeros((T, grad.n_handle, 3), dtype=torch.float64))
    # rigid frames of the handles (BaseScene.set_handle_frames): the poses of every step and d(loss)/d(position, world rotation vector on the left)
    grad.n_frame = getattr(sys, "n_frame", 0)
    if grad.n_frame:
        grad.frame_pos = Field(torch.zeros((T, grad.n_frame, 3), dtype=torch.float64))
        grad.frame_quat = Field(torch.zeros((T, grad.n_frame, 4), dtype=torch.float64))
        grad.frame_grad = Field(torch.zeros((T, grad.n_frame, 6), dtype=torch.float64))
    # ties (BaseScene.set_ties): d(loss)/d(weight of tie i) per reverse step
    grad.n_tie = getattr(sys, "n_tie", 0)
    if grad.n_tie:
        grad.tie_grad = Field(torch.zeros((T, grad.n_tie), dtype=torch.float64))
    # half-space colliders (BaseScene.set_colliders): the offsets of every step and d(loss)/d(offset, mu) per reverse step
    grad.n_collider = getattr(sys, "n_collider", 0)
    if grad.n_collider:
        grad.collider_offsets = Field(torch.zeros((T, grad.n_collider), dtype=torch.float64))
        grad.collider_grad = Field(torch.zeros((T, grad.n_collider, 2), dtype=torch.float64))
    # sphere colliders (BaseScene.set_spheres): the centres and previous centres of every step and d(loss)/d(c, cp, mu, R) per reverse step
    grad.n_sphere = getattr(sys, "n_sphere", 0)
    if grad.n_sphere:
        grad.sphere_centres = Field(torch.zeros((T, grad.n_sphere, 3), dtype=torch.float64))
        grad.sphere_centres_prev = Field(torch.zeros((T, grad.n_sphere, 3), dtype=torch.float64))
        grad.sphere_grad = Field(torch.zeros((T, grad.n_sphere, 8), dtype=torch.float64))
    # capsule colliders (BaseScene.set_capsules): the endpoints (a, b) and previous endpoints of every step and d(loss)/d(a, b, ap, bp, mu, R) per reverse step
    grad.n_capsule = getattr(sys, "n_capsule", 0)
    if grad.n_capsule:
        grad.capsule_ends = Field(torch.zeros((T, grad.n_capsule, 2, 3), dtype=torch.float64))
        grad.capsule_ends_prev = Field(torch.zeros((T, grad.n_capsule, 2, 3), dtype=torch.float64))
        grad.capsule_grad = Field(torch.zeros((T, grad.n_capsule, 14), dtype=torch.float64))
    # rounded-box colliders (BaseScene.set_boxes): the poses (centre (3), unit quaternion (4)) and previous poses of every step and
    # d(loss)/d(c, theta, cp, theta_p, mu, r) per reverse step
    grad.n_box = getattr(sys, "n_box", 0)
    if grad.n_box:
        grad.box_poses = Field(torch.zeros((T, grad.n_box, 7), dtype=torch.float64))
        grad.box_poses_prev = Field(torch.zeros((T, grad.n_box, 7), dtype=torch.float64))
        grad.box_grad = Field(torch.zeros((T, grad.n_box, 14), dtype=torch.float64))
    # sampled distance-field colliders (BaseScene.set_sdfs): the poses (centre (3), unit quaternion (4)) and previous poses of every step and
    # d(loss)/d(c, theta, cp, theta_p, mu, offset) per reverse step
    grad.n_sdf = getattr(sys, "n_sdf", 0)
    if grad.n_sdf:
        grad.sdf_poses = Field(torch.zeros((T, grad.n_sdf, 7), dtype=torch.float64))
        grad.sdf_poses_prev = Field(torch.zeros((T, grad.n_sdf, 7), dtype=torch.float64))
        grad.sdf_grad = Field(torch.zeros((T, grad.n_sdf, 14), dtype=torch.float64))
    # wind (BaseScene.set_wind): the wind velocity of every step and d(loss)/d(W of the step, c_n, c_t) per reverse step
    grad.n_wind = getattr(sys, "n_wind", 0)
    if grad.n_wind:
        grad.wind_velocity = Field(torch.zeros((T, 3), dtype=torch.float64))
        grad.wind_grad = Field(torch.zeros((T, 5), dtype=torch.float64))


def wind_velocity_grad(grad):
    """(T, 3) d(loss)/d(wind velocity trajectory): row s is wind_grad[s, 0:3] (the columns 3 and 4 are the step's shares of d(loss)/d(c_n), d(loss)/d(c_t))"""
    if not grad.n_wind:
        raise ValueError("wind_velocity_grad: the scene has no wind")
    return grad.wind_grad.t[:, 0:3].clone()


def sdf_pose_grad(grad):
    """(T, n, 6) d(loss)/d(pose trajectory of the sampled fields) -- [0:3] the centre, [3:6] a world-frame rotation vector applied on the left of the
    step's orientation -- when each step's previous pose was the pose of the step before: row s is sdf_grad[s, :, 0:6] + sdf_grad[s + 1, :, 6:12].
    Raises if the tape shows another trajectory."""
    if not grad.n_sdf:
        raise ValueError("sdf_pose_grad: the scene has no fields")
    e, ep, g = grad.sdf_poses.t, grad.sdf_poses_prev.t, grad.sdf_grad.t
    if not torch.equal(ep[1:], e[:-1]):
        s = int((ep[1:] != e[:-1]).reshape(len(e) - 1, -1).any(dim=1).nonzero()[0, 0]) + 1
        raise ValueError(f"sdf_pose_grad: the previous poses of step {s} are not the poses of step {s - 1}")
    out = g[:, :, 0:6].clone()
    out[:-1] += g[1:, :, 6:12]
    return out


def box_pose_grad(grad):
    """(T, n, 6) d(loss)/d(pose trajectory) -- [0:3] the centre, [3:6] a world-frame rotation vector applied on the left of the step's orientation --
    when each step's previous pose was the pose of the step before: row s is box_grad[s, :, 0:6] + box_grad[s + 1, :, 6:12].  Raises if the tape
    shows another trajectory."""
    if not grad.n_box:
        raise ValueError("box_pose_grad: the scene has no boxes")
    e, ep, g = grad.box_poses.t, grad.box_poses_prev.t, grad.box_grad.t
    if not torch.equal(ep[1:], e[:-1]):
        s = int((ep[1:] != e[:-1]).reshape(len(e) - 1, -1).any(dim=1).nonzero()[0, 0]) + 1
        raise ValueError(f"box_pose_grad: the previous poses of step {s} are not the poses of step {s - 1}")
    out = g[:, :, 0:6].clone()
    out[:-1] += g[1:, :, 6:12]
    return out


def capsule_end_grad(grad):
    """(T, n, 2, 3) d(loss)/d(endpoint trajectory) when each step's previous endpoints were the endpoints of the step before: row s is
    capsule_grad[s, :, 0:6] + capsule_grad[s + 1, :, 6:12].  Raises if the tape shows another trajectory."""
    if not grad.n_capsule:
        raise ValueError("capsule_end_grad: the scene has no capsules")
    e, ep, g = grad.capsule_ends.t, grad.capsule_ends_prev.t, grad.capsule_grad.t
    if not torch.equal(ep[1:], e[:-1]):
        s = int((ep[1:] != e[:-1]).reshape(len(e) - 1, -1).any(dim=1).nonzero()[0, 0]) + 1
        raise ValueError(f"capsule_end_grad: the previous endpoints of step {s} are not the endpoints of step {s - 1}")
    out = g[:, :, 0:6].clone()
    out[:-1] += g[1:, :, 6:12]
    return out.reshape(len(g), -1, 2, 3)


def sphere_centre_grad(grad):
    """(T, n, 3) d(loss)/d(centre trajectory) when each step's previous centre was the centre of the step before: row s is
    sphere_grad[s, :, 0:3] + sphere_grad[s + 1, :, 3:6].  Raises if the tape shows another trajectory."""
    if not grad.n_sphere:
        raise ValueError("sphere_centre_grad: the scene has no spheres")
    c, cp, g = grad.sphere_centres.t, grad.sphere_centres_prev.t, grad.sphere_grad.t
    if not torch.equal(cp[1:], c[:-1]):
        s = int((cp[1:] != c[:-1]).reshape(len(c) - 1, -1).any(dim=1).nonzero()[0, 0]) + 1
        raise ValueError(f"sphere_centre_grad: the previous centres of step {s} are not the centres of step {s - 1}")
    out = g[:, :, 0:3].clone()
    out[:-1] += g[1:, :, 3:6]
    return out


def handle_tape_reset(grad):
    if grad.n_wind:
        grad.wind_velocity.fill(0)
        grad.wind_grad.fill(0)
    if grad.n_tie:
        grad.tie_grad.fill(0)
    if grad.n_collider:
        grad.collider_offsets.fill(0)
        grad.collider_grad.fill(0)
    if grad.n_sphere:
        grad.sphere_centres.fill(0)
        grad.sphere_centres_prev.fill(0)
        grad.sphere_grad.fill(0)
    if grad.n_capsule:
        grad.capsule_ends.fill(0)
        grad.capsule_ends_prev.fill(0)
        grad.capsule_grad.fill(0)
    if grad.n_box:
        grad.box_poses.fill(0)
        grad.box_poses_prev.fill(0)
        grad.box_grad.fill(0)
    if grad.n_sdf:
        grad.sdf_poses.fill(0)
        grad.sdf_poses_prev.fill(0)
        grad.sdf_grad.fill(0)
    if grad.n_handle:
        grad.handle_targets.fill(0)
        grad.handle_grad.fill(0)
    if grad.n_frame:
        grad.frame_pos.fill(0)
        grad.frame_quat.fill(0)
        grad.frame_grad.fill(0)


def handle_tape_record(grad, sys, step):
    """the targets (framed rows at c + R r) and the frame poses of step `step` onto the tape"""
    if grad.n_handle:
        grad.handle_targets.t[step] = torch.as_tensor(sys._handle_t)
    if grad.n_frame:
        grad.frame_pos.t[step] = torch.as_tensor(sys._frame_pos)
        grad.frame_quat.t[step] = torch.as_tensor(sys._frame_quat)
    if grad.n_collider:
        grad.collider_offsets.t[step] = torch.as_tensor(sys._col_o)
    if grad.n_wind:   # the wind velocity of the step just completed
        grad.wind_velocity.t[step] = torch.as_tensor(sys._wind_W)
    if grad.n_sphere:   # the step just completed: its centres, and where the balls were when it started
        grad.sphere_centres.t[step] = torch.as_tensor(sys._sph_cp)
        grad.sphere_centres_prev.t[step] = torch.as_tensor(sys._sph_cp_step)
    if grad.n_capsule:   # likewise: the endpoints of the step just completed, and where the rods were when it started
        grad.capsule_ends.t[step] = torch.as_tensor(sys._cap_ep)
        grad.capsule_ends_prev.t[step] = torch.as_tensor(sys._cap_ep_step)
    if grad.n_box:   # likewise: the poses of the step just completed, and where the boxes were when it started
        grad.box_poses.t[step] = torch.as_tensor(np.concatenate([sys._box_cp, sys._box_qp], axis=1))
        grad.box_poses_prev.t[step] = torch.as_tensor(np.concatenate([sys._box_cp_step, sys._box_qp_step], axis=1))
    if grad.n_sdf:   # likewise for the sampled fields
        grad.sdf_poses.t[step] = torch.as_tensor(np.concatenate([sys._sdf_cp, sys._sdf_qp], axis=1))
        grad.sdf_poses_prev.t[step] = torch.as_tensor(np.concatenate([sys._sdf_cp_step, sys._sdf_qp_step], axis=1))


def handle_tape_push(grad, sys, step):
    """the targets and the frame poses of step `step` back into the scene: the reverse step re-assembles at x_step and reads them"""
    # (with every handle on a frame the poses say it all: 7 numbers per frame go to the device, not n x 3 rows)
    if grad.n_handle and not (grad.n_frame and (sys._frame_of >= 0).all()):
        sys.set_handle_targets(grad.handle_targets.t[step].numpy())
    if grad.n_frame:
        sys.set_frame_poses(grad.frame_pos.t[step].numpy(), grad.frame_quat.t[step].numpy())
    if grad.n_collider:   # the offsets of step `step`: the reverse step evaluates d, d0 and the blocks with them
        sys.set_collider_offsets(grad.collider_offsets.t[step].numpy())
    if grad.n_wind:   # the wind velocity of step `step`: the reverse step evaluates r with it
        sys.set_wind_velocity(grad.wind_velocity.t[step].numpy())
    if grad.n_sphere:   # the centres and previous centres of step `step`: the reverse step evaluates the contact frame with them
        sys.set_sphere_centres(grad.sphere_centres.t[step].numpy(), grad.sphere_centres_prev.t[step].numpy())
    if grad.n_capsule:   # the endpoints and previous endpoints of step `step`: the reverse step evaluates t0, the contact frame and the slip with them
        e, ep = grad.capsule_ends.t[step].numpy(), grad.capsule_ends_prev.t[step].numpy()
        sys.set_capsule_ends(e[:, 0], e[:, 1], ep[:, 0], ep[:, 1])
    if grad.n_box:   # the poses and previous poses of step `step`: the reverse step evaluates b0, the contact frame and the slip with them
        e, ep = grad.box_poses.t[step].numpy(), grad.box_poses_prev.t[step].numpy()
        sys.set_box_poses(e[:, 0:3], e[:, 3:7], ep[:, 0:3], ep[:, 3:7])
    if grad.n_sdf:   # the poses and previous poses of step `step`: the reverse step evaluates y0, the contact frame and the slip with them
        e, ep = grad.sdf_poses.t[step].numpy(), grad.sdf_poses_prev.t[step].numpy()
        sys.set_sdf_poses(e[:, 0:3], e[:, 3:7], ep[:, 0:3], ep[:, 3:7])


def handle_tape_pull(grad, ctx, step):
    """handle_grad[step] += d(loss)/d(targets of step `step`) of the reverse step just taken, frame_grad[step] += the same reduced to the frames"""
    if grad.n_handle:
        grad.handle_grad.t[step] += torch.as_tensor(ctx.handle_grad())
    if grad.n_frame:
        grad.frame_grad.t[step] += torch.as_tensor(ctx.frame_grad())
    if grad.n_tie:   # tie_grad[step] += d(loss)/d(tie weights) of the reverse step just taken, at the tape state x_step
        grad.tie_grad.t[step] += torch.as_tensor(ctx.tie_grad(grad.pos_buffer.t[step]))
    if grad.n_collider:   # collider_grad[step] += d(loss)/d(offsets of step `step`, mu) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.collider_grad.t[step] += torch.as_tensor(ctx.collider_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))
    if grad.n_wind:   # wind_grad[step] += d(loss)/d(W of step `step`, c_n, c_t) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.wind_grad.t[step] += torch.as_tensor(ctx.wind_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))
    if grad.n_sphere:   # sphere_grad[step] += d(loss)/d(c, cp of step `step`, mu, R) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.sphere_grad.t[step] += torch.as_tensor(ctx.sphere_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))
    if grad.n_capsule:   # capsule_grad[step] += d(loss)/d(a, b, ap, bp of step `step`, mu, R) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.capsule_grad.t[step] += torch.as_tensor(ctx.capsule_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))
    if grad.n_box:   # box_grad[step] += d(loss)/d(c, theta, cp, theta_p of step `step`, mu, r) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.box_grad.t[step] += torch.as_tensor(ctx.box_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))
    if grad.n_sdf:   # sdf_grad[step] += d(loss)/d(c, theta, cp, theta_p of step `step`, mu, offset) of the reverse step just taken, at the tape state (x_step, x_{step-1})
        grad.sdf_grad.t[step] += torch.as_tensor(ctx.sdf_grad(grad.pos_buffer.t[step], grad.pos_buffer.t[step - 1]))


class Grad:
    def __init__(self, sys, tot_timestep, n_parts, friction_loss=False, f_loss_ratio=0.001, vertical_only=False):
        # analytic_grad_single.py:5-26
        self.n_part = n_parts
        self.tot_NV = sys.tot_NV
        dev = sys.device
        T = tot_timestep
        z = lambda *shape: Field(torch.zeros(shape, dtype=torch.float64, device=dev))
        self.pos_buffer = z(T, sys.tot_NV, 3)
        self.gripper_pos_buffer = Field(torch.zeros((T, max(n_parts, 1), 3), dtype=torch.float64))
        self.gripper_rot_buffer = Field(torch.zeros((T, max(n_parts, 1), 4), dtype=torch.float64))
        self.cloth_cnt = sys.cloth_cnt
        self.NF = sys.cloths[0].NF
        self.ref_angle_buffer = z(T, sys.cloth_cnt, self.NF, 3)
        self.dt = sys.dt
        self.pos_grad = z(T, sys.tot_NV, 3)
        self.x_hat_grad = z(sys.tot_NV * 3)
        self.gripper_grad = Field(torch.zeros((T, max(n_parts, 1), 6), dtype=torch.float64))
        self.angleref_grad = z(T, sys.cloth_cnt, self.NF, 3)
        self.mass = Field(torch.zeros(sys.tot_NV, dtype=torch.float64))
        self.tot_timestep = T
        self.damping = 1.0
        self.friction_loss = friction_loss
        self.f_loss_ratio = f_loss_ratio
        self.vertical_only = vertical_only
        self.last_stats = {}
        # keys of tsl_param_grad_keys (e.g. "k_tie", "k_handle"): every reverse step adds their contribution to grad_params, as analytic_grad_system.Grad does
        self.param_keys = []
        self.grad_params = {}
        handle_tape_init(self, sys, T)

    def reset(self):
        self.pos_buffer.fill(0)
        self.pos_grad.fill(0)
        self.angleref_grad.fill(0)
        self.grad_params = {}
        handle_tape_reset(self)

    def init_mass(self, sys):
        self.mass.copy_from(sys.mass)

    def wind_velocity_grad(self):
        """(T, 3) d(loss)/d(wind velocity of every step) = wind_grad[:, 0:3]"""
        return wind_velocity_grad(self)

    def sphere_centre_grad(self):
        """(T, n, 3) d(loss)/d(centre trajectory of the spheres); raises if a step's previous centres were not the centres of the step before"""
        return sphere_centre_grad(self)

    def capsule_end_grad(self):
        """(T, n, 2, 3) d(loss)/d(endpoint trajectory of the capsules); raises if a step's previous endpoints were not the endpoints of the step before"""
        return capsule_end_grad(self)

    def box_pose_grad(self):
        """(T, n, 6) d(loss)/d(pose trajectory of the boxes: centre, world-frame rotation vector); raises if a step's previous poses were not the poses of
        the step before"""
        return box_pose_grad(self)

    def sdf_pose_grad(self):
        """(T, n, 6) d(loss)/d(pose trajectory of the sampled fields: centre, world-frame rotation vector); raises if a step's previous poses were not
        the poses of the step before"""
        return sdf_pose_grad(self)

    # :37-51
    def copy_pos(self, sys, step):
        self.pos_buffer.t[step].copy_(sys.pos.t)
        self.ref_angle_buffer.t[step].view(-1, 3).copy_(sys._ref_angle[: self.cloth_cnt * self.NF])
        handle_tape_record(self, sys, step)
        if self.n_part > 0 and hasattr(sys, "gripper"):
            self.gripper_pos_buffer.t[step].copy_(sys.gripper.pos.t)
            self.gripper_rot_buffer.t[step].copy_(sys.gripper.rot.t)

    # :176-185
    def clamp_grad(self, step):
        self.pos_grad.t[step].clamp_(-1000, 1000)
        self.angleref_grad.t[step].clamp_(-1000, 1000)

    # :118-139
    def get_gripper_grad(self, step, sys):
        sys.gripper.get_rotmat()
        sys.gripper.gather_grad(sys.tmp_z_frozen, sys)
        dp = sys.gripper.d_pos.to_numpy(); da = sys.gripper.d_angle.to_numpy()
        g = self.gripper_grad.t
        for j in range(self.n_part):
            if self.vertical_only:
                g[step, j, 2] = float(dp[j][2])
            else:
                g[step, j, 0:3] = torch.as_tensor(dp[j]); g[step, j, 3:6] = torch.as_tensor(da[j])

    # :217-257
    def transfer_grad(self, step, sys, f_contact):
        handle_tape_push(self, sys, step)
        ctx = sys._ensure_ctx()
        ctx.set_param("contact", 0.0 if f_contact is None else 1.0)
        self.last_stats = ctx.adjoint_step(step, self.tot_timestep, self.pos_buffer.t, self.pos_grad.t, self.ref_angle_buffer.t, self.angleref_grad.t,
                                           sys.tmp_z_frozen.t, self.damping)
        self.check_solve(step)
        handle_tape_pull(self, ctx, step)
        if self.param_keys:
            for k, v in ctx.param_grads(self.pos_buffer.t[step], self.ref_angle_buffer.t[step - 1], self.param_keys).items():
                self.grad_params[k] = self.grad_params.get(k, 0.0) + v
        # leave the scene in the state the reference leaves it in (copy_pos_and_refangle + gripper.set)
        sys.copy_pos_and_refangle(self, step)
        if self.n_part > 0 and hasattr(sys, "gripper"):
            sys.gripper.set(self.gripper_pos_buffer, self.gripper_rot_buffer, step)
            if step > 0:
                self.get_gripper_grad(step, sys)

    def check_solve(self, step):
        """The reference's H.solve is an exact sparse solve (sparse_solver.py:85-105); an adjoint solve that did NOT converge would
        silently corrupt pos_grad / gripper_grad of every earlier step, so it raises (set ``allow_unconverged`` to collect instead)."""
        st = self.last_stats
        self.worst_rel_residual = max(getattr(self, "worst_rel_residual", 0.0), st["rel_residual"])
        if st["flag"] == 3:
            self.unconverged = getattr(self, "unconverged", 0) + 1
            if not getattr(self, "allow_unconverged", False):
                from .._lib import TslError
                raise TslError(f"transfer_grad(step {step}): linear solve not converged (rel_residual {st['rel_residual']:.3e} after {st['iters']} iterations, "
                               f"method {st['method']}); the gradients of earlier steps would be wrong")

    # ---- loss seeds
    def get_loss(self, sys):  # :259-263
        self.pos_grad.t[:, : sys.cloths[0].NV, 0] = -1

    def get_loss_sheet(self, sys):  # :265-269
        self.pos_grad.t[1:, : sys.cloths[0].NV, 0] = 1

    def get_loss_book(self, sys):  # :274-278
        self.pos_grad.t[1:, : sys.cloths[0].NV, 0] = -1

    def _fold_rows(self, sys, row_a, row_b):
        """hinges (f, l) of cloth 0 whose own wing lies on grid row ``row_a`` and the opposite wing on ``row_b``"""
        c = sys.cloths[0]
        f2v = c.f2v.to_numpy(); cf = c.counter_face.to_numpy(); cp = c.counter_point.to_numpy()
        fi, l = np.nonzero(cf > np.arange(c.NF)[:, None])
        p1 = f2v[fi, l]
        p2 = f2v[cf[fi, l], cp[fi, l]]
        m = (p1 // (c.M + 1) == row_a) & (p2 // (c.M + 1) == row_b)
        return fi[m], l[m]

    def get_loss_fold(self, sys, curve7, curve8, rows=((6, 8), (7, 9))):  # :280-294
        ag = self.angleref_grad.t
        for (ra, rb), val in zip(rows, (curve7, curve8)):
            fi, l = self._fold_rows(sys, ra, rb)
            ag[self.tot_timestep - 1, 0, torch.as_tensor(fi), torch.as_tensor(l)] = val

    def get_loss_interact(self, sys):  # :408-420
        c = sys.cloths[0]; e = sys.elastics[3]
        j = self.tot_timestep - 1
        self.pos_grad.t[j, c.offset:c.offset + c.NV, 0] = 1
        self.pos_grad.t[j, e.offset:e.offset + e.n_verts, 0] = -1 * 256.0 / 144.0

    def get_loss_interact_1(self, sys):  # :422-426
        e = sys.elastics[3]
        self.pos_grad.t[self.tot_timestep - 1, e.offset:e.offset + e.n_verts, 0] = 1

    def get_loss_pick(self, sys):  # :323-327
        c = sys.cloths[0]
        sel = c.offset + np.nonzero(np.arange(c.NV) // (c.M + 1) == 8)[0]
        self.pos_grad.t[:, torch.as_tensor(sel), 2] = -1

    def get_loss_pick_fold(self, sys):  # :373-382
        fi, l = self._fold_rows(sys, 7, 9)
        self.angleref_grad.t[:, 0, torch.as_tensor(fi), torch.as_tensor(l)] = -1

    def get_loss_push(self, sys, target_pos):  # :296-300
        c = sys.cloths[0]
        j = self.tot_timestep - 1
        t = torch.as_tensor(np.asarray(target_pos), dtype=torch.float64, device=self.pos_grad.t.device)
        self.pos_grad.t[j, c.offset:c.offset + c.NV] = 2 * (self.pos_buffer.t[j, c.offset:c.offset + c.NV] - t)

    def get_loss_lift(self, sys):  # :302-312
        e = sys.elastics[0]
        j = self.tot_timestep - 1
        sl = slice(e.offset, e.offset + e.n_verts)
        d = self.pos_buffer.t[j, sl] - self.pos_buffer.t[0, sl]
        d[:, 0] += 0.012; d[:, 1] += 0.012
        self.pos_grad.t[j, sl] = d

    def get_loss_balance(self, sys):  # :428-443 (the cloth-centre entry keeps the value of the LAST ball vertex, like the kernel)
        e = sys.elastics[0]
        tt = sys.cloths[0].offset + (sys.cloth_N + 1) // 2 * (sys.cloth_M + 1) + (sys.cloth_M + 1) // 2
        pb = self.pos_buffer.t
        sl = slice(e.offset, e.offset + e.n_verts)
        d = 2 * (pb[1:, sl, 0:2] - pb[1:, tt:tt + 1, 0:2])
        self.pos_grad.t[1:, sl, 0:2] = d
        self.pos_grad.t[1:, tt, 0:2] = -d[:, -1, :]

    def get_loss_throwing(self, sys):  # :462-471
        e = sys.elastics[0]; c = sys.cloths[0]
        self.pos_grad.t[1:, e.offset:e.offset + e.n_verts, 2] = -1
        pb = self.pos_buffer.t
        i = torch.arange(sys.cloth_M)
        self.pos_grad.t[1:, c.offset + i, 2] = 20 * pb[1:, c.offset + i, 2]
        k = c.offset + i + sys.cloth_N * (sys.cloth_M + 1)
        self.pos_grad.t[1:, k, 2] = 20 * pb[1:, k, 2]

    # ---- seeds no driver of the reference calls (kept for the surface: analytic_grad_single.py:314-321, 329-371, 384-406, 445-460)
    def get_loss_sep(self, sys):  # :314-321: pull two sheets apart along x, seeds on every tape step
        c0, c1 = sys.cloths[0], sys.cloths[1]
        self.pos_grad.t[:, c0.offset:c0.offset + c0.NV, 0] = 1
        self.pos_grad.t[:, c1.offset:c1.offset + c1.NV, 0] = -1

    def get_loss_bounce(self, sys):  # :329-371: seed on the first grid row at the apex after step 40 (and on the higher of its neighbours)
        c = sys.cloths[0]
        T = self.tot_timestep
        row = slice(c.offset, c.offset + c.M + 1)
        zsum = self.pos_buffer.t[:, row, 2].sum(dim=1).cpu().numpy()
        tt = T - 1
        max_z = -1.0
        for j in range(40, T):
            if zsum[j] > max_z:
                max_z = zsum[j]; tt = j
        pb, pg = self.pos_buffer.t, self.pos_grad.t
        if tt < T - 1:
            k = tt - 1 if zsum[tt - 1] > zsum[tt + 1] else tt + 1
            pg[k, row, 2] = 2 * (pb[k, row, 2] - sys.target)
        pg[tt, row, 2] = 2 * (pb[tt, row, 2] - sys.target)
        return tt

    def get_loss_card(self, sys):  # :384-388 (the same rows as get_loss_pick)
        self.get_loss_pick(sys)

    def get_loss_slide_simple(self, sys):  # :390-393
        c = sys.cloths[0]
        self.pos_grad.t[self.tot_timestep - 1, c.offset:c.offset + c.NV, 0] = 1

    def get_loss_deliver(self, sys):  # :395-406: final cloth pose 1 cm (every axis) beyond the pose of tape step 69
        c = sys.cloths[0]
        j = self.tot_timestep - 1
        sl = slice(c.offset, c.offset + c.NV)
        self.pos_grad.t[j, sl] = 2 * (self.pos_buffer.t[j, sl] - self.pos_buffer.t[69, sl] - 0.01)

    def get_loss_side(self, sys):  # :445-460: get_loss_balance towards the vertex a quarter of the way along the cloth
        e = sys.elastics[0]
        tt = sys.cloths[0].offset + (sys.cloth_N + 1) // 4 * (sys.cloth_M + 1) + (sys.cloth_M + 1) // 2
        pb = self.pos_buffer.t
        sl = slice(e.offset, e.offset + e.n_verts)
        d = 2 * (pb[1:, sl, 0:2] - pb[1:, tt:tt + 1, 0:2])
        self.pos_grad.t[1:, sl, 0:2] = d
        self.pos_grad.t[1:, tt, 0:2] = -d[:, -1, :]

    # :492-516
    def accumulate_gripper_grad(self, traj, max_dist):
        g = self.gripper_grad.t
        for step in range(self.tot_timestep - 2, 1, -1):
            for j in range(self.n_part):
                if traj.calculate_dist(step + 1, max_dist, j) > traj.max_moving_dist - 0.00005:
                    g[step, j] += g[step + 1, j]

    def apply_action_limit_grad(self, traj, max_dist):
        g = self.gripper_grad.t
        tr = traj.traj.t
        for step in range(1, self.tot_timestep):
            for j in range(self.n_part):
                dist = traj.calculate_dist(step, max_dist, j)
                if dist > traj.max_moving_dist:
                    d = (tr[step, j] - tr[step - 1, j]).to(g.dtype)
                    g[step, j, 0:3] += d[0:3] * (dist - traj.max_moving_dist) * 10000000
                    g[step, j, 3:6] += d[3:6] * (dist - traj.max_moving_dist) * 100000
