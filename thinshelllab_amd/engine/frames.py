"""Rigid frames for soft handles (BaseScene.set_handle_frames): the host side in NumPy -- quaternion algebra in the convention of
``gripper_single.quat_to_rotmat`` (q = (s, x, y, z), R(q) for a unit q), the checks of ``tsl_set_handle_frames`` / ``tsl_set_frame_poses`` with the
library's messages, and the targets t_i = c + R r_i in the order of additions of ``k_frame_targets``."""
import math

import numpy as np

from .gripper_single import quat_to_rotmat


def quat_normalize(q):
    """q / |q|, the norm added in the order of the library (frame_host.hpp)"""
    q = np.asarray(q, dtype=np.float64)
    s, x, y, z = (float(a) for a in q)
    return q / math.sqrt(((s * s + x * x) + y * y) + z * z)


def quat_mul(a, b):
    """Hamilton product a (x) b: R(a (x) b) = R(a) R(b)"""
    s1, x1, y1, z1 = a
    s2, x2, y2, z2 = b
    return np.array([s1 * s2 - x1 * x2 - y1 * y2 - z1 * z2,
                     s1 * x2 + x1 * s2 + y1 * z2 - z1 * y2,
                     s1 * y2 - x1 * z2 + y1 * s2 + z1 * x2,
                     s1 * z2 + x1 * y2 - y1 * x2 + z1 * s2])


def quat_exp(theta):
    """the unit quaternion exp(theta / 2) of the rotation vector theta: R = exp([theta]x); exact at theta = 0 (sin(a) / a through np.sinc)"""
    theta = np.asarray(theta, dtype=np.float64)
    half = 0.5 * float(np.linalg.norm(theta))
    return np.concatenate([[math.cos(half)], 0.5 * float(np.sinc(half / math.pi)) * theta])


def compose(pos, quat, delta_pos, delta_theta):
    """(pos + delta_pos, exp(delta_theta / 2) (x) quat renormalised) per frame: the world-frame rotation vector applied on the left, R <- exp([d theta]x) R"""
    pos = np.asarray(pos, dtype=np.float64) + np.asarray(delta_pos, dtype=np.float64)
    quat = np.array([quat_normalize(quat_mul(quat_exp(dt), q)) for dt, q in zip(np.asarray(delta_theta, dtype=np.float64), quat)]).reshape(-1, 4)
    return pos, quat


def validate_frames(n_handle, frame_ids, local_points, n_frames):
    """The checks of tsl_set_handle_frames on the host, with its messages: returns (int32 frame ids, float64 local points) or raises ValueError naming
    the offender -- frames without handles, a frame index outside [-1, n_frames), a non-finite local point of a framed handle."""
    f = np.asarray(frame_ids)
    if f.ndim != 1 or (f.size and not np.issubdtype(f.dtype, np.integer)):
        raise ValueError(f"set_handle_frames: frame ids must be a flat list of integers (got shape {f.shape}, dtype {f.dtype})")
    n_frames = int(n_frames)
    if n_frames < 0:
        raise ValueError(f"set_handle_frames: n_frame = {n_frames} is negative")
    if n_frames == 0:   # (removes all frames: no list is read)
        return np.zeros(0, np.int32), np.zeros((0, 3))
    if n_handle == 0:
        raise ValueError(f"set_handle_frames: {n_frames} frames asked for, but there are no handles (tsl_set_handles comes first)")
    if len(f) != n_handle:
        raise ValueError(f"set_handle_frames: {len(f)} frame ids for {n_handle} handles")
    r = np.asarray(local_points, dtype=np.float64)
    if r.shape != (n_handle, 3):
        raise ValueError(f"set_handle_frames: local points of shape {r.shape} for {n_handle} handles (expected ({n_handle}, 3))")
    for i, fi in enumerate(f.tolist()):
        if fi < -1 or fi >= n_frames:
            raise ValueError(f"set_handle_frames: frame index {fi} of handle {i} outside [-1, {n_frames})")
        if fi >= 0 and not np.isfinite(r[i]).all():
            raise ValueError(f"set_handle_frames: local point ({r[i, 0]:g}, {r[i, 1]:g}, {r[i, 2]:g}) of handle {i} (frame {fi}) is not finite")
    return f.astype(np.int32), r.copy()


def validate_poses(n_frame, pos, quat):
    """The checks of tsl_set_frame_poses on the host, with its messages: returns (positions (n_frame, 3), unit quaternions (n_frame, 4))"""
    c = np.array(pos, dtype=np.float64)
    q = np.array(quat, dtype=np.float64)
    if c.shape != (n_frame, 3) or q.shape != (n_frame, 4):
        raise ValueError(f"set_frame_poses: positions of shape {c.shape} and quaternions of shape {q.shape} for {n_frame} frames "
                         f"(expected ({n_frame}, 3) and ({n_frame}, 4))")
    for j in range(n_frame):
        if not np.isfinite(c[j]).all():
            raise ValueError(f"set_frame_poses: position ({c[j, 0]:g}, {c[j, 1]:g}, {c[j, 2]:g}) of frame {j} is not finite")
        n = math.sqrt(float(q[j] @ q[j])) if np.isfinite(q[j]).all() else float("nan")
        if not (n > 0.0 and math.isfinite(n)):
            raise ValueError(f"set_frame_poses: quaternion ({q[j, 0]:g}, {q[j, 1]:g}, {q[j, 2]:g}, {q[j, 3]:g}) of frame {j} is zero or not finite")
        q[j] = quat_normalize(q[j])
    return c, q


def frame_targets(targets, frame_of, local, pos, quat):
    """the targets with the rows of framed handles rewritten: t_i = c + R r_i, the three products added left to right, then c (k_frame_targets)"""
    t = np.array(targets, dtype=np.float64)
    for j in range(len(pos)):
        R = quat_to_rotmat(quat[j])
        m = np.asarray(frame_of) == j
        r = np.asarray(local)[m]
        t[m] = pos[j] + ((R[:, 0] * r[:, :1] + R[:, 1] * r[:, 1:2]) + R[:, 2] * r[:, 2:3])
    return t
