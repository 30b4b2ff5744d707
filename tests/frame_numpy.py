"""NumPy restatement of rigid frames for soft handles (csrc/k_frame.hpp): handle i of frame f_i has the local point r_i, frame j the
pose (c_j, q_j) with q = (s, x, y, z), and the target of a framed handle is t_i = c_j + R(q_j) r_i; f_i = -1 is a free handle whose world target
stays what it was.  The handle term itself is tests/handle_numpy.py, which reads the targets."""
import numpy as np


def rotmat(q):
    """R of the unit quaternion q / |q| (the formula of engine/gripper_single.quat_to_rotmat, written out again)"""
    s, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def rotvec_matrix(theta):
    """exp([theta]x) by Rodrigues' formula"""
    theta = np.asarray(theta, dtype=np.float64)
    phi = np.linalg.norm(theta)
    if phi == 0.0:
        return np.eye(3)
    a = theta / phi
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(phi) * K + (1.0 - np.cos(phi)) * (K @ K)


def targets(t_world, frame_of, local, pos, quat, Rs=None):
    """(n, 3): rows of framed handles c + R r, rows of free handles as in t_world.  Rs: rotation matrices to use instead of rotmat(quat[j])"""
    t = np.array(t_world, dtype=np.float64)
    for j in range(len(pos)):
        m = np.asarray(frame_of) == j
        R = rotmat(quat[j]) if Rs is None else Rs[j]
        t[m] = pos[j] + np.asarray(local)[m] @ R.T
    return t


def reduce_rows(rows, arms, frame_of, n_frame):
    """(n_frame, 6): (sum_i rows_i, sum_i arms_i x rows_i) over the handles of every frame; also the sum of the absolute values of the terms"""
    out, mag = np.zeros((n_frame, 6)), np.zeros((n_frame, 6))
    for j in range(n_frame):
        m = np.asarray(frame_of) == j
        a, f = arms[m], rows[m]
        out[j, :3] = f.sum(0)
        out[j, 3:] = np.cross(a, f).sum(0)
        mag[j, :3] = np.abs(f).sum(0)
        mag[j, 3] = (np.abs(a[:, 1] * f[:, 2]) + np.abs(a[:, 2] * f[:, 1])).sum()
        mag[j, 4] = (np.abs(a[:, 2] * f[:, 0]) + np.abs(a[:, 0] * f[:, 2])).sum()
        mag[j, 5] = (np.abs(a[:, 0] * f[:, 1]) + np.abs(a[:, 1] * f[:, 0])).sum()
    return out, mag


def wrench(force_rows, t, frame_of, pos):
    """force and moment about c_j of frame j's handles: force_rows are the rows k w_i (t_i - x_{v_i}) (handle_numpy.force), arms t_i - c_j"""
    f = np.asarray(frame_of)
    arms = t - np.asarray(pos)[np.maximum(f, 0)]
    return reduce_rows(force_rows, arms, f, len(pos))


def pose_grad(target_rows, frame_of, local, quat, n_frame, Rs=None):
    """chain rule from rows g_i = d(loss)/d(t_i) to (d/dc_j, d/dtheta_j), theta_j a world rotation vector applied on the left (R <- exp([theta]x) R):
    d t_i = d c + d theta x (R r_i), so the rows reduce with the arms R r_i"""
    f = np.asarray(frame_of)
    arms = np.zeros((len(f), 3))
    for j in range(n_frame):
        R = rotmat(quat[j]) if Rs is None else Rs[j]
        arms[f == j] = np.asarray(local)[f == j] @ R.T
    return reduce_rows(target_rows, arms, f, n_frame)
