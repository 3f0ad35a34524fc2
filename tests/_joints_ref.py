"""numpy restatement of the reference's joint-axis arithmetic (compute_joints.py:10-122) for the tests, including
transforms3d's ``aff2axangle`` / ``mat2axangle`` (restated from the published library: eig of R^T with the last
eigenvalue within 1e-5 of 1, the direction-dependent sine and atan2; the 4x4 eig with tolerance 1e-8 and the point
divided by w), and the closed-form screw axis the kernel uses.  Needs neither transforms3d nor pytorch3d."""
import math

import numpy as np


# ---- transforms3d.axangles, restated ---------------------------------------------------------------------------
def mat2axangle(mat, unit_thresh=1e-5):
    M = np.asarray(mat, dtype=np.float64)
    L, W = np.linalg.eig(M.T)
    i = np.where(np.abs(L - 1.0) < unit_thresh)[0]
    if not len(i):
        raise ValueError("no unit eigenvector corresponding to eigenvalue 1")
    direction = np.real(W[:, i[-1]]).squeeze()
    cosa = (np.trace(M) - 1.0) / 2.0
    if abs(direction[2]) > 1e-8:
        sina = (M[1, 0] + (cosa - 1.0) * direction[0] * direction[1]) / direction[2]
    elif abs(direction[1]) > 1e-8:
        sina = (M[0, 2] + (cosa - 1.0) * direction[0] * direction[2]) / direction[1]
    else:
        sina = (M[2, 1] + (cosa - 1.0) * direction[1] * direction[2]) / direction[0]
    angle = math.atan2(sina, cosa)
    return direction, angle


def aff2axangle(aff):
    R = np.asarray(aff)
    direction, angle = mat2axangle(R[:3, :3])
    L, Q = np.linalg.eig(R)
    i = np.where(abs(np.real(L) - 1.0) < 1e-8)[0]
    if not len(i):
        raise ValueError("no unit eigenvector corresponding to eigenvalue 1")
    point = np.real(Q[:, i[-1]]).squeeze()
    point /= point[3]
    return direction, angle, point


# ---- pytorch3d.transforms.quaternion_to_matrix (real first), fp64 ---------------------------------------------
def quat_to_matrix(q):
    w, x, y, z = np.asarray(q, np.float64)
    s = 2.0 / (w * w + x * x + y * y + z * z)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def screw(axis, angle, point, shift=0.0):
    """4x4 rotation by `angle` about the line through `point` along `axis`, then `shift` along the axis."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    R = rotation(a, angle)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(point) - R @ np.asarray(point) + shift * a
    return T


# ---- the reference's per-sample pipeline ----------------------------------------------------------------------
def init_position(p, d):
    m = np.argmax(np.abs(d))
    return p - (p[m] / d[m]) * d


def pose_mean(coords_step, cluster):
    c = coords_step[list(cluster)]
    A = np.zeros((4, 4))
    for q in c[:, 3:]:
        A += np.outer(q, q)
    A /= len(c)
    return np.mean(c[:, :3], axis=0), np.linalg.eigh(A)[1][:, -1]


def pose_matrix(pos, q):
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(q)
    T[:3, 3] = pos
    return T


def relative_motion(P0, C0, P1, C1):
    """T_r1 of compute_joints.py:93-102 from the 4x4 mean poses (np.linalg.inv as the reference)."""
    inv = np.linalg.inv
    T_r = inv(P0) @ P1
    T_c1 = inv(P0) @ C1
    T_c0 = inv(P0) @ C0
    return inv(T_c0) @ (inv(T_r) @ T_c1)


def closed_form(T):
    """The kernel's screw axis of a 4x4: (unit d, theta in [0, pi], canonical point)."""
    R, t = T[:3, :3], T[:3, 3]
    c = ((R[0, 0] + R[1, 1] + R[2, 2]) - 1.0) * 0.5
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    theta = math.atan2(s, c)
    if c >= 0:
        d = v / s
    else:
        B = 0.5 * (R + R.T) - c * np.eye(3)
        m = int(np.argmax(np.diag(B)))
        d = B[:, m] / np.linalg.norm(B[:, m])
        if d @ v < 0:
            d = -d
    tp = t - (d @ t) * d
    p = 0.5 * (tp + np.cross(d, tp) / math.tan(0.5 * theta))
    return d, theta, init_position(p, d)


def sample_steps(S, num_steps, interval, start=0):
    """(sequence, step_prev, step) of every sample, in the reference's order."""
    out = []
    for s in range(S):
        for a in range(interval):
            steps = list(range(start + a, start + num_steps, interval))
            out += [(s, i0, i1) for i0, i1 in zip(steps[:-1], steps[1:])]
    return out


# The reference's point comes from np.linalg.eig of the 4x4, whose eigenvalue 1 is defective as soon as the motion has
# an axial component: LAPACK then returns w ~ 1e-16 and the point is rounding noise (1e-3 .. 1e-1 on the fixture's
# noisy and cyclic cases, ~5e-8 when the axial shift stays below 1e-7).  WELL_POSED bounds the shift |d . t| under
# which the tests compare points with the reference.
WELL_POSED = 1e-6


def samples(coords, parent, child, start, num_steps, interval, reference=True):
    """Per-sample (axis, angle, point, axial shift) of one joint; coords (S,T,K,7).  reference=True goes through
    aff2axangle and init_position as the reference does, False through closed_form."""
    out = []
    for s, i0, i1 in sample_steps(coords.shape[0], num_steps, interval, start):
        P0, C0 = (pose_matrix(*pose_mean(coords[s, i0], c)) for c in (parent, child))
        P1, C1 = (pose_matrix(*pose_mean(coords[s, i1], c)) for c in (parent, child))
        T = relative_motion(P0, C0, P1, C1)
        dc, thc, pc = closed_form(T)
        shift = abs(dc @ T[:3, 3])
        if reference:
            d, th, p = aff2axangle(T)
            out.append((d, th, init_position(p[:3], d), shift))
        else:
            out.append((dc, thc, pc, shift))
    return out
