"""numpy restatement of the three joint-motion contracts of include/creg.h (creg_link_poses_f64, creg_joint_positions_f64,
creg_motion_error_f64) for the tests, and a synthetic 4-link tree with exact kinematics whose joint positions are known."""
import math

import numpy as np

import _joints_ref as JR

TWO_PI = 6.283185307179586


def rigid_inv(M):
    R, t = M[:3, :3], M[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ t
    return out


def skew_and_cos(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v, (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5


def link_poses(coords, link_clusters):
    """(S,T,L,4,4): the mean pose of every link at every step, as creg_joint_axes_f64 computes it."""
    S, T = coords.shape[:2]
    out = np.zeros((S, T, len(link_clusters), 4, 4))
    for s in range(S):
        for t in range(T):
            for l, c in enumerate(link_clusters):
                out[s, t, l] = JR.pose_matrix(*JR.pose_mean(coords[s, t], c))
    return out


def joint_positions(link_T, joints, local_axis, local_pos, ref_seq=0, ref_step=0, start_step=0, num_steps=None):
    S, T = link_T.shape[:2]
    n = T - start_step if num_steps is None else num_steps
    J = len(joints)
    q, tilt, slip = (np.zeros((J, S, n)) for _ in range(3))
    keys = ("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")
    out = {k: np.full(J, np.nan) for k in keys}
    out.update(n_used=np.zeros(J, np.int32), lower_at=np.full((J, 2), -1, np.int32), upper_at=np.full((J, 2), -1, np.int32))
    for j, (p, c) in enumerate(joints):
        a, pt = np.asarray(local_axis[j], np.float64), np.asarray(local_pos[j], np.float64)[:3]
        X0 = rigid_inv(link_T[ref_seq, ref_step, p]) @ link_T[ref_seq, ref_step, c]
        for s in range(S):
            w_prev = u = 0.0
            for i in range(n):
                X = rigid_inv(link_T[s, start_step + i, p]) @ link_T[s, start_step + i, c]
                D = rigid_inv(X0) @ X
                R = D[:3, :3]
                v, cs = skew_and_cos(R)
                w = math.atan2(v @ a, cs) if np.isfinite(v @ a) and np.isfinite(cs) else math.nan
                if i == 0:
                    u = w
                else:
                    d = w - w_prev
                    u = u + (d - TWO_PI * np.rint(d / TWO_PI))
                w_prev = w
                q[j, s, i] = u
                if np.isfinite(w):
                    ve, ce = skew_and_cos(JR.rotation(a, -w) @ R) if np.linalg.norm(a) > 0 else skew_and_cos(R)
                    tilt[j, s, i] = math.atan2(np.linalg.norm(ve), ce)
                else:
                    tilt[j, s, i] = math.nan
                slip[j, s, i] = np.linalg.norm(R @ pt + D[:3, 3] - pt)
        ok = np.isfinite(q[j]) & np.isfinite(tilt[j]) & np.isfinite(slip[j])
        out["n_used"][j] = ok.sum()
        if ok.any():
            uu = np.where(ok, q[j], np.inf)
            out["lower"][j], out["lower_at"][j] = uu.min(), np.unravel_index(np.argmin(uu), uu.shape)
            uu = np.where(ok, q[j], -np.inf)
            out["upper"][j], out["upper_at"][j] = uu.max(), np.unravel_index(np.argmax(uu), uu.shape)
            out["tilt_rms"][j], out["tilt_max"][j] = math.sqrt((tilt[j][ok] ** 2).sum() / ok.sum()), tilt[j][ok].max()
            out["slip_rms"][j], out["slip_max"][j] = math.sqrt((slip[j][ok] ** 2).sum() / ok.sum()), slip[j][ok].max()
    out.update(q=q, tilt=tilt, slip=slip)
    return out


def motion_error(A, A0, B, B0, point):
    P, L = A.shape[:2]
    rot, pos = np.zeros((P, L)), np.zeros((P, L))
    for p in range(P):
        for l in range(L):
            Ma, Mb = A[p, l] @ rigid_inv(A0[l]), B[p, l] @ rigid_inv(B0[l])
            v, c = skew_and_cos(Ma[:3, :3].T @ Mb[:3, :3])
            rot[p, l] = math.atan2(np.linalg.norm(v), c)
            x = np.append(point[l], 1.0)
            pos[p, l] = np.linalg.norm((Ma @ x)[:3] - (Mb @ x)[:3])
    return rot, pos


# ---- a synthetic tree with exact kinematics -------------------------------------------------------------------
TREE_PARENTS = [-1, 0, 1, 1]
TREE_CLUSTERS = [[0, 1], [2], [3, 4, 5], [6]]
TREE_JOINTS = [(0, 1), (1, 2), (1, 3)]
RAMP_JOINT = 1                                     # joint (1, 2): 0 -> -200 deg in sequence 0, 0 -> 170 deg in sequence 1


def random_rigid(rng, scale=0.2):
    from scipy.spatial.transform import Rotation
    M = np.eye(4)
    M[:3, :3] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix()
    M[:3, 3] = rng.normal(size=3) * scale
    return M


def _pose_row(M, sign):
    from scipy.spatial.transform import Rotation
    x, y, z, w = Rotation.from_matrix(M[:3, :3]).as_quat()
    return np.array([*M[:3, 3], *(sign * np.array([w, x, y, z]))])


def synthetic_tree(S=2, T=60, seed=0):
    """coords (S,T,7,7) of the 4-link tree, and what the contracts must recover from it: joints, local_axis (J,3) and
    local_pos (J,4) in each child's MEASURED frame (the link's mean pose), q_true (J,S,T).  Every cluster rides rigidly on its
    link (a fixed offset), so the mean pose of a link is its pose times one fixed transform; the quaternion signs are random.
    The root moves too.  Joint RAMP_JOINT sweeps 0 -> -200 deg in sequence 0 and 0 -> 170 deg in sequence 1 (0 -> 90 deg in
    any further one); the others follow incommensurate sines with a phase and an amplitude per sequence."""
    rng = np.random.default_rng(seed)
    K = 7
    offsets = [random_rigid(rng, 0.05) for _ in range(K)]
    rest = [random_rigid(rng) for _ in TREE_PARENTS]
    axes = [None] + [v / np.linalg.norm(v) for v in rng.normal(size=(3, 3))]
    points = [None] + list(rng.normal(size=(3, 3)) * 0.1)
    tt = np.arange(T) / max(T - 1, 1)
    q_true = np.zeros((3, S, T))
    targets = [-200.0, 170.0] + [90.0] * max(S - 2, 0)
    for s in range(S):
        q_true[0, s] = (0.8 - 0.1 * s) * np.sin(3.1 * tt + 0.7 * s + 0.3)
        q_true[RAMP_JOINT, s] = math.radians(targets[s]) * tt
        q_true[2, s] = (0.6 + 0.07 * s) * np.sin(4.3 * tt + 1.1 * s + 1.9) - 0.2
    # the fixed transform between a link's pose and its measured mean pose
    mean_off = []
    for c in TREE_CLUSTERS:
        rows = np.array([_pose_row(offsets[k], 1.0) for k in range(K)])
        mean_off.append(JR.pose_matrix(*JR.pose_mean(rows, c)))
    coords = np.zeros((S, T, K, 7))
    for s in range(S):
        for t in range(T):
            pose = [None] * 4
            for l, par in enumerate(TREE_PARENTS):
                if par < 0:
                    pose[l] = rest[l] @ JR.screw([0.2, 0.3, 0.9], 0.3 * tt[t] + 0.1 * s, [0.0, 0.1, 0.0], 0.05 * tt[t])
                else:
                    pose[l] = pose[par] @ rest[l] @ JR.screw(axes[l], q_true[l - 1, s, t], points[l])
                for k in TREE_CLUSTERS[l]:
                    coords[s, t, k] = _pose_row(pose[l] @ offsets[k], rng.choice([-1.0, 1.0]))
    local_axis = np.array([mean_off[c][:3, :3].T @ axes[c] for _, c in TREE_JOINTS])
    local_pos = np.array([rigid_inv(mean_off[c]) @ np.append(points[c], 1.0) for _, c in TREE_JOINTS])
    return {"coords": coords, "link_clusters": TREE_CLUSTERS, "joints": TREE_JOINTS, "local_axis": local_axis,
            "local_pos": local_pos, "q_true": q_true}


def expected_positions(q_true, ref_seq, ref_step, start_step, num_steps):
    """What the contract recovers from exact kinematics: the first used step of each sequence relative to the reference pose,
    wrapped into (-pi, pi], then the true increments."""
    first = q_true[:, :, start_step] - q_true[:, ref_seq, ref_step][:, None]
    first = first - TWO_PI * np.rint(first / TWO_PI)
    sl = q_true[:, :, start_step:start_step + num_steps]
    return first[:, :, None] + (sl - sl[:, :, :1])
