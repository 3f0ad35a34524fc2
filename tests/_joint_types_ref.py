"""numpy restatement of the two joint-type contracts of include/creg.h (creg_joint_types_f64, creg_joint_slides_f64) for
the tests, and a typed synthetic tree with exact kinematics: five links, one prismatic and one fixed joint among revolute
ones, whose kinds, slide direction and slide positions are known."""
import math

import numpy as np

import _joint_motion_ref as M
import _joints_ref as JR

TURN_MIN, SLIDE_MIN = 2e-4, 1e-6
KINDS = {"fixed": 0, "revolute": 1, "prismatic": 2}


def _angle(R):
    v, c = M.skew_and_cos(R)
    return math.atan2(math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), c)


def norm3(t):
    """|t| as the contract states it: sqrt((t0 t0 + t1 t1) + t2 t2)."""
    return math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])


def joint_types(coords, link_clusters, joints, start_step=0, num_steps=1, interval=1, turn_min=TURN_MIN, slide_min=None):
    S = coords.shape[0]
    steps = JR.sample_steps(S, num_steps, interval, start_step)
    J, NS = len(joints), len(steps)
    out = {"sample_angle": np.zeros((J, NS)), "sample_slide": np.zeros((J, NS, 3)), "sample_kind": np.zeros((J, NS), np.int32),
           "counts": np.zeros((J, 4), np.int32), "type": np.zeros(J, np.int32), "slide_axis": np.full((J, 3), np.nan),
           "global_axis": np.full((J, 3), np.nan), "global_pos": np.zeros((J, 3))}
    poses = {}                                     # (sequence, step, link) -> mean pose, computed once
    for j, (p, c) in enumerate(joints):
        pose = lambda s, i, l: poses[(s, i, l)] if (s, i, l) in poses else poses.setdefault(
            (s, i, l), JR.pose_matrix(*JR.pose_mean(coords[s, i], link_clusters[l])))
        acc, first = np.zeros((3, 3)), None
        for k, (s, i0, i1) in enumerate(steps):
            X0 = M.rigid_inv(pose(s, i0, p)) @ pose(s, i0, c)
            X1 = M.rigid_inv(pose(s, i1, p)) @ pose(s, i1, c)
            D = M.rigid_inv(X0) @ X1
            th, t = _angle(D[:3, :3]), D[:3, 3]
            if not (np.isfinite(th) and np.all(np.isfinite(t))):
                kind = -1
            elif th >= turn_min:
                kind = 1
            elif norm3(t) >= slide_min:
                kind = 2
            else:
                kind = 0
            out["sample_angle"][j, k], out["sample_slide"][j, k], out["sample_kind"][j, k] = th, t, kind
            out["counts"][j, 3 if kind < 0 else kind] += 1
            if kind == 2:
                acc += np.outer(t, t)
                first = t if first is None else first
        n_still, n_turn, n_slide, _ = out["counts"][j]
        out["type"][j] = 1 if n_turn else (2 if n_slide else (0 if n_still else -1))
        C0 = pose(0, start_step, c)
        out["global_pos"][j] = C0[:3, 3].astype(np.float32)
        if n_slide:
            a = np.linalg.eigh(acc)[1][:, -1]
            a = -a if a @ first < 0 else a
            out["slide_axis"][j], out["global_axis"][j] = a, C0[:3, :3] @ a
    return out


def joint_slides(link_T, joints, local_axis, ref_seq=0, ref_step=0, start_step=0, num_steps=None):
    S, T = link_T.shape[:2]
    n = T - start_step if num_steps is None else num_steps
    J = len(joints)
    q, tilt, slip = (np.zeros((J, S, n)) for _ in range(3))
    keys = ("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")
    out = {k: np.full(J, np.nan) for k in keys}
    out.update(n_used=np.zeros(J, np.int32), lower_at=np.full((J, 2), -1, np.int32), upper_at=np.full((J, 2), -1, np.int32))
    for j, (p, c) in enumerate(joints):
        a = np.asarray(local_axis[j], np.float64)
        X0 = M.rigid_inv(link_T[ref_seq, ref_step, p]) @ link_T[ref_seq, ref_step, c]
        for s in range(S):
            for i in range(n):
                D = M.rigid_inv(X0) @ (M.rigid_inv(link_T[s, start_step + i, p]) @ link_T[s, start_step + i, c])
                d = D[:3, 3]
                q[j, s, i] = (d[0] * a[0] + d[1] * a[1]) + d[2] * a[2]
                tilt[j, s, i] = _angle(D[:3, :3])
                slip[j, s, i] = norm3(d - q[j, s, i] * a)
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


# ---- the typed synthetic tree ---------------------------------------------------------------------------------
TREE_PARENTS = [-1, 0, 1, 1, 2]
TREE_CLUSTERS = [[0, 1], [2], [3, 4, 5], [6], [7]]
TREE_JOINTS = [(0, 1), (1, 2), (1, 3), (2, 4)]
TREE_TYPES = ["revolute", "prismatic", "fixed", "revolute"]
PRISMATIC, FIXED = 1, 2                            # rows of TREE_JOINTS


def _translation(x):
    T = np.eye(4)
    T[:3, 3] = x
    return T


def typed_tree(S=2, T=20, seed=0, types=TREE_TYPES, root_moves=True):
    """coords (S,T,8,7) of the five-link tree and what the contracts must recover from it.  Every cluster rides rigidly on its
    link at a fixed offset, the quaternion signs are random, the root moves too.  Every sequence starts from the same robot
    pose with every cluster's orientation the identity -- a registration's frame 0 -- so offsets and rest poses are
    translations, every joint stands at 0 at step 0 and a link's measured frame is its own frame moved by a translation: a
    joint's axis in the child's measured frame is its axis.  Joint positions grow monotonically along every sequence (a turn
    of at least 0.5 rad and a slide of at least 0.05 over the sequence, at T <= 400 steps 1.2e-3 rad and 1.2e-4 per step),
    so at turn_min = 2e-4 and slide_min = 1e-6 no sample is near a threshold; ``types`` turns joints into other kinds (the
    all-revolute control).  ``root_moves=False`` keeps the root at rest, as a robot's base is: ``replay_urdf`` compares motions in
    the world's frame with the URDF's root standing still, so only such a tree can hold its bound.  Returns coords, link_clusters, joints, types, links (the kinematic tree's dicts), axes (J,3),
    q_true (J,S,T)."""
    rng = np.random.default_rng(seed)
    K, J = 8, len(TREE_JOINTS)
    offsets = [_translation(rng.normal(size=3) * 0.05) for _ in range(K)]
    rest = [_translation(rng.normal(size=3) * 0.2) for _ in TREE_PARENTS]
    axes = np.array([v / np.linalg.norm(v) for v in rng.normal(size=(J, 3))])
    points = rng.normal(size=(J, 3)) * 0.1
    tt = np.arange(T) / max(T - 1, 1)
    q_true = np.zeros((J, S, T))
    for j, kind in enumerate(types):
        for s in range(S):
            if kind == "revolute":
                q_true[j, s] = (0.5 + 0.13 * j + 0.07 * s) * tt + (0.3 + 0.05 * s) * tt * tt
            elif kind == "prismatic":
                q_true[j, s] = (0.05 + 0.01 * s) * tt + (0.03 + 0.004 * j) * tt * tt
    coords = np.zeros((S, T, K, 7))
    for s in range(S):
        for t in range(T):
            pose = [None] * len(TREE_PARENTS)
            for l, par in enumerate(TREE_PARENTS):
                if par < 0:
                    pose[l] = rest[l]
                    if root_moves:
                        pose[l] = rest[l] @ JR.screw([0.2, 0.3, 0.9], (0.3 + 0.1 * s) * tt[t], [0.0, 0.1, 0.0], 0.05 * tt[t])
                    continue
                j = l - 1
                if types[j] == "revolute":
                    move = JR.screw(axes[j], q_true[j, s, t], points[j])
                else:
                    move = _translation(axes[j] * q_true[j, s, t])       # a fixed joint stands at 0
                pose[l] = pose[par] @ rest[l] @ move
            for l, cl in enumerate(TREE_CLUSTERS):
                for k in cl:
                    coords[s, t, k] = M._pose_row(pose[l] @ offsets[k], rng.choice([-1.0, 1.0]))
    links = [{"id": l, "parent_id": None if p < 0 else p, "cluster_idx": list(c)}
             for l, (p, c) in enumerate(zip(TREE_PARENTS, TREE_CLUSTERS))]
    return {"coords": coords, "link_clusters": TREE_CLUSTERS, "joints": TREE_JOINTS, "types": list(types), "links": links,
            "axes": axes, "q_true": q_true}


def separation(ref, turn_min=TURN_MIN, slide_min=SLIDE_MIN, factor=1e-6):
    """True when no finite sample's theta or |t| lies within a factor 1 +- ``factor`` of its threshold: only then are the
    kinds safe against rounding."""
    th = ref["sample_angle"][np.isfinite(ref["sample_angle"])]
    t = ref["sample_slide"].reshape(-1, 3)
    t = np.array([norm3(x) for x in t[np.all(np.isfinite(t), axis=1)]])
    near = lambda x, m: np.any((x > m * (1 - factor)) & (x < m * (1 + factor)))
    return not near(th, turn_min) and not near(t, slide_min)
