"""Case builders and an ordered restatement for the edge suite of creg_joint_axes_f64 (k_joint_axes, csrc/joints.hip):
tests/test_joint_axes_edges_cpu.py checks the cases' own conditions on the CPU, tests/test_gpu_joint_axes_edges.py compares
the kernel with the restatement.  Both files take their cases from ``case(name)`` here, so neither has a copy of its own.

    joint_axes_ref   every output of ops.joint_axes in numpy float64: per-sample values from _joints_ref.samples(...,
                 reference=False), the usable rule of creg.h (theta >= 2e-4 and everything finite; an unusable sample has a NaN
                 axis and point), then ``aggregate``: the first usable sample, signs aligned to it, the top eigenvector of
                 sum a a^T (eigh) with the sign of the first axis, the mean of the usable points, and the first-pose frame work of
                 compute_joints.optimize_joint_axis (child matrix rounded to float32, g, the t* closed form with its midpoint
                 branch, local = inv(Tc) @ ...).  A joint with count 0 gets NaN outputs; first_pose is _joints_ref.pose_mean.
    aggregate    takes ``keep`` (a mask of samples to sum) and ``sign_from`` (the sample whose axis gives the sign): the CPU
                 file uses them to restate a kernel that forgot a wave's partial, a stride round or the first usable sample.
                 a a^T does not change when a is negated, so which axes are flipped before the sum cannot move the
                 eigenvector: the alignment decides local_axis' sign and nothing else, and ``sign_from`` is all of it.
    jitter       normal noise on xyz and on the quaternion components (non-unit quaternions are legal: quat_to_matrix divides
                 by |q|^2), so that the sample axes spread by about 0.1 and every sample matters to the aggregates.
    reverse_sequence   one sequence run backwards: its sample axes point the other way.
    rest_then_move     the robot keeps its pose bit for bit over the first n_rest steps (theta exactly 0: unusable samples), so
                 the first usable sample is n_rest - 1; ``backwards`` runs the moving part the other way, which negates local_axis
                 and leaves sum a a^T nearly alone -- a sign taken from anything but the first usable sample's axis is wrong for
                 one of the two.
    threshold_pair, on_the_line, two_link   single joints between two one-cluster links.
"""
import functools
import math

import numpy as np

import _joint_types_ref as JT
import _joints_ref as JR

THETA_MIN = 2e-4
NT, WAVE, MAX_SAMPLES = 256, 64, 4096
TOL = 1e-9                                                       # the aggregates' bound: the suite's own for these outputs at NS = 18
OUTPUTS = ("local_axis", "local_pos", "global_pos", "global_axis")
REST = (70, 130, 200, 300, 520)
THRESHOLD_MARGIN = 1e-3
BAD_SEQ, BAD_STEP, BAD_CLUSTER, BAD_LINK = 1, 120, 4, 2          # the non-finite pose: cluster 4 is the second of link 2's three


# ------------------------------------------------------------------------------------------ the restatement
def _bad_poses(coords, clusters):
    """(S,T) bool: a pose row of one of ``clusters`` is not finite at that step."""
    return ~np.isfinite(coords[:, :, sorted(set(clusters))]).all(axis=(2, 3))


def per_sample(coords, parent, child, start, num_steps, interval):
    """axis (NS,3), angle (NS), point (NS,3), usable (NS) of one joint.  A sample that touches a pose which is not finite is
    unusable, its angle is not stated (NaN here; the kernel's may be finite when only a position is not)."""
    coords = np.asarray(coords, np.float64)
    steps = JR.sample_steps(coords.shape[0], num_steps, interval, start)
    NS = len(steps)
    bad = _bad_poses(coords, list(parent) + list(child))
    clean = coords
    if bad.any():
        clean = coords.copy()
        clean[bad] = (0, 0, 0, 1, 0, 0, 0)
    with np.errstate(all="ignore"):
        smp = JR.samples(clean, parent, child, start, num_steps, interval, reference=False)
    axis, angle, point = np.full((NS, 3), np.nan), np.full(NS, np.nan), np.full((NS, 3), np.nan)
    usable = np.zeros(NS, bool)
    for i, ((s, i0, i1), (d, th, p, _)) in enumerate(zip(steps, smp)):
        if bad[s, i0] or bad[s, i1]:
            continue
        angle[i] = th
        if th >= THETA_MIN and np.isfinite(th) and np.isfinite(d).all() and np.isfinite(p).all():
            axis[i], point[i], usable[i] = d, p, True
    return axis, angle, point, usable


def scatter(axis, usable):
    """sum a a^T over the usable samples and its eigenvalues, ascending."""
    a = axis[usable]
    M = a.T @ a
    return M, np.linalg.eigvalsh(M)


def aggregate(axis, point, usable, pose_parent, pose_child, keep=None, sign_from=None):
    """The per-joint outputs from the per-sample ones and the two first poses ((xyz, wxyz) each).  ``keep`` (NS) bool: the
    samples a kernel summed (None: all).  ``sign_from``: the sample whose axis signs local_axis (None: the first usable one).
    Returns a dict with OUTPUTS, count, first (the first usable sample, -1 without one) and midpoint (the ru + rv == 0 branch)."""
    out = {"local_axis": np.full(3, np.nan), "local_pos": np.full(4, np.nan), "global_pos": np.full(3, np.nan),
           "global_axis": np.full(3, np.nan), "count": 0, "first": -1, "midpoint": False}
    if not usable.any():
        return out
    first = int(np.argmax(usable))
    a0 = axis[first if sign_from is None else sign_from]
    use = usable if keep is None else usable & keep
    if not use.any():
        return out
    a = axis[use]
    a = np.where((a @ axis[first] < 0)[:, None], -a, a)              # the alignment: a no-op under a a^T, kept as creg.h states it
    ax = np.linalg.eigh(a.T @ a)[1][:, -1]
    if ax @ a0 < 0:
        ax = -ax
    pos = point[use].mean(axis=0)
    (tp, _), (tc, qc) = pose_parent, pose_child
    Rc = JR.quat_to_matrix(qc)
    Tc = JR.pose_matrix(tc, qc).astype(np.float32).astype(np.float64)
    g = (Tc @ np.append(pos, 1.0))[:3]
    u, v = tp - g, tc - g
    su, sv = u @ ax, v @ ax
    ru, rv = np.linalg.norm(u - su * ax), np.linalg.norm(v - sv * ax)
    t = su + (sv - su) * (ru / (ru + rv)) if ru + rv > 0 else 0.5 * (su + sv)
    local = np.linalg.inv(Tc) @ np.append(g + t * ax, 1.0)
    out.update(local_axis=ax, local_pos=local, global_pos=(Tc @ local)[:3], global_axis=Rc @ ax, count=int(use.sum()), first=first,
               midpoint=not ru + rv > 0)
    return out


def joint_axes_ref(coords, link_clusters, joints, start, num_steps, interval):
    """Every output of ops.joint_axes as numpy arrays, plus first (J) and midpoint (J)."""
    coords = np.asarray(coords, np.float64)
    J, NS = len(joints), len(JR.sample_steps(coords.shape[0], num_steps, interval, start))
    out = {"sample_axis": np.zeros((J, NS, 3)), "sample_angle": np.zeros((J, NS)), "sample_point": np.zeros((J, NS, 3)),
           "sample_usable": np.zeros((J, NS), bool), "local_axis": np.zeros((J, 3)), "local_pos": np.zeros((J, 4)),
           "global_pos": np.zeros((J, 3)), "global_axis": np.zeros((J, 3)), "count": np.zeros(J, np.int32),
           "first_pose": np.zeros((J, 2, 7)), "first": np.zeros(J, np.int64), "midpoint": np.zeros(J, bool)}
    for j, (p, c) in enumerate(joints):
        axis, angle, point, usable = per_sample(coords, link_clusters[p], link_clusters[c], start, num_steps, interval)
        poses = [JR.pose_mean(coords[0, start], link_clusters[l]) for l in (p, c)]
        agg = aggregate(axis, point, usable, *poses)
        out["sample_axis"][j], out["sample_angle"][j], out["sample_point"][j], out["sample_usable"][j] = axis, angle, point, usable
        out["first_pose"][j] = [np.concatenate(x) for x in poses]
        for k in OUTPUTS + ("count", "first", "midpoint"):
            out[k][j] = agg[k]
    return out


def reaggregate(c, ref, j, **kw):
    """Joint j of case c again from the restatement's per-sample values, with ``aggregate``'s keep / sign_from."""
    p, ch = c["joints"][j]
    poses = [(ref["first_pose"][j, x, :3], ref["first_pose"][j, x, 3:]) for x in (0, 1)]
    return aggregate(ref["sample_axis"][j], ref["sample_point"][j], ref["sample_usable"][j], *poses, **kw)


# ------------------------------------------------------------------------------------------ the builders
def jitter(coords, scale, seed):
    """coords plus normal noise of ``scale`` on every xyz and quaternion component."""
    return coords + np.random.default_rng(seed).normal(scale=scale, size=coords.shape)


def reverse_sequence(coords, s):
    out = coords.copy()
    out[s] = coords[s][::-1]
    return out


def rest_then_move(coords, n_rest, backwards=False):
    """(1, n_rest + T - 1, K, 7) from sequence 0 of coords (S,T,K,7): its first pose n_rest times, then its steps 1 .. T - 1;
    ``backwards`` takes the sequence from its end.  Samples 0 .. n_rest - 2 join equal poses, sample n_rest - 1 is the first that moves."""
    seq = coords[0][::-1] if backwards else coords[0]
    return np.ascontiguousarray(np.concatenate([np.repeat(seq[:1], n_rest, axis=0), seq[1:]])[None])


def _row(M, sign=1.0):
    """[xyz, wxyz] of a 4x4 rigid matrix."""
    R = M[:3, :3]
    w = 0.5 * math.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0))
    if w > 0.1:
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    else:                                                        # near a half turn: the largest of x, y, z first
        m = int(np.argmax(np.diag(R)))
        n, o = (m + 1) % 3, (m + 2) % 3
        x = 0.5 * math.sqrt(max(1.0 + R[m, m] - R[n, n] - R[o, o], 0.0))
        q = np.zeros(4)
        q[1 + m], q[1 + n], q[1 + o], q[0] = x, (R[n, m] + R[m, n]) / (4 * x), (R[o, m] + R[m, o]) / (4 * x), (R[o, n] - R[n, o]) / (4 * x)
    return np.array([*M[:3, 3], *(sign * q)])


TWO_LINKS, TWO_JOINT = [[0], [1]], [(0, 1)]
TWO_AXIS, TWO_POINT = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]), np.array([0.1, 0.2, -0.05])


def two_link(S, T, rate, seed=0):
    """coords (S,T,2,7): cluster 0 the parent, slowly moving, cluster 1 the child turning about TWO_AXIS through TWO_POINT of the
    parent's frame by ``rate`` .. 1.3 ``rate`` (1 + 0.1 s) rad per step, growing along the sequence; quaternion signs random."""
    rng = np.random.default_rng(seed)
    rest_p, rest_c = JT._translation(rng.normal(size=3) * 0.2), JT._translation(rng.normal(size=3) * 0.2)
    coords = np.zeros((S, T, 2, 7))
    for s in range(S):
        for t in range(T):
            tt = t / max(T - 1, 1)
            P = rest_p @ JR.screw([0.2, 0.3, 0.9], (0.3 + 0.1 * s) * tt, [0.0, 0.1, 0.0], 0.05 * tt)
            q = rate * (1 + 0.1 * s) * (t + 0.15 * t * tt)
            C = P @ rest_c @ JR.screw(TWO_AXIS, q, TWO_POINT)
            coords[s, t, 0], coords[s, t, 1] = _row(P, rng.choice([-1.0, 1.0])), _row(C, rng.choice([-1.0, 1.0]))
    return coords


def threshold_pair():
    """Two (1,2,2,7) coords: the child turns once by 2e-4 (1 - 1e-3) and by 2e-4 (1 + 1e-3) rad, the parent stands at the identity."""
    out = []
    for angle in (THETA_MIN * (1 - THRESHOLD_MARGIN), THETA_MIN * (1 + THRESHOLD_MARGIN)):
        c = np.zeros((1, 2, 2, 7))
        c[0, :, :, 3] = 1.0
        c[0, 1, 1] = _row(JR.screw(TWO_AXIS, angle, TWO_POINT))
        out.append(c)
    return out


ON_LINE_PARENT_Z, ON_LINE_CHILD_Z = -0.25, 0.5


def on_the_line(T=6, rate=0.3):
    """(1,T,2,7): the joint line is the z axis; the parent stands on it at z = -0.25, the child turns about it at z = 0.5.  Every
    quaternion is (cos, 0, 0, sin) and every x and y an exact zero, so both mean positions have distance exactly 0 from the line
    and t* takes its midpoint branch: global_pos = (0, 0, 0.125)."""
    c = np.zeros((1, T, 2, 7))
    c[0, :, 0, 2], c[0, :, 0, 3] = ON_LINE_PARENT_Z, 1.0
    for t in range(T):
        c[0, t, 1] = (0, 0, ON_LINE_CHILD_Z, math.cos(0.5 * rate * t), 0, 0, math.sin(0.5 * rate * t))
    return c


# ------------------------------------------------------------------------------------------ the cases, by name
def _tree(S, T, scale, seed):
    t = JT.typed_tree(S=S, T=T, seed=seed, types=["revolute"] * 4)
    coords = jitter(t["coords"], scale, seed + 100)
    if S >= 2:
        coords = reverse_sequence(coords, S - 1)
    return {"coords": coords, "link_clusters": t["link_clusters"], "joints": t["joints"], "reversed": S - 1 if S >= 2 else None}


def _two(S, T, rate, scale, seed):
    coords = jitter(two_link(S, T, rate, seed), scale, seed + 100)
    if S >= 2:
        coords = reverse_sequence(coords, S - 1)
    return {"coords": coords, "link_clusters": TWO_LINKS, "joints": TWO_JOINT, "reversed": S - 1 if S >= 2 else None}


# name -> (builder, its arguments, num_steps, interval, NS)
SIZES = {
    "ns63": (_tree, (3, 22, 2e-5, 1), 22, 1, 63),
    "ns64": (_tree, (2, 33, 2e-5, 2), 33, 1, 64),
    "ns65": (_two, (1, 66, 4e-3, 2e-5, 3), 66, 1, 65),
    "ns255": (_tree, (3, 86, 2e-5, 4), 86, 1, 255),
    "ns256": (_tree, (2, 129, 2e-5, 5), 129, 1, 256),
    "ns257": (_tree, (1, 258, 2e-5, 6), 258, 1, 257),
    "ns296_interval4": (_tree, (1, 300, 2e-5, 7), 300, 4, 296),
    "ns511_interval2": (_two, (1, 513, 2e-3, 2e-5, 8), 513, 2, 511),
    "ns513": (_tree, (3, 172, 2e-5, 9), 172, 1, 513),
    "ns927": (_tree, (3, 310, 2e-5, 10), 310, 1, 927),
    "ns4096": (_two, (2, 2049, 3e-3, 1e-4, 11), 2049, 1, 4096),
    "large_turns": (_two, (2, 34, 2.0, 2e-3, 12), 34, 1, 66),
}
REFUSED = {4097: (1, 4098), 4098: (2, 2050)}                     # NS -> (S, num_steps) at interval 1
NS_TARGETS = (63, 64, 65, 255, 256, 257, 511, 513, 927, 4096)
REST_CASES = tuple(f"rest{n}{d}" for n in REST for d in ("", "_back"))
BAD_CASES = tuple(f"bad_{v}_{k}" for v in ("nan", "inf") for k in ("x", "qy"))
BAD_COMPONENT = {"x": 0, "qy": 5}
ALL_CASES = tuple(SIZES) + REST_CASES + ("clean",) + BAD_CASES + ("below", "above", "on_the_line")
REST_MOVE = 40                                                   # steps of the moving part


@functools.lru_cache(maxsize=None)
def case(name):
    """{"coords" (S,T,K,7), "link_clusters", "joints", "num_steps", "interval", "NS", "reversed"}; start_step is 0 everywhere."""
    if name in SIZES:
        build, args, num_steps, interval, NS = SIZES[name]
        return dict(build(*args), num_steps=num_steps, interval=interval, NS=NS)
    if name.startswith("rest"):
        n = int(name[4:].split("_")[0])
        base = _tree(1, REST_MOVE, 2e-5, 20 + n)
        coords = rest_then_move(base["coords"], n, name.endswith("_back"))
        return dict(base, coords=coords, num_steps=coords.shape[1], interval=1, NS=coords.shape[1] - 1, n_rest=n)
    if name == "clean" or name in BAD_CASES:
        c = dict(_tree(2, 156, 2e-5, 30), num_steps=156, interval=1, NS=310)
        if name != "clean":
            _, value, comp = name.split("_")
            coords = c["coords"].copy()
            coords[BAD_SEQ, BAD_STEP, BAD_CLUSTER, BAD_COMPONENT[comp]] = np.nan if value == "nan" else np.inf
            c["coords"] = coords
        return c
    if name in ("below", "above"):
        return {"coords": threshold_pair()[name == "above"], "link_clusters": TWO_LINKS, "joints": TWO_JOINT, "num_steps": 2,
                "interval": 1, "NS": 1, "reversed": None}
    if name == "on_the_line":
        return {"coords": on_the_line(), "link_clusters": TWO_LINKS, "joints": TWO_JOINT, "num_steps": 6, "interval": 1, "NS": 5,
                "reversed": None}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """joint_axes_ref of a case, computed once and left unchanged."""
    c = case(name)
    ref = joint_axes_ref(c["coords"], c["link_clusters"], c["joints"], 0, c["num_steps"], c["interval"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def bad_samples(c):
    """The two samples of a 'bad_*' case that touch the pose which is not finite (interval 1, sequence-major)."""
    per = c["num_steps"] - 1
    return [BAD_SEQ * per + BAD_STEP - 1, BAD_SEQ * per + BAD_STEP]
