"""Drop-in for the reference's ``PointCloud/compute_joints.py``: joint axes of the kinematic tree and the URDF writer
(SURVEY 8(f) N4).

``estimate_joint_axes_from_tree`` (:216-268) is ONE launch of ``creg_joint_axes_f64``: every joint, every sequence,
phase and step, with the per-link mean poses (:10-39), the relative motions (:41-52, :93-102), the screw axes
(transforms3d's ``aff2axangle`` in closed form), the principal axis and the refined joint point (:124-214).
``get_cluster_pose_mean``, ``average_quaternions`` and ``calculate_joint_axis_relative`` go through the same launch as
batches of one.  ``relative_transform`` and ``optimize_joint_axis`` take poses and axes the caller already holds; they
are the kernel's closed forms restated on the host for a single joint (4x4 products and one 3x3 eigen problem).
``create_urdf`` (:274-388) writes the same XML; its per-link transforms come from ``creg_link_clouds_f64``.
The axis sign follows creg.h's convention: the first usable sample of a joint has a positive angle (the reference's
sign follows np.linalg.eig, so the two agree up to one sign per joint).  ``visualize_urdf`` (pybullet GUI) is out of
scope.  No CPU fallback.

This project's own, beyond the reference: ``estimate_typed_joints_from_tree`` also tells prismatic and fixed joints
(``creg_joint_types_f64``), and ``estimate_joint_motion``, ``set_joint_limits`` and ``replay_urdf`` recover every joint's
positions, write the observed limits and check the written file against the registration; ``cloud_fit_poses`` and
``cloud_fit`` check its meshes against the raw clouds (``ops.point_mesh_distance``), ``surface_cover_poses`` and ``cloud_cover``
the raw clouds against its meshes (``ops.mesh_cover``: surface no point lies near); ``fit_cloud_poses`` and ``fit_positions``
fit the joint positions and the base pose to clouds (``ops.pose_fit_system``, Levenberg-Marquardt); ``refine_joint_frames``,
``set_joint_frames`` and ``refine_urdf_joints`` refine the joint frames themselves against the clouds, a bundle adjustment on
``ops.link_moments`` (``link_twists``, ``twist_system``), and write them into a copy of the URDF.
"""
import os
import xml.etree.ElementTree as ET
from types import SimpleNamespace

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from . import _lib, ops


def _jet(x):
    """matplotlib's ``get_cmap("jet")(x)`` for scalar x: its 256-entry lookup table, restated."""
    N = 256
    segs = {"red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
            "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
            "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}
    rgba = []
    for ch in ("red", "green", "blue"):
        a = np.array(segs[ch], dtype=float)
        xs, y0, y1 = a[:, 0] * (N - 1), a[:, 1], a[:, 2]
        xind = (N - 1) * np.linspace(0, 1, N)
        ind = np.searchsorted(xs, xind)[1:-1]
        dist = (xind[1:-1] - xs[ind - 1]) / (xs[ind] - xs[ind - 1])
        lut = np.clip(np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0, 1)
        i = int(x * N)
        rgba.append(lut[min(max(i, 0), N - 1)])
    return tuple(rgba) + (1.0,)


def _coords(cm_list):
    c = [np.asarray(cm.coords, np.float64) for cm in cm_list]
    if len({x.shape for x in c}) != 1:
        raise ValueError(f"every sequence needs the same (T, K): got {[x.shape for x in c]}")
    return torch.as_tensor(np.stack(c), device=_lib.device(getattr(cm_list[0], "_M", None))).contiguous()


def _one_joint(coords, link_clusters, start_step=0, num_steps=1, interval=1):
    return ops.joint_axes(coords, link_clusters, [(0, 1)], start_step, num_steps, interval)


def get_cluster_pose_mean(cm, cluster, step):
    """Mean xyz and average quaternion of the clusters at one step (compute_joints.py:10-19)."""
    c = torch.as_tensor(np.asarray(cm.coords, np.float64)[step][None, None], device=_lib.device()).contiguous()
    fp = _one_joint(c, [list(cluster), list(cluster)])["first_pose"][0, 0].cpu().numpy()
    return fp[:3].copy(), fp[3:].copy()


def average_quaternions(quaternions):
    """Top eigenvector of (1/n) sum q q^T (compute_joints.py:21-39); its sign is the eigen solver's."""
    q = np.asarray(quaternions, np.float64).reshape(-1, 4)
    c = np.concatenate([np.zeros((len(q), 3)), q], axis=1)[None, None]
    cl = list(range(len(q)))
    return _one_joint(torch.as_tensor(c, device=_lib.device()).contiguous(), [cl, cl])["first_pose"][0, 0, 3:].cpu().numpy()


def _pose_matrix(pose):
    pos, ori = pose
    q = np.asarray(ori, np.float64)
    w, x, y, z = q
    s = 2.0 / (q * q).sum()
    T = np.eye(4)
    T[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    T[:3, 3] = pos
    return T


def relative_transform(pose_parent, pose_child):
    """inv(T_parent) @ T_child of two (position, quaternion) poses (compute_joints.py:41-52)."""
    return np.linalg.inv(_pose_matrix(pose_parent)) @ _pose_matrix(pose_child)


def calculate_joint_axis_relative(poses_parent, poses_child):
    """Per-step screw axis of the child relative to the parent (compute_joints.py:54-122): lists (axes, angles, poses),
    one entry per consecutive pair.  Each (axis, angle) pair has angle in [0, pi]; a step below the usable angle gets
    NaN axis and point."""
    n = len(poses_parent)
    if n < 2:
        return [], [], []
    c = np.zeros((1, n, 2, 7))
    for i, ((pp, po), (cp, co)) in enumerate(zip(poses_parent, poses_child)):
        c[0, i, 0] = np.concatenate([pp, po])
        c[0, i, 1] = np.concatenate([cp, co])
    out = _one_joint(torch.as_tensor(c, device=_lib.device()).contiguous(), [[0], [1]], 0, n, 1)
    ax, an, pt = (out[k][0].cpu().numpy() for k in ("sample_axis", "sample_angle", "sample_point"))
    return list(ax), list(an), list(pt)


def optimize_joint_axis(poses_parent, poses_child, axes, poses):
    """Principal axis, global axes, refined global point and its child-frame homogeneous point
    (compute_joints.py:124-214), with the kernel's closed forms: the top eigenvector of sum a a^T, sign of the first axis,
    and refine_position's minimiser t* = s_u + (s_v - s_u) r_u / (r_u + r_v) (midpoint when both distances vanish)."""
    a = np.array([x / np.linalg.norm(x) for x in axes])
    a0 = a[0]
    w, V = np.linalg.eigh(a.T @ a)
    principal_axis = V[:, -1]
    if np.dot(principal_axis, a0) < 0:
        principal_axis = -principal_axis
    principal_pos = np.mean(poses, axis=0)
    global_axes = [_pose_matrix(p)[:3, :3] @ principal_axis for p in poses_child]
    Tc = _pose_matrix(poses_child[0]).astype(np.float32).astype(np.float64)
    g = (Tc @ np.append(principal_pos, 1.0))[:3]
    u, v = np.asarray(poses_parent[0][0]) - g, np.asarray(poses_child[0][0]) - g
    su, sv = u @ principal_axis, v @ principal_axis
    ru, rv = np.linalg.norm(u - su * principal_axis), np.linalg.norm(v - sv * principal_axis)
    t = su + (sv - su) * (ru / (ru + rv)) if ru + rv > 0 else 0.5 * (su + sv)
    local = np.linalg.inv(Tc) @ np.append(g + t * principal_axis, 1.0)
    return principal_axis, global_axes, (Tc @ local)[:3], local


def _tree_pairs(links):
    """The tree's joints as (parent, child) indices into ``links``, in the links' order."""
    by_id = {l["id"]: i for i, l in enumerate(links)}
    return [(by_id[l["parent_id"]], i) for i, l in enumerate(links) if l["parent_id"] is not None]


def _need_a_turning_step(count, pid, cid):
    if count == 0:
        raise ValueError(f"joint between parent link {pid} and child link {cid}: no step turns the child by at least "
                         f"{ops.JOINT_THETA_MIN} rad relative to the parent, its axis is undefined")


def estimate_joint_axes_from_tree(links, cm_list, start_step=0, num_steps=500, interval=1):
    """Joint axes between connected links of the kinematics tree (compute_joints.py:216-268), one launch.  Returns the
    reference's list of dicts (parent_link, child_link, local_axis, local_pos, global_pos, global_axis) in its order.
    A joint without a usable step (the child never turns relative to its parent) raises ValueError."""
    pairs = _tree_pairs(links)
    out = ops.joint_axes(_coords(cm_list), [list(l["cluster_idx"]) for l in links], pairs, start_step, num_steps, interval)
    res = {k: out[k].cpu().numpy() for k in ("local_axis", "local_pos", "global_pos", "global_axis", "count")}
    joint_data = []
    for j, (p, c) in enumerate(pairs):
        pid, cid = links[p]["id"], links[c]["id"]
        _need_a_turning_step(res["count"][j], pid, cid)
        print(f"Joint between parent link {pid} and child link {cid}: axis {res['local_axis'][j]}")
        joint_data.append({"parent_link": pid, "child_link": cid, "local_axis": res["local_axis"][j],
                           "local_pos": res["local_pos"][j], "global_pos": res["global_pos"][j],
                           "global_axis": res["global_axis"][j]})
    return joint_data


JOINT_TYPE_NAMES = {0: "fixed", 1: "revolute", 2: "prismatic"}       # urdf_fk's numbering
JOINT_UNITS = {"revolute": "rad", "prismatic": "length", "fixed": None}   # "length": the clouds' own unit


def estimate_typed_joints_from_tree(links, cm_list, start_step=0, num_steps=500, interval=1, slide_min=None, turn_min=None):
    """``estimate_joint_axes_from_tree`` for trees whose joints may also slide or not move at all (this project's own): one
    ``ops.joint_axes`` and one ``ops.joint_types`` launch over the same samples.  A sample turns when the child's relative
    rotation reaches ``turn_min`` rad (None: ``ops.JOINT_THETA_MIN``), slides when it does not and the relative translation
    reaches ``slide_min`` (the clouds' unit, required), and stands still otherwise; a joint with a turning sample is revolute,
    else one with a sliding sample prismatic, else fixed.  Returns the reference's list of dicts plus "type" ("revolute" |
    "prismatic" | "fixed") and "counts" (still, turn, slide, bad samples).  A revolute joint's other entries are those of
    ``estimate_joint_axes_from_tree``; a prismatic joint's local_axis is the slide direction in the child's frame, its
    local_pos (0,0,0,1) -- the joint point is the child's origin -- and global_axis / global_pos the same at sequence 0, step
    ``start_step``; a fixed joint has the same point and a NaN axis.  ValueError for a joint without a finite sample, or for
    a revolute one whose axis is undefined (possible only with ``turn_min`` below ``ops.JOINT_THETA_MIN``)."""
    turn_min = ops.JOINT_THETA_MIN if turn_min is None else turn_min
    pairs = _tree_pairs(links)
    coords, clusters = _coords(cm_list), [list(l["cluster_idx"]) for l in links]
    kinds = ops.joint_types(coords, clusters, pairs, start_step, num_steps, interval, turn_min, slide_min)
    axes = ops.joint_axes(coords, clusters, pairs, start_step, num_steps, interval)
    res = {k: axes[k].cpu().numpy() for k in ("local_axis", "local_pos", "global_pos", "global_axis", "count")}
    typ = {k: kinds[k].cpu().numpy() for k in ("type", "counts", "slide_axis", "global_axis", "global_pos")}
    joint_data = []
    for j, (p, c) in enumerate(pairs):
        pid, cid = links[p]["id"], links[c]["id"]
        if typ["type"][j] < 0:
            raise ValueError(f"joint between parent link {pid} and child link {cid}: no sample with finite poses, its kind is "
                             f"undefined")
        name = JOINT_TYPE_NAMES[int(typ["type"][j])]
        if name == "revolute":
            _need_a_turning_step(res["count"][j], pid, cid)
            jd = {k: res[k][j] for k in ("local_axis", "local_pos", "global_pos", "global_axis")}
        else:
            jd = {"local_axis": typ["slide_axis"][j], "local_pos": np.array([0.0, 0.0, 0.0, 1.0]),
                  "global_pos": typ["global_pos"][j], "global_axis": typ["global_axis"][j]}
        print(f"Joint between parent link {pid} and child link {cid}: {name}, axis {jd['local_axis']}")
        joint_data.append({"parent_link": pid, "child_link": cid, **jd, "type": name,
                           "counts": [int(x) for x in typ["counts"][j]]})
    return joint_data


def link_transforms(links, cm, time_step=0):
    """create_urdf's per-link transform (compute_joints.py:278-287): the float32 mean of the clusters' float32 matrices
    at time_step, from creg_link_clouds_f64 (no points)."""
    dev = _lib.device(getattr(cm, "_M", None))
    c = torch.as_tensor(np.asarray(cm.coords, np.float64)[time_step:time_step + 1], device=dev).contiguous()
    K = c.shape[1]
    M = torch.eye(4, dtype=torch.float64, device=dev).repeat(1, K, 1, 1)
    _, mm, _, _, _ = ops.link_clouds(c, M, [list(l["cluster_idx"]) for l in links],
                                     torch.zeros(0, 3, dtype=torch.float64, device=dev), np.zeros(K + 1, np.int64),
                                     mean_matrices=True)
    mm = mm[0].cpu().numpy()
    return {l["id"]: mm[i] for i, l in enumerate(links)}


def create_urdf(links, joint_data, cm, output_file="robot.urdf", mesh_dir="", time_step=0):
    """Write the estimated robot as URDF (compute_joints.py:274-388): same elements, names, attributes, mesh paths,
    layout and XML declaration.  A joint dict may carry "type" (``estimate_typed_joints_from_tree``; without the key the joint
    is revolute and every byte the reference's): "prismatic" writes the same origin and axis expressions with
    <limit ... lower="0.0" upper="0.0"> for ``set_joint_limits`` to fill, "fixed" the origin alone."""
    for joint in joint_data:
        if joint.get("type", "revolute") not in JOINT_UNITS:
            raise ValueError(f"joint_{joint['child_link']}: unknown joint type {joint['type']!r}")
    robot = ET.Element("robot", name="estimated_robot")
    link_transforms_ = link_transforms(links, cm, time_step)
    link_pos_local = {}
    for joint in joint_data:
        child_frame = link_transforms_[joint["child_link"]]
        link_pos_local[joint["child_link"]] = child_frame[:3, 3] - joint["global_pos"][:3]
    colors = [_jet(i / len(links)) for i in range(len(links))]
    for link in links:
        link_elem = ET.SubElement(robot, "link", name=f"link_{link['id']}")
        transform = link_transforms_[link["id"]]
        if link["parent_id"] is None:
            link_pos_local[link["id"]] = transform[:3, 3]
        xyz = " ".join(map(str, link_pos_local[link["id"]]))
        rpy = " ".join(map(str, np.zeros(3)))
        visual = ET.SubElement(link_elem, "visual")
        ET.SubElement(visual, "origin", xyz=xyz, rpy=rpy)
        geometry = ET.SubElement(visual, "geometry")
        mesh_filename = os.path.join(mesh_dir, f"{link['id']:04}.stl")
        ET.SubElement(geometry, "mesh", filename=mesh_filename, scale="1 1 1")
        material = ET.SubElement(visual, "material", name=f"material_{link['id']}")
        rgba = colors[link["id"]][:3] + (1,)
        ET.SubElement(material, "color", rgba=" ".join(map(str, rgba)))
        collision = ET.SubElement(link_elem, "collision")
        ET.SubElement(collision, "origin", xyz=xyz, rpy=rpy)
        geometry = ET.SubElement(collision, "geometry")
        ET.SubElement(geometry, "mesh", filename=mesh_filename, scale="1 1 1")
        inertial = ET.SubElement(link_elem, "inertial")
        ET.SubElement(inertial, "origin", xyz=xyz, rpy=rpy)
        ET.SubElement(inertial, "mass", value="1.0")
        ET.SubElement(inertial, "inertia", ixx="0.1", ixy="0.0", ixz="0.0", iyy="0.1", iyz="0.0", izz="0.1")
    for joint in joint_data:
        kind = joint.get("type", "revolute")
        joint_elem = ET.SubElement(robot, "joint", name=f"joint_{joint['child_link']}", type=kind)
        ET.SubElement(joint_elem, "parent", link=f"link_{joint['parent_link']}")
        ET.SubElement(joint_elem, "child", link=f"link_{joint['child_link']}")
        parent_transform = link_transforms_[joint["parent_link"]]
        child_transform = link_transforms_[joint["child_link"]]
        local_pos = np.linalg.inv(parent_transform) @ np.append(joint["global_pos"], 1)
        origin_xyz = " ".join(map(str, local_pos[:3] + link_pos_local[joint["parent_link"]]))
        relative_rot = np.linalg.inv(parent_transform[:3, :3]) @ child_transform[:3, :3]
        origin_rpy = " ".join(map(str, R.from_matrix(relative_rot).as_euler("xyz")))
        ET.SubElement(joint_elem, "origin", xyz=origin_xyz, rpy=origin_rpy)
        if kind == "fixed":                                       # no axis, no limit
            continue
        local_axis = np.linalg.inv(parent_transform[:3, :3]) @ np.append(joint["global_axis"], 0)[:3]
        local_axis = local_axis / np.linalg.norm(local_axis)
        ET.SubElement(joint_elem, "axis", xyz=" ".join(map(str, local_axis)))
        if kind == "prismatic":                                   # no placeholder range: set_joint_limits writes the observed one
            ET.SubElement(joint_elem, "limit", effort="100", velocity="100", lower="0.0", upper="0.0")
        else:
            ET.SubElement(joint_elem, "limit", effort="100", velocity="100", lower="-3.14159", upper="3.14159")
    tree = ET.ElementTree(robot)
    ET.indent(tree, space="  ", level=0)
    if os.path.dirname(output_file):
        os.makedirs(os.path.dirname(output_file), exist_ok=True)
    tree.write(output_file, encoding="utf-8", xml_declaration=True)
    print(f"URDF file saved as {output_file}")


def set_inertials(urdf_file, inertials):
    """Rewrite the <inertial> block of every link that ``inertials`` names (this project's own; ``link.link_inertia`` computes
    the values): inertials = {link name: {"mass", "com" (3), "inertia" (ixx, ixy, ixz, iyy, iyz, izz about com)}} in the
    MESH's frame.  The link's <visual><origin> (xyz t, rpy -> R, URDF's fixed-axis roll-pitch-yaw) maps the mesh into the link
    frame: origin xyz = R com + t with rpy 0 0 0, inertia = R I R^T.  Links not named keep their block; every other element,
    the indentation and the XML declaration stay as ``create_urdf`` wrote them.  A named link must already hold the block
    ``create_urdf`` writes -- <inertial> with <origin>, <mass> and <inertia> -- since only attributes are rewritten:
    ValueError naming the link otherwise, KeyError for a name the file does not have; nothing is written in either case."""
    tree = ET.parse(urdf_file)
    by_name = {l.get("name"): l for l in tree.getroot().findall("link")}
    for name, val in inertials.items():
        link = by_name[name]
        origin = link.find("visual/origin")
        attr = origin.attrib if origin is not None else {}         # URDF's defaults: no origin, or no attribute, is zero
        t = np.array(attr.get("xyz", "0 0 0").split(), np.float64)
        rpy = np.array(attr.get("rpy", "0 0 0").split(), np.float64)
        Rm = R.from_euler("xyz", rpy).as_matrix()                  # extrinsic x, y, z: Rz(yaw) Ry(pitch) Rx(roll)
        ixx, ixy, ixz, iyy, iyz, izz = np.asarray(val["inertia"], np.float64)
        I = Rm @ np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]]) @ Rm.T
        com = Rm @ np.asarray(val["com"], np.float64) + t
        inertial = link.find("inertial")
        if inertial is None or any(inertial.find(k) is None for k in ("origin", "mass", "inertia")):
            raise ValueError(f"{urdf_file}: link {name} has no <inertial> block with <origin>, <mass> and <inertia> to rewrite")
        inertial.find("origin").attrib.update(xyz=" ".join(map(str, com)), rpy=" ".join(map(str, np.zeros(3))))
        inertial.find("mass").set("value", str(float(val["mass"])))
        inertial.find("inertia").attrib.update(ixx=str(I[0, 0]), ixy=str(I[0, 1]), ixz=str(I[0, 2]), iyy=str(I[1, 1]),
                                               iyz=str(I[1, 2]), izz=str(I[2, 2]))
    tree.write(urdf_file, encoding="utf-8", xml_declaration=True)


def set_collision_meshes(urdf_file, suffix="_hull"):
    """Point every link's <collision><geometry><mesh> at the file ``link.link_mesh(..., hull=True)`` wrote (this project's own):
    the ``filename`` X.stl becomes X<suffix>.stl.  Nothing else changes: every other element and attribute, the indentation
    and the XML declaration stay as ``create_urdf`` wrote them.  Every link must hold the block ``create_urdf`` writes -- a
    <collision> with a <geometry><mesh> whose filename ends in .stl -- ValueError naming the link otherwise, and nothing is
    written in that case."""
    tree = ET.parse(urdf_file)
    for link in tree.getroot().findall("link"):
        mesh = link.find("collision/geometry/mesh")
        name = mesh.get("filename") if mesh is not None else None
        if name is None or not name.endswith(".stl"):
            raise ValueError(f"{urdf_file}: link {link.get('name')} has no <collision><geometry><mesh> with an .stl filename to rewrite")
        mesh.set("filename", name[:-len(".stl")] + suffix + ".stl")
    tree.write(urdf_file, encoding="utf-8", xml_declaration=True)


def estimate_joint_motion(links, joint_data, cm_list, start_step=0, num_steps=500, time_step=0):
    """Where every joint of ``joint_data`` stood at every step of every sequence, and how well "one revolute axis through one
    point" explains the two links' relative motion (this project's own; ``ops.link_poses`` and ``ops.joint_positions``, three
    launches in all).  The position is zero at sequence 0, step ``time_step``: the pose ``create_urdf`` writes as the URDF's
    zero.  One dict per joint, in ``joint_data``'s order: parent_link, child_link, positions (S,num_steps) rad unwrapped along
    each sequence, lower, upper (the observed range), lower_at, upper_at ((sequence, step) of each, None without a usable
    sample), tilt_rms, tilt_max (rad: the rotation the axis does not explain), slip_rms, slip_max (how far the joint point
    moves in the child's frame) and n_used (samples with finite figures).  No figure is turned into a verdict.  IndexError
    for steps past T, as numpy indexing would raise.
    Typed ``joint_data`` (``estimate_typed_joints_from_tree``): the revolute joints go through ``ops.joint_positions`` and the
    prismatic and fixed ones through ``ops.joint_slides`` -- a fixed joint with a zero axis -- one call of each kind at most,
    merged in ``joint_data``'s order.  A prismatic joint's positions, lower and upper are slides in the clouds' unit, its tilt
    the whole relative rotation and its slip the motion off the axis; a fixed joint's positions are zero.  Every dict then
    also carries "type" and "unit" ("rad", "length" for the clouds' unit, None for a fixed joint)."""
    by_id = {l["id"]: i for i, l in enumerate(links)}
    pairs = [(by_id[j["parent_link"]], by_id[j["child_link"]]) for j in joint_data]
    link_T = ops.link_poses(_coords(cm_list), [list(l["cluster_idx"]) for l in links])
    typed = any("type" in j for j in joint_data)
    kinds = [j.get("type", "revolute") for j in joint_data]
    turning = [i for i, k in enumerate(kinds) if k == "revolute"]
    sliding = [i for i, k in enumerate(kinds) if k != "revolute"]
    res = [None] * len(joint_data)                                 # per joint: its row of whichever call took it
    if turning or not sliding:
        out = ops.joint_positions(link_T, [pairs[i] for i in turning],
                                  np.array([joint_data[i]["local_axis"] for i in turning], np.float64).reshape(-1, 3),
                                  np.array([np.asarray(joint_data[i]["local_pos"], np.float64)[:3] for i in turning]).reshape(-1, 3),
                                  0, time_step, start_step, num_steps)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for row, i in enumerate(turning):
            res[i] = {k: v[row] for k, v in out.items()}
    if sliding:
        axes = np.array([joint_data[i]["local_axis"] if kinds[i] == "prismatic" else np.zeros(3) for i in sliding], np.float64)
        out = ops.joint_slides(link_T, [pairs[i] for i in sliding], axes.reshape(-1, 3), 0, time_step, start_step, num_steps)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for row, i in enumerate(sliding):
            res[i] = {k: v[row] for k, v in out.items()}
    motion = []
    for j, jd in enumerate(joint_data):
        used = int(res[j]["n_used"])
        at = lambda a: (int(a[0]), int(start_step + a[1])) if used else None
        m = {"parent_link": jd["parent_link"], "child_link": jd["child_link"], "positions": res[j]["q"],
             "lower_at": at(res[j]["lower_at"]), "upper_at": at(res[j]["upper_at"]), "n_used": used}
        m.update({k: float(res[j][k]) for k in ("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")})
        if typed:
            m.update(type=kinds[j], unit=JOINT_UNITS[kinds[j]])
        motion.append(m)
    return motion


def set_joint_limits(urdf_file, motion, pad=0.0):
    """Rewrite the <limit> of every joint ``motion`` names (``estimate_joint_motion``'s list; joint ``joint_{child_link}``) with
    its observed range: lower = min(lower - pad, 0), upper = max(upper + pad, 0) in rad, written with ``str()``, so the file's
    zero pose stays inside the limits.  A joint whose padded span reaches 2 pi becomes type="continuous" and loses lower and
    upper.  Effort, velocity, every other element, the indentation and the XML declaration stay as ``create_urdf`` wrote them.
    KeyError for a joint the file does not have, ValueError for one without a <limit>, with n_used = 0 or a negative pad;
    nothing is written in either case.  A motion dict may carry "type" (``estimate_joint_motion`` on typed joints): a
    prismatic joint gets lower = min(lower, 0), upper = max(upper, 0) in the clouds' unit -- ``pad`` is an angle and leaves it
    alone -- and never becomes continuous; a fixed joint has no limit and is skipped."""
    pad = float(pad)
    if not pad >= 0.0:
        raise ValueError(f"set_joint_limits: pad must be >= 0 rad, got {pad}")
    tree = ET.parse(urdf_file)
    by_name = {j.get("name"): j for j in tree.getroot().findall("joint")}
    todo = []
    for m in motion:
        name = f"joint_{m['child_link']}"
        joint = by_name[name]
        kind = m.get("type", "revolute")
        if kind == "fixed":
            continue
        limit = joint.find("limit")
        if limit is None:
            raise ValueError(f"{urdf_file}: joint {name} has no <limit> to rewrite")
        if m["n_used"] == 0 or not (np.isfinite(m["lower"]) and np.isfinite(m["upper"])):
            raise ValueError(f"{urdf_file}: joint {name} has no usable sample, its range is undefined")
        own_pad = pad if kind == "revolute" else 0.0               # the pad is an angle
        todo.append((joint, limit, min(float(m["lower"]) - own_pad, 0.0), max(float(m["upper"]) + own_pad, 0.0), kind))
    for joint, limit, lower, upper, kind in todo:
        if kind == "revolute" and upper - lower >= 2.0 * np.pi:
            joint.set("type", "continuous")
            for k in ("lower", "upper"):
                limit.attrib.pop(k, None)
        else:
            limit.attrib.update(lower=str(lower), upper=str(upper))
    tree.write(urdf_file, encoding="utf-8", xml_declaration=True)


def replay_urdf(urdf_file, links, motion, cm_list, start_step, num_steps, time_step=0):
    """Check the written URDF without a ground truth: pose it at every recovered joint position (and at zero) in one
    ``ops.urdf_fk`` call and compare how each link moved from the zero pose with how the registration saw it move from
    sequence 0, step ``time_step`` (``ops.link_poses``, ``ops.motion_error``; the compared point is the registered link
    position at that step).  The file's meshes are not read.  One dict per link, in ``links``' order: link (id), rot_rms,
    rot_max (rad), pos_rms, pos_max (the clouds' unit), rot_max_at, pos_max_at ((sequence, step), None when no sample is
    finite) and n_used."""
    from .sim_data import UrdfRobot
    robot = UrdfRobot(urdf_file, load_meshes=False)
    coords = _coords(cm_list)
    reg = ops.link_poses(coords, [list(l["cluster_idx"]) for l in links])      # (S,T,L,4,4)
    S, n, n_links = reg.shape[0], int(num_steps), len(links)
    if start_step < 0 or n < 1 or start_step + n > reg.shape[1]:
        raise IndexError(f"steps [{start_step}, {start_step + n}) are out of bounds for axis 0 with size {reg.shape[1]}")
    q_by_name = {f"joint_{m['child_link']}": np.asarray(m["positions"], np.float64).reshape(S, n) for m in motion}
    names = robot.fk_table()["names"]
    q = np.zeros((S * n + 1, len(names)))                                      # the last row is the zero pose
    for col, name in enumerate(names):
        if name in q_by_name:
            q[:-1, col] = q_by_name[name].reshape(-1)
    fk = ops.urdf_fk(robot.fk_table(), q, np.eye(4))                           # (S*n+1, L_urdf, 4, 4)
    order = torch.as_tensor([robot.link_index[f"link_{l['id']}"] for l in links], device=fk.device)
    fk = fk[:, order]
    B = reg[:, start_step:start_step + n].reshape(S * n, n_links, 4, 4)
    B0 = reg[0, time_step].contiguous()
    rot, pos = ops.motion_error(fk[:-1].contiguous(), fk[-1].contiguous(), B.contiguous(), B0, B0[:, :3, 3].contiguous())
    rot, pos = rot.cpu().numpy().reshape(S, n, n_links), pos.cpu().numpy().reshape(S, n, n_links)
    report = []
    for i, l in enumerate(links):
        ok = np.isfinite(rot[:, :, i]) & np.isfinite(pos[:, :, i])
        r = {"link": l["id"], "n_used": int(ok.sum())}
        for key, e in (("rot", rot[:, :, i]), ("pos", pos[:, :, i])):
            if ok.any():
                e = np.where(ok, e, -np.inf)
                s, k = np.unravel_index(np.argmax(e), e.shape)
                r.update({f"{key}_rms": float(np.sqrt((e[ok] ** 2).sum() / ok.sum())), f"{key}_max": float(e[s, k]),
                          f"{key}_max_at": (int(s), int(start_step + k))})
            else:
                r.update({f"{key}_rms": float("nan"), f"{key}_max": float("nan"), f"{key}_max_at": None})
        report.append(r)
    return report


def _fit_figures(dist):
    """n, mean, rms, p95, max, max_at and unexplained of one set of distances: the statistics cover the finite ones."""
    dist = np.asarray(dist, np.float64)
    ok = np.isfinite(dist)
    out = {"n": int(dist.size), "unexplained": int(dist.size - ok.sum())}
    if ok.any():
        d = dist[ok]
        out.update(mean=float(d.mean()), rms=float(np.sqrt((d * d).sum() / d.size)), p95=float(np.percentile(d, 95)),
                   max=float(d.max()), max_at=int(np.flatnonzero(ok)[np.argmax(d)]))
    else:
        out.update(mean=float("nan"), rms=float("nan"), p95=float("nan"), max=float("nan"), max_at=None)
    return out


def cloud_fit_poses(robot, link_T, clouds, d_max=np.inf):
    """How well a robot's meshes, posed by ``link_T``, explain one cloud per pose (this project's own): robot a ``UrdfRobot``
    loaded with its meshes, link_T (P,L,4,4) device poses in ``robot.links``' order (``ops.urdf_fk``), clouds a list of P (n_p,3)
    arrays of world points.  ONE ``ops.point_mesh_distance`` call for all poses.  Returns a dict:
    "poses", one dict per pose with n, mean, rms, p95, max, max_at (the point's row in its cloud) and unexplained (points
    farther than ``d_max`` from every triangle, or NaN; their distance is ``inf``), the statistics over the finite distances;
    "links", one dict per link with link (name), n (finite points whose nearest triangle is the link's) and rms; "all", the
    pose figures over every point (max_at a (pose, row) pair); and "dist" / "link", lists of P host arrays with every point's
    distance and link index (-1 where no triangle was within ``d_max``).  No threshold turns a figure into a verdict.  Not seen
    from this side: mesh surface that no point lies near (``surface_cover_poses`` measures that direction), and a wrong link
    that happens to lie on the right surface."""
    dev = link_T.device
    if link_T.dim() == 3:
        link_T = link_T[None]
    if len(clouds) != link_T.shape[0]:
        raise ValueError(f"cloud_fit_poses: {link_T.shape[0]} poses need as many clouds, got {len(clouds)}")
    parts = [np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]
    cut = np.concatenate([[0], np.cumsum([len(c) for c in parts])]).astype(np.int64)
    pts = torch.as_tensor(np.concatenate(parts) if parts else np.zeros((0, 3)), device=dev)
    tri = torch.as_tensor(np.ascontiguousarray(robot.tri, np.float64).reshape(-1, 3, 3), device=dev)
    dist, _, link = ops.point_mesh_distance(tri, torch.as_tensor(robot.tri_start, device=dev), link_T, pts,
                                            torch.as_tensor(cut, device=dev), d_max)
    dist, link = dist.cpu().numpy(), link.cpu().numpy()
    poses = [_fit_figures(dist[cut[p]:cut[p + 1]]) for p in range(len(parts))]
    overall = _fit_figures(dist)
    if overall["max_at"] is not None:
        p = int(np.searchsorted(cut, overall["max_at"], side="right") - 1)
        overall["max_at"] = (p, int(overall["max_at"] - cut[p]))
    ok = np.isfinite(dist)
    per_link = []
    for l, name in enumerate(robot.links):
        d = dist[ok & (link == l)]
        per_link.append({"link": name, "n": int(d.size), "rms": float(np.sqrt((d * d).sum() / d.size)) if d.size else float("nan")})
    return {"poses": poses, "links": per_link, "all": overall,
            "dist": [dist[cut[p]:cut[p + 1]] for p in range(len(parts))], "link": [link[cut[p]:cut[p + 1]] for p in range(len(parts))]}


def cloud_fit_link_poses(urdf_file, links, motion, cm_list, start_step, num_steps, time_step=0):
    """The poses ``cloud_fit`` puts the URDF's meshes at -> (robot, link_T (S*num_steps,L,4,4) device poses in ``robot.links``'
    order): the file with its meshes (``UrdfRobot(path)``: every visual origin as written), the ``q`` rows of ``replay_urdf``
    through one ``ops.urdf_fk`` call, and every pose moved by the registered motion of the root link,
    G = reg[s,t,root] reg[0,time_step,root]^-1 from ``ops.link_poses`` (the raw clouds carry a per-frame translation that the
    URDF's fixed base does not): link_T = G A(q).  The file is taken at its word.  ``create_urdf`` keeps the reference's origin
    expressions, which add offsets taken in the world frame to offsets taken in link frames; they hold when the registered link
    frames of (sequence 0, ``time_step``) are unrotated, which is how the registration defines step 0 (DESIGN N4 has the
    figures for both cases).  At another ``time_step`` the file's zero pose is off, and this check says so, as the replay does."""
    robot, q, G = _cloud_fit_state(urdf_file, links, motion, cm_list, start_step, num_steps, time_step)
    fk = ops.urdf_fk(robot.fk_table(), q, np.eye(4))                           # (S*n, L_urdf, 4, 4)
    return robot, (G[:, None] @ fk).contiguous()


def _cloud_fit_state(urdf_file, links, motion, cm_list, start_step, num_steps, time_step=0):
    """(robot, q (S*num_steps,J) host rows in ``fk_table()``'s order, G (S*num_steps,4,4) device root motions) of
    ``cloud_fit_link_poses``: what the cloud fit poses the file by, and what ``fit_positions`` starts from."""
    from .sim_data import UrdfRobot
    robot = UrdfRobot(urdf_file)
    coords = _coords(cm_list)
    reg = ops.link_poses(coords, [list(l["cluster_idx"]) for l in links])      # (S,T,L,4,4)
    S, n = reg.shape[0], int(num_steps)
    if start_step < 0 or n < 1 or start_step + n > reg.shape[1]:
        raise IndexError(f"steps [{start_step}, {start_step + n}) are out of bounds for axis 0 with size {reg.shape[1]}")
    q_by_name = {f"joint_{m['child_link']}": np.asarray(m["positions"], np.float64).reshape(S, n) for m in motion}
    names = robot.fk_table()["names"]
    q = np.zeros((S * n, len(names)))
    for col, name in enumerate(names):
        if name in q_by_name:
            q[:, col] = q_by_name[name].reshape(-1)
    (root,) = [i for i, l in enumerate(links) if l["parent_id"] is None]
    G = reg[:, start_step:start_step + n, root].reshape(S * n, 4, 4) @ torch.linalg.inv(reg[0, time_step, root])
    return robot, q, G


def cloud_fit(urdf_file, links, motion, cm_list, raw_dirs, start_step, num_steps, time_step=0, d_max=np.inf):
    """Check the written URDF against the raw clouds it was made from (this project's own): the file's meshes, posed by the
    file's joints at the recovered positions of every step of every sequence (``cloud_fit_link_poses``), against that step's
    ``robot.ply`` under ``raw_dirs[s]`` (``cluster_icp.read_point_cloud``), in one ``cloud_fit_poses`` call, whose dict is
    returned with "sequences" added: the pose figures over each sequence's points (max_at a (step, row) pair).  Pose
    s * num_steps + k is step ``start_step + k`` of sequence s.  Distances are in the clouds' unit."""
    from .cluster_icp import read_point_cloud
    robot, link_T = cloud_fit_link_poses(urdf_file, links, motion, cm_list, start_step, num_steps, time_step)
    S, n = len(cm_list), int(num_steps)
    clouds = [np.asarray(read_point_cloud(os.path.join(raw_dirs[s], f"{start_step + k:04}", "robot.ply")).points, np.float64)
              for s in range(S) for k in range(n)]
    fit = cloud_fit_poses(robot, link_T, clouds, d_max)
    fit["sequences"] = []
    for s in range(S):
        sizes = [len(c) for c in clouds[s * n:(s + 1) * n]]
        cut = np.concatenate([[0], np.cumsum(sizes)])
        fig = _fit_figures(np.concatenate(fit["dist"][s * n:(s + 1) * n]) if n else np.zeros(0))
        if fig["max_at"] is not None:
            k = int(np.searchsorted(cut, fig["max_at"], side="right") - 1)
            fig["max_at"] = (int(start_step + k), int(fig["max_at"] - cut[k]))
        fit["sequences"].append(fig)
    return fit


def subdivide_mesh(tri, tri_start, max_edge):
    """Split every triangle with an edge longer than ``max_edge`` into four at its edge midpoints, until none is left (host
    numpy): tri (F,3,3), tri_start (L+1) -> (tri (F',3,3) f64, tri_start (L+1) int64, parent_row (F') int64 the input row every
    output row is a part of).  A triangle's parts take its place, so the rows stay grouped by link and in the input's order; the
    surface and its area are unchanged, and a mesh already fine comes back as it was.  ``mesh_cover`` counts a triangle as
    covered when a point is near any part of it, so the triangle is the resolution of that measurement: a mesh with triangles
    larger than the points' spacing is subdivided first (``surface_cover_poses(..., max_edge=...)``)."""
    tri = np.array(tri, np.float64).reshape(-1, 3, 3)
    tri_start = np.asarray(tri_start, np.int64)
    max_edge = float(max_edge)
    if not max_edge > 0.0:
        raise ValueError(f"subdivide_mesh: max_edge must be > 0, got {max_edge}")
    if not np.isfinite(tri).all():
        raise ValueError("subdivide_mesh: the triangles must be finite")
    parent = np.arange(len(tri), dtype=np.int64)
    while True:
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        longest = np.maximum(np.maximum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1)), np.linalg.norm(a - c, axis=1))
        split = longest > max_edge
        if not split.any():
            break
        count = np.where(split, 4, 1)
        at = np.cumsum(count) - count                                          # the first output row of every input row
        src = np.repeat(np.arange(len(tri)), count)
        out, parent = tri[src], parent[src]
        s = np.flatnonzero(split)
        a, b, c = a[s], b[s], c[s]
        ab, bc, ca = (a + b) * 0.5, (b + c) * 0.5, (c + a) * 0.5
        for k, part in enumerate(((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))):
            out[at[s] + k] = np.stack(part, 1)
        tri = out
    owner = np.searchsorted(tri_start, parent, side="right") - 1
    return tri, np.searchsorted(owner, np.arange(len(tri_start)), side="left").astype(np.int64), parent


def _cover_figures(area, dist, n_near):
    """The figures of one set of poses: area (F) per triangle, dist and n_near (p,F) -> area (of the mesh, one pose), uncovered
    (area share of the triangles with dist = inf, over all p poses), mean, rms, p95 and max over the covered triangles weighted
    by area (p95: the smallest distance at which the covered area at or below it reaches 95 %), max_at ((pose, row), the first
    such) and thin (area share of the triangles covered with n_near == 1)."""
    area, dist, n_near = np.asarray(area, np.float64), np.asarray(dist, np.float64), np.asarray(n_near)
    w = np.broadcast_to(area, dist.shape)
    ok = np.isfinite(dist)
    total = float(w.sum())
    share = lambda mask: float(w[mask].sum() / total) if total > 0 else float("nan")
    out = {"area": float(area.sum()), "uncovered": share(~ok), "thin": share(ok & (n_near == 1))}
    wk, d = w[ok], dist[ok]
    if wk.sum() > 0:
        order = np.argsort(d, kind="stable")
        cum = np.cumsum(wk[order])
        k = min(int(np.searchsorted(cum, 0.95 * cum[-1], side="left")), len(order) - 1)
        flat = int(np.flatnonzero(ok.reshape(-1))[np.argmax(d)])
        out.update(mean=float((wk * d).sum() / wk.sum()), rms=float(np.sqrt((wk * d * d).sum() / wk.sum())), p95=float(d[order[k]]),
                   max=float(d.max()), max_at=(flat // dist.shape[1], flat % dist.shape[1]))
    else:
        out.update(mean=float("nan"), rms=float("nan"), p95=float("nan"), max=float("nan"), max_at=None)
    return out


def surface_cover_poses(robot, link_T, clouds, d_max=np.inf, max_edge=None):
    """How much of a robot's mesh surface, posed by ``link_T``, has a point of its pose's cloud near it (this project's own): the
    other direction of ``cloud_fit_poses``, with its arguments; it sees a link posed where no cloud is, a link that exists twice
    and a bloated mesh, which leave every cloud point explained.  ONE ``ops.mesh_cover`` call for all poses.  With ``max_edge`` the
    meshes are subdivided first (``subdivide_mesh``): a triangle counts as covered when a point is within ``d_max`` of any part of
    it.  All shares are shares of area (link-frame areas; poses are rigid).  Returns a dict:
    "poses", one dict per pose with area, uncovered (area share of the triangles farther than ``d_max`` from every point; their
    distance is ``inf``), mean, rms, p95 and max of the distance over the covered triangles, weighted by area, max_at (the
    triangle's row) and thin (area share of the triangles covered by exactly one point within ``d_max``);
    "links", one dict per link with link (name), area, uncovered (over all poses), rms, and never, the area share of its
    triangles covered in NO pose -- the figure that survives a surface being out of a frame's sight;
    "all", the pose figures over every pose (max_at a (pose, row) pair) and never;
    "dist" and "n_near" (P,F) and "seen" (F: covered in some pose) as host arrays, "area" (F) and "tri_start" (L+1) of the mesh
    that was measured, and "parent_row" (F) when it was subdivided.  No threshold turns a figure into a verdict.  Not seen from
    this side either: which camera could have seen a surface; a surface none ever sees counts as uncovered."""
    dev = link_T.device
    if link_T.dim() == 3:
        link_T = link_T[None]
    if len(clouds) != link_T.shape[0]:
        raise ValueError(f"surface_cover_poses: {link_T.shape[0]} poses need as many clouds, got {len(clouds)}")
    tri, tri_start, parent = np.ascontiguousarray(robot.tri, np.float64).reshape(-1, 3, 3), np.asarray(robot.tri_start, np.int64), None
    if max_edge is not None:
        tri, tri_start, parent = subdivide_mesh(tri, tri_start, max_edge)
    parts = [torch.as_tensor(c, dtype=torch.float64).reshape(-1, 3).to(dev) for c in clouds]
    cut = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    pts = torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.float64, device=dev)
    dist, _, n_near = ops.mesh_cover(torch.as_tensor(tri, device=dev), torch.as_tensor(tri_start, device=dev), link_T, pts,
                                     torch.as_tensor(cut, device=dev), d_max)
    dist, n_near = dist.cpu().numpy(), n_near.cpu().numpy()
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    seen = np.isfinite(dist).any(0)
    never = lambda rows: float(area[rows][~seen[rows]].sum() / area[rows].sum()) if area[rows].sum() > 0 else float("nan")
    poses = []
    for p in range(dist.shape[0]):
        fig = _cover_figures(area, dist[p:p + 1], n_near[p:p + 1])
        fig["max_at"] = None if fig["max_at"] is None else fig["max_at"][1]
        poses.append(fig)
    per_link = []
    for l, name in enumerate(robot.links):
        rows = slice(int(tri_start[l]), int(tri_start[l + 1]))
        fig = _cover_figures(area[rows], dist[:, rows], n_near[:, rows])
        per_link.append({"link": name, "area": fig["area"], "uncovered": fig["uncovered"], "rms": fig["rms"], "never": never(rows)})
    overall = dict(_cover_figures(area, dist, n_near), never=never(slice(0, len(area))))
    out = {"poses": poses, "links": per_link, "all": overall, "dist": dist, "n_near": n_near, "seen": seen, "area": area,
           "tri_start": tri_start}
    if parent is not None:
        out["parent_row"] = parent
    return out


def cloud_cover(urdf_file, links, motion, cm_list, raw_dirs, start_step, num_steps, time_step=0, d_max=np.inf):
    """The other direction of ``cloud_fit`` (this project's own): how much of the written URDF's mesh surface, at the poses of
    ``cloud_fit_link_poses``, has a point of that step's raw cloud within ``d_max`` -- the clouds ``cloud_fit`` reads, in one
    ``surface_cover_poses`` call, whose dict is returned with "sequences" added: the pose figures over each sequence's poses
    (max_at a (step, row) pair).  Pose s * num_steps + k is step ``start_step + k`` of sequence s.  The meshes this project writes
    have triangles no larger than a voxel and are measured as they are."""
    from .cluster_icp import read_point_cloud
    robot, link_T = cloud_fit_link_poses(urdf_file, links, motion, cm_list, start_step, num_steps, time_step)
    S, n = len(cm_list), int(num_steps)
    clouds = [np.asarray(read_point_cloud(os.path.join(raw_dirs[s], f"{start_step + k:04}", "robot.ply")).points, np.float64)
              for s in range(S) for k in range(n)]
    cover = surface_cover_poses(robot, link_T, clouds, d_max)
    cover["sequences"] = []
    for s in range(S):
        fig = _cover_figures(cover["area"], cover["dist"][s * n:(s + 1) * n], cover["n_near"][s * n:(s + 1) * n])
        if fig["max_at"] is not None:
            fig["max_at"] = (int(start_step + fig["max_at"][0]), int(fig["max_at"][1]))
        cover["sequences"].append(fig)
    return cover


FIT_METRICS = ("point", "feature")                                              # the curvature of the two Levenberg-Marquardt drivers
FIT_LAMBDA_MIN, FIT_LAMBDA_STOP = 1e-12, 1e8                                   # the floor of the damping, and where a pose gives up


def _base_steps(delta, center):
    """(P,4,4) rigid motions X -> R(w)(X - center) + center + v of base steps delta (P,6) = w | v: Rodrigues' formula, exact; below
    an angle of 1e-8 the two series' leading terms stand in for sin t / t and (1 - cos t) / t^2 (their error is below 1e-17)."""
    w, v = delta[:, :3], delta[:, 3:6]
    t = torch.linalg.vector_norm(w, dim=1)
    tiny = t < 1e-8
    ts = torch.where(tiny, torch.ones_like(t), t)
    a = torch.where(tiny, torch.ones_like(t), torch.sin(ts) / ts)
    b = torch.where(tiny, torch.full_like(t, 0.5), (1.0 - torch.cos(ts)) / (ts * ts))
    K = torch.zeros(len(w), 3, 3, dtype=w.dtype, device=w.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    R = torch.eye(3, dtype=w.dtype, device=w.device) + a[:, None, None] * K + b[:, None, None] * (K @ K)
    U = torch.zeros(len(w), 4, 4, dtype=w.dtype, device=w.device)
    U[:, :3, :3], U[:, 3, 3] = R, 1.0
    U[:, :3, 3] = center + v - (R @ center[:, :, None])[:, :, 0]
    return U


def _fit_arguments(who, J, clouds, q0, base0, d_max, max_iter, lam0, dev):
    """The arguments ``fit_cloud_poses`` and ``refine_joint_frames`` share, checked (ValueError with ``who`` in front) and coerced ->
    (d_max, max_iter, parts: the P clouds as (n_p,3) host arrays, q (P,J) and G (P,4,4): fresh f64 device tensors)."""
    d_max, max_iter = float(d_max), int(max_iter)
    if not d_max >= 0.0 or max_iter < 0 or not lam0 > 0.0:
        raise ValueError(f"{who}: d_max >= 0, max_iter >= 0 and lam0 > 0 expected, got {d_max}, {max_iter}, {lam0}")
    parts = [np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]
    P = len(parts)
    q = torch.as_tensor(np.array(q0, np.float64).reshape(-1, J) if not isinstance(q0, torch.Tensor) else q0, dtype=torch.float64, device=dev).clone()
    if P < 1 or tuple(q.shape) != (P, J):
        raise ValueError(f"{who}: {P} clouds need q0 ({P},{J}), got {tuple(q.shape)}")
    G = torch.eye(4, dtype=torch.float64, device=dev) if base0 is None else torch.as_tensor(base0, dtype=torch.float64, device=dev)
    if tuple(G.shape) not in ((4, 4), (P, 4, 4)):
        raise ValueError(f"{who}: base0 must be (4,4) or ({P},4,4), got {tuple(G.shape)}")
    return d_max, max_iter, parts, q, G.expand(P, 4, 4).clone()


def _joint_rows(who, names, items, what=""):
    """The table rows of ``items``, joint names or rows (``what`` names the argument in the ValueError for an unknown name)."""
    out = set()
    for item in items:
        if isinstance(item, str) and item not in names:
            raise ValueError(f"{who}: no joint named {item!r} among {names}" + (f" ({what})" if what else ""))
        out.add(names.index(item) if isinstance(item, str) else int(item))
    return out


def _pack_clouds(parts, robot, dev):
    """The clouds of a fit on the device, packed for ``ops.point_mesh_distance``: pts (N,3), cut (P+1) its pt_start, pose_of (N),
    live (N) not NaN, n_live (P) f64, center (P,3) the mean of a pose's live points, and the robot's tri (F,3,3) and tri_start."""
    P = len(parts)
    cut_host = np.concatenate([[0], np.cumsum([len(c) for c in parts])]).astype(np.int64)
    pts = torch.as_tensor(np.concatenate(parts) if cut_host[-1] else np.zeros((0, 3)), device=dev)
    cut = torch.as_tensor(cut_host, device=dev)
    pose_of = torch.repeat_interleave(torch.arange(P, device=dev), cut[1:] - cut[:-1])
    live = ~torch.isnan(pts).any(1)
    n_live = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, pose_of, live.to(torch.float64))
    center = torch.zeros(P, 3, dtype=torch.float64, device=dev).index_add_(0, pose_of, torch.where(live[:, None], pts, torch.zeros_like(pts)))
    center = center / n_live.clamp_min(1.0)[:, None]
    tri = torch.as_tensor(np.ascontiguousarray(robot.tri, np.float64).reshape(-1, 3, 3), device=dev)
    tri_start = torch.as_tensor(robot.tri_start, device=dev)
    return SimpleNamespace(pts=pts, cut=cut, pose_of=pose_of, live=live, n_live=n_live, center=center, tri=tri, tri_start=tri_start)


def _truncated_cost(c, tri, link_T, d_max):
    """Steps 2 and 3 of an iteration on the clouds ``c`` of ``_pack_clouds``: one ``ops.point_mesh_distance`` call -> (tri_idx (N),
    cost (P) the sum of min(d^2, d_max^2) over a pose's live points, within (P) int64 its live points within ``d_max``)."""
    dist, tri_idx, _ = ops.point_mesh_distance(tri, c.tri_start, link_T, c.pts, c.cut, d_max)
    d2 = torch.where(c.live, torch.clamp(dist * dist, max=d_max * d_max), torch.zeros_like(dist))
    cost = torch.zeros(len(c.n_live), dtype=torch.float64, device=dist.device).index_add_(0, c.pose_of, d2)
    within = torch.zeros(len(c.n_live), dtype=torch.int64, device=dist.device).index_add_(0, c.pose_of, (c.live & torch.isfinite(dist)).to(torch.int64))
    return tri_idx, cost, within


def _rms(n_live, cost):
    """sqrt(cost / live points) per pose on the host, NaN for a pose without live points."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n_live > 0, np.sqrt(cost / np.maximum(n_live, 1.0)), np.nan)


def _fit_metric(who, metric):
    if metric not in FIT_METRICS:
        raise ValueError(f"{who}: metric must be one of {FIT_METRICS}, got {metric!r}")
    return metric


def fit_cloud_poses(robot, clouds, q0, base0=None, d_max=np.inf, max_iter=30, fit_base=True, lock=(), lam0=1e-3, tol=1e-10,
                    metric="point"):
    """Fit a robot's joint values and base pose to one cloud per pose by Levenberg-Marquardt on the point-to-mesh distance (this
    project's own): robot a ``UrdfRobot`` loaded with its meshes, clouds a list of P (n_p,3) arrays of world points, q0 (P,J) the
    starting joint values in ``robot.fk_table()``'s order, base0 (4,4) or (P,4,4) the starting root poses (identity when None).
    The state is q (P,J) and G (P,4,4); all P poses advance in lock-step, every device call covers all of them.  An iteration:
      1  link_T = G urdf_fk(q), as ``cloud_fit_link_poses`` composes it
      2  one ``ops.point_mesh_distance`` call
      3  per pose the truncated cost, sum of min(d^2, d_max^2) over the live (not NaN) points
      4  the last step of a pose is accepted iff its cost did not rise: lambda <- max(lambda / 10, 1e-12); otherwise the pose's
         state is restored and lambda <- 10 lambda
      5  ``ops.pose_fit_system`` (a pose whose step was rejected keeps the system of the state it went back to)
      6  (H_f + lambda diag(H_f)) delta = g_f over the free parameters, batched in fp64 on the device (``torch.linalg``).  Left
         out: fixed joints, the joints named in ``lock`` (names or table rows), the base when ``fit_base`` is False, and a
         parameter whose diagonal entry is exactly 0 -- no matched point moves with it; it gets delta = 0 and is reported in
         ``unobserved``.  A failed factorisation counts as a rejection: no step, lambda <- 10 lambda
      7  q += delta_q and G_p <- [X -> R(w)(X - center_p) + center_p + v] G_p, center_p the mean of the pose's live points
    A pose stops when an accepted step has max |delta| < ``tol``, when lambda > 1e8, or after ``max_iter`` steps.  ``lam0``,
    ``tol``, the floor and the factors of 10 are settings of the algorithm, not measurements.  Returns a dict of host values: q
    (P,J), base (P,4,4), cost_history (P lists, non-increasing by construction: the first entry is the start, one more per step
    tried), iterations (P) steps tried, rms_before and rms_after (P) = sqrt(cost / live points), unobserved (P,6+J) bool in the
    order rotation, translation, joints, n (P) the points within ``d_max`` at the returned state, and names (the joints' names in
    the table's order).
    ``metric`` chooses the curvature of step 5 alone; the cost, the gradient, the accept rule, the stops and every returned figure
    are the same.  "point": H = sum J^T J of ``ops.pose_fit_system`` (6 + J <= 64), which converges linearly along a surface.
    "feature": H = sum J^T Pi J, Pi the projector onto the normal space of the vertex, edge or face each point matched -- the exact
    Hessian of the squared distance to that feature -- from one ``ops.link_moments(metric="feature")`` call about center_p,
    ``link_twists(structure=False)`` and ``twist_system``; no cap on the joint count.  With a ``d_max`` well below the starting
    misalignment the feature step has been seen to jump far while the truncated cost still fell: keep ``d_max`` above it.
    Not done here: joint limits, warm starts from a neighbouring frame."""
    metric = _fit_metric("fit_cloud_poses", metric)
    table = robot.fk_table()
    names, kinds = list(table["names"]), np.asarray(table["type"])
    J, D = len(names), 6 + len(names)
    dev = _lib.device()
    d_max, max_iter, parts, q, G = _fit_arguments("fit_cloud_poses", J, clouds, q0, base0, d_max, max_iter, lam0, dev)
    P = len(parts)
    locked = _joint_rows("fit_cloud_poses", names, lock)
    free0 = np.array([bool(fit_base)] * 6 + [kinds[j] in (1, 2) and j not in locked for j in range(J)])
    free0 = torch.as_tensor(free0, device=dev)
    c = _pack_clouds(parts, robot, dev)
    pts, cut, n_live, center, tri, tri_start, eye = c.pts, c.cut, c.n_live, c.center, c.tri, c.tri_start, np.eye(4)
    lam = torch.full((P,), float(lam0), dtype=torch.float64, device=dev)
    active = n_live > 0
    stepped = torch.zeros(P, dtype=torch.bool, device=dev)
    small = torch.zeros(P, dtype=torch.bool, device=dev)
    iters = torch.zeros(P, dtype=torch.int64, device=dev)
    unobserved = torch.zeros(P, D, dtype=torch.bool, device=dev)
    H_cur = g_cur = cost_cur = n_cur = q_prev = G_prev = None
    history = []
    for it in range(max_iter + 1):
        link_T = (G[:, None] @ ops.urdf_fk(table, q, eye)).contiguous()
        tri_idx, cost, within = _truncated_cost(c, tri, link_T, d_max)
        if it == 0:
            accept, cost_cur, n_cur = torch.ones(P, dtype=torch.bool, device=dev), cost, within
        else:
            accept = stepped & (cost <= cost_cur)
            back = stepped & ~accept
            q, G = torch.where(back[:, None], q_prev, q), torch.where(back[:, None, None], G_prev, G)
            lam = torch.where(accept, (lam / 10.0).clamp_min(FIT_LAMBDA_MIN), torch.where(back, lam * 10.0, lam))
            cost_cur, n_cur = torch.where(accept, cost, cost_cur), torch.where(accept, within, n_cur)
            active = active & ~(accept & small) & ~(lam > FIT_LAMBDA_STOP)
        history.append(cost_cur)
        if it == max_iter or not bool(active.any()):
            break
        if metric == "feature":
            ref = center[:, None, :].expand(P, link_T.shape[1], 3).contiguous()
            mom, cnt, fmom = ops.link_moments(tri, tri_start, link_T, pts, cut, tri_idx, ref, d_max, metric="feature")
            H, g, _ = twist_system(mom, cnt, link_twists(table, link_T, q, center, ref, structure=False), fmom)
        else:
            H, g, _, _ = ops.pose_fit_system(tri, tri_start, link_T, pts, cut, tri_idx, table, center, d_max)
        if H_cur is None:
            H_cur, g_cur = H, g
        else:
            H_cur, g_cur = torch.where(accept[:, None, None], H, H_cur), torch.where(accept[:, None], g, g_cur)
        diag = torch.diagonal(H_cur, dim1=1, dim2=2)
        free = free0[None] & (diag != 0.0)
        unobserved = torch.where(active[:, None], free0[None] & (diag == 0.0), unobserved)
        m = free.to(torch.float64)
        A = H_cur * m[:, :, None] * m[:, None, :] + torch.diag_embed(lam[:, None] * diag * m + (1.0 - m))
        chol, info = torch.linalg.cholesky_ex(A)
        delta = torch.cholesky_solve((g_cur * m)[:, :, None], chol)[:, :, 0]
        failed = (info != 0) | ~torch.isfinite(delta).all(1)
        stepped = active & ~failed
        delta = torch.where(stepped[:, None] & free, delta, torch.zeros_like(delta))
        lam = torch.where(active & failed, lam * 10.0, lam)
        iters = iters + active.to(torch.int64)
        small = delta.abs().amax(1) < tol
        q_prev, G_prev = q, G
        q = torch.where(delta[:, 6:] != 0.0, q + delta[:, 6:], q)
        moved = (delta[:, :6] != 0.0).any(1)
        G = torch.where(moved[:, None, None], _base_steps(delta[:, :6], center) @ G, G)
    history = torch.stack(history).cpu().numpy()
    iters = iters.cpu().numpy()
    n_live = n_live.cpu().numpy()
    return {"q": q.cpu().numpy(), "base": G.cpu().numpy(),
            "cost_history": [history[:min(int(iters[p]), len(history) - 1) + 1, p].tolist() for p in range(P)],
            "iterations": iters, "rms_before": _rms(n_live, history[0]), "rms_after": _rms(n_live, history[-1]),
            "unobserved": unobserved.cpu().numpy(), "n": n_cur.cpu().numpy(), "names": names}


def fit_positions(urdf_file, links, motion, cm_list, raw_dirs, start_step, num_steps, time_step=0, d_max=np.inf, max_iter=30,
                  metric="point"):
    """Fit the written URDF's joint positions to the raw clouds, frame by frame (this project's own): the poses of ``cloud_fit``
    -- the replay's ``q`` rows and the registered root motion G -- are the start, every frame is fitted with the base free
    (``fit_cloud_poses``, which states ``metric``), ``d_max`` is the cloud fit's limit.  Returns ``fit_cloud_poses``' dict with
    "positions" added, the fitted values (J,S,num_steps) in the order of ``motion`` (the layout of ``joint_positions.npy``), and "shift" (J), per joint
    the largest |q_fit - q_registered|.  The URDF and its limits are not touched."""
    from .cluster_icp import read_point_cloud
    robot, q, G = _cloud_fit_state(urdf_file, links, motion, cm_list, start_step, num_steps, time_step)
    S, n = len(cm_list), int(num_steps)
    clouds = [np.asarray(read_point_cloud(os.path.join(raw_dirs[s], f"{start_step + k:04}", "robot.ply")).points, np.float64)
              for s in range(S) for k in range(n)]
    fit = fit_cloud_poses(robot, clouds, q, G, d_max=d_max, max_iter=max_iter, fit_base=True, metric=metric)
    positions = np.array([np.asarray(m["positions"], np.float64).reshape(S, n) for m in motion]).reshape(len(motion), S, n)
    shift = np.zeros(len(motion))
    for j, m in enumerate(motion):
        name = f"joint_{m['child_link']}"
        if name in fit["names"]:
            fitted = fit["q"][:, fit["names"].index(name)].reshape(S, n)
            shift[j] = float(np.abs(fitted - positions[j]).max())
            positions[j] = fitted
    fit["positions"], fit["shift"] = positions, shift
    return fit


# ------------------------------------------------------------------------------------------ refining the joint frames
def joint_frame_basis(axis):
    """u1, u2 (J,3) host arrays of the table's unit axes (J,3): k the index of the smallest |a_k| (the lowest at a tie),
    u1 = normalize(a x e_k), u2 = a x u1.  A joint's frame parameters turn about and shift along these two: the component of a
    frame twist along the axis itself moves nothing."""
    axis = np.asarray(axis, np.float64).reshape(-1, 3)
    e = np.eye(3)[np.argmin(np.abs(axis), axis=1)]
    u1 = np.cross(axis, e)
    u1 = u1 / np.linalg.norm(u1, axis=1, keepdims=True).clip(1e-300)
    return u1, np.cross(axis, u1)


def _cross_matrix(v):
    """(...,3,3) [v]x of (...,3)."""
    K = torch.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype, device=v.device)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return K


def link_twists(table, link_T, q, center, ref, origin=None, structure=True):
    """The twist of every parameter on every link, about ``ref`` (this project's own; plain torch on the device): table from
    ``UrdfRobot.fk_table()``, link_T (P,L,4,4), q (P,J), center (P,3), ref (P,L,3) f64 device tensors, ``origin`` (J,4,4) the
    joint origins when they differ from the table's -> Tw (P,L,6,M): rows 0..2 Omega, 3..5 V, so that a point c of link l moves by
    Omega x (c - ref[p,l]) + V per unit of the parameter; zero where the parameter does not move the link (chain bit clear).
    Columns: rotation about center_p (0..2), translation (3..5), the joints (6 + j: a_j and a_j x (rho - o_j) for a revolute one,
    a_j as V for a prismatic one -- the columns of ``ops.pose_fit_system``), and with ``structure`` the frame parameters
    6 + J + 4 j + m of joint j in its own frame, (w, v) = (u1, 0), (u2, 0), (0, u1), (0, u2) of ``joint_frame_basis``: the model
    origin[j] <- origin[j] E with everything attached to the child pre-multiplied by E^-1, so the child moves by E M(q) E^-1 and
    nothing moves at q = 0.  Revolute, R_q = Rot(a, q_j): Omega = W_r (w - R_q w), V = W_r (v - R_q v) at o_j, carried to rho by
    + Omega x (rho - o_j).  Prismatic: V = q_j W_r (w x a), two parameters.  Fixed: none."""
    dev, dt = link_T.device, torch.float64
    P, L = link_T.shape[:2]
    J = len(table["parent"])
    kinds, parent, child = np.asarray(table["type"]), np.asarray(table["parent"]), np.asarray(table["child"])
    axis_h = np.asarray(table["axis"], np.float64).reshape(-1, 3)
    origin = torch.as_tensor(np.ascontiguousarray(table["origin"]), dtype=dt, device=dev) if origin is None else origin
    chain = ops.joint_chains(table)
    M = 6 + J + (4 * J if structure else 0)
    Tw = torch.zeros(P, L, 6, M, dtype=dt, device=dev)
    eye3 = torch.eye(3, dtype=dt, device=dev)
    Tw[:, :, :3, :3] = eye3
    Tw[:, :, 3:, 3:6] = eye3
    Tw[:, :, 3:, :3] = _cross_matrix(ref - center[:, None, :]).transpose(-1, -2)      # column k: e_k x (rho - center)
    u1_h, u2_h = joint_frame_basis(axis_h)
    for j in range(J):
        pa, ch, kind = int(parent[j]), int(child[j]), int(kinds[j])
        if kind not in (1, 2) or not (0 <= pa < L and 0 <= ch < L):
            continue
        on = torch.as_tensor([float((int(chain[l]) >> j) & 1) for l in range(L)], dtype=dt, device=dev)[None, :, None]
        W = link_T[:, pa] @ origin[j]
        Wr, o = W[:, :3, :3], W[:, :3, 3]
        a = torch.as_tensor(axis_h[j], device=dev)
        aw = (Wr @ a)[:, None, :]                                                     # (P,1,3)
        arm = ref - o[:, None, :]                                                     # (P,L,3)
        col = 6 + J + 4 * j
        if kind == 1:
            Tw[:, :, :3, 6 + j] = aw * on
            Tw[:, :, 3:, 6 + j] = torch.linalg.cross(aw.expand(P, L, 3), arm) * on
            if structure:
                K = _cross_matrix(a)
                Rq = eye3 + torch.sin(q[:, j])[:, None, None] * K + (1.0 - torch.cos(q[:, j]))[:, None, None] * (K @ K)
                for m, u in enumerate((u1_h[j], u2_h[j])):
                    u = torch.as_tensor(u, device=dev)
                    Om = (Wr @ (u - Rq @ u)[:, :, None])[:, None, :, 0]               # (P,1,3)
                    Tw[:, :, :3, col + m] = Om * on
                    Tw[:, :, 3:, col + m] = torch.linalg.cross(Om.expand(P, L, 3), arm) * on
                    Tw[:, :, 3:, col + 2 + m] = Om * on
        else:
            Tw[:, :, 3:, 6 + j] = aw * on
            if structure:
                for m, u in enumerate((u1_h[j], u2_h[j])):
                    v = torch.as_tensor(np.cross(u, axis_h[j]), device=dev)
                    Tw[:, :, 3:, col + m] = (q[:, j, None] * (Wr @ v))[:, None, :] * on
    return Tw


_UPPER6 = [(a, b) for a in range(6) for b in range(a, 6)]           # the order of fmom's 21 sums
_UNPACK6 = [_UPPER6.index((min(a, b), max(a, b))) for a in range(6) for b in range(6)]      # entry (a, b) of M6 <- which of the 21


def twist_system(mom, cnt, Tw, fmom=None):
    """The normal system of twist columns from link moments (this project's own; plain torch on the device): mom (P,L,16) and cnt
    (P,L) of ``ops.link_moments`` taken about the point the twists Tw (P,L,6,M) of ``link_twists`` are given about ->
    (H (P,M,M), g (P,M), cost (P)).  With S2 = sum d d^T, S1 = sum d, n, Sx = sum d x r, Sr = sum r of (p, l):
    H[a][b] = sum_l Om_a^T (tr(S2) I - S2) Om_b + (Om_a x S1).V_b + (Om_b x S1).V_a + n V_a.V_b, g[a] = sum_l Om_a.Sx + V_a.Sr,
    cost = sum_l mom[15] -- per link one 6 x 6 matrix [[tr(S2) I - S2, [S1]x], [-[S1]x, n I]] between the twists.  With fmom
    (P,L,21) of ``ops.link_moments(metric="feature")`` that matrix is instead M6 = sum A^T Pi A, unpacked from its upper triangle:
    the curvature of the matched features in place of the point-to-point one; g and the cost come from mom either way."""
    P, L = mom.shape[:2]
    if fmom is not None:
        M6 = fmom[..., _UNPACK6].reshape(P, L, 6, 6)
    else:
        M6 = torch.zeros(P, L, 6, 6, dtype=mom.dtype, device=mom.device)
        S2 = mom[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(P, L, 3, 3)
        eye3 = torch.eye(3, dtype=mom.dtype, device=mom.device)
        X = _cross_matrix(mom[..., 6:9])
        M6[..., :3, :3] = (mom[..., 0] + mom[..., 3] + mom[..., 5])[..., None, None] * eye3 - S2
        M6[..., :3, 3:], M6[..., 3:, :3] = X, -X
        M6[..., 3:, 3:] = cnt.to(mom.dtype)[..., None, None] * eye3
    H = (Tw.transpose(-1, -2) @ M6 @ Tw).sum(1)
    g = (Tw.transpose(-1, -2) @ mom[..., 9:15, None]).sum(1)[..., 0]
    return H, g, mom[..., 15].sum(1)


def refine_joint_frames(robot, clouds, q0, base0=None, d_max=np.inf, max_iter=30, fit_base=True, lock=(), lock_frames=(), lam0=1e-3,
                        tol=1e-10, metric="point"):
    """Refine the frames of a robot's movable joints against one cloud per pose: a bundle adjustment by Levenberg-Marquardt on the
    point-to-mesh distance (this project's own).  Shared by all poses: per revolute joint four frame parameters, per prismatic
    joint two (``link_twists``).  Per pose: its joint values and base pose, as in ``fit_cloud_poses``, whose arguments, settings
    and stops these are; ``lock_frames`` names the joints whose frame stays.  The geometry of the zero pose is held fixed: a step
    E_j of joint j's frame is origin[j] <- E_pj^-1 origin[j] E_j (pj the joint whose child is j's parent, if it has a step) and
    the triangles of link child[j] pre-multiplied by E_j^-1, so the posed meshes at q = 0 do not move.  One lambda and one accept
    / reject on the total truncated cost sum_p sum min(d^2, d_max^2).  An iteration:
      1  link_T = G urdf_fk(current origins, q)        2  one ``ops.point_mesh_distance`` call on the current triangles
      3  the cost                                      4  accept iff the total did not rise, else restore everything, lambda <- 10 lambda
      5  ``ops.link_moments`` about center_p and ``twist_system``
      6  the damped arrowhead solve by Schur complement, batched in fp64 on the device: A_p = H_pp + lambda diag,
         (H_ss + lambda diag H_ss - sum_p H_sp A_p^-1 H_ps) ds = g_s - sum_p H_sp A_p^-1 g_p, d_p = A_p^-1 (g_p - H_ps ds).
         Left out: what ``fit_cloud_poses`` leaves out, the frames in ``lock_frames``, and a parameter whose diagonal entry is
         exactly 0 -- for a frame parameter the diagonal summed over the poses: a joint that never left 0 (``unobserved_frames``)
      7  q, G as in ``fit_cloud_poses``; the origins and triangles as above
    Returns ``fit_cloud_poses``' dict with one cost_history of totals (non-increasing by construction), iterations the steps
    tried, rms_before / rms_after per pose and rms_all_before / rms_all_after over all live points, frames (J,4,4) the accumulated
    E_j = E_j(1) E_j(2) ... (``set_joint_frames`` writes them into a URDF), unobserved_frames (J,4) bool, and the final origin
    (J,4,4), tri (F,3,3) and link_T (P,L,4,4).  ``robot`` is not changed.  ``metric`` is ``fit_cloud_poses``': "feature" takes
    step 5's curvature from ``ops.link_moments(metric="feature")`` and ``twist_system(..., fmom)``, everything else as it is."""
    metric = _fit_metric("refine_joint_frames", metric)
    table0 = robot.fk_table()
    table = {k: v for k, v in table0.items() if not k.startswith("_dev")}
    names, kinds = list(table["names"]), np.asarray(table["type"])
    J, Dp, Ds = len(names), 6 + len(names), 4 * len(names)
    n_links = int(table["n_links"])
    dev, dt = _lib.device(), torch.float64
    d_max, max_iter, parts, q, G = _fit_arguments("refine_joint_frames", J, clouds, q0, base0, d_max, max_iter, lam0, dev)
    P = len(parts)
    locked, locked_f = (_joint_rows("refine_joint_frames", names, v, k) for k, v in (("lock", lock), ("lock_frames", lock_frames)))
    free_p0 = torch.as_tensor(np.array([bool(fit_base)] * 6 + [kinds[j] in (1, 2) and j not in locked for j in range(J)]), device=dev)
    free_s0 = torch.as_tensor(np.array([(kinds[j] == 1 or (kinds[j] == 2 and m < 2)) and j not in locked_f
                                        for j in range(J) for m in range(4)], bool).reshape(Ds), device=dev)
    c = _pack_clouds(parts, robot, dev)
    pts, cut, n_live, center, tri, tri_start = c.pts, c.cut, c.n_live, c.center, c.tri, c.tri_start
    ref = center[:, None, :].expand(P, n_links, 3).contiguous()
    tri_start_host = np.asarray(robot.tri_start, np.int64)
    # the tables of the update: which joint's step a joint's origin is pre-multiplied by, and which a triangle's; J = "none"
    child_joint = {int(c): j for j, c in enumerate(table["child"])}
    before = torch.as_tensor([child_joint.get(int(pa), J) for pa in table["parent"]], dtype=torch.int64, device=dev).reshape(J)
    tri_joint = torch.as_tensor(np.repeat([child_joint.get(l, J) for l in range(n_links)], np.diff(tri_start_host).clip(0)),
                                dtype=torch.int64, device=dev)
    origin = torch.as_tensor(np.ascontiguousarray(table["origin"]), dtype=dt, device=dev).clone()
    u1, u2 = (torch.as_tensor(u, device=dev) for u in joint_frame_basis(table["axis"]))
    revolute = torch.as_tensor((kinds == 1).astype(np.float64), device=dev)[:, None]
    frames = torch.eye(4, dtype=dt, device=dev).expand(J, 4, 4).clone()
    eye, eye_dev = np.eye(4), torch.eye(4, dtype=dt, device=dev)
    lam = float(lam0)
    active = bool((n_live > 0).any())
    stepped = small = False
    iters = 0
    unobserved = torch.zeros(P, Dp, dtype=torch.bool, device=dev)
    unobserved_s = torch.zeros(Ds, dtype=torch.bool, device=dev)
    H_cur = g_cur = total_cur = cost_cur = n_cur = prev = cost_first = None
    history = []
    for it in range(max_iter + 1):
        link_T = (G[:, None] @ ops.urdf_fk(table, q, eye, origin=origin)).contiguous()
        tri_idx, cost, within = _truncated_cost(c, tri, link_T, d_max)
        total = float(cost.sum())
        if it == 0:
            accept, total_cur, cost_cur, n_cur, cost_first, link_T_cur = True, total, cost, within, cost, link_T
        else:
            accept = stepped and total <= total_cur
            if stepped and not accept:
                q, G, origin, tri, frames = prev
                lam *= 10.0
            elif accept:
                lam = max(lam / 10.0, FIT_LAMBDA_MIN)
                total_cur, cost_cur, n_cur, link_T_cur = total, cost, within, link_T
            active = active and not (accept and small) and not lam > FIT_LAMBDA_STOP
        history.append(total_cur)
        if it == max_iter or not active:
            break
        if accept:                                                # a rejected step keeps the system of the state it went back to
            mom, cnt, *fmom = ops.link_moments(tri, tri_start, link_T, pts, cut, tri_idx, ref, d_max, metric=metric)
            H_cur, g_cur, _ = twist_system(mom, cnt, link_twists(table, link_T, q, center, ref, origin), *fmom)
        dp = torch.diagonal(H_cur[:, :Dp, :Dp], dim1=1, dim2=2)
        ds = torch.diagonal(H_cur[:, Dp:, Dp:], dim1=1, dim2=2).sum(0)
        free_p, free_s = free_p0[None] & (dp != 0.0), free_s0 & (ds != 0.0)
        unobserved, unobserved_s = free_p0[None] & (dp == 0.0), free_s0 & (ds == 0.0)
        mp, ms = free_p.to(dt), free_s.to(dt)
        A = H_cur[:, :Dp, :Dp] * mp[:, :, None] * mp[:, None, :] + torch.diag_embed(lam * dp * mp + (1.0 - mp))
        B = H_cur[:, :Dp, Dp:] * mp[:, :, None] * ms[None, None, :]
        chol, info = torch.linalg.cholesky_ex(A)
        sol = torch.cholesky_solve(torch.cat([B, (g_cur[:, :Dp] * mp)[:, :, None]], 2), chol)       # A_p^-1 (H_ps | g_p)
        S = H_cur[:, Dp:, Dp:].sum(0) * ms[:, None] * ms[None, :] + torch.diag(lam * ds * ms + (1.0 - ms)) \
            - (B.transpose(1, 2) @ sol[:, :, :Ds]).sum(0)
        rhs = g_cur[:, Dp:].sum(0) * ms - (B.transpose(1, 2) @ sol[:, :, Ds:]).sum(0)[:, 0]
        chol_s, info_s = torch.linalg.cholesky_ex(S)
        delta_s = torch.cholesky_solve(rhs[:, None], chol_s)[:, 0] * ms
        delta_p = (sol[:, :, Ds] - (sol[:, :, :Ds] @ delta_s[:, None])[:, :, 0]) * mp
        failed = bool((info != 0).any()) or bool(info_s != 0) or not bool(torch.isfinite(delta_s).all() & torch.isfinite(delta_p).all())
        iters += 1
        stepped = not failed
        if failed:
            lam *= 10.0
            continue
        small = float(torch.maximum(delta_p.abs().max(), delta_s.abs().max())) < tol
        prev = (q, G, origin, tri, frames)
        q = torch.where(delta_p[:, 6:] != 0.0, q + delta_p[:, 6:], q)
        moved = (delta_p[:, :6] != 0.0).any(1)
        G = torch.where(moved[:, None, None], _base_steps(delta_p[:, :6], center) @ G, G)
        s = delta_s.reshape(J, 4)
        turned = (s != 0.0).any(1)
        w = s[:, 0:1] * u1 + s[:, 1:2] * u2
        v = (s[:, 2:3] * u1 + s[:, 3:4] * u2) * revolute
        E = _base_steps(torch.cat([w, v], 1), torch.zeros(J, 3, dtype=dt, device=dev))
        E = torch.where(turned[:, None, None], E, eye_dev)
        E_inv = torch.cat([torch.linalg.inv(E), eye_dev[None]])                # row J: no step
        changed = turned | torch.cat([turned, torch.zeros(1, dtype=torch.bool, device=dev)])[before]
        origin = torch.where(changed[:, None, None], E_inv[before] @ origin @ E, origin)
        frames = torch.where(turned[:, None, None], frames @ E, frames)
        Ei = E_inv[tri_joint]
        shifted = torch.einsum("fij,fvj->fvi", Ei[:, :3, :3], tri) + Ei[:, None, :3, 3]
        tri = torch.where(torch.cat([turned, torch.zeros(1, dtype=torch.bool, device=dev)])[tri_joint][:, None, None], shifted, tri).contiguous()
    n_live_h = n_live.cpu().numpy()
    rms_all = lambda total: float(np.sqrt(total / n_live_h.sum())) if n_live_h.sum() > 0 else float("nan")
    return {"q": q.cpu().numpy(), "base": G.cpu().numpy(), "cost_history": history, "iterations": iters,
            "rms_before": _rms(n_live_h, cost_first.cpu().numpy()), "rms_after": _rms(n_live_h, cost_cur.cpu().numpy()),
            "rms_all_before": rms_all(history[0]), "rms_all_after": rms_all(history[-1]), "unobserved": unobserved.cpu().numpy(),
            "n": n_cur.cpu().numpy(), "names": names, "frames": frames.cpu().numpy(),
            "unobserved_frames": unobserved_s.reshape(J, 4).cpu().numpy(), "origin": origin.cpu().numpy(), "tri": tri.cpu().numpy(),
            "link_T": link_T_cur.cpu().numpy()}


def _xyz_rpy(T):
    """(xyz, rpy) strings of a rigid 4x4 in URDF's fixed-axis roll-pitch-yaw, the convention ``set_inertials`` reads."""
    return " ".join(map(str, T[:3, 3])), " ".join(map(str, R.from_matrix(T[:3, :3]).as_euler("xyz")))


def _read_origin(elem):
    """The 4x4 of an element's <origin> child (identity without one), xyz and rpy as ``set_inertials`` reads them."""
    T = np.eye(4)
    o = elem.find("origin")
    if o is not None:
        T[:3, :3] = R.from_euler("xyz", np.array(o.get("rpy", "0 0 0").split(), np.float64)).as_matrix()
        T[:3, 3] = np.array(o.get("xyz", "0 0 0").split(), np.float64)
    return T


def set_joint_frames(urdf_file, frames_by_name, output_file):
    """Write refined joint frames into a copy of a URDF (this project's own): frames_by_name = {joint name: E (4,4)}, the
    accumulated steps ``refine_joint_frames`` returns in "frames".  Every joint's <origin> becomes E_pj^-1 O E_j (pj the named
    joint whose child is this joint's parent; a joint that is not named has E = identity), and the <visual>, <collision> and
    <inertial> origins of a named joint's child link are pre-multiplied by E_j^-1 -- xyz and rpy in URDF's fixed-axis
    roll-pitch-yaw, as ``set_inertials`` reads them -- so the file's zero pose keeps its geometry.  An origin that does not change
    keeps its text; a rewritten element without an <origin> (URDF's identity) gets one as its first child; <axis>, limits, names,
    meshes and the layout are untouched; ``urdf_file`` is only read.  KeyError for a name the file does not have, ValueError for
    a frame that is not (4,4) or a named joint whose child link the file does not hold; nothing is written in either case."""
    tree = ET.parse(urdf_file)
    root = tree.getroot()
    joints = {j.get("name"): j for j in root.findall("joint")}
    links = {l.get("name"): l for l in root.findall("link")}
    E = {}
    for name, frame in frames_by_name.items():
        if name not in joints:
            raise KeyError(f"{urdf_file}: no joint named {name!r}")
        frame = np.asarray(frame, np.float64)
        if frame.shape != (4, 4):
            raise ValueError(f"set_joint_frames: the frame of {name} must be (4,4), got {frame.shape}")
        E[name] = frame
    by_child = {j.find("child").get("link"): name for name, j in joints.items()}
    todo = []
    for name, j in joints.items():
        before = by_child.get(j.find("parent").get("link"))
        if name not in E and before not in E:
            continue
        T = np.linalg.inv(E[before]) @ _read_origin(j) if before in E else _read_origin(j)
        todo.append((j, T @ E[name] if name in E else T))
    for name in E:
        link = links.get(joints[name].find("child").get("link"))
        if link is None:
            raise ValueError(f"{urdf_file}: joint {name} has no child link in the file")
        Ei = np.linalg.inv(E[name])
        for tag in ("visual", "collision", "inertial"):
            for block in link.findall(tag):
                todo.append((block, Ei @ _read_origin(block)))
    for elem, T in todo:
        xyz, rpy = _xyz_rpy(T)
        if elem.find("origin") is None:
            elem.insert(0, ET.Element("origin"))
        elem.find("origin").attrib.update(xyz=xyz, rpy=rpy)
    if os.path.dirname(output_file):
        os.makedirs(os.path.dirname(output_file), exist_ok=True)
    tree.write(output_file, encoding="utf-8", xml_declaration=True)


def frame_shift(frame, axis, kind=1):
    """What an accumulated frame step E (4,4) did to a joint with unit axis ``axis`` in its own frame -> (angle between the old
    axis and the new one E_r a in rad, distance of the old joint point -- the frame's origin -- from the new line through E_t
    along E_r a; None for a joint that does not turn, whose line has no position)."""
    frame, a = np.asarray(frame, np.float64), np.asarray(axis, np.float64)
    b = frame[:3, :3] @ a
    angle = float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))
    if kind != 1:
        return angle, None
    t = -frame[:3, 3]
    return angle, float(np.linalg.norm(t - (t @ b) * b / (b @ b)))


def refine_urdf_joints(urdf_file, links, motion, cm_list, raw_dirs, start_step, num_steps, output_file, time_step=0, d_max=np.inf,
                       max_iter=30, metric="point"):
    """Refine the written URDF's joint frames against the raw clouds and write the result beside it (this project's own): the
    poses of ``cloud_fit`` are the start, all loaded frames are fitted at once with the base free (``refine_joint_frames``,
    with its ``metric``),
    ``d_max`` is the cloud fit's limit, and ``set_joint_frames`` writes ``output_file``; ``urdf_file`` is only read.  Returns
    ``refine_joint_frames``' dict with "positions" (J,S,num_steps) and "shift" (J) as ``fit_positions`` adds them, and "joints",
    per joint of ``motion`` a dict of joint, axis_angle and line_distance (``frame_shift`` of its accumulated step) and
    max_shift."""
    from .cluster_icp import read_point_cloud
    robot, q, G = _cloud_fit_state(urdf_file, links, motion, cm_list, start_step, num_steps, time_step)
    S, n = len(cm_list), int(num_steps)
    clouds = [np.asarray(read_point_cloud(os.path.join(raw_dirs[s], f"{start_step + k:04}", "robot.ply")).points, np.float64)
              for s in range(S) for k in range(n)]
    fit = refine_joint_frames(robot, clouds, q, G, d_max=d_max, max_iter=max_iter, fit_base=True, metric=metric)
    table = robot.fk_table()
    set_joint_frames(urdf_file, {name: fit["frames"][j] for j, name in enumerate(fit["names"])
                                 if not np.array_equal(fit["frames"][j], np.eye(4))}, output_file)
    positions = np.array([np.asarray(m["positions"], np.float64).reshape(S, n) for m in motion]).reshape(len(motion), S, n)
    shift, joints = np.zeros(len(motion)), []
    for j, m in enumerate(motion):
        name = f"joint_{m['child_link']}"
        row = {"joint": name, "axis_angle": 0.0, "line_distance": None, "max_shift": 0.0}
        if name in fit["names"]:
            k = fit["names"].index(name)
            fitted = fit["q"][:, k].reshape(S, n)
            shift[j] = float(np.abs(fitted - positions[j]).max())
            positions[j] = fitted
            row["axis_angle"], row["line_distance"] = frame_shift(fit["frames"][k], table["axis"][k], int(table["type"][k]))
            row["max_shift"] = float(shift[j])
        joints.append(row)
    fit["positions"], fit["shift"], fit["joints"] = positions, shift, joints
    return fit
