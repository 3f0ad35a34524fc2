"""Synthetic raw frames from a URDF + its triangle meshes, with the call surface of the
reference's ``Sim/sim_data.py`` where it makes sense: ``SimEnv(urdf_path, base_position, base_orientation,
dof=..., global_scale=...)`` with ``joint_params / joint_list / dof_list / joint_limits``,
``angle_list(num_step, step_size, dof, joint_limits, scale, seed_i)`` (:372-430, restated call for call on
numpy's legacy generator, so the joint trajectories are the reference's), ``data_collection(env, data_path,
angle_list=..., noise_flag=..., num_points=...)`` and ``save_step_data`` (:231-244: ``{step:04}/robot.ply`` +
``joint_cfg.txt``, ``noise.txt``).

What differs, by design: the reference steps a PyBullet simulation and fuses depth renders of 20 virtual
cameras (:166-198, :262-330); this build evaluates the URDF's forward kinematics itself and samples the visual
mesh surfaces by area on the GPU (``creg_sample_mesh_f64``), then applies the same noise model (:337-343) and the
same farthest-point down-sampling to ``num_points`` (:346,349; ``creg_fps_f64``).  Frames are therefore
geometry-faithful but include surfaces a camera ring would not see.  PyBullet, OpenGL and Open3D are not
needed.  Mesh formats: STL (binary / ASCII) and OBJ; COLLADA visuals raise.  The sampling and the
down-sampling have no CPU fallback.

``data_collection(..., source="depth")`` builds the frames the reference's way instead: one depth buffer per camera,
every pixel back-projected, the per-camera clouds fused (``SimEnv.depth_cloud``); with ``SimEnv(ground_flag=True)`` the
robot stands on a ground plane that is removed per camera by RANSAC plane segmentation at the reference's parameters
(``ops.segment_plane``: 0.001, 6, 1000; sim_data.py:311-319).

Self-colliding poses are rejected as the reference's generator does (sim_data.py:200-208, :276-281, :473-527), by this
project's own contract: the posed ``<visual>`` triangles of every non-adjacent link pair, mesh against mesh, for all poses of
a sequence in one launch (``ops.mesh_collide`` / ``SimEnv.collisions``; include/creg.h states the contract).  PyBullet's
check -- convex hulls of the ``<collision>`` geometry with Bullet's margins after a physics step -- cannot be pinned without
PyBullet and is not imitated.  ``data_collection(..., check_collision=True)`` stops a sequence at its first colliding step,
``collect(..., reject_collisions=True)`` / ``--reject_collisions`` skips colliding seeds.  A collision margin
(``collision_margin`` / ``--collision_margin``, ``SimEnv.collisions(margin=...)``) also rejects poses whose links pass closer
than the margin without touching: the minimum mesh distance of every tested link pair comes from ``ops.mesh_clearance`` /
``SimEnv.clearance``, again one launch for a sequence.  With no margin the check is the one above, unchanged.
Neither check sees a link wholly inside another (no edge pierces a face, and the clearance is positive):
``containment=True`` / ``--containment`` adds a point-in-mesh query (``ops.mesh_contain`` / ``SimEnv.containment``: winding
numbers of the posed meshes at ``UrdfRobot.containment_points``), one more launch for a sequence.  Without it nothing changes.
"""
import os
import struct
import xml.etree.ElementTree as ET

import numpy as np
import torch

from . import _lib, ops
from .cluster_icp import PointCloud
from .fps import farthest_point_sample


# ------------------------------------------------------------------------------------------ joint trajectories
def angle_list(num_step, step_size, dof, joint_limits, scale, seed_i):
    """(num_step, dof) joint angles in radians: per joint, random targets inside the scaled limits at least
    20 % of the range away, approached in steps of step_size * (1 + U[0,1)) degrees (sim_data.py:372-430)."""
    start_rate, low_step_limit = 0.5, 0.2
    np.random.seed(seed_i)
    limits_deg = np.asarray(joint_limits, np.float64) * 180 / np.pi
    scaled = limits_deg * np.asarray(scale, np.float64).reshape(-1, 1)
    span = np.abs(scaled[:, 1] - scaled[:, 0])
    start = scaled[:, 0] + start_rate * (scaled[:, 1] - scaled[:, 0])
    columns = []
    for j in range(dof):
        col = []
        while len(col) < num_step:
            while True:
                target = np.random.rand() * (scaled[j][1] - scaled[j][0]) + scaled[j][0]
                if np.abs(target - start[j]) > low_step_limit * span[j]:
                    break
            step = step_size * (1 + np.random.rand())
            n = int(np.abs(target - start[j]) / step) + 1
            direction = 1 if target > start[j] else -1
            stop = start[j] + direction * step * n
            col += list(np.linspace(start[j], stop, n, endpoint=False))
            start[j] = stop
        columns.append(np.array(col)[:num_step])
    return np.vstack(columns).T * np.pi / 180


# ------------------------------------------------------------------------------------------ meshes
def _load_stl(path):
    with open(path, "rb") as f:
        raw = f.read()
    n = struct.unpack_from("<I", raw, 80)[0] if len(raw) >= 84 else -1
    if n >= 0 and len(raw) == 84 + 50 * n:                      # binary: 80-byte header, count, 50-byte records
        rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", 9), ("a", "<u2")]), count=n, offset=84)
        return rec["v"].astype(np.float64).reshape(n, 3, 3)
    verts = [ln.split()[1:4] for ln in raw.decode("ascii", "replace").splitlines() if ln.strip().startswith("vertex")]
    v = np.asarray(verts, np.float64)
    if len(v) == 0 or len(v) % 3:
        raise IOError(f"{path}: neither a binary nor an ASCII STL")
    return v.reshape(-1, 3, 3)


def _load_obj(path):
    verts, tris = [], []
    with open(path, "r", errors="replace") as f:
        for ln in f:
            tok = ln.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                idx = [int(t.split("/")[0]) for t in tok[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                for a in range(1, len(idx) - 1):                # fan triangulation of polygons
                    tris.append([idx[0], idx[a], idx[a + 1]])
    v = np.asarray(verts, np.float64)
    return v[np.asarray(tris, np.int64)] if tris else np.zeros((0, 3, 3))


def _dae_node_matrix(node, ns):
    """Local transform of a COLLADA <node>: its <matrix> / <translate> / <rotate> / <scale> children composed in
    document order (COLLADA 1.4.1, 5.5 'node': post-multiplied in the order listed)."""
    M = np.eye(4)
    for ch in node:
        tag = ch.tag[len(ns):] if ch.tag.startswith(ns) else ch.tag
        if tag not in ("matrix", "translate", "rotate", "scale") or ch.text is None:
            continue
        v = [float(x) for x in ch.text.split()]
        T = np.eye(4)
        if tag == "matrix":
            T = np.asarray(v, np.float64).reshape(4, 4)          # row-major in the document
        elif tag == "translate":
            T[:3, 3] = v[:3]
        elif tag == "scale":
            T[0, 0], T[1, 1], T[2, 2] = v[:3]
        else:                                                    # rotate: axis x y z, angle in degrees
            T[:3, :3] = _axis_angle(v[:3], np.deg2rad(v[3])) if np.linalg.norm(v[:3]) > 0 else np.eye(3)
        M = M @ T
    return M


def _load_dae(path):
    """Triangles of a COLLADA 1.4 document: every <instance_geometry> of the visual scene with its node transforms,
    <triangles> / <polylist> / <polygons> primitives (polygons fan-triangulated), the asset's unit (metres per unit) and
    up axis applied the way PyBullet's URDF importer does (Y_UP -> +90 degrees about x, X_UP -> -90 degrees about y;
    Bullet LoadMeshFromCollada.cpp).  Materials, normals and texture coordinates are not needed for surface sampling."""
    root = ET.parse(path).getroot()
    ns = root.tag[: root.tag.index("}") + 1] if root.tag.startswith("{") else ""
    f = lambda e, q: e.find(q.replace("c:", ns))
    fa = lambda e, q: e.findall(q.replace("c:", ns))
    unit, up = 1.0, "Y_UP"                                       # COLLADA's defaults
    asset = f(root, "c:asset")
    if asset is not None:
        u = f(asset, "c:unit")
        if u is not None and u.get("meter"):
            unit = float(u.get("meter"))
        a = f(asset, "c:up_axis")
        if a is not None and a.text:
            up = a.text.strip()
    geoms = {}
    for g in fa(root, "c:library_geometries/c:geometry"):
        mesh = f(g, "c:mesh")
        if mesh is None:
            continue
        sources = {}
        for src in fa(mesh, "c:source"):
            fa_ = f(src, "c:float_array")
            acc = f(src, "c:technique_common/c:accessor")
            if fa_ is None or fa_.text is None:
                continue
            stride = int(acc.get("stride", "3")) if acc is not None else 3
            sources["#" + src.get("id")] = np.asarray(fa_.text.split(), np.float64).reshape(-1, stride)
        verts = {}
        for v in fa(mesh, "c:vertices"):
            for inp in fa(v, "c:input"):
                if inp.get("semantic") == "POSITION":
                    verts["#" + v.get("id")] = sources[inp.get("source")]
        tris = []
        for prim in list(fa(mesh, "c:triangles")) + list(fa(mesh, "c:polylist")) + list(fa(mesh, "c:polygons")):
            inputs = fa(prim, "c:input")
            stride = max(int(i.get("offset", "0")) for i in inputs) + 1
            vin = next(i for i in inputs if i.get("semantic") == "VERTEX")
            pos, voff = verts[vin.get("source")][:, :3], int(vin.get("offset", "0"))
            kind = prim.tag[len(ns):]
            plists = [np.asarray(p_.text.split(), np.int64) for p_ in fa(prim, "c:p") if p_.text]
            if kind == "triangles":
                idx = np.concatenate(plists)[voff::stride] if plists else np.zeros(0, np.int64)
                tris.append(pos[idx].reshape(-1, 3, 3))
            else:
                if kind == "polylist":
                    counts = np.asarray(f(prim, "c:vcount").text.split(), np.int64)
                    idx = plists[0][voff::stride]
                    polys, at = [], 0
                    for c in counts:
                        polys.append(idx[at:at + c]); at += c
                else:
                    polys = [pl[voff::stride] for pl in plists]
                for poly in polys:
                    for a in range(1, len(poly) - 1):
                        tris.append(pos[[poly[0], poly[a], poly[a + 1]]][None])
        geoms["#" + g.get("id")] = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
    out = []

    def walk(node, M):
        M = M @ _dae_node_matrix(node, ns)
        for ig in fa(node, "c:instance_geometry"):
            t = geoms.get(ig.get("url"))
            if t is not None and len(t):
                out.append(t @ M[:3, :3].T + M[:3, 3])
        for ch in fa(node, "c:node"):
            walk(ch, M)

    scenes = fa(root, "c:library_visual_scenes/c:visual_scene")
    for sc in scenes:
        for node in fa(sc, "c:node"):
            walk(node, np.eye(4))
    if not out:                                                  # no scene graph: every geometry as it stands
        out = [t for t in geoms.values() if len(t)]
    if not out:
        raise IOError(f"{path}: no triangle geometry found")
    tri = np.concatenate(out) * unit
    if up == "Y_UP":
        tri = tri @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]).T      # (x, y, z) -> (x, -z, y)
    elif up == "X_UP":
        tri = tri @ np.array([[0, 0, -1.0], [0, 1.0, 0], [1.0, 0, 0]]).T     # (x, y, z) -> (-z, y, x)
    return tri


def load_mesh(path):
    """(F,3,3) float64 triangles of an STL, OBJ or COLLADA (.dae) file."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".stl":
        return _load_stl(path)
    if ext == ".obj":
        return _load_obj(path)
    if ext == ".dae":
        return _load_dae(path)
    raise NotImplementedError(f"{path}: only STL, OBJ and COLLADA visuals are supported")


def _primitive(geom):
    """Triangles of a URDF <box>/<cylinder>/<sphere> visual."""
    tag = geom.tag
    if tag == "box":
        sx, sy, sz = (float(v) / 2 for v in geom.get("size").split())
        c = np.array([[x, y, z] for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)])
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        return np.array([[c[q[0]], c[q[a]], c[q[a + 1]]] for q in quads for a in (1, 2)])
    if tag in ("cylinder", "sphere"):
        r = float(geom.get("radius"))
        seg = 24
        th = np.linspace(0, 2 * np.pi, seg + 1)
        tris = []
        if tag == "cylinder":
            h = float(geom.get("length")) / 2
            for a, b in zip(th[:-1], th[1:]):
                pa, pb = np.array([r * np.cos(a), r * np.sin(a)]), np.array([r * np.cos(b), r * np.sin(b)])
                tris += [[[*pa, -h], [*pb, -h], [*pb, h]], [[*pa, -h], [*pb, h], [*pa, h]],
                         [[0, 0, h], [*pa, h], [*pb, h]], [[0, 0, -h], [*pb, -h], [*pa, -h]]]
        else:
            ph = np.linspace(0, np.pi, seg // 2 + 1)
            pt = lambda t, p: [r * np.sin(p) * np.cos(t), r * np.sin(p) * np.sin(t), r * np.cos(p)]
            for a, b in zip(th[:-1], th[1:]):
                for c0, c1 in zip(ph[:-1], ph[1:]):
                    tris += [[pt(a, c0), pt(a, c1), pt(b, c1)], [pt(a, c0), pt(b, c1), pt(b, c0)]]
        return np.asarray(tris, np.float64)
    raise NotImplementedError(f"URDF geometry <{tag}>")


# ------------------------------------------------------------------------------------------ URDF
def _rpy_matrix(rpy):
    """URDF fixed-axis roll-pitch-yaw: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _origin(elem):
    T = np.eye(4)
    o = elem.find("origin") if elem is not None else None
    if o is not None:
        T[:3, :3] = _rpy_matrix([float(v) for v in o.get("rpy", "0 0 0").split()])
        T[:3, 3] = [float(v) for v in o.get("xyz", "0 0 0").split()]
    return T


def _axis_angle(axis, q):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(q) * K + (1 - np.cos(q)) * (K @ K)


class UrdfRobot:
    """Kinematic tree + visual triangles of a URDF.  ``links`` in file order; ``joints`` in file order (PyBullet
    numbers joints the same way); ``tri`` (F,3,3) in link frames, ``tri_link`` (F,), ``cum_area`` (F,), ``tri_start`` (L+1,)
    int64: link l owns rows tri_start[l]:tri_start[l+1] of ``tri``.  ``load_meshes=False`` keeps the kinematic tree only: no
    mesh file is resolved or read, ``tri``, ``tri_link`` and ``cum_area`` are empty and ``tri_start`` is all zero.
    ``geometry="collision"`` reads every link's <collision> elements instead of its <visual> ones (their own origins and
    scales): the hulls of a URDF written with ``--collision_hull``."""

    def __init__(self, urdf_path, global_scale=1.0, package_dirs=(), load_meshes=True, geometry="visual"):
        if geometry not in ("visual", "collision"):
            raise ValueError(f"geometry must be 'visual' or 'collision', got {geometry!r}")
        self.geometry = geometry
        self.path = os.path.abspath(urdf_path)
        root = ET.parse(self.path).getroot()
        self.links = [l.get("name") for l in root.findall("link")]
        self.link_index = {n: i for i, n in enumerate(self.links)}
        self.joints = []
        for j in root.findall("joint"):
            lim = j.find("limit")
            ax = j.find("axis")
            self.joints.append({
                "name": j.get("name"), "type": j.get("type"),
                "parent": j.find("parent").get("link"), "child": j.find("child").get("link"),
                "origin": _origin(j), "axis": [float(v) for v in (ax.get("xyz") if ax is not None else "1 0 0").split()],
                "limit": [float(lim.get("lower", 0)), float(lim.get("upper", 0))] if lim is not None else [0.0, 0.0]})
        for j in self.joints:
            j["origin"][:3, 3] *= global_scale
        children = {j["child"] for j in self.joints}
        roots = [l for l in self.links if l not in children]
        if len(roots) != 1:
            raise ValueError(f"{urdf_path}: expected one root link, found {roots}")
        self.root = roots[0]
        if not load_meshes:
            self.tri, self.tri_link, self.cum_area = np.zeros((0, 3, 3)), np.zeros(0, np.int32), np.zeros(0)
            self.tri_start = np.zeros(len(self.links) + 1, np.int64)
            return
        tris, owner = [], []
        for l in root.findall("link"):
            for vis in l.findall(geometry):
                geom = vis.find("geometry")
                if geom is None or len(geom) == 0:
                    continue
                g = geom[0]
                if g.tag == "mesh":
                    t = load_mesh(self._resolve(g.get("filename"), package_dirs))
                    t = t * np.array([float(v) for v in g.get("scale", "1 1 1").split()])
                else:
                    t = _primitive(g)
                T = _origin(vis)
                t = (t @ T[:3, :3].T + T[:3, 3]) * global_scale
                tris.append(t)
                owner.append(np.full(len(t), self.link_index[l.get("name")], np.int32))
        if not tris:
            raise ValueError(f"{urdf_path}: no {geometry} geometry")
        self.tri = np.concatenate(tris)
        self.tri_link = np.concatenate(owner)
        e1, e2 = self.tri[:, 1] - self.tri[:, 0], self.tri[:, 2] - self.tri[:, 0]
        area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        keep = area > 0                                          # degenerate facets carry no surface
        self.tri, self.tri_link, area = self.tri[keep], self.tri_link[keep], area[keep]
        self.cum_area = np.cumsum(area)
        if np.any(np.diff(self.tri_link) < 0):
            raise ValueError(f"{urdf_path}: tri_link is not non-decreasing (the triangles of a link must be contiguous)")
        self.tri_start = np.searchsorted(self.tri_link, np.arange(len(self.links) + 1), side="left").astype(np.int64)

    def _resolve(self, filename, package_dirs):
        if filename.startswith("package://"):
            rel = filename[len("package://"):]
            cands = [os.path.join(d, rel) for d in package_dirs] + [os.path.join(d, rel.split("/", 1)[-1]) for d in package_dirs]
            here = os.path.dirname(self.path)
            for up in range(4):                                  # packages usually sit a few levels above urdf/
                cands += [os.path.join(here, rel), os.path.join(here, rel.split("/", 1)[-1])]
                here = os.path.dirname(here)
        else:
            # relative names: next to the URDF, or relative to one of its ancestors / the working directory (the
            # reference's URDFs name meshes from the repository root, where its scripts are run)
            cands = [filename] if os.path.isabs(filename) else []
            here = os.path.dirname(self.path)
            for up in range(6):
                cands.append(os.path.join(here, filename))
                here = os.path.dirname(here)
            cands += [os.path.join(d, filename) for d in package_dirs] + [os.path.abspath(filename)]
        for c in cands:
            if os.path.exists(c):
                return c
        raise FileNotFoundError(f"mesh {filename!r} of {self.path} not found (tried {cands[:3]} ...)")

    def collision_pairs(self, excluded_pairs=()):
        """(M,2) int32 link pairs the self-collision check tests: every i < j of links that own triangles, minus parent-child
        pairs (joined links intersect at every pose) and minus ``excluded_pairs`` [(name, name), ...] in either order; a name
        that is no link is ignored, like the reference's ``link_name_to_index.get`` (sim_data.py:210-219)."""
        skip = {frozenset((self.link_index[j["parent"]], self.link_index[j["child"]])) for j in self.joints}
        for a, b in excluded_pairs:
            ia, ib = self.link_index.get(a), self.link_index.get(b)
            if ia is not None and ib is not None:
                skip.add(frozenset((ia, ib)))
        owns = np.diff(self.tri_start) > 0
        n = len(self.links)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if owns[i] and owns[j] and frozenset((i, j)) not in skip]
        return np.asarray(pairs, np.int32).reshape(-1, 2)

    def containment_points(self, max_per_link=16):
        """(pts (N,3) float64, pt_start (L+1) int64): the query points ``ops.mesh_contain`` poses with each link, in link frames.
        Per link the vertices are welded by exact equality and the triangle mesh split into connected components; each
        component gives one point, the first vertex of its first triangle.  Components go by descending triangle count, then by
        first row, and at most ``max_per_link`` (<= 16) are kept.  One vertex per component suffices: when no edge pierces a
        face, a connected piece of surface lies wholly on one side of a closed mesh."""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        if not 1 <= int(max_per_link) <= 16:
            raise ValueError(f"containment_points: max_per_link must be 1 .. 16, got {max_per_link}")
        pts, start = [], [0]
        for l in range(len(self.links)):
            t = self.tri[self.tri_start[l]:self.tri_start[l + 1]]
            if len(t):
                _, vid = np.unique(t.reshape(-1, 3), axis=0, return_inverse=True)
                vid = vid.reshape(-1, 3)
                n = int(vid.max()) + 1
                rows, cols = np.concatenate([vid[:, 0], vid[:, 1]]), np.concatenate([vid[:, 1], vid[:, 2]])
                _, label = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)
                comp = label[vid[:, 0]]                              # a triangle's three vertices share one component
                ids, first_row, count = np.unique(comp, return_index=True, return_counts=True)
                order = np.lexsort((first_row, -count))[:int(max_per_link)]
                pts.extend(t[first_row[order], 0])
            start.append(len(pts))
        return np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(start, np.int64)

    def fk(self, q_by_joint, base=None):
        """Link poses (L,4,4) float64 for joint positions {name: value} (missing joints at 0)."""
        T = np.tile(np.eye(4), (len(self.links), 1, 1))
        T[self.link_index[self.root]] = np.eye(4) if base is None else base
        done = {self.root}
        pending = list(self.joints)
        while pending:
            rest = []
            for j in pending:
                if j["parent"] not in done:
                    rest.append(j)
                    continue
                M = np.eye(4)
                q = float(q_by_joint.get(j["name"], 0.0))
                if j["type"] in ("revolute", "continuous"):
                    M[:3, :3] = _axis_angle(j["axis"], q)
                elif j["type"] == "prismatic":
                    a = np.asarray(j["axis"], np.float64)
                    M[:3, 3] = a / np.linalg.norm(a) * q
                T[self.link_index[j["child"]]] = T[self.link_index[j["parent"]]] @ j["origin"] @ M
                done.add(j["child"])
            if len(rest) == len(pending):
                raise ValueError(f"{self.path}: joints {[j['name'] for j in rest]} hang off unknown links")
            pending = rest
        return T

    def fk_table(self):
        """The joint table ``ops.urdf_fk`` (creg_urdf_fk_f64) walks, built once per robot: joints in the topological order
        ``fk`` resolves them in, with ``parent`` / ``child`` link indices, ``type`` (0 fixed, 1 revolute or continuous,
        2 prismatic), ``origin`` (J,4,4) already scaled by ``global_scale``, ``axis`` (J,3) normalised as ``_axis_angle`` does,
        ``names`` (table row -> joint name), ``root`` and ``n_links``."""
        if getattr(self, "_fk_table", None) is None:
            done, order, pending = {self.root}, [], list(self.joints)
            while pending:
                rest = []
                for j in pending:
                    if j["parent"] in done:
                        order.append(j)
                        done.add(j["child"])
                    else:
                        rest.append(j)
                if len(rest) == len(pending):
                    raise ValueError(f"{self.path}: joints {[j['name'] for j in rest]} hang off unknown links")
                pending = rest
            kind = {"revolute": 1, "continuous": 1, "prismatic": 2}
            unit = lambda a: a / np.linalg.norm(a) if np.linalg.norm(a) > 0 else np.array([1.0, 0.0, 0.0])   # a fixed joint may carry "0 0 0"
            axis = np.array([unit(np.asarray(j["axis"], np.float64)) for j in order]).reshape(-1, 3)
            names = [j["name"] for j in order]
            self._fk_table = {
                "parent": np.array([self.link_index[j["parent"]] for j in order], np.int32),
                "child": np.array([self.link_index[j["child"]] for j in order], np.int32),
                "type": np.array([kind.get(j["type"], 0) for j in order], np.int32),
                "origin": np.array([j["origin"] for j in order], np.float64).reshape(-1, 4, 4),
                "axis": axis, "names": names,
                "root": self.link_index[self.root], "n_links": len(self.links)}
        return self._fk_table

    def q_rows(self, q_by_joint_list):
        """(P,J) joint values in ``fk_table()``'s order from P dicts {name: value} (missing joints at 0, as in ``fk``)."""
        names = self.fk_table()["names"]
        return np.array([[float(q.get(n, 0.0)) for n in names] for q in q_by_joint_list], np.float64).reshape(-1, len(names))


def ground_mesh(size, cells):
    """(2 cells^2, 3, 3) triangles of a cells x cells grid of quads over [-size, size]^2 at z = 0.  Tessellated because the
    rasteriser does not clip: it drops a facet with a vertex at or behind a camera's near plane, so one large quad would vanish
    from every camera that stands over it, while small cells lose only a strip at the camera's feet."""
    cells = int(cells)
    if cells < 1 or not size > 0:
        raise ValueError("ground_mesh: size > 0 and cells >= 1")
    t = np.linspace(-float(size), float(size), cells + 1)
    x0, y0 = (a.reshape(-1) for a in np.meshgrid(t[:-1], t[:-1], indexing="ij"))
    x1, y1 = (a.reshape(-1) for a in np.meshgrid(t[1:], t[1:], indexing="ij"))
    z = np.zeros_like(x0)
    a, b, c, d = (np.stack(v, 1) for v in ((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)))
    return np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3, 3)


def _checked_margin(margin):
    margin = float(margin)
    if not margin >= 0.0:
        raise ValueError(f"collision margin must be >= 0 (inf allowed), got {margin}")
    return margin


def _margin_kw(margin):
    """The keyword a positive margin travels in; none at 0.0, so that the call without margins is today's call."""
    return {"margin": margin} if _checked_margin(margin) > 0.0 else {}


def _containment_kw(containment):
    """The keyword the containment check travels in; none when it is off, so that the call without it is today's call."""
    return {"containment": True} if containment else {}


def _inside_lines(env, link_T, use_excluded):
    """['X inside Y (step s)', ...] of a sequence, for the printed lines of the callers below (one more launch)."""
    return [f"{inner} inside {outer} (step {step})" for step, found in enumerate(env.containment(link_T, use_excluded))
            for inner, outer, _, _ in found]


class SimEnv:
    """The part of the reference's SimEnv (sim_data.py:15-64) that describes the robot: revolute joints in URDF
    order with their limits (:66-82), the first ``dof`` of them driven, the rest parked at mid range (:131-157)."""

    def __init__(self, urdf_path, base_position=[0, 0, 0], base_orientation=[0, 0, 0], gui=False, dof=5,
                 ground_flag=False, radius=1.5, num_cameras=3, global_scale=1.0, package_dirs=(), ground_size=None, ground_cells=32,
                 excluded_pairs=(), geometry="visual"):
        if gui:
            raise NotImplementedError("gui=True needs PyBullet's viewer (out of scope)")
        self.dof = dof
        self.robot = UrdfRobot(urdf_path, global_scale, package_dirs, geometry=geometry)   # "collision": the written hulls
        self.base = np.eye(4)
        self.base[:3, :3] = _rpy_matrix(base_orientation)
        self.base[:3, 3] = base_position
        self.joint_params = {j["name"]: list(j["limit"]) for j in self.robot.joints if j["type"] == "revolute"}
        self.joint_list = list(self.joint_params.keys())
        self.dof_list = self.joint_list[:dof]
        self.joint_limits = np.array([self.joint_params[j] for j in self.dof_list])
        self._dev = None
        self._dev_raster = None
        self._dev_collide = {}
        self._dev_contain = None
        self.excluded_pairs = [tuple(pr) for pr in excluded_pairs]   # parameters.json's 'excluded_pairs' (link names)
        self._setup_cameras(radius, num_cameras)
        # the ground the reference stands its robot on (ground_flag): seen by the raster passes of depth_cloud only
        self.ground_tri = ground_mesh(radius if ground_size is None else ground_size, ground_cells) if ground_flag else None

    def _setup_cameras(self, radius, num_cameras=20, cam_angle=20):
        """The reference's camera ring (sim_data.py:88-116): fewer than 20 cameras evenly on a circle at `cam_angle` degrees
        elevation; 20 or more drawn from numpy's GLOBAL RandomState like the reference (uniform azimuth, elevation in
        [0, pi/2)); all on a sphere of `radius` looking at the origin, +z up, fov 60, aspect 1, near 0.1, far 4.
        `self.cameras` keeps the reference's dict list; `self.cam_frames` (C,12) = eye | forward | right | up."""
        if num_cameras < 20:
            theta = np.linspace(0, 2 * np.pi, num_cameras, endpoint=False)
            phi = np.pi * np.array([cam_angle] * num_cameras) / 180
        else:
            theta = np.random.rand(num_cameras) * 2 * np.pi
            phi = np.random.rand(num_cameras) * np.pi / 2
        xs, ys, zs = radius * np.cos(theta) * np.cos(phi), radius * np.sin(theta) * np.cos(phi), radius * np.sin(phi)
        self.cameras = [{'camera_pos': [x, y, z], 'target_pos': [0, 0, 0], 'up_vector': [0, 0, 1], 'fov': 60, 'aspect': 1.0,
                         'near_val': 0.1, 'far_val': 4} for x, y, z in zip(xs, ys, zs)]
        frames = []
        for c in self.cameras:
            e = np.asarray(c['camera_pos'], np.float64)
            f = (np.asarray(c['target_pos'], np.float64) - e)
            f = f / np.linalg.norm(f)
            s_ = np.cross(f, np.asarray(c['up_vector'], np.float64))
            s_ = s_ / np.linalg.norm(s_)
            frames.append(np.concatenate([e, f, s_, np.cross(s_, f)]))
        self.cam_frames = np.asarray(frames)

    def visible(self, joint_positions, pts, width=800, height=800, eps=0.004, link_T=None):
        """Which of `pts` (n,3 world points, device tensor) some camera of the ring sees (creg_visibility_f64).
        `link_T` (L,4,4) device poses (a row of ops.urdf_fk) replace the host forward kinematics and its upload."""
        tri, _, own = self._device_mesh()
        T = torch.as_tensor(self.robot.fk(joint_positions, self.base), device=tri.device) if link_T is None else link_T
        cams = torch.as_tensor(self.cam_frames, device=tri.device)
        c = self.cameras[0]
        return ops.visibility(tri, own, T, cams, pts, c['fov'], c['aspect'], c['near_val'], c['far_val'], width, height, eps)

    def _device_mesh(self):
        if self._dev is None:
            d = _lib.device()
            r = self.robot
            self._dev = (torch.as_tensor(r.tri, device=d).contiguous(), torch.as_tensor(r.cum_area, device=d),
                         torch.as_tensor(r.tri_link, device=d))
        return self._dev

    def _raster_mesh(self):
        """Device triangles the depth cameras see: the robot's and, with a ground, its cells on link index L (an identity pose
        row appended to link_T)."""
        if self._dev_raster is None:
            tri, _, own = self._device_mesh()
            if self.ground_tri is not None:
                g = torch.as_tensor(self.ground_tri, device=tri.device)
                tri = torch.cat([tri, g]).contiguous()
                own = torch.cat([own, torch.full((g.shape[0],), len(self.robot.links), dtype=own.dtype, device=own.device)])
            self._dev_raster = (tri, own)
        return self._dev_raster

    def depth_cloud(self, joint_positions, width=800, height=800, link_T=None, rng=None, remove_ground=True):
        """The posed robot as the camera ring's depth images see it: one depth buffer per camera (creg_raster_depth_f64, with the
        ground if the env has one), every finite pixel back-projected (creg_depth_points_f64) -> (points (M,3), offsets (C+1)),
        camera c owning rows offsets[c]:offsets[c+1].  With a ground, each camera's cloud goes through ops.segment_plane at the
        reference's parameters (0.001, 6, 1000; hypotheses drawn from ``rng``, a numpy Generator, default seed 0) and loses its
        plane's inliers (``remove_ground=False`` keeps them)."""
        tri, own = self._raster_mesh()
        T = torch.as_tensor(self.robot.fk(joint_positions, self.base), device=tri.device) if link_T is None else link_T
        if self.ground_tri is not None:
            T = torch.cat([T, torch.eye(4, dtype=T.dtype, device=T.device)[None]])
        cams = torch.as_tensor(self.cam_frames, device=tri.device)
        c = self.cameras[0]
        depth = ops.raster_depth(tri, own, T.contiguous(), cams, c['fov'], c['aspect'], c['near_val'], c['far_val'], width, height)
        pts, off = ops.depth_points(depth, cams, c['fov'], c['aspect'])
        if self.ground_tri is None or not remove_ground or pts.shape[0] == 0:
            return pts, off
        _, mask, _, _ = ops.segment_plane(pts, off, distance_threshold=0.001, ransac_n=6, num_iterations=1000,
                                          rng=np.random.default_rng(0) if rng is None else rng)
        gone = torch.cat([torch.zeros(1, dtype=torch.int64, device=pts.device), torch.cumsum(mask.to(torch.int64), 0)])
        return pts[~mask], off - gone[off]

    def set_joint_positions(self, commands, manual_positions=0):
        """Joint name -> position: commanded for the driven joints, mid range (+ manual offset) for the others.
        (The reference reads the positions back from the physics step; here they are exact.)"""
        q = {}
        for j_id, name in enumerate(self.joint_list):
            lo, hi = sorted(self.joint_params[name])
            q[name] = float(commands[j_id]) if name in self.dof_list else (hi + lo) / 2 + manual_positions * (hi - lo) / 2
        return q

    def sample_surface(self, joint_positions, n, rng, link_T=None):
        """n area-weighted surface points of the posed robot, on the GPU (creg_sample_mesh_f64).
        `link_T` (L,4,4) device poses (a row of ops.urdf_fk) replace the host forward kinematics and its upload."""
        tri, cum, own = self._device_mesh()
        T = torch.as_tensor(self.robot.fk(joint_positions, self.base), device=tri.device) if link_T is None else link_T
        u = torch.as_tensor(rng.random((n, 3)), device=tri.device)
        return ops.sample_mesh(tri, cum, own, T, u)

    def _collide_inputs(self, use_excluded):
        """(host pairs, device pairs, device tri_start) of the tested link pairs, uploaded once per env and choice."""
        tri = self._device_mesh()[0]
        r = self.robot
        key = bool(use_excluded)
        if key not in self._dev_collide:
            host = r.collision_pairs(self.excluded_pairs if key else ())
            self._dev_collide[key] = (host, torch.as_tensor(host, device=tri.device), torch.as_tensor(r.tri_start, device=tri.device))
        return self._dev_collide[key]

    def _contain_inputs(self):
        """(device pts, device pt_start, host pt_start) of ``robot.containment_points()``, uploaded once per env."""
        if self._dev_contain is None:
            dev = self._device_mesh()[0].device
            pts, start = self.robot.containment_points()
            self._dev_contain = (torch.as_tensor(pts, device=dev), torch.as_tensor(start, device=dev), start)
        return self._dev_contain

    def _inside(self, link_T, use_excluded):
        """Per pose a list of (m, inner_link, outer_link, n_inside, winding of the first inside point): one launch
        (creg_mesh_contain_f64) over the tested pairs in both directions."""
        tri = self._device_mesh()[0]
        r = self.robot
        host, pairs, tri_start = self._collide_inputs(use_excluded)
        pts, pt_start, h_start = self._contain_inputs()
        inside, first, wind = ops.mesh_contain(tri, tri_start, pts, pt_start, link_T, pairs, want_winding=True)
        inside, first, wind = inside.cpu().numpy(), first.cpu().numpy(), wind.cpu().numpy()
        out = []
        for p in range(inside.shape[0]):
            found = []
            for m, d in zip(*np.nonzero(inside[p])):
                inner, outer = host[m, d], host[m, 1 - d]
                found.append((int(m), r.links[inner], r.links[outer], int(inside[p, m, d]),
                              float(wind[p, m, d, first[p, m, d] - h_start[inner]])))
            out.append(found)
        return out

    def containment(self, link_T, use_excluded=False):
        """Links wholly inside another at P poses, in one launch (creg_mesh_contain_f64): link_T as ``collisions`` takes it.
        Returns per pose a list of (inner_link, outer_link, n_inside, winding) for every tested pair and direction with an
        inside point: how many of the inner link's ``robot.containment_points()`` have a winding number above 0.5 in magnitude
        in the outer link's posed mesh, and the winding number of the first of them.  Not detected: a shell beyond a link's 16
        largest connected components, and a point on the surface."""
        return [[f[1:] for f in found] for found in self._inside(link_T, use_excluded)]

    def collisions(self, link_T, use_excluded=False, margin=0.0, containment=False):
        """Self and floor contacts of P poses in one launch (creg_mesh_collide_f64): link_T (P,L,4,4) -- or (L,4,4) -- device
        poses (ops.urdf_fk).  Returns one (self_contact, floor_contact) per pose: self_contact lists (link_a, link_b, count,
        tri_a, tri_b) for every tested link pair with colliding triangles -- their number and the smallest colliding pair as
        rows of ``robot.tri``; the tested pairs are ``robot.collision_pairs()``, minus the env's ``excluded_pairs`` when
        ``use_excluded``.  floor_contact lists the non-root links whose posed box reaches below z = 0, and is empty unless the
        env was built with ``ground_flag=True`` (the root stands on the ground).
        ``margin > 0`` counts a pair closer than ``margin`` as a contact, and a link whose box reaches below z = ``margin`` as a
        floor contact: the result is ``clearance(link_T, margin, use_excluded)``, whose entries hold the pair's DISTANCE in
        place of the count (0.0 for a piercing pair) and the closest triangle pair.  ``margin=0.0`` is the check without
        margins, unchanged.
        ``containment=True`` also lists a pair with a link wholly inside the other (``containment``: one more launch) that is
        not listed already, as (link_a, link_b, 0, -1, -1) in the tested pair's order; ``False`` makes no such launch."""
        margin = _checked_margin(margin)
        if margin > 0.0:
            return self.clearance(link_T, margin, use_excluded, **_containment_kw(containment))
        tri = self._device_mesh()[0]
        r = self.robot
        host, pairs, tri_start = self._collide_inputs(use_excluded)
        count, first, box = ops.mesh_collide(tri, tri_start, link_T, pairs, want_boxes=True)
        count, first, low = count.cpu().numpy(), first.cpu().numpy(), box[:, :, 2].cpu().numpy()
        root = r.link_index[r.root]
        out = []
        for p in range(count.shape[0]):
            self_c = [(r.links[host[m, 0]], r.links[host[m, 1]], int(count[p, m]), int(first[p, m, 0]), int(first[p, m, 1]))
                      for m in np.flatnonzero(count[p])]
            floor_c = [r.links[l] for l in np.flatnonzero(low[p] < 0) if l != root] if self.ground_tri is not None else []
            out.append((self_c, floor_c))
        if containment:
            for (self_c, _), found in zip(out, self._inside(link_T, use_excluded)):
                for m in sorted({f[0] for f in found}):
                    pr = (r.links[host[m, 0]], r.links[host[m, 1]])
                    if pr not in [c[:2] for c in self_c]:
                        self_c.append(pr + (0, -1, -1))
        return out

    def clearance(self, link_T, margin, use_excluded=False, containment=False):
        """How far apart the links are at P poses, in one launch (creg_mesh_clearance_f64 with d_max = ``margin``): link_T as
        ``collisions`` takes it.  Returns one (near, floor_near) per pose: near lists (link_a, link_b, distance, tri_a, tri_b)
        for every tested link pair with distance < ``margin`` -- for all tested pairs with ``margin=inf`` --, the minimum
        distance between the two posed meshes (0.0 where an edge pierces a face) and the triangle pair that attains it as rows
        of ``robot.tri``.  floor_near lists the non-root links whose posed box reaches below z = ``margin``, on a ground only.
        A mesh wholly inside another has a positive distance (include/creg.h) unless ``containment=True``: then a pair with
        a link wholly inside the other (``containment``: one more launch) gets distance 0.0 -- a listed entry keeps its
        witness, an unlisted pair is added with the witness (-1, -1).  Still not detected: a shell beyond a link's 16 largest
        connected components, and a point on the surface."""
        margin = _checked_margin(margin)
        tri = self._device_mesh()[0]
        r = self.robot
        host, pairs, tri_start = self._collide_inputs(use_excluded)
        dist, wit, box = ops.mesh_clearance(tri, tri_start, link_T, pairs, margin, want_boxes=True)
        dist, wit, low = dist.cpu().numpy(), wit.cpu().numpy(), box[:, :, 2].cpu().numpy()
        root = r.link_index[r.root]
        out = []
        for p in range(dist.shape[0]):
            near = [(r.links[host[m, 0]], r.links[host[m, 1]], float(dist[p, m]), int(wit[p, m, 0]), int(wit[p, m, 1]))
                    for m in range(dist.shape[1]) if dist[p, m] < margin or margin == np.inf]
            floor_c = [r.links[l] for l in np.flatnonzero(low[p] < margin) if l != root] if self.ground_tri is not None else []
            out.append((near, floor_c))
        if containment:
            for (near, _), found in zip(out, self._inside(link_T, use_excluded)):
                for m in sorted({f[0] for f in found}):
                    pr = (r.links[host[m, 0]], r.links[host[m, 1]])
                    at = [i for i, c in enumerate(near) if c[:2] == pr]
                    if at:
                        near[at[0]] = pr + (0.0,) + near[at[0]][3:]
                    else:
                        near.append(pr + (0.0, -1, -1))
        return out

    def surface_distance(self, link_T, clouds, d_max=np.inf):
        """How far the points of P clouds lie from the robot's meshes at P poses, in one launch (creg_point_mesh_f64): link_T
        (P,L,4,4) -- or (L,4,4) -- device poses (ops.urdf_fk) and ``clouds``, one (n_p,3) array of world points per pose (host
        arrays or device tensors).  Returns (dist, tri, link), each a list with one host array per pose: the distance of every
        point from the posed meshes (``inf`` beyond ``d_max``), the row of ``robot.tri`` that attains it and the index in
        ``robot.links`` of the link that owns that row (-1 where no triangle was within ``d_max``): a part segmentation of the
        cloud.  The other direction -- mesh surface that no point lies near -- is ``surface_coverage``'s."""
        tri = self._device_mesh()[0]
        if link_T.dim() == 3:
            link_T = link_T[None]
        if len(clouds) != link_T.shape[0]:
            raise ValueError(f"surface_distance: {link_T.shape[0]} poses need as many clouds, got {len(clouds)}")
        parts = [torch.as_tensor(c, dtype=torch.float64).reshape(-1, 3).to(tri.device) for c in clouds]
        cut = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
        pts = torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.float64, device=tri.device)
        tri_start = self._collide_inputs(False)[2]
        out = ops.point_mesh_distance(tri, tri_start, link_T, pts, torch.as_tensor(cut, device=tri.device), d_max)
        return tuple([a[cut[p]:cut[p + 1]] for p in range(len(parts))] for a in (o.cpu().numpy() for o in out))

    def surface_coverage(self, link_T, clouds, d_max=np.inf, max_edge=None):
        """How much of the robot's mesh surface at P poses has a point of that pose's cloud within ``d_max``, in one launch
        (creg_mesh_cover_f64): ``surface_distance``'s arguments, and ``max_edge`` to subdivide the meshes first (a triangle is the
        resolution of the measurement).  ``compute_joints.surface_cover_poses``, which states the returned dict: per pose, per
        link and overall the uncovered share of area and the distance figures, and per link ``never``, the share covered in no
        pose.  The environment's ground is not part of the measurement."""
        from .compute_joints import surface_cover_poses
        return surface_cover_poses(self.robot, link_T, clouds, d_max, max_edge)

    def fit_pose(self, clouds, q0, base0=None, d_max=np.inf, max_iter=30, fit_base=True, lock=(), lam0=1e-3, tol=1e-10, metric="point"):
        """Where do the joints stand in these clouds?  Fit the robot's joint values, and its base pose when ``fit_base``, to one
        cloud of world points per pose, starting from q0 (P,J) in ``robot.fk_table()``'s order and ``base0`` (this environment's
        base when None): ``compute_joints.fit_cloud_poses``, which states the algorithm, its settings and the returned dict.
        ``metric="feature"`` takes the curvature of the matched vertex, edge or face instead of the point-to-point one."""
        from .compute_joints import fit_cloud_poses
        return fit_cloud_poses(self.robot, clouds, q0, self.base if base0 is None else base0, d_max=d_max, max_iter=max_iter,
                               fit_base=fit_base, lock=lock, lam0=lam0, tol=tol, metric=metric)

    def refine_joints(self, clouds, q0, base0=None, d_max=np.inf, max_iter=30, fit_base=True, lock=(), lock_frames=(), lam0=1e-3,
                      tol=1e-10, metric="point"):
        """Where do the joint axes and origins lie in these clouds?  Refine the frames of the robot's movable joints, shared by
        all poses, together with every pose's joint values and base pose (``fit_pose``'s arguments, ``metric`` included; ``lock_frames`` names the
        joints whose frame stays): ``compute_joints.refine_joint_frames``, which states the algorithm and the returned dict.
        The environment's robot is not changed; ``compute_joints.set_joint_frames`` writes the result's "frames" into a URDF."""
        from .compute_joints import refine_joint_frames
        return refine_joint_frames(self.robot, clouds, q0, self.base if base0 is None else base0, d_max=d_max, max_iter=max_iter,
                                   fit_base=fit_base, lock=lock, lock_frames=lock_frames, lam0=lam0, tol=tol, metric=metric)

    def self_collision_check(self, joint_positions, link_T=None, use_excluded=False, margin=0.0, containment=False):
        """(self_contact, floor_contact) of one pose, the reference's return pair (sim_data.py:200-208); see ``collisions``.
        `link_T` (L,4,4) device poses replace the host forward kinematics and its upload."""
        if link_T is None:
            link_T = torch.as_tensor(self.robot.fk(joint_positions, self.base), device=self._device_mesh()[0].device)
        return self.collisions(link_T, use_excluded, **_margin_kw(margin), **_containment_kw(containment))[0]

    def reset(self):
        self._dev = None
        self._dev_raster = None
        self._dev_collide = {}
        self._dev_contain = None


def save_step_data(step_id, combined_pcds, joint_positions, data_path, dof_list):
    """{step:04}/robot.ply (binary little-endian, double x/y/z as Open3D writes points) + joint_cfg.txt
    (sim_data.py:231-244)."""
    sub = data_path + f"{step_id:04}/"
    os.makedirs(sub, exist_ok=True)
    pts = np.asarray(combined_pcds.points, np.float64)
    with open(sub + "robot.ply", "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                 "property double z\nend_header\n" % len(pts)).encode("ascii"))
        f.write(np.ascontiguousarray(pts, "<f8").tobytes())
    with open(sub + "joint_cfg.txt", "w") as f:
        for name, pos in joint_positions.items():
            if name in dof_list:
                f.write(f"{name}:{pos:,.6f}\n")


def data_collection(env, data_path=None, width=800, height=800, visualize=False, angle_list=None, ground_flag=False,
                    noise_flag=False, num_points=5000, collision_flag=False, oversample=4, seed=0, occlusion=True, link_T=None,
                    source="surface", check_collision=False, collision_margin=0.0, containment=False):
    """One sequence: for every row of ``angle_list`` pose the robot, sample surface points, keep those that at least one
    camera of the ring sees (``occlusion``: depth buffers of ``width`` x ``height`` like the reference's rendered images,
    sim_data.py:286-306; more samples are drawn until ``oversample * num_points`` visible ones exist), add the
    reference's noise (translation N(0, 0.01) per frame and N(0, 0.0005) per point, not on the first frame;
    sim_data.py:333-343), farthest-point down-sample to ``num_points`` (:346,349) and save.
    ``link_T`` (P,L,4,4), optional: device link poses of all rows at once (ops.urdf_fk); row ``jp_id`` poses step ``jp_id``
    in place of the host forward kinematics.
    ``source="depth"`` takes the points the reference's way instead (sim_data.py:283-329): the fused back-projected depth
    images of the camera ring at ``width`` x ``height`` (``SimEnv.depth_cloud``), so the density follows the pixels;
    ``ground_flag=True`` then removes the ground per camera and needs an env built with ``ground_flag=True``.  Noise,
    down-sampling and saving are the same; ``oversample`` and ``occlusion`` do not apply.  (``source="surface"`` ignores
    ``ground_flag``.)
    ``check_collision=True`` checks every row for self and floor contacts before any frame is made (one ``ops.urdf_fk`` over
    all rows unless ``link_T`` was given, one ``SimEnv.collisions`` launch); ``collision_flag=True`` then applies the env's
    ``excluded_pairs``, as in the reference.  At the first colliding step s it prints ``collision detected`` with the pairs,
    generates and saves only the steps before s, writes no ``noise.txt`` and returns (True, record): the reference breaks at
    that step (sim_data.py:276-281).  With no colliding row the clouds and files are those of ``check_collision=False``.
    ``collision_margin`` > 0 also stops at a row whose links pass closer than the margin (``SimEnv.collisions(margin=...)``);
    at 0.0 the check is the one without margins.  ``containment=True`` (with ``check_collision``) also stops at a row with a
    link wholly inside another (``SimEnv.collisions(containment=True)``) and prints ``X inside Y`` for it.
    Returns (collision, list of PointCloud) like the reference; collision is False when nothing was checked."""
    if visualize:
        raise NotImplementedError("visualize=True needs Open3D's viewer (out of scope)")
    if source not in ("surface", "depth"):
        raise ValueError(f"data_collection: source must be 'surface' or 'depth', got {source!r}")
    if source == "depth" and ground_flag and env.ground_tri is None:
        raise ValueError("data_collection: ground_flag=True needs an env built with SimEnv(..., ground_flag=True)")
    stop = None
    if check_collision and len(angle_list):
        poses = link_T
        if poses is None:
            qs = [env.set_joint_positions(cmd) for cmd in np.asarray(angle_list)]
            poses = ops.urdf_fk(env.robot.fk_table(), env.robot.q_rows(qs), env.base)
        for step, (self_c, floor_c) in enumerate(env.collisions(poses[:len(angle_list)], use_excluded=collision_flag,
                                                               **_margin_kw(collision_margin), **_containment_kw(containment))):
            if len(self_c) + len(floor_c) > 0:
                print('collision detected', self_c, floor_c)
                if containment:
                    for inner, outer, _, _ in env.containment(poses[step], collision_flag)[0]:
                        print(f"{inner} inside {outer}")
                stop = step
                break
    rng = np.random.default_rng(seed)
    noise, record = [], []
    for jp_id, cmd in enumerate(np.asarray(angle_list)):
        if stop is not None and jp_id >= stop:
            break
        q = env.set_joint_positions(cmd)
        want = oversample * num_points
        pose = {} if link_T is None else {"link_T": link_T[jp_id]}
        if source == "depth":
            pts, _ = env.depth_cloud(q, width, height, rng=rng, remove_ground=ground_flag, **pose)
            if pts.shape[0] < num_points:
                raise RuntimeError(f"only {pts.shape[0]} depth pixels of the camera ring hit the robot")
        else:
            pts = env.sample_surface(q, want, rng, **pose)
        if occlusion and source == "surface":
            kept = pts[env.visible(q, pts, width, height, **pose)]
            draws = 1
            while kept.shape[0] < want and draws < 16:            # interior / hidden surfaces: draw until enough are visible
                more = env.sample_surface(q, want, rng, **pose)
                kept = torch.cat([kept, more[env.visible(q, more, width, height, **pose)]])
                draws += 1
            if kept.shape[0] < num_points:
                raise RuntimeError(f"only {kept.shape[0]} of the sampled surface points are visible from the camera ring")
            pts = kept[:max(want, num_points)] if kept.shape[0] >= want else kept
        if noise_flag and jp_id != 0:
            pos_noise = rng.normal(0, 0.01, size=3)
            noise.append(pos_noise)
            pts = pts + torch.as_tensor(pos_noise, device=pts.device)
            pts = pts + torch.as_tensor(rng.normal(0, 0.0005, size=tuple(pts.shape)), device=pts.device)
        sel = farthest_point_sample(pts, num_points)
        cloud = PointCloud(pts[torch.as_tensor(sel, device=pts.device)].cpu().numpy())
        if data_path is not None:
            save_step_data(jp_id, cloud, q, data_path, env.dof_list)
        record.append(cloud)
    if stop is not None:
        return True, record
    if noise_flag and data_path is not None:
        np.savetxt(data_path + "noise.txt", np.array(noise).reshape(-1, 3), fmt="%.6f")
    return False, record


def sequence_collides(env, a_list, use_excluded=False, margin=0.0, closest=None, containment=False, inside=None):
    """The link pairs that collide somewhere in the sequence ``a_list`` (num_step, dof): a list of (link_a, link_b) names, a
    floor contact as ('ground', link); empty when every step is free.  One ``ops.urdf_fk`` and one ``SimEnv.collisions`` launch
    for the whole sequence.  ``margin > 0`` also lists the pairs that pass closer than the margin; a list given as ``closest``
    then receives (distance, step, link_a, link_b) of the closest such pair.  ``containment=True`` also lists the pairs with a
    link wholly inside the other; a list given as ``inside`` then receives 'X inside Y (step s)' strings."""
    qs = [env.set_joint_positions(cmd) for cmd in np.asarray(a_list)]
    if not qs:
        return []
    link_T = ops.urdf_fk(env.robot.fk_table(), env.robot.q_rows(qs), env.base)
    found, best = [], None
    if containment and inside is not None:
        inside.extend(_inside_lines(env, link_T, use_excluded))
    for step, (self_c, floor_c) in enumerate(env.collisions(link_T, use_excluded, **_margin_kw(margin), **_containment_kw(containment))):
        for pr in [(c[0], c[1]) for c in self_c] + [("ground", l) for l in floor_c]:
            if pr not in found:
                found.append(pr)
        if margin > 0.0:
            for c in self_c:
                if best is None or c[2] < best[0]:
                    best = (c[2], step, c[0], c[1])
    if closest is not None and best is not None:
        closest.append(best)
    return found


def collect(robot, robot_params, num_step=10, step_size=4, epochs=5, scale=0.9, noise=True, num_points=5000,
            num_cameras=20, root=".", source="surface", ground=False, pix=800,
            reject_collisions=False, max_seeds=100, collision_margin=0.0, containment=False):
    """`epochs` sequences of `num_step` frames under data/raw/{robot}/{step_size}_deg_{num_cameras}_cams/V{seed:04}/
    -- the directory layout of the reference's collect() (sim_data.py:465-531), which match() globs
    (mlp_reg.py:424).  robot_params needs the reference's keys 'gt' (URDF path), 'dof' and optionally 'sim_ori'.
    Seeds are 0..epochs-1 by default.  ``reject_collisions=True`` runs the reference's loop instead (:473-527): seeds 0, 1, 2, ...
    are tried in turn, the whole ``angle_list`` of a seed is checked before any frame is made (``sequence_collides``, with
    robot_params' 'excluded_pairs' applied when its 'collision_exclusion' is true), a colliding seed is skipped with a printed
    line naming its pairs and writes nothing, and the loop stops at `epochs` kept seeds.  After ``max_seeds`` seeds it raises,
    naming the pair that collided most often: the one to put into 'excluded_pairs'.
    ``collision_margin`` > 0 (with ``reject_collisions``) also skips a seed whose links pass closer than the margin anywhere in
    its sequence; the printed line then names the closest pair and its distance.  ``containment=True`` (with
    ``reject_collisions``) also skips a seed with a link wholly inside another anywhere in its sequence, which neither of the two
    checks above can see; the printed line then says ``X inside Y``.
    ``source="depth"`` collects depth-camera frames of ``pix`` x ``pix`` images, ``ground`` stands the robot on the ground
    plane and removes it per camera (the reference's --pix / --ground); the ground needs the depth source."""
    if ground and source != "depth":
        raise ValueError("collect: ground=True needs source='depth' (the surface sampler has no ground to remove)")
    collision_margin = _checked_margin(collision_margin)
    if collision_margin > 0.0 and not reject_collisions:
        raise ValueError("collect: collision_margin needs reject_collisions=True")
    if containment and not reject_collisions:
        raise ValueError("collect: containment needs reject_collisions=True")
    paths, tally, seed = [], {}, 0
    use_excluded = bool(robot_params.get("collision_exclusion", False))
    while len(paths) < epochs:
        if reject_collisions and seed >= max_seeds:
            worst = max(tally, key=tally.get) if tally else None
            raise RuntimeError(f"collect: only {len(paths)} of {epochs} collision-free seeds among the first {max_seeds}; the pair "
                               f"that collided most often is {worst} ({tally.get(worst, 0)} seeds): if its links may touch, add it "
                               f"to the robot's 'excluded_pairs' and set 'collision_exclusion'")
        np.random.seed(seed)                                       # the ring of >= 20 cameras draws from the global state
        env = SimEnv(os.path.join(root, robot_params["gt"]), base_orientation=robot_params.get("sim_ori", [0, 0, 0]),
                     dof=robot_params["dof"], radius=robot_params.get("cam_dist", 1.5), num_cameras=num_cameras, ground_flag=ground,
                     excluded_pairs=robot_params.get("excluded_pairs", []))
        a_list = angle_list(num_step, step_size, robot_params["dof"], env.joint_limits, np.array([scale] * robot_params["dof"]), seed)
        closest, inside = [], []
        contain = {"containment": True, "inside": inside} if containment else {}
        if collision_margin > 0.0:
            hit = sequence_collides(env, a_list, use_excluded, margin=collision_margin, closest=closest, **contain)
        else:
            hit = sequence_collides(env, a_list, use_excluded, **contain) if reject_collisions else []
        if hit and inside:
            print(f"seed {seed}: {', '.join(inside)}: collision detected {hit}, skipped")
            for pr in hit:
                tally[pr] = tally.get(pr, 0) + 1
        elif hit and closest:
            d, step, la, lb = closest[0]
            print(f"seed {seed}: within the collision margin {collision_margin:g}: {hit}, closest {la} - {lb} at {d:.6g} (step {step}), skipped")
        elif hit:
            print(f"seed {seed}: collision detected {hit}, skipped")
            for pr in hit:
                tally[pr] = tally.get(pr, 0) + 1
        else:
            data_path = os.path.join(root, f"data/raw/{robot}/{step_size}_deg_{num_cameras}_cams/V{seed:04}/")
            os.makedirs(data_path, exist_ok=True)
            data_collection(env, data_path=data_path, width=pix, height=pix, angle_list=a_list, ground_flag=ground, noise_flag=noise,
                            num_points=num_points, seed=seed, source=source)
            paths.append(data_path)
        env.reset()
        seed += 1
    return paths


def _parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--robot', type=str, default='franka')
    ap.add_argument('--pix', type=int, default=800, help="width and height of the depth buffers")
    ap.add_argument('--depth', action='store_true', help="depth-camera frames (fused back-projected depth images) instead of surface samples")
    ap.add_argument('--ground', action='store_true', help="stand the robot on a ground plane and remove it per camera (needs --depth)")
    ap.add_argument('--scale', type=float, default=0.9)
    ap.add_argument('--step_size', type=int, default=4)
    ap.add_argument('--num_step', type=int, default=10)
    ap.add_argument('--epoch', type=int, default=5)
    ap.add_argument('--no_noise', action='store_true')
    ap.add_argument('--num_points', type=int, default=5000)
    ap.add_argument('--num_cameras', type=int, default=20)
    ap.add_argument('--reject_collisions', action='store_true', help="skip seeds whose sequence self-collides (or touches the ground), like the reference's collect()")
    ap.add_argument('--collision_margin', type=float, default=None, help="with --reject_collisions: also skip seeds whose links pass closer than this distance (default: the robot's 'collision_margin' in parameters.json, else 0)")
    ap.add_argument('--containment', action='store_true', default=None, help="with --reject_collisions: also skip seeds with a link wholly inside another (default: the robot's 'collision_containment' in parameters.json, else off)")
    return ap


def parse_args(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.containment and not args.reject_collisions:
        ap.error("--containment needs --reject_collisions: containment belongs to the collision check")
    if args.collision_margin is not None and not args.reject_collisions:
        ap.error("--collision_margin needs --reject_collisions: the margin belongs to the collision check")
    if args.collision_margin is not None and not args.collision_margin >= 0:
        ap.error("--collision_margin must be >= 0")
    if args.ground and not args.depth:
        ap.error("--ground needs --depth: only the depth-camera frames have a ground to remove")
    return args


def main(argv=None):
    """python -m autourdf_amd.sim_data --robot wx200_5 [...]: the reference's flags (sim_data.py:537-551) minus --gui / --vis,
    plus --depth, --reject_collisions, --collision_margin and --containment; reads 'gt' / 'dof' / 'sim_ori' of the robot from
    ./parameters.json, and its 'collision_margin' / 'collision_containment' when the option is not given."""
    import json
    args = parse_args(argv)
    with open('parameters.json') as f:
        params = json.load(f)[args.robot]
    if 'gt' not in params:
        raise SystemExit(f"parameters.json has no 'gt' URDF path for {args.robot!r} (use the reference's parameters.json)")
    margin = {}
    if args.reject_collisions:                                    # the option wins over the robot's entry
        m = args.collision_margin if args.collision_margin is not None else float(params.get("collision_margin", 0.0))
        margin = {"collision_margin": m} if m > 0 else {}
        if args.containment or (args.containment is None and bool(params.get("collision_containment", False))):
            margin["containment"] = True
    for p in collect(args.robot, params, args.num_step, args.step_size, args.epoch, args.scale, not args.no_noise,
                     args.num_points, args.num_cameras, source="depth" if args.depth else "surface", ground=args.ground, pix=args.pix,
                     reject_collisions=args.reject_collisions, **margin):
        print(p)


if __name__ == "__main__":
    main()
