"""Host-side truth for the lattice hull tests (imports nothing from the package): the certificate checker for the contract
of ``creg_lattice_hull_i32`` in exact integers, an exact brute-force hull for a few dozen points, the exact 6 x volume of a
triangulation, and the input builders.  Every determinant is below 6 * 2^45 for |coordinate| <= 16383, so int64 is exact."""
import itertools

import numpy as np

LIMIT = 16383


def _p(points):
    return np.asarray(points, np.int64).reshape(-1, 3)


def planes(points, tris):
    """Normal (F,3) and offset (F) of every face in int64: det(b-a, c-a, p-a) = n . p - d0."""
    P, T = _p(points), np.asarray(tris, np.int64).reshape(-1, 3)
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    n = np.cross(b - a, c - a)
    return n, (n * a).sum(1)


def volume6(points, tris):
    """Exact 6 x signed volume enclosed by a closed triangulation (positive when the normals point outward)."""
    P, T = _p(points), np.asarray(tris, np.int64).reshape(-1, 3)
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    return int((a * np.cross(b, c)).sum())


def certificate(points, tris, extreme_xyz=None):
    """The contract of a status-0 link, checked in full.  Returns the list of violations (empty = certified).
    extreme_xyz: coordinates that must all be among the vertices used (the extreme points of the set)."""
    P = _p(points)
    T = np.asarray(tris)
    bad = []
    if T.ndim != 2 or T.shape[1] != 3 or len(T) < 4:
        return [f"triangles of shape {T.shape}: at least 4 rows of 3 are needed"]
    T = T.astype(np.int64)
    if T.min() < 0 or T.max() >= len(P):
        return [f"vertex index outside 0 .. {len(P) - 1}"]
    if np.abs(P).max() > LIMIT:
        bad.append("coordinate beyond the limit")
    edges = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    key = edges[:, 0] * len(P) + edges[:, 1]
    uniq, cnt = np.unique(key, return_counts=True)
    if (cnt != 1).any():
        bad.append(f"{int((cnt != 1).sum())} directed edges occur more than once")
    rev = edges[:, 1] * len(P) + edges[:, 0]
    if not np.isin(rev, uniq).all():
        bad.append(f"{int((~np.isin(rev, uniq)).sum())} directed edges without their reverse (the surface is open)")
    if (edges[:, 0] == edges[:, 1]).any():
        bad.append("an edge from a vertex to itself")
    V, E, F = len(np.unique(T)), len(uniq) // 2, len(T)
    if V - E + F != 2:
        bad.append(f"V - E + F = {V} - {E} + {F} = {V - E + F}, not 2")
    # one component: faces joined through shared vertices
    parent = np.arange(len(P))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    if len({find(v) for v in np.unique(T)}) != 1:
        bad.append("the surface has more than one component")
    n, d0 = planes(P, T)
    if (~n.any(axis=1)).any():
        bad.append(f"{int((~n.any(axis=1)).sum())} triangles of zero area")
    worst, below = np.full(F, -1, np.int64), np.zeros(F, bool)
    for s in range(0, len(P), 4096):                              # (points, faces) determinants, a slab at a time
        D = P[s:s + 4096] @ n.T - d0
        worst = np.maximum(worst, D.max(0))
        below |= (D < 0).any(0)
    if (worst > 0).any():
        bad.append(f"{int((worst > 0).sum())} faces have a point strictly above them (largest determinant {int(worst.max())})")
    if (~below).any():
        bad.append(f"{int((~below).sum())} faces have no point strictly below them (an inward or flat face)")
    if volume6(P, T) <= 0:
        bad.append(f"6 x volume = {volume6(P, T)} is not positive")
    if extreme_xyz is not None:
        used = {tuple(p) for p in P[np.unique(T)].tolist()}
        missing = [tuple(p) for p in _p(extreme_xyz).tolist() if tuple(p) not in used]
        if missing:
            bad.append(f"{len(missing)} extreme points are no vertex of the hull, e.g. {missing[0]}")
    return bad


def brute_hull(points):
    """Exact hull of at most 40 points by trying every plane through three of them: (triangles (F,3) of indices into points,
    sorted extreme indices).  Each facet polygon is gift-wrapped in its own plane (corners only) and fanned, outward.
    ValueError if the points span no volume."""
    P = _p(points)
    if len(P) > 40:
        raise ValueError("brute_hull is for at most 40 points")
    _, first = np.unique(P, axis=0, return_index=True)
    ids = sorted(first.tolist())
    seen, tris = set(), []
    for i, j, k in itertools.combinations(ids, 3):
        n = np.cross(P[j] - P[i], P[k] - P[i])
        if not n.any():
            continue
        d = (P[ids] - P[i]) @ n
        if (d > 0).any() and (d < 0).any():
            continue
        if not d.any():
            raise ValueError("the points are coplanar")
        if (d > 0).any():
            n = -n                                                # outward: every point on or below
        g = np.gcd.reduce(np.abs(n))
        plane = tuple((n // g).tolist()) + (int(n @ P[i]) // int(g),)
        if plane in seen:
            continue
        seen.add(plane)
        on = [ids[q] for q in np.nonzero(d == 0)[0]]
        start = min(on, key=lambda q: tuple(P[q]))
        poly, cur = [start], start
        while True:
            nxt = None
            for q in on:
                if q == cur:
                    continue
                if nxt is None:
                    nxt = q
                    continue
                t = int(n @ np.cross(P[nxt] - P[cur], P[q] - P[cur]))
                if t < 0 or (t == 0 and ((P[q] - P[cur]) ** 2).sum() > ((P[nxt] - P[cur]) ** 2).sum()):
                    nxt = q                                       # q is to the right of cur -> nxt, or farther on the same ray
            if nxt == start:
                break
            poly.append(nxt)
            cur = nxt
            if len(poly) > len(on):
                raise AssertionError("gift wrapping did not close")
        tris += [(poly[0], poly[t], poly[t + 1]) for t in range(1, len(poly) - 1)]
    if not tris:
        raise ValueError("the points span no volume")
    T = np.array(tris, np.int64)
    return T, sorted(np.unique(T).tolist())


def scipy_hull(points):
    """Qhull's hull through scipy: (triangles (F,3) int64 turned outward by Qhull's own facet normals, sorted extreme indices).
    On lattice input Qhull's answer is certificate-clean with the exact volume (tests/test_hull_cpu.py checks the cases the GPU
    tests lean on), so ``vertices`` serve as the extreme set."""
    from scipy.spatial import ConvexHull
    P = _p(points)
    h = ConvexHull(P.astype(np.float64))
    T = h.simplices.astype(np.int64)
    n, _ = planes(P, T)
    flip = (n * h.equations[:, :3]).sum(1) < 0
    T[flip] = T[flip][:, [0, 2, 1]]
    return T, sorted(h.vertices.tolist())


# ---------------------------------------------------------------------------------------------------------- builders
def lattice_ball(r):
    """Every integer point with x^2 + y^2 + z^2 <= r^2, in lexicographic order (r = 12: 7153 points)."""
    g = np.arange(-r, r + 1)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return X[(X ** 2).sum(1) <= r * r].astype(np.int32)


def lattice_block(nx, ny, nz):
    """The filled nx x ny x nz block of integer points from the origin."""
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def block_corners(nx, ny, nz):
    return np.array(list(itertools.product((0, nx - 1), (0, ny - 1), (0, nz - 1))), np.int32)


def random_lattice(n, seed, span=50):
    return np.random.default_rng(seed).integers(-span, span + 1, (n, 3)).astype(np.int32)


def voxel_verts(occ):
    """The marching-cubes vertices of a 0/1 volume at level 0.5, as the mesher numbers space: voxel (x,y,z) of the unpadded
    grid sits at half-voxel coordinates 2 (x,y,z) + 1, and every lattice edge between an occupied and an empty voxel carries
    one vertex at its midpoint.  occ: bool array (X,Y,Z).  Returns (V,3) int32 (axis by axis, each in linear voxel order)."""
    O = np.pad(np.asarray(occ, bool), 1)
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        at = np.argwhere(O[tuple(lo)] != O[tuple(hi)])           # padded index of the edge's low voxel
        v = 2 * (at - 1) + 1
        v[:, a] += 1
        out.append(v)
    return np.ascontiguousarray(np.concatenate(out), np.int32)       # (argwhere's rows are a transposed view: make them C order)


def ellipsoid_occ(rx, ry, rz):
    gx, gy, gz = (np.arange(-r, r + 1) for r in (rx, ry, rz))
    X, Y, Z = np.meshgrid(gx, gy, gz, indexing="ij")
    return (X / rx) ** 2 + (Y / ry) ** 2 + (Z / rz) ** 2 <= 1.0


def limit_tetra():
    """A tetrahedron with corners at +-16383, and the integer points used against its face (0,1,2): the face's plane is
    x + y + z = -16383, its outward normal (-1,-1,-1)."""
    L = LIMIT
    return np.array([[L, -L, -L], [-L, L, -L], [-L, -L, L], [L, L, L]], np.int32)


def toy_link_clouds(n_links=4, n=1500, seed=0):
    """Link clouds of a toy robot: noisy points in boxes and ellipsoids of a few centimetres, one (n,3) float64 array per link."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(n_links):
        r = rng.uniform(0.02, 0.07, 3)
        x = rng.uniform(-1, 1, (n, 3))
        if l % 2:
            x = x[(x ** 2).sum(1) <= 1.0]
        out.append(x * r + rng.uniform(-0.05, 0.05, 3))
    return out


def write_toy_urdf(path, mesh_dir, n_links, skip_collision_of=None):
    """A chain of n_links links in the layout ``compute_joints.create_urdf`` writes: per link a <visual>, a <collision> that
    names the same {i:04}.stl under mesh_dir, and an <inertial>; revolute joints between neighbours; two-space indentation and
    an XML declaration.  skip_collision_of: a link index written without its <collision> block."""
    import xml.etree.ElementTree as ET
    robot = ET.Element("robot", name="estimated_robot")
    for i in range(n_links):
        link = ET.SubElement(robot, "link", name=f"link_{i}")
        xyz, rpy = f"{0.01 * i} 0.0 {-0.02 * i}", "0.0 0.0 0.0"
        visual = ET.SubElement(link, "visual")
        ET.SubElement(visual, "origin", xyz=xyz, rpy=rpy)
        ET.SubElement(ET.SubElement(visual, "geometry"), "mesh", filename=f"{mesh_dir}{i:04}.stl", scale="1 1 1")
        ET.SubElement(ET.SubElement(visual, "material", name=f"material_{i}"), "color", rgba="0.0 0.0 0.5 1")
        if i != skip_collision_of:
            collision = ET.SubElement(link, "collision")
            ET.SubElement(collision, "origin", xyz=xyz, rpy=rpy)
            ET.SubElement(ET.SubElement(collision, "geometry"), "mesh", filename=f"{mesh_dir}{i:04}.stl", scale="1 1 1")
        inertial = ET.SubElement(link, "inertial")
        ET.SubElement(inertial, "origin", xyz=xyz, rpy=rpy)
        ET.SubElement(inertial, "mass", value="1.0")
        ET.SubElement(inertial, "inertia", ixx="0.1", ixy="0.0", ixz="0.0", iyy="0.1", iyz="0.0", izz="0.1")
    for i in range(1, n_links):
        joint = ET.SubElement(robot, "joint", name=f"joint_{i}", type="revolute")
        ET.SubElement(joint, "parent", link=f"link_{i - 1}")
        ET.SubElement(joint, "child", link=f"link_{i}")
        ET.SubElement(joint, "origin", xyz="0.0 0.0 0.1", rpy="0.0 0.0 0.0")
        ET.SubElement(joint, "axis", xyz="0.0 0.0 1.0")
        ET.SubElement(joint, "limit", effort="100", velocity="100", lower="-3.14159", upper="3.14159")
    tree = ET.ElementTree(robot)
    ET.indent(tree, space="  ", level=0)
    tree.write(path, encoding="utf-8", xml_declaration=True)


def pack(links):
    """Concatenated (n,3) int32 points and (L+1) int64 offsets of a list of point arrays."""
    links = [np.asarray(p, np.int32).reshape(-1, 3) for p in links]
    off = np.concatenate([[0], np.cumsum([len(p) for p in links])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(links) if links else np.zeros((0, 3), np.int32)), off
