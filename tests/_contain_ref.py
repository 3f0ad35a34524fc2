"""numpy restatement of the containment contract (include/creg.h, creg_mesh_contain_f64), written from the contract in its
operation order, plus the same term in np.longdouble as ground truth and the scenes the containment tests share.

    posed point    x = ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i with the point's own link's pose
    gate           x is evaluated against link b iff lo_b <= x <= hi_b on all three axes (the exact posed link box), else 0.0
    term           a = v0 - x, b = v1 - x, c = v2 - x; det = dot(a, cross(b, c));
                   den = (((la*lb)*lc + dot(a,b)*lc) + dot(b,c)*la) + dot(c,a)*lb; omega = 2*atan2(det, den)
    decision       w = S / (4 pi), inside iff |w| > 0.5

The total is np.sum here (pairwise), the device adds in its own fixed tree and has its own atan2: values are compared within the
bound K * 2^-53 * sum|omega| / (4 pi) of the tests, integers, gated zeros and decisions exactly."""
import functools

import numpy as np

from _collide_ref import all_pairs, box_mesh, pack, pose, random_rotation, rigid, uv_sphere   # noqa: F401  (shared with the tests)

FOUR_PI = 4.0 * np.pi
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps    # is long double wider than fp64 on this machine


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def pose_points(pts, T):
    """(n,3) link-frame points under the 4x4 pose T, by the vertex formula."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty_like(pts)
    for i in range(3):
        out[:, i] = ((T[i, 0] * pts[:, 0] + T[i, 1] * pts[:, 1]) + T[i, 2] * pts[:, 2]) + T[i, 3]
    return out


def omega(tri, x, dtype=np.float64):
    """The terms of the posed triangles tri (n,3,3) at the point x (3): (n) signed solid angles, computed in ``dtype``."""
    tri, x = np.asarray(tri, dtype), np.asarray(x, dtype)
    a, b, c = tri[:, 0] - x, tri[:, 1] - x, tri[:, 2] - x
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    det = dot(a, cross(b, c))
    den = (((la * lb) * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
    return 2 * np.arctan2(det, den)


def winding(tri, x):
    """w of the contract in fp64 with np.sum for the total."""
    return np.float64(np.sum(omega(tri, x))) / FOUR_PI


def winding_truth(tri, x):
    """(w, sum|omega| / (4 pi)) with every operation in np.longdouble (the posed fp64 vertices and point are the inputs)."""
    om = omega(tri, x, np.longdouble)
    four_pi = 16 * np.arctan(np.longdouble(1))
    return np.sum(om) / four_pi, np.float64(np.sum(np.abs(om)) / four_pi)


def is_inside(w):
    return np.abs(w) > 0.5


def mesh_contain(tri, tri_start, pts, pt_start, link_T, pairs, q_stride, truth=False):
    """inside (P,M,2) int32, first (P,M,2) int32, winding (P,M,2,Q) f64 and link_box (P,L,6) of creg_mesh_contain_f64; with
    ``truth`` also the long-double winding numbers and sum|omega| / (4 pi), both (P,M,2,Q), 0 where gated out."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, L, M, Q = link_T.shape[0], link_T.shape[1], len(pairs), int(q_stride)
    inside = np.zeros((P, M, 2), np.int32)
    first = np.full((P, M, 2), -1, np.int32)
    wind = np.zeros((P, M, 2, Q))
    exact = np.zeros((P, M, 2, Q), np.longdouble)
    mag = np.zeros((P, M, 2, Q))
    box = np.empty((P, L, 6))
    box[..., :3], box[..., 3:] = np.inf, -np.inf
    for p in range(P):
        posed = [pose(tri[tri_start[l]:tri_start[l + 1]], link_T[p, l]) for l in range(L)]
        points = [pose_points(pts[pt_start[l]:pt_start[l + 1]], link_T[p, l]) for l in range(L)]
        for l in range(L):
            if len(posed[l]):
                box[p, l, :3], box[p, l, 3:] = posed[l].reshape(-1, 3).min(0), posed[l].reshape(-1, 3).max(0)
        for m, (la, lb) in enumerate(pairs):
            if not (0 <= la < L and 0 <= lb < L) or la == lb:
                continue
            for d, (inner, outer) in enumerate(((la, lb), (lb, la))):
                for j, x in enumerate(points[inner]):
                    if not ((box[p, outer, :3] <= x).all() and (x <= box[p, outer, 3:]).all()):
                        continue
                    wind[p, m, d, j] = winding(posed[outer], x)
                    if truth:
                        exact[p, m, d, j], mag[p, m, d, j] = winding_truth(posed[outer], x)
                    if is_inside(wind[p, m, d, j]):
                        inside[p, m, d] += 1
                        if first[p, m, d] < 0:
                            first[p, m, d] = pt_start[inner] + j
    return (inside, first, wind, box, exact, mag) if truth else (inside, first, wind, box)


def open_cube(h):
    """The cube [-h,h]^3 with its +x face (two triangles) removed: the winding number at its centre is 5/6."""
    full = box_mesh(h, h, h)
    keep = ~((full[:, :, 0] == h).all(1))
    assert keep.sum() == 10
    return full[keep]


# ------------------------------------------------------------------------------------------ scenes of the GPU tests
SPHERES = ((8, 5), (16, 9), (256, 130))                          # closed UV spheres of 64, 256 and 66 048 triangles
CAPS = (1, 63, 65, 255, 257, 513, 32769)                         # open caps: around a wave, a chunk, two chunks, the grid stride
MESH_SIZE = 0.2                                                  # the diameter of every container below
KEEP_OFF = 1e-2                                                  # every evaluated point keeps this fraction of the posed box's diagonal from the surface
# which of a container scene's points are evaluated (inside the posed box) and which are gated to exactly 0.0, in pts order:
# near the centre, a third of the way to a corner, near a corner, beyond the box, on the hi face, one ulp beyond it, on the lo
# face, one ulp beyond it
EVALUATED = np.array([True, True, True, False, True, False, True, False])


def surface_distance(posed, x):
    from _clearance_ref import pt_tri2
    return float(np.sqrt(pt_tri2(np.tile(x, (len(posed), 1)), posed[:, 0], posed[:, 1], posed[:, 2]).min()))


@functools.lru_cache(maxsize=None)
def _sphere(seg, rings):
    mesh = uv_sphere(MESH_SIZE / 2, seg, rings)
    mesh.setflags(write=False)                                   # shared among the tests: left unchanged
    return mesh


def container_mesh(kind, size):
    """The closed sphere SPHERES[size], or the open cap of the first ``size`` triangles of the largest one."""
    return _sphere(*SPHERES[size]) if kind == "sphere" else _sphere(*SPHERES[-1])[:size]


def container_scene(mesh, seed=11):
    """Link 0: ``mesh`` under a random pose, owning one point (its first vertex's link-frame position pushed to (9,9,9): far
    from link 1).  Link 1: a small far cube under the identity pose, so that its eight points, given in world coordinates, are
    posed to exactly themselves -- see EVALUATED for where they lie about link 0's posed box.  An evaluated point closer than
    KEEP_OFF box diagonals to the surface is redrawn inside the box (on its face for the face points).  -> tri, tri_start, pts, pt_start,
    link_T (1,2,4,4), pairs [[1, 0]]: direction 0 tests the eight points against the container."""
    rng = np.random.default_rng(seed)
    T0 = rigid(random_rotation(rng), rng.uniform(-0.3, 0.3, 3))
    posed = pose(mesh, T0)
    lo, hi = posed.reshape(-1, 3).min(0), posed.reshape(-1, 3).max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    face = np.array([0.0, lo[1] + 0.05 * (hi[1] - lo[1]), lo[2] + 0.07 * (hi[2] - lo[2])])
    x = np.array([mid + half * (0.01, -0.02, 0.015), mid + half * (0.3, -0.3, 0.3), mid + half * (0.93, 0.93, -0.93),
                  mid + half * (1.5, 0.0, 0.0), face, face, face, face])
    x[4, 0], x[5, 0], x[6, 0], x[7, 0] = hi[0], np.nextafter(hi[0], np.inf), lo[0], np.nextafter(lo[0], -np.inf)
    for j in np.flatnonzero(EVALUATED):
        for _ in range(1000):
            if surface_distance(posed, x[j]) >= KEEP_OFF * np.linalg.norm(hi - lo):
                break
            keep0 = x[j, 0]
            x[j] = lo + rng.random(3) * (hi - lo)
            if j >= 4:
                x[j, 0] = keep0
        assert ((lo <= x[j]) & (x[j] <= hi)).all() and surface_distance(posed, x[j]) >= KEEP_OFF * np.linalg.norm(hi - lo)
    x[5, 1:], x[7, 1:] = x[4, 1:], x[6, 1:]
    tri, start = pack([mesh, box_mesh(0.01, 0.01, 0.01) + 5.0])
    pts = np.concatenate([[[9.0, 9.0, 9.0]], x])
    pt_start = np.array([0, 1, 9], np.int64)
    return tri, start, pts, pt_start, np.array([[T0, np.eye(4)]]), np.array([[1, 0]], np.int32)


def nested_cubes(P=3, seed=5, flip=False, opened=False):
    """A small cube (link 1, half 0.02) inside a large one (link 0, half 0.1), not touching, both under one random rigid motion
    per pose; a third cube (link 2) far outside.  Points: the 8 corners of each cube pulled 10 % towards its centre and the
    centre itself (9 per link).  ``flip`` reverses link 0's orientation, ``opened`` removes its +x face."""
    rng = np.random.default_rng(seed)
    big = open_cube(0.1) if opened else box_mesh(0.1, 0.1, 0.1)
    if flip:
        big = big[:, ::-1]
    tri, start = pack([big, box_mesh(0.02, 0.02, 0.02), box_mesh(0.02, 0.02, 0.02)])
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    pts = np.concatenate([np.concatenate([0.9 * h * corners, np.zeros((1, 3))]) for h in (0.1, 0.02, 0.02)])
    pt_start = np.array([0, 9, 18, 27], np.int64)
    link_T = []
    for _ in range(P):
        G = rigid(random_rotation(rng), rng.uniform(-0.2, 0.2, 3))
        link_T.append([G, G @ rigid(random_rotation(rng), rng.uniform(-0.05, 0.05, 3)), G @ rigid(random_rotation(rng), (0.4, 0.1, -0.2))])
    return tri, start, pts, pt_start, np.array(link_T), all_pairs(3)


def worst_ratio(tri, tri_start, pts, pt_start, link_T, pairs, q_stride):
    """The largest |w_fp64 - w_longdouble| / (2^-53 sum|omega| / (4 pi)) of the restatement over the evaluated points."""
    _, _, w, _, exact, mag = mesh_contain(tri, tri_start, pts, pt_start, link_T, pairs, q_stride, truth=True)
    on = mag > 0
    return float((np.abs(w[on].astype(np.longdouble) - exact[on]) / (np.longdouble(2.0) ** -53 * mag[on])).max()) if on.any() else 0.0
