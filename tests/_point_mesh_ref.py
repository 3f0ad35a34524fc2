"""numpy restatement of the point-to-mesh contract (include/creg.h, creg_point_mesh_f64), written from the header in its operation
order, a long-double brute force without gating, and the analytic cases the point-mesh tests share.

    posed vertex   w_i = ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i                         (_collide_ref.pose)
    live           a point with no NaN coordinate; its box is lo = hi = the point
    gap2(p, box)   = (g_x^2 + g_y^2) + g_z^2,  g_k = max(0, max(lo[k] - p[k], p[k] - hi[k]))
    contributes    gap2(p_i, box_f) <= d_max * d_max, box_f the exact box of the three posed vertices
    d2(i, f)       pt_tri2(p_i; a, b, c), the header's seven cases                        (_clearance_ref._pt_tri2)
    result         best = +inf, idx = -1; ascending rows replace them when d2 < best

Elementwise numpy operations are single IEEE operations, so the values are the kernel's."""
import numpy as np

from _clearance_ref import _cm, _pt_tri2, gap2
from _collide_ref import box_mesh, pack, pose, random_rotation, rigid, uv_sphere  # noqa: F401  (re-exported to the tests)

INF = np.inf
BLOCK = 1 << 20                                                  # point-triangle terms evaluated at a time


def posed_mesh(tri, tri_start, T):
    """(F,3,3) posed triangles of one pose, T (L,4,4); rows outside every link stay NaN (there are none for a valid tri_start)."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    out = np.full_like(tri, np.nan)
    for l in range(len(tri_start) - 1):
        out[tri_start[l]:tri_start[l + 1]] = pose(tri[tri_start[l]:tri_start[l + 1]], T[l])
    return out


def point_gap2(p, lo, hi):
    """The header's gap2(p, box): p (n,1,3) against boxes (1,F,3)."""
    g = np.maximum(0.0, np.maximum(lo - p, p - hi))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def pose_points(W, pts, dmax2):
    """(dist2, tri_idx) of points (n,3) against posed triangles W (F,3,3), the contract of one pose."""
    n, F = len(pts), len(W)
    dist2, idx = np.full(n, INF), np.full(n, -1, np.int32)
    if n == 0 or F == 0:
        return dist2, idx
    lo, hi = W.min(1), W.max(1)
    live = ~np.isnan(pts).any(1)
    step = max(1, BLOCK // F)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, step):
            p = pts[i0:i0 + step]
            ok = (point_gap2(p[:, None], lo[None], hi[None]) <= dmax2) & live[i0:i0 + step, None]
            ii, ff = np.nonzero(ok)                              # row-major: ascending f per point
            if len(ii) == 0:
                continue
            d = _pt_tri2(_cm(p[ii]), _cm(W[ff, 0]), _cm(W[ff, 1]), _cm(W[ff, 2]))
            full = np.full(ok.shape, INF)
            full[ii, ff] = np.where(np.isnan(d), INF, d)         # a d2 that is not below +inf never replaces the running best
            best = full.min(1)
            first = np.argmax(full == best[:, None], axis=1)     # the smallest row with exactly those bits
            hit = best < INF
            dist2[i0:i0 + step] = best
            idx[i0:i0 + step] = np.where(hit, first, -1)
    return dist2, idx


def point_mesh(tri, tri_start, link_T, pts, pt_start, d_max):
    """dist2 (N) f64, tri_idx (N) int32, link_box (P,L,6) f64 of creg_point_mesh_f64."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    P, L, N = link_T.shape[0], link_T.shape[1], len(pts)
    dmax2 = np.float64(d_max) * np.float64(d_max)
    dist2, idx = np.full(N, INF), np.full(N, -1, np.int32)
    box = np.empty((P, L, 6))
    box[..., :3], box[..., 3:] = INF, -INF
    for p in range(P):
        W = posed_mesh(tri, tri_start, link_T[p])
        for l in range(L):
            v = W[tri_start[l]:tri_start[l + 1]].reshape(-1, 3)
            if len(v):
                box[p, l, :3], box[p, l, 3:] = v.min(0), v.max(0)
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        dist2[s:e], idx[s:e] = pose_points(W, pts[s:e], dmax2)
    return dist2, idx, box


def wrapper(dist2, tri_idx, tri_start, d_max):
    """dist, tri_idx, link of ops.point_mesh_distance from the entry's outputs: sqrt, +inf beyond d_max, the row's owner."""
    dmax2 = np.float64(d_max) * np.float64(d_max)
    with np.errstate(invalid="ignore"):
        dist = np.where(dist2 > dmax2, INF, np.sqrt(dist2))
    owner = (np.searchsorted(np.asarray(tri_start), tri_idx, side="right") - 1).astype(np.int32)
    return dist, tri_idx, np.where(tri_idx >= 0, owner, -1).astype(np.int32)


def tri_d2(W, f, pts):
    """The restated d2 of points (n,3) against the posed rows f (n) of W."""
    return _pt_tri2(_cm(pts), _cm(W[f, 0]), _cm(W[f, 1]), _cm(W[f, 2]))


# ------------------------------------------------------------------------------------------ long-double brute force, no gating
def brute_long_double(W, pts):
    """Distances (n) in long double of points from posed triangles W (F,3,3): projection on the plane when it falls inside the
    triangle, else the nearest of the three edges as clamped segments -- another formulation than the header's regions."""
    ld = np.longdouble
    W, pts = np.asarray(W, ld), np.asarray(pts, ld)
    a, b, c = W[None, :, 0], W[None, :, 1], W[None, :, 2]
    p = pts[:, None]

    def seg(u, v):
        e = v - u
        ee = (e * e).sum(-1)
        t = np.where(ee > 0, ((p - u) * e).sum(-1) / np.where(ee > 0, ee, 1), 0)
        t = np.clip(t, 0, 1)
        r = p - (u + e * t[..., None])
        return (r * r).sum(-1)

    d2 = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    h = ((p - a) * nrm).sum(-1)
    foot = p - nrm * (h / np.where(nn > 0, nn, 1))[..., None]
    inside = (nn > 0)
    for u, v in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(v - u, foot - u) * nrm).sum(-1) >= 0)
    d2 = np.where(inside, np.minimum(d2, h * h / np.where(nn > 0, nn, 1)), d2)
    return np.sqrt(d2.min(1)).astype(np.float64)


# ------------------------------------------------------------------------------------------ analytic cases: one triangle
TRI = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
H = 0.75
# name -> (point, expected DISTANCE as a formula): one point in each of the seven Voronoi regions, and one on the triangle
ONE_TRIANGLE = {
    "face": ([1, 1, H], H),
    "vertex_a": ([-1, -2, 2], np.sqrt(1.0 + 4.0 + 4.0)),
    "vertex_b": ([6, -1, 2], np.sqrt(4.0 + 1.0 + 4.0)),
    "vertex_c": ([-1, 6, -2], np.sqrt(1.0 + 4.0 + 4.0)),
    "edge_ab": ([2, -1, H], np.sqrt(1.0 + H * H)),
    "edge_ac": ([-2, 2, 1], np.sqrt(4.0 + 1.0)),
    "edge_bc": ([3, 3, 1], np.sqrt(2.0 + 1.0)),                  # the foot is (2,2,0) on x + y = 4
    "on_triangle": ([1, 2, 0], 0.0),
}

# the unit cube [0,1]^3 as 12 triangles: point -> expected distance
CUBE = box_mesh(0.5, 0.5, 0.5) + 0.5
CUBE_CASES = {
    "off_face": ([0.5, 0.25, 1.5], 0.5),
    "off_edge": ([0.5, 2.0, 2.0], np.sqrt(2.0)),
    "off_corner": ([2.0, 2.0, 2.0], np.sqrt(3.0)),
    "off_corner_negative": ([-1.0, -2.0, -2.0], 3.0),
    "inside": ([0.5, 0.5, 0.875], 0.125),                        # unsigned: the nearest face
    "inside_centre": ([0.5, 0.5, 0.5], 0.5),
}


def scene_diagonal(tri, tri_start, link_T, pts):
    """Diagonal of the box of all posed vertices of all poses and all finite points: the scale of the value tolerance."""
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    v = [posed_mesh(tri, tri_start, T).reshape(-1, 3) for T in link_T]
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    v = np.concatenate(v + [pts[np.isfinite(pts).all(1)]])
    return float(np.linalg.norm(v.max(0) - v.min(0)))
