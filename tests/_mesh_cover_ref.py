"""numpy restatement of the mesh-cover contract (include/creg.h, creg_mesh_cover_f64), written from the header: the transposed
reduction of the point-to-mesh matrix (tests/_point_mesh_ref.py), with labels, and a long-double brute force of the point side.

    posed vertex, live, gap2, contributes, d2(i, f)    those of _point_mesh_ref, word for word
    label(i)       pt_row[i] if pt_row is given, else i
    result of f    best = +inf, idx = -1, near = 0; every live point i of the pose to which f contributes replaces (best, idx) by
                   (d2, label) iff d2 < best or (d2 == best and idx >= 0 and label < idx); near += (d2 < +inf and d2 <= d_max^2)

so dist2 is the column minimum of the gated matrix, pt_idx the smallest label with exactly its bits and n_near the column's count
of values within d_max^2.  Elementwise numpy operations are single IEEE operations, so the values are the kernel's."""
import numpy as np

import _point_mesh_ref as pref
from _clearance_ref import _cm, _pt_tri2

INF = np.inf
BLOCK = 1 << 20                                                  # point-triangle terms evaluated at a time


def gated_matrix(W, pts, dmax2):
    """(n,F) d2 of points (n,3) against posed triangles W (F,3,3): +inf where the triangle does not contribute to the point, where
    the point is not live and where d2 is not below +inf (a NaN from an infinite coordinate replaces nothing)."""
    n, F = len(pts), len(W)
    full = np.full((n, F), INF)
    if n == 0 or F == 0:
        return full
    lo, hi = W.min(1), W.max(1)
    live = ~np.isnan(pts).any(1)
    step = max(1, BLOCK // F)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, step):
            p = pts[i0:i0 + step]
            ok = (pref.point_gap2(p[:, None], lo[None], hi[None]) <= dmax2) & live[i0:i0 + step, None]
            ii, ff = np.nonzero(ok)
            if len(ii) == 0:
                continue
            d = _pt_tri2(_cm(p[ii]), _cm(W[ff, 0]), _cm(W[ff, 1]), _cm(W[ff, 2]))
            full[i0 + ii, ff] = np.where(np.isnan(d), INF, d)
    return full


def pose_cover(W, pts, labels, dmax2):
    """(dist2, pt_idx, n_near) of posed triangles W (F,3,3) against points (n,3) with int labels (n): the contract of one pose."""
    full = gated_matrix(W, pts, dmax2)
    return reduce_matrix(full, labels, dmax2)


def reduce_matrix(full, labels, dmax2):
    n, F = full.shape
    if n == 0:
        return np.full(F, INF), np.full(F, -1, np.int32), np.zeros(F, np.int32)
    best = full.min(0)
    hit = best < INF
    lab = np.where(full == best[None], np.asarray(labels, np.int64)[:, None], np.iinfo(np.int64).max).min(0)
    near = ((full < INF) & (full <= dmax2)).sum(0).astype(np.int32)
    return best, np.where(hit, lab, -1).astype(np.int32), near


def mesh_cover(tri, tri_start, link_T, pts, pt_start, d_max, pt_row=None):
    """dist2 (P,F) f64, pt_idx (P,F) int32, n_near (P,F) int32, link_box (P,L,6) f64 of creg_mesh_cover_f64 (valid tri_start: every
    row is owned)."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    P, L, N, F = link_T.shape[0], link_T.shape[1], len(pts), len(tri)
    labels = np.arange(N) if pt_row is None else np.asarray(pt_row)
    dmax2 = np.float64(d_max) * np.float64(d_max)
    dist2, idx, near = np.full((P, F), INF), np.full((P, F), -1, np.int32), np.zeros((P, F), np.int32)
    box = np.empty((P, L, 6))
    box[..., :3], box[..., 3:] = INF, -INF
    for p in range(P):
        W = pref.posed_mesh(tri, tri_start, link_T[p])
        for l in range(L):
            v = W[tri_start[l]:tri_start[l + 1]].reshape(-1, 3)
            if len(v):
                box[p, l, :3], box[p, l, 3:] = v.min(0), v.max(0)
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        dist2[p], idx[p], near[p] = pose_cover(W, pts[s:e], labels[s:e], dmax2)
    return dist2, idx, near, box


def wrapper(dist2, d_max):
    """dist of ops.mesh_cover from the entry's dist2: sqrt, +inf beyond d_max."""
    dmax2 = np.float64(d_max) * np.float64(d_max)
    with np.errstate(invalid="ignore"):
        return np.where(dist2 > dmax2, INF, np.sqrt(dist2))


def ambiguous(tri, tri_start, link_T, pts, pt_start, d_max, tol2):
    """(P,F) bool: the triangles whose pt_idx or n_near a result within ``tol2`` (on squared distances) of the restatement's may
    differ in: the runner-up d2 is within tol2 of the minimum, or some restated d2 is within tol2 of d_max^2."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    link_T = link_T[None] if link_T.ndim == 3 else link_T
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    dmax2 = np.float64(d_max) * np.float64(d_max)
    out = np.zeros((link_T.shape[0], len(tri)), bool)
    for p in range(link_T.shape[0]):
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        full = gated_matrix(pref.posed_mesh(tri, tri_start, link_T[p]), pts[s:e], dmax2)
        if full.shape[0] >= 2:
            two = np.partition(full, 1, axis=0)[:2]
            with np.errstate(invalid="ignore"):
                out[p] |= np.isfinite(two[1]) & (two[1] - two[0] <= tol2)
        if np.isfinite(dmax2) and full.shape[0]:
            out[p] |= (np.isfinite(full) & (np.abs(full - dmax2) <= tol2)).any(0)
    return out


class OpsWith:
    """``autourdf_amd.ops`` with some names replaced, for ``monkeypatch.setattr(compute_joints, "ops", OpsWith(ops, mesh_cover=stub))``:
    the package's own namespace is left as it is (tests/test_host_cpu.py lists it name by name)."""

    def __init__(self, real, **over):
        self._real, self._over = real, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._real, name)


# ------------------------------------------------------------------------------------------ long-double brute force, no gating
def brute_long_double(W, pts):
    """Distances (F) in long double of posed triangles W (F,3,3) from the nearest of the points: the transpose of
    _point_mesh_ref.brute_long_double's matrix -- projection on the plane when it falls inside the triangle, else the nearest of the
    three edges as clamped segments -- minimised over the points."""
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
    return np.sqrt(d2.min(0)).astype(np.float64)


# ------------------------------------------------------------------------------------------ the scene both test files share
LINK_SIZES = (0, 1, 255, 256, 257, 300)
POSE_POINTS = (0, 65, 129)
EDGE_SEED = 23
EDGE_D_MAX = 0.02
WIDTH_SIZES = (16, 17, 32, 33, 64, 65, 128, 129)                 # around every width at which the kernel holds a short chunk 16 .. 1 times
WIDTH_POINTS = (200,)


def edge_scene(pose_points=POSE_POINTS, seed=EDGE_SEED, link_sizes=LINK_SIZES):
    """Links of 0, 1, 255, 256, 257 and 300 triangles (strips of a sphere's rows: a link then starts off a multiple of 256), three
    poses owning 0, 65 and 129 points: half of them near posed vertices (within about d_max), the others anywhere in the scene, a
    NaN point and a point with an infinite coordinate among them."""
    rng = np.random.default_rng(seed)
    meshes = [np.zeros((0, 3, 3)) if n == 0 else np.array([[[-0.15, -0.1, 0.0], [0.15, -0.1, 0.0], [0.0, 0.2, 0.0]]]) if n == 1
              else pref.uv_sphere(0.1, n=n) for n in link_sizes]
    tri, start = pref.pack(meshes)
    P, L = len(pose_points), len(link_sizes)
    link_T = np.array([[pref.rigid(pref.random_rotation(rng), rng.uniform(-0.15, 0.15, 3)) for _ in range(L)] for _ in range(P)])
    pt_start = np.concatenate([[0], np.cumsum(pose_points)]).astype(np.int64)
    pts = []
    for p, n in enumerate(pose_points):
        W = pref.posed_mesh(tri, start, link_T[p])
        on = W[rng.integers(0, len(W), n), rng.integers(0, 3, n)] + rng.normal(scale=0.4 * EDGE_D_MAX, size=(n, 3))
        off = rng.uniform(-0.3, 0.3, (n, 3))
        x = np.where((np.arange(n) % 2 == 0)[:, None], on, off)
        if n >= 64:
            x[7, 1] = np.nan
            x[n - 1, 2] = np.inf
        pts.append(x)
    return tri, start, link_T, np.concatenate(pts), pt_start
