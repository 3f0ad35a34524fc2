"""numpy / scipy restatement of the link mesher's contract (DESIGN N4): statistical outlier removal, voxel occupancy,
marching cubes at level 0.5 on the padded 0/1 volume, one pass of simple smoothing and the STL records.  Imports nothing
from autourdf_amd; the case table comes from the generator under tools/."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = load_generator()
TABLE = _GEN.build_table()
AXES_OTHER = ((1, 2), (0, 2), (0, 1))


def edge_owner(e):
    """(offset of the owning node from the cell's low corner, axis) of edge e."""
    a, j = e >> 2, e & 3
    b, c = AXES_OTHER[a]
    o = [0, 0, 0]
    o[b], o[c] = j & 1, j >> 1
    return tuple(o), a


# ---------------------------------------------------------------------------------------- (a) outliers
def statistical_outlier(points, offsets, nb_neighbors=20, std_ratio=2.0):
    """(keep uint8 (n), avg (n), thr (L)): mean distance to the k' = min(nb, n_link) nearest points of the own link, self
    included; threshold mean + ratio * std (ddof 1) over the points with avg > 0; fewer than two such points: thr NaN."""
    from scipy.spatial import cKDTree
    points = np.asarray(points, np.float64).reshape(-1, 3)
    L = len(offsets) - 1
    avg, thr, keep = np.zeros(len(points)), np.full(L, np.nan), np.zeros(len(points), np.uint8)
    for l in range(L):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        if hi == lo:
            continue
        p = points[lo:hi]
        k = min(nb_neighbors, hi - lo)
        d, _ = cKDTree(p).query(p, k=k)
        d = np.asarray(d, np.float64).reshape(hi - lo, k)
        a = d.sum(axis=1) / k
        avg[lo:hi] = a
        pos = a[a > 0]
        if len(pos) >= 2:
            mean = pos.mean()
            thr[l] = mean + std_ratio * np.sqrt(((pos - mean) ** 2).sum() / (len(pos) - 1))
            keep[lo:hi] = (a > 0) & (a < thr[l])
    return keep, avg, thr


def min_threshold_gap(avg, thr, offsets):
    """Smallest |avg_i - thr| / thr over the points with avg > 0 of links that have a threshold."""
    gap = np.inf
    for l in range(len(offsets) - 1):
        a = avg[int(offsets[l]):int(offsets[l + 1])]
        a = a[a > 0]
        if len(a) and np.isfinite(thr[l]):
            gap = min(gap, float(np.min(np.abs(a - thr[l]) / thr[l])))
    return gap


# ---------------------------------------------------------------------------------------- (b) occupancy
def voxelize(points, voxel_size):
    """(origin (3), dims (3) int, padded 0/1 volume (dims + 2)) of one link's kept points."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    origin = p.min(axis=0) - voxel_size / 2
    q = (p - origin) / voxel_size
    idx = np.floor(q).astype(np.int64)
    dims = idx.max(axis=0) + 1
    vol = np.zeros(tuple(dims + 2), np.uint8)
    vol[idx[:, 0] + 1, idx[:, 1] + 1, idx[:, 2] + 1] = 1
    return origin, dims, vol


def min_quotient_gap(points, voxel_size):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    q = (p - (p.min(axis=0) - voxel_size / 2)) / voxel_size
    return float(np.min(np.abs(q - np.rint(q))))


# ---------------------------------------------------------------------------------------- (c) marching cubes
def marching_cubes(vol):
    """(verts_h (V,3) int32 in half-voxel units of the unpadded grid, tris (F,3) int32) of a padded 0/1 volume.
    Vertices: by owning node in linear-index order, then axis; triangles: by cell in linear-index order, then table order."""
    vol = np.asarray(vol) != 0
    X, Y, Z = vol.shape
    act = np.zeros((X, Y, Z, 3), bool)
    act[:-1, :, :, 0] = vol[:-1] != vol[1:]
    act[:, :-1, :, 1] = vol[:, :-1] != vol[:, 1:]
    act[:, :, :-1, 2] = vol[:, :, :-1] != vol[:, :, 1:]
    vid = (np.cumsum(act.reshape(-1)) - act.reshape(-1)).reshape(X, Y, Z, 3)     # exclusive scan: node-major, then axis
    node = np.argwhere(act)
    verts = (2 * node[:, :3] - 1).astype(np.int32)
    verts[np.arange(len(node)), node[:, 3]] += 1
    mask = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        mask |= vol[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
    cells = np.argwhere((mask != 0) & (mask != 255))
    cm = mask[cells[:, 0], cells[:, 1], cells[:, 2]]
    lin = (cells[:, 0] * Y + cells[:, 1]) * Z + cells[:, 2]        # a cell sorts as the node at its low corner
    rows, keys = [np.zeros((0, 3), np.int64)], [np.zeros(0, np.int64)]
    for m in np.unique(cm):
        sel = cells[cm == m]
        for t, tri in enumerate(TABLE[m]):
            cols = []
            for e in tri:
                (ox, oy, oz), a = edge_owner(e)
                assert act[sel[:, 0] + ox, sel[:, 1] + oy, sel[:, 2] + oz, a].all()
                cols.append(vid[sel[:, 0] + ox, sel[:, 1] + oy, sel[:, 2] + oz, a])
            rows.append(np.stack(cols, 1))
            keys.append(lin[cm == m] * 8 + t)                       # cell order, then table order
    tris = np.concatenate(rows)[np.argsort(np.concatenate(keys), kind="stable")]
    return verts.reshape(-1, 3), tris.astype(np.int32).reshape(-1, 3)


def edge_balance(tris):
    """True iff every directed edge a->b occurs exactly as often as b->a."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return True
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(e.max()) + 1
    fwd = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    bwd = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return len(fwd[0]) == len(bwd[0]) and bool((fwd[0] == bwd[0]).all() and (fwd[1] == bwd[1]).all())


def six_volume(verts_h, tris):
    """Six times the signed enclosed volume in half-voxel units cubed: an exact integer."""
    v = np.asarray(verts_h, np.int64)
    t = np.asarray(tris, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return int(np.einsum("ij,ij->i", a, np.cross(b, c)).sum())


# ---------------------------------------------------------------------------------------- (d) smoothing, (e) STL
def smooth_sums(verts_h, tris):
    """(integer neighbour sums (V,3), degrees (V)): for every triangle (a,b,c), b joins a's multiset, c b's and a c's."""
    v = np.asarray(verts_h, np.int64)
    t = np.asarray(tris, np.int64)
    s, deg = np.zeros_like(v), np.zeros(len(v), np.int64)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        np.add.at(s, t[:, i], v[t[:, j]])
        np.add.at(deg, t[:, i], 1)
    return s, deg


def world_vertices(verts_h, tris, origin, voxel_size, smooth=True):
    v = np.asarray(verts_h, np.int64).astype(np.float64)
    if smooth:
        s, deg = smooth_sums(verts_h, tris)
        v = (np.asarray(verts_h, np.int64) + s).astype(np.float64) / (1 + deg)[:, None].astype(np.float64)
    return np.asarray(origin, np.float64) + (voxel_size / 2) * v


def stl_records(vertices, tris):
    """(F,4,3) float32: unit normal of the float32-rounded vertices (fp64 arithmetic, zero for a zero-area facet), then them."""
    v32 = np.asarray(vertices, np.float64).astype(np.float32)
    t = np.asarray(tris, np.int64)
    rec = np.zeros((len(t), 4, 3), np.float32)
    if len(t) == 0:
        return rec
    p = v32[t].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.sqrt((n * n).sum(axis=1))
    ok = ln > 0
    n[ok] /= ln[ok, None]
    n[~ok] = 0
    rec[:, 0] = n.astype(np.float32)
    rec[:, 1:] = v32[t]
    return rec


def mesh_link(points, voxel_size, smooth=True):
    origin, dims, vol = voxelize(points, voxel_size)
    verts_h, tris = marching_cubes(vol)
    vertices = world_vertices(verts_h, tris, origin, voxel_size, smooth)
    return dict(origin=origin, dims=dims, verts_h=verts_h, triangles=tris, vertices=vertices,
                stl_records=stl_records(vertices, tris))
