"""N4 link meshing: outlier removal, voxel occupancy and marching cubes, exact lattice hulls."""
import numpy as np

import torch

from .. import _lib
from ._common import _host_offsets_ok, _need, _p, _stream, _workspace

MESH_MAX_NEIGHBORS = 32
HULL_MAX_COORD = 16383
HULL_STATUS = {0: "ok", 1: "fewer than 4 points", 2: "all points identical", 3: "all points collinear", 4: "all points coplanar",
               5: f"a coordinate beyond {HULL_MAX_COORD}", 6: "offsets are no range of the points", 7: "face slots exhausted",
               8: "round bound exhausted", 9: "a horizon that is no closed cycle"}


def _mesh_inputs(points, offsets, what):
    points = _need(points, torch.float64, "points")
    offsets = _need(offsets, torch.int64, "offsets")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (n,3)")
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError(f"{what}: offsets must be (L+1) with L >= 1")
    off = offsets.cpu().numpy()
    if not _host_offsets_ok(off, points.shape[0]):
        raise ValueError(f"{what}: offsets must be non-decreasing from 0 to len(points)")
    return points, offsets, off


def _check_mesh(rc, what):
    """CREG_EINVAL of the meshing entry points is a refusal of the caller's values: ValueError with the library's text."""
    if rc == -1:
        raise ValueError(_lib.load(False).creg_last_error().decode())
    _lib.check(rc, what)


def statistical_outlier(points: torch.Tensor, offsets: torch.Tensor, nb_neighbors: int = 20, std_ratio: float = 2.0):
    """Statistical outlier removal of every link in one set of launches (creg_statistical_outlier_f64; DESIGN N4).
    points (n,3) f64 concatenated, offsets (L+1) int64.  Returns (keep (n) uint8, avg (n) f64, thr (L) f64)."""
    L_ = _lib.load()
    points, offsets, _ = _mesh_inputs(points, offsets, "statistical_outlier")
    if not 1 <= int(nb_neighbors) <= MESH_MAX_NEIGHBORS:
        raise ValueError(f"statistical_outlier: nb_neighbors must be in [1, {MESH_MAX_NEIGHBORS}], got {nb_neighbors}")
    n, L = points.shape[0], offsets.numel() - 1
    dev = points.device
    avg = torch.empty(n, dtype=torch.float64, device=dev)
    thr = torch.empty(L, dtype=torch.float64, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    _check_mesh(L_.creg_statistical_outlier_f64(_p(points) if n else None, n, _p(offsets), L, int(nb_neighbors), float(std_ratio),
                                                _p(avg), _p(thr), _p(keep), _stream()), "creg_statistical_outlier_f64")
    return keep, avg, thr


def voxel_layout(dims, n_kept):
    """Node offsets (L+1) int64 of the padded volumes, or ValueError for a link without points, a padded axis above 1024
    nodes or more than 2^28 nodes in total (creg_voxel_layout: host arrays only, no device call)."""
    L_ = _lib.load(check_device=False)
    dims = np.ascontiguousarray(dims, np.int32).reshape(-1, 3)
    n_kept = np.ascontiguousarray(n_kept, np.int64).reshape(-1)
    if len(n_kept) != len(dims) or len(dims) < 1:
        raise ValueError("voxel_layout: dims must be (L,3) and n_kept (L) with L >= 1")
    node_off = np.zeros(len(dims) + 1, np.int64)
    _check_mesh(L_.creg_voxel_layout(dims.ctypes.data, n_kept.ctypes.data, len(dims), node_off.ctypes.data), "creg_voxel_layout")
    return node_off


def voxel_mesh(points: torch.Tensor, offsets: torch.Tensor, voxel_size: float, smooth: bool = True, keep=None):
    """Voxel occupancy, marching cubes at level 0.5, one simple smoothing pass and STL records of every link in one set of
    launches (DESIGN N4).  points (n,3) f64 concatenated, offsets (L+1) int64, keep (n) uint8 or None (= every point).
    Returns one dict per link: vertices (V,3) f64, verts_h (V,3) int32 (half-voxel units), triangles (F,3) int32,
    stl_records (F,4,3) f32, origin (3) f64, dims (3) int32.  The host waits twice: for the grid sizes, then for the
    vertex and triangle totals."""
    L_ = _lib.load()
    points, offsets, _ = _mesh_inputs(points, offsets, "voxel_mesh")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0 and np.isfinite(voxel_size)):
        raise ValueError(f"voxel_mesh: voxel_size must be positive and finite, got {voxel_size}")
    n, L = points.shape[0], offsets.numel() - 1
    dev = points.device
    if keep is not None:
        keep = _need(keep, torch.uint8, "keep")
        if tuple(keep.shape) != (n,):
            raise ValueError("voxel_mesh: keep must be (n)")
    st = _stream()
    origin = torch.empty(L, 3, dtype=torch.float64, device=dev)
    dims = torch.empty(L, 3, dtype=torch.int32, device=dev)
    n_kept = torch.empty(L, dtype=torch.int64, device=dev)
    _check_mesh(L_.creg_voxel_bounds_f64(_p(points) if n else None, n, _p(offsets), L, _p(keep), voxel_size, _p(origin), _p(dims),
                                         _p(n_kept), st), "creg_voxel_bounds_f64")
    dims_h = dims.cpu().numpy()                                      # first wait: the grids size everything below
    node_off_h = voxel_layout(dims_h, n_kept.cpu().numpy())
    total = int(node_off_h[-1])
    node_off = torch.from_numpy(node_off_h).to(dev)
    occ = torch.empty(total, dtype=torch.uint8, device=dev)
    _check_mesh(L_.creg_voxel_fill_f64(_p(points), n, _p(offsets), L, _p(keep), voxel_size, _p(origin), _p(dims), _p(node_off), total,
                                       _p(occ), st), "creg_voxel_fill_f64")
    ws_bytes = int(L_.creg_mc_workspace_bytes(total))
    ws = _workspace(dev, ws_bytes)
    voff = torch.empty(L + 1, dtype=torch.int64, device=dev)
    toff = torch.empty(L + 1, dtype=torch.int64, device=dev)
    _check_mesh(L_.creg_mc_count_u8(_p(occ), _p(dims), _p(node_off), L, total, _p(voff), _p(toff), _p(ws), ws_bytes, st),
                "creg_mc_count_u8")
    voff_h, toff_h = voff.cpu().numpy(), toff.cpu().numpy()          # second wait: the totals size the outputs
    V, F = int(voff_h[-1]), int(toff_h[-1])
    verts_h = torch.empty(V, 3, dtype=torch.int32, device=dev)
    tris = torch.empty(F, 3, dtype=torch.int32, device=dev)
    _check_mesh(L_.creg_mc_emit_i32(_p(dims), _p(node_off), L, total, _p(voff), V, F, _p(verts_h) if V else None,
                                    _p(tris) if F else None, _p(ws), ws_bytes, st), "creg_mc_emit_i32")
    vertices = torch.empty(V, 3, dtype=torch.float64, device=dev)
    rec = torch.empty(F, 4, 3, dtype=torch.float32, device=dev)
    fb = int(L_.creg_mesh_finish_workspace_bytes(V)) if smooth else 0
    fws = _workspace(dev, fb)
    _check_mesh(L_.creg_mesh_finish_f64(_p(verts_h) if V else None, V, _p(tris) if F else None, F, _p(voff), _p(toff), L, _p(origin),
                                        voxel_size, 1 if smooth else 0, _p(vertices) if V else None, _p(rec) if F else None,
                                        _p(fws), fb, st), "creg_mesh_finish_f64")
    origin_h = origin.cpu().numpy()
    return [dict(vertices=vertices[voff_h[l]:voff_h[l + 1]], verts_h=verts_h[voff_h[l]:voff_h[l + 1]],
                 triangles=tris[toff_h[l]:toff_h[l + 1]], stl_records=rec[toff_h[l]:toff_h[l + 1]],
                 origin=origin_h[l], dims=dims_h[l]) for l in range(L)]


def lattice_hull(verts_h: torch.Tensor, offsets, origin=None, voxel_size=None, strict: bool = True):
    """Exact convex hull of every link's lattice points in one launch (creg_lattice_hull_i32 / _emit_i32; DESIGN N4).
    verts_h (n,3) int32 concatenated (``voxel_mesh``'s verts_h: half-voxel units, |v| <= 16383), offsets (L+1) int64 (tensor
    or array).  With origin (L,3) f64 and voxel_size the emitting launch also writes STL records of
    origin + (voxel_size / 2) * v.  Returns one dict per link: triangles (F,3) int32 (indices local to the link, outward),
    vertex_ids (sorted unique int64), status (int, 0 = a certified hull; ``HULL_STATUS`` names the others) and stl_records
    (F,4,3) f32 when asked.  A link of non-zero status has no triangles; strict=True raises ValueError naming the first such
    link instead.  A coordinate beyond the limit or offsets that do not run from 0 to n without decreasing raise ValueError
    before anything is launched.  The host waits once, for the face counts."""
    L_ = _lib.load()
    verts_h = _need(verts_h, torch.int32, "verts_h")
    if verts_h.dim() != 2 or verts_h.shape[1] != 3:
        raise ValueError("lattice_hull: verts_h must be (n,3)")
    off_h = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64).reshape(-1)
    n, L = verts_h.shape[0], len(off_h) - 1
    if L < 1 or not _host_offsets_ok(off_h, n):
        raise ValueError("lattice_hull: offsets must be (L+1), L >= 1, non-decreasing from 0 to len(verts_h)")
    if (origin is None) != (voxel_size is None):
        raise ValueError("lattice_hull: origin and voxel_size go together")
    dev = verts_h.device
    max_abs = int(verts_h.abs().max().item()) if n else 0
    if max_abs > HULL_MAX_COORD:
        raise ValueError(f"lattice_hull: a coordinate of magnitude {max_abs} is beyond the limit of {HULL_MAX_COORD}")
    if origin is not None:
        origin = torch.as_tensor(origin, dtype=torch.float64).to(dev).contiguous()
        voxel_size = float(voxel_size)
        if tuple(origin.shape) != (L, 3):
            raise ValueError("lattice_hull: origin must be (L,3)")
        if not (voxel_size > 0 and np.isfinite(voxel_size)):
            raise ValueError(f"lattice_hull: voxel_size must be positive and finite, got {voxel_size}")
    st = _stream()
    off = torch.from_numpy(off_h).to(dev)
    ws_bytes = int(L_.creg_lattice_hull_workspace_bytes(n, L))
    ws = _workspace(dev, ws_bytes)
    status = torch.empty(L, dtype=torch.int32, device=dev)
    count = torch.empty(L, dtype=torch.int32, device=dev)
    _check_mesh(L_.creg_lattice_hull_i32(_p(verts_h) if n else None, n, _p(off), off_h.ctypes.data, L, max_abs, _p(status), _p(count),
                                         _p(ws), ws_bytes, st), "creg_lattice_hull_i32")
    status_h, count_h = status.cpu().numpy(), count.cpu().numpy()    # the one wait: the face counts size the triangles
    if strict and status_h.any():
        l = int(np.nonzero(status_h)[0][0])
        raise ValueError(f"lattice_hull: link {l} ({off_h[l + 1] - off_h[l]} points) has no hull: "
                         f"{HULL_STATUS.get(int(status_h[l]), 'status %d' % status_h[l])}")
    toff_h = np.concatenate([[0], np.cumsum(count_h.astype(np.int64))]).astype(np.int64)
    F = int(toff_h[-1])
    toff = torch.from_numpy(toff_h).to(dev)
    tris = torch.empty(F, 3, dtype=torch.int32, device=dev)
    rec = torch.empty(F, 4, 3, dtype=torch.float32, device=dev) if origin is not None else None
    _check_mesh(L_.creg_lattice_hull_emit_i32(_p(verts_h) if n else None, n, _p(off), L, _p(toff), F, _p(origin),
                                              voxel_size if origin is not None else 0.0, _p(tris) if F else None,
                                              _p(rec) if (rec is not None and F) else None, _p(ws), ws_bytes, st),
                "creg_lattice_hull_emit_i32")
    out = []
    for l in range(L):
        t = tris[toff_h[l]:toff_h[l + 1]]
        d = dict(triangles=t, vertex_ids=torch.unique(t.reshape(-1).to(torch.int64)), status=int(status_h[l]))
        if rec is not None:
            d["stl_records"] = rec[toff_h[l]:toff_h[l + 1]]
        out.append(d)
    return out
