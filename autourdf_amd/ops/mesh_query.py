"""Queries on a posed URDF: forward kinematics, mesh pair queries (collide, clearance, contain), point-to-mesh distance,
the pose-fit system, link moments and mass properties."""
import numpy as np

import torch

from .. import _lib
from ._common import _device_offsets_ok, _need, _p, _shapes_expected, _stream, _table_on, _workspace
from ._common import joint_chains  # noqa: F401  -- defined beside _table_on, its one user in the package; public from here

MESH_CONTAIN_MAX_POINTS = 16
POSE_FIT_MAX_D = 64
MESH_INERTIA_KEYS = ("sums", "volume", "area", "closure", "mass", "com", "inertia", "principal", "axes")


def urdf_fk(table, q, base, want_lines: bool = False, origin=None):
    """Batched forward kinematics (creg_urdf_fk_f64): ``table`` from ``UrdfRobot.fk_table()``, q (P,J) joint values in the
    table's order and base (4,4), host arrays or f64 device tensors -> link_T (P,L,4,4) f64 on the device, and
    joint_lines (P,J,6) = world position of the joint frame | unit world axis when ``want_lines``.  One launch for all P.
    ``origin`` (J,4,4) f64 on the device stands in for the table's origins in this call alone; the table's upload is not touched."""
    L = _lib.load()
    dev = _lib.device(q, base)
    parent, child, kind, table_origin, axis = _table_on(dev, table)
    q = _need(torch.as_tensor(q, dtype=torch.float64, device=dev), torch.float64, "q")
    base = _need(torch.as_tensor(base, dtype=torch.float64, device=dev), torch.float64, "base")
    J, n_links = parent.shape[0], int(table["n_links"])
    if q.dim() != 2 or q.shape[1] != J or tuple(base.shape) != (4, 4):
        raise ValueError(f"urdf_fk: q must be (P,{J}) and base (4,4), got {tuple(q.shape)} and {tuple(base.shape)}")
    if origin is None:
        origin = table_origin
    else:
        origin = _need(origin, torch.float64, "origin")
        if tuple(origin.shape) != (J, 4, 4) or origin.device != dev:
            raise ValueError(f"urdf_fk: origin must be ({J},4,4) on {dev}, got {tuple(origin.shape)} on {origin.device}")
    P = q.shape[0]
    link_T = torch.empty(P, n_links, 4, 4, dtype=torch.float64, device=dev)
    lines = torch.empty(P, J, 6, dtype=torch.float64, device=dev) if want_lines else None
    _lib.check(L.creg_urdf_fk_f64(_p(parent), _p(child), _p(kind), _p(origin), _p(axis), J, n_links, int(table["root"]), _p(q), P,
                                  _p(base), _p(link_T), _p(lines), _stream()), "creg_urdf_fk_f64")
    return (link_T, lines) if want_lines else link_T


def _mesh_args(tri, tri_start, link_T):
    """tri, tri_start and link_T as every mesh query takes them -> ([(name, expected shape, tensor)] with link_T (L,4,4) lifted to
    (1,L,4,4), whether the three shapes fit)."""
    tri, link_T, tri_start = _need(tri, torch.float64, "tri"), _need(link_T, torch.float64, "link_T"), _need(tri_start, torch.int64, "tri_start")
    if link_T.dim() == 3:
        link_T = link_T[None]
    ok = tri.dim() == 3 and tuple(tri.shape[1:]) == (3, 3) and link_T.dim() == 4 and tuple(link_T.shape[2:]) == (4, 4) \
        and link_T.shape[0] >= 1 and tri_start.dim() == 1 and tri_start.shape[0] == link_T.shape[1] + 1
    return [("tri", "(F,3,3)", tri), ("tri_start", "(L+1)", tri_start), ("link_T", "(P,L,4,4)", link_T)], ok


def _mesh_pair_args(who, tri, tri_start, link_T, pairs):
    """The argument checks ``mesh_collide`` and ``mesh_clearance`` share -> (tri, tri_start, link_T (P,L,4,4), pairs, F, P, L, M)."""
    arrays, ok = _mesh_args(tri, tri_start, link_T)
    arrays.append(("pairs", "(M,2)", _need(pairs, torch.int32, "pairs")))
    tri, tri_start, link_T, pairs = (t for _, _, t in arrays)
    if not (ok and pairs.dim() == 2 and pairs.shape[1] == 2):
        raise _shapes_expected(who, arrays)
    F, (P, n_links), M = tri.shape[0], link_T.shape[:2], pairs.shape[0]
    if n_links < 1:
        raise ValueError(f"{who}: at least one link")
    ok = _device_offsets_ok(tri_start, F)
    if M:
        ok = ok & (pairs >= 0).all() & (pairs < n_links).all() & (pairs[:, 0] != pairs[:, 1]).all()
    if not bool(ok):
        raise ValueError(f"{who}: tri_start must run from 0 to {F} without decreasing, and every pair must name two "
                         f"different links in [0, {n_links})")
    return tri, tri_start, link_T, pairs, F, P, n_links, M


def _mesh_pair_call(L, entry, tri, tri_start, link_T, pairs, outs, want_boxes, points=(), params=(), size_params=()):
    """The tail the mesh pair queries share: the optional link_box, the workspace ``creg_mesh_<entry>_workspace_bytes`` asks for,
    null pointers for an empty ``tri`` or ``pairs`` (then for the outputs too) and the call -> link_box or None.  ``points`` go
    between F and link_T, ``params`` between M and the outputs, ``size_params`` after M in the workspace call."""
    F, (P, n_links), M, dev = tri.shape[0], link_T.shape[:2], pairs.shape[0], tri.device
    boxes = torch.empty(P, n_links, 6, dtype=torch.float64, device=dev) if want_boxes else None
    ws_bytes = getattr(L, f"creg_mesh_{entry}_workspace_bytes")(F, n_links, P, M, *size_params)
    ws = _workspace(dev, ws_bytes)
    name = f"creg_mesh_{entry}_f64"
    _lib.check(getattr(L, name)(_p(tri) if F else None, _p(tri_start), F, *points, _p(link_T), n_links, P, _p(pairs) if M else None, M,
                                *params, *(_p(o) if M else None for o in outs), _p(boxes), _p(ws), ws_bytes, _stream()), name)
    return boxes


def mesh_collide(tri, tri_start, link_T, pairs, want_boxes: bool = False):
    """Self-collision of posed link meshes (creg_mesh_collide_f64; the contract is in include/creg.h): tri (F,3,3) f64
    link-frame triangles, tri_start (L+1) int64 (link l owns rows tri_start[l]:tri_start[l+1]), link_T (P,L,4,4) f64 -- or
    (L,4,4) for P = 1 -- and pairs (M,2) int32 link indices, all on the device -> count (P,M) int32 colliding triangle pairs,
    first (P,M,2) int32 the smallest colliding (a, b) as rows of tri or (-1,-1), and link_box (P,L,6) f64 = min xyz | max xyz of
    every posed link when ``want_boxes``.  One call for all P and M.  Raises for a pair outside [0, L) or naming one link twice
    and for a tri_start that does not run 0 .. F without decreasing (both are read back: the one synchronisation)."""
    L = _lib.load()
    tri, tri_start, link_T, pairs, F, P, n_links, M = _mesh_pair_args("mesh_collide", tri, tri_start, link_T, pairs)
    count = torch.empty(P, M, dtype=torch.int32, device=tri.device)
    first = torch.empty(P, M, 2, dtype=torch.int32, device=tri.device)
    boxes = _mesh_pair_call(L, "collide", tri, tri_start, link_T, pairs, (count, first), want_boxes)
    return (count, first, boxes) if want_boxes else (count, first)


def mesh_clearance(tri, tri_start, link_T, pairs, d_max, want_boxes: bool = False):
    """Clearance of posed link meshes (creg_mesh_clearance_f64; the contract is in include/creg.h): the inputs of
    ``mesh_collide`` and a margin ``d_max`` >= 0 (``inf`` allowed) -> dist (P,M) f64, the minimum distance between the two
    meshes of every link pair at every pose -- 0.0 where they collide by ``mesh_collide``'s predicate, ``+inf`` where they
    are farther apart than ``d_max`` (no triangle pair within the margin by the box test, or a found minimum above it) --,
    witness (P,M,2) int32 the triangle pair (rows of tri) that attains the kernel's minimum, (-1,-1) where no triangle pair
    was within the margin by the box test, and link_box (P,L,6) when ``want_boxes``.  One call for all P and M; the argument
    checks are ``mesh_collide``'s, plus a ValueError for a negative or NaN ``d_max``."""
    L = _lib.load()
    d_max = float(d_max)
    if not d_max >= 0.0:
        raise ValueError(f"mesh_clearance: d_max must be >= 0 (inf allowed), got {d_max}")
    tri, tri_start, link_T, pairs, F, P, n_links, M = _mesh_pair_args("mesh_clearance", tri, tri_start, link_T, pairs)
    dist2 = torch.empty(P, M, dtype=torch.float64, device=tri.device)
    witness = torch.empty(P, M, 2, dtype=torch.int32, device=tri.device)
    boxes = _mesh_pair_call(L, "clearance", tri, tri_start, link_T, pairs, (dist2, witness), want_boxes, params=(d_max,))
    dist = torch.where(dist2 > d_max * d_max, torch.full_like(dist2, float("inf")), torch.sqrt(dist2))
    return (dist, witness, boxes) if want_boxes else (dist, witness)


def mesh_contain(tri, tri_start, pts, pt_start, link_T, pairs, want_winding: bool = False, want_boxes: bool = False):
    """Is a link wholly inside another (creg_mesh_contain_f64; the contract is in include/creg.h): the inputs of
    ``mesh_collide`` plus pts (N,3) f64 query points in link frames and pt_start (L+1) int64 (link l owns rows
    pt_start[l]:pt_start[l+1], at most 16 of them; ``UrdfRobot.containment_points``), all on the device -> inside (P,M,2) int32,
    the number of points of link pairs[m][d] whose generalized winding number in the posed mesh of link pairs[m][1-d] exceeds
    0.5 in magnitude, first (P,M,2) int32 the smallest such row of pts or -1, then winding (P,M,2,Q) f64 when ``want_winding``
    (Q the largest point count of a link, at least 1; 0.0 for a point outside the other link's box and for unused slots) and
    link_box (P,L,6) when ``want_boxes``.  One call for all P, M and both directions; the argument checks are
    ``mesh_collide``'s, plus a ValueError for a pt_start that does not run 0 .. N without decreasing or gives a link more than
    16 points."""
    L = _lib.load()
    tri, tri_start, link_T, pairs, F, P, n_links, M = _mesh_pair_args("mesh_contain", tri, tri_start, link_T, pairs)
    pts, pt_start = _need(pts, torch.float64, "pts"), _need(pt_start, torch.int64, "pt_start")
    if pts.dim() != 2 or pts.shape[1] != 3 or pt_start.dim() != 1 or pt_start.shape[0] != n_links + 1:
        raise ValueError(f"mesh_contain: pts (N,3) / pt_start (L+1) expected, got {tuple(pts.shape)}, {tuple(pt_start.shape)}")
    N = pts.shape[0]
    ok, hi = (int(v) for v in torch.stack([_device_offsets_ok(pt_start, N), (pt_start[1:] - pt_start[:-1]).max()]).cpu())
    if not ok or hi > MESH_CONTAIN_MAX_POINTS:
        raise ValueError(f"mesh_contain: pt_start must run from 0 to {N} without decreasing and give a link at most "
                         f"{MESH_CONTAIN_MAX_POINTS} points")
    Q = max(hi, 1)
    dev = tri.device
    inside = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    first = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    winding = torch.empty(P, M, 2, Q, dtype=torch.float64, device=dev) if want_winding else None
    boxes = _mesh_pair_call(L, "contain", tri, tri_start, link_T, pairs, (inside, first, winding), want_boxes,
                            points=(_p(pts) if N else None, _p(pt_start), N), params=(Q,), size_params=(Q,))
    return (inside, first) + ((winding,) if want_winding else ()) + ((boxes,) if want_boxes else ())


def _morton_order(pts, pt_start, P):
    """A permutation of pts' rows that keeps every pose's rows where they are as a set and orders them by a 30-bit Morton key,
    10 bits per axis over the pose's own bounding box (NaN and infinite coordinates count as 0: any order is a valid one)."""
    N, dev = pts.shape[0], pts.device
    pose = torch.repeat_interleave(torch.arange(P, device=dev), pt_start[1:] - pt_start[:-1], output_size=N)
    x = torch.nan_to_num(pts, nan=0.0, posinf=0.0, neginf=0.0)
    at = pose[:, None].expand(N, 3)
    lo = torch.full((P, 3), float("inf"), dtype=pts.dtype, device=dev).scatter_reduce(0, at, x, "amin")
    hi = torch.full((P, 3), float("-inf"), dtype=pts.dtype, device=dev).scatter_reduce(0, at, x, "amax")
    ext = (hi - lo)[pose]
    cell = ((x - lo[pose]) * torch.where(ext > 0, 1023.0 / ext, torch.zeros_like(ext))).clamp_(0, 1023).to(torch.int64)
    for shift, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):      # spread 10 bits to every third
        cell = (cell | (cell << shift)) & mask
    key = (pose << 30) | (cell[:, 0] << 2) | (cell[:, 1] << 1) | cell[:, 2]
    return torch.argsort(key)


def _point_query_args(who, tri, tri_start, link_T, pts, pt_start, d_max, more=()):
    """The argument checks the three point queries share: ``d_max`` >= 0, dtypes, contiguity and shapes of the mesh, of pts (N,3)
    and pt_start (P+1), and of ``more`` = ((name, tensor, dtype, expected shape in N, P, L), ...) -> (d_max, tri, tri_start, link_T
    (P,L,4,4), pts, pt_start, *more's tensors, F, P, L, N, device).  Nothing is read back."""
    d_max = float(d_max)
    if not d_max >= 0.0:
        raise ValueError(f"{who}: d_max must be >= 0 (inf allowed), got {d_max}")
    arrays, ok = _mesh_args(tri, tri_start, link_T)
    arrays += [("pts", "(N,3)", _need(pts, torch.float64, "pts")), ("pt_start", "(P+1)", _need(pt_start, torch.int64, "pt_start"))]
    arrays += [(name, want, _need(t, dtype, name)) for name, t, dtype, want in more]
    tri, tri_start, link_T, pts, pt_start = (t for _, _, t in arrays[:5])
    ok = ok and link_T.shape[1] >= 1 and pts.dim() == 2 and pts.shape[1] == 3 and pt_start.dim() == 1 and pt_start.shape[0] == link_T.shape[0] + 1
    if ok:
        size = {"N": pts.shape[0], "P": link_T.shape[0], "L": link_T.shape[1], "3": 3}
        ok = all(tuple(t.shape) == tuple(size[d] for d in want[1:-1].split(",")) for _, want, t in arrays[5:])
    if not ok:
        raise _shapes_expected(who, arrays)
    return (d_max,) + tuple(t for _, _, t in arrays) + (tri.shape[0], link_T.shape[0], link_T.shape[1], pts.shape[0], tri.device)


def point_mesh_distance(tri, tri_start, link_T, pts, pt_start, d_max=float("inf"), sort: bool = True, want_boxes: bool = False):
    """Distance from world points to posed link meshes (creg_point_mesh_f64; the contract is in include/creg.h): tri (F,3,3) f64
    link-frame triangles, tri_start (L+1) int64, link_T (P,L,4,4) f64 -- or (L,4,4) for P = 1 --, pts (N,3) f64 world points and
    pt_start (P+1) int64 (pose p owns rows pt_start[p]:pt_start[p+1]), all on the device, and ``d_max`` >= 0 (``inf`` allowed)
    -> dist (N) f64, the distance from every point to its pose's mesh, ``+inf`` where it exceeds ``d_max`` (no triangle within
    ``d_max`` by the box test, or a found minimum above it; also for a NaN point), tri_idx (N) int32 the row of tri that attains
    the kernel's minimum or -1 where no triangle was within ``d_max`` by the box test, link (N) int32 the link that owns that row
    or -1, and link_box (P,L,6) when ``want_boxes``.  One call for all poses.
    ``sort=True`` hands the kernel every pose's points in Morton order (10 bits per axis over the pose's own bounding box) and
    scatters the results back, so that a tile of 64 points is compact and the kernel's box culls bite; a point's result does
    not depend on the order, so no bit of any output changes.
    ValueError before any launch: a bad shape or dtype, a tri_start that does not run 0 .. F or a pt_start that does not run
    0 .. N without decreasing (both are read back: the one synchronisation), a negative or NaN ``d_max``."""
    L = _lib.load()
    d_max, tri, tri_start, link_T, pts, pt_start, F, P, n_links, N, dev = _point_query_args(
        "point_mesh_distance", tri, tri_start, link_T, pts, pt_start, d_max)
    if not bool(_device_offsets_ok(tri_start, F) & _device_offsets_ok(pt_start, N)):
        raise ValueError(f"point_mesh_distance: tri_start must run from 0 to {F} and pt_start from 0 to {N} without decreasing")
    order = _morton_order(pts, pt_start, P) if sort and N else None
    dist2 = torch.empty(N, dtype=torch.float64, device=dev)
    tri_idx = torch.empty(N, dtype=torch.int32, device=dev)
    boxes = torch.empty(P, n_links, 6, dtype=torch.float64, device=dev) if want_boxes else None
    ws_bytes = L.creg_point_mesh_workspace_bytes(F, n_links, P, N)
    ws = _workspace(dev, ws_bytes)
    sent = pts if order is None else pts[order].contiguous()
    _lib.check(L.creg_point_mesh_f64(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(sent) if N else None,
                                     _p(pt_start), N, d_max, _p(dist2) if N else None, _p(tri_idx) if N else None, _p(boxes), _p(ws),
                                     ws_bytes, _stream()), "creg_point_mesh_f64")
    if order is not None:
        dist2, tri_idx = torch.empty_like(dist2).index_copy_(0, order, dist2), torch.empty_like(tri_idx).index_copy_(0, order, tri_idx)
    dist = torch.where(dist2 > d_max * d_max, torch.full_like(dist2, float("inf")), torch.sqrt(dist2))
    owner = (torch.searchsorted(tri_start, tri_idx.to(torch.int64), right=True) - 1).to(torch.int32)
    link = torch.where(tri_idx >= 0, owner, torch.full_like(owner, -1))
    return (dist, tri_idx, link) + ((boxes,) if want_boxes else ())


def mesh_cover(tri, tri_start, link_T, pts, pt_start, d_max=float("inf"), sort: bool = True, want_boxes: bool = False):
    """The other direction of ``point_mesh_distance`` (creg_mesh_cover_f64; the contract is in include/creg.h): the same inputs
    -> dist (P,F) f64, the distance from every posed triangle to its pose's points, ``+inf`` where it exceeds ``d_max`` (no
    point within ``d_max`` by the box test, or a found minimum above it: surface no point lies near), pt_idx (P,F) int32 the
    row of pts that attains the kernel's minimum (the smallest on equal bits) or -1 where no point was within ``d_max`` by the
    box test, n_near (P,F) int32 the number of the pose's points within ``d_max`` of the triangle, and link_box (P,L,6) when
    ``want_boxes``.  One call for all poses.
    ``sort=True`` hands the kernel every pose's points in Morton order with their own rows as labels, so that a tile of 64
    points is compact and the kernel's box cull bites; the outputs are a function of the set of (point, row) pairs, so no bit
    of any output changes.
    ValueError before any launch: ``point_mesh_distance``'s."""
    L = _lib.load()
    d_max, tri, tri_start, link_T, pts, pt_start, F, P, n_links, N, dev = _point_query_args(
        "mesh_cover", tri, tri_start, link_T, pts, pt_start, d_max)
    if not bool(_device_offsets_ok(tri_start, F) & _device_offsets_ok(pt_start, N)):
        raise ValueError(f"mesh_cover: tri_start must run from 0 to {F} and pt_start from 0 to {N} without decreasing")
    order = _morton_order(pts, pt_start, P) if sort and N else None
    dist2 = torch.empty(P, F, dtype=torch.float64, device=dev)
    pt_idx = torch.empty(P, F, dtype=torch.int32, device=dev)
    n_near = torch.empty(P, F, dtype=torch.int32, device=dev)
    boxes = torch.empty(P, n_links, 6, dtype=torch.float64, device=dev) if want_boxes else None
    ws_bytes = L.creg_mesh_cover_workspace_bytes(F, n_links, P, N)
    ws = _workspace(dev, ws_bytes)
    sent = pts if order is None else pts[order].contiguous()
    rows = None if order is None else order.to(torch.int32)
    _lib.check(L.creg_mesh_cover_f64(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(sent) if N else None,
                                     _p(pt_start), _p(rows), N, d_max, _p(dist2) if F else None, _p(pt_idx) if F else None,
                                     _p(n_near) if F else None, _p(boxes), _p(ws), ws_bytes, _stream()), "creg_mesh_cover_f64")
    dist = torch.where(dist2 > d_max * d_max, torch.full_like(dist2, float("inf")), torch.sqrt(dist2))
    return (dist, pt_idx, n_near) + ((boxes,) if want_boxes else ())


def pose_fit_system(tri, tri_start, link_T, pts, pt_start, tri_idx, table, center, d_max=float("inf")):
    """The Gauss-Newton system of fitting a robot's base pose and joint values to clouds (creg_pose_fit_system_f64; the contract
    is in include/creg.h): tri, tri_start, link_T, pts, pt_start and ``d_max`` as ``point_mesh_distance`` takes them, tri_idx (N)
    int32 the rows it returned (in the order of ``pts``: its ``sort=True`` results are already scattered back), ``table`` from
    ``UrdfRobot.fk_table()`` and center (P,3) f64 the point each pose's base rotation turns about -> (H (P,D,D), g (P,D),
    cost (P), n (P) int64) on the device, D = 6 + J: rotation about ``center``, translation, then the table's joints.  One call
    for all poses.  The table and its chain masks go up once per robot and device and are kept in the dict (``_dev_fit``, as
    ``urdf_fk`` keeps ``_dev``): change a copy of a table without those keys.  tri_start and pt_start are not read back; the
    kernel clamps them.  ValueError before any launch: a bad shape or dtype, a negative or NaN ``d_max``, D > 64."""
    L = _lib.load()
    d_max, tri, tri_start, link_T, pts, pt_start, tri_idx, center, F, P, n_links, N, dev = _point_query_args(
        "pose_fit_system", tri, tri_start, link_T, pts, pt_start, d_max,
        (("tri_idx", tri_idx, torch.int32, "(N)"), ("center", center, torch.float64, "(P,3)")))
    J = len(table["parent"])
    if n_links != int(table["n_links"]) or 6 + J > POSE_FIT_MAX_D:
        raise ValueError(f"pose_fit_system: the table has {table['n_links']} links and {J} joints; link_T has {n_links} links and "
                         f"6 + joints must be <= {POSE_FIT_MAX_D}")
    parent, child, kind, origin, axis, chain = _table_on(dev, table, chains=True)
    D = 6 + J
    H = torch.empty(P, D, D, dtype=torch.float64, device=dev)
    g = torch.empty(P, D, dtype=torch.float64, device=dev)
    cost = torch.empty(P, dtype=torch.float64, device=dev)
    n = torch.empty(P, dtype=torch.int64, device=dev)
    ws_bytes = L.creg_pose_fit_workspace_bytes(P, N, J)
    ws = _workspace(dev, ws_bytes)
    tab = lambda t: _p(t) if J else None
    _lib.check(L.creg_pose_fit_system_f64(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(pts) if N else None,
                                          _p(pt_start), N, d_max, _p(tri_idx) if N else None, tab(parent), tab(child), tab(kind),
                                          tab(origin), tab(axis), J, _p(chain), _p(center), _p(H), _p(g), _p(cost), _p(n), _p(ws),
                                          ws_bytes, _stream()), "creg_pose_fit_system_f64")
    return H, g, cost, n


def link_moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max=float("inf"), metric="point"):
    """The 16 moment sums per (pose, link) of the correspondences (creg_link_moments_f64; the contract is in include/creg.h): tri,
    tri_start, link_T, pts, pt_start, tri_idx and ``d_max`` as ``pose_fit_system`` takes them, ref (P,L,3) f64 the point the
    moments of every (pose, link) are taken about -> (mom (P,L,16) f64, cnt (P,L) int64) on the device: per (pose, link) the sums
    of d d^T (6: xx xy xz yy yz zz), d (3), d x r (3), r (3) and r.r over its contributing points, d = c - ref, and their number.
    One call for all poses; no joint table and no limit on a parameter count (``compute_joints.twist_system`` turns the moments
    into a normal system).  With ``metric="feature"`` one call of creg_feature_moments_f64 instead -> (mom, cnt, fmom): the same
    mom and cnt, bit for bit, and fmom (P,L,21) f64, the upper triangle (row-major, a <= b) of the 6 x 6 curvature sum A^T Pi A of
    the matched features between the twists (Omega, V), Pi the projector onto the normal space of the vertex, edge or face the
    point matched (``twist_system(..., fmom=fmom)``).  tri_start and pt_start are not read back; the kernel clamps them.
    ValueError before any launch: a bad shape or dtype, a negative or NaN ``d_max``, a ``metric`` other than "point" or "feature"."""
    if metric not in ("point", "feature"):
        raise ValueError(f"link_moments: metric must be 'point' or 'feature', got {metric!r}")
    L = _lib.load()
    d_max, tri, tri_start, link_T, pts, pt_start, tri_idx, ref, F, P, n_links, N, dev = _point_query_args(
        "link_moments", tri, tri_start, link_T, pts, pt_start, d_max,
        (("tri_idx", tri_idx, torch.int32, "(N)"), ("ref", ref, torch.float64, "(P,L,3)")))
    mom = torch.empty(P, n_links, 16, dtype=torch.float64, device=dev)
    cnt = torch.empty(P, n_links, dtype=torch.int64, device=dev)
    outs = (mom, cnt) + ((torch.empty(P, n_links, 21, dtype=torch.float64, device=dev),) if metric == "feature" else ())
    name = "creg_feature_moments" if metric == "feature" else "creg_link_moments"
    ws_bytes = getattr(L, name + "_workspace_bytes")(P, N, n_links)
    ws = _workspace(dev, ws_bytes)
    _lib.check(getattr(L, name + "_f64")(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(pts) if N else None,
                                         _p(pt_start), N, d_max, _p(tri_idx) if N else None, _p(ref), *(_p(o) for o in outs), _p(ws),
                                         ws_bytes, _stream()), name + "_f64")
    return outs


def mesh_inertia(tri, tri_start, density=1.0):
    """Mass properties of closed link meshes (creg_mesh_inertia_f64; the contract is in include/creg.h): tri (F,3,3) f64 and
    tri_start (L+1) int64 on the device, as ``mesh_collide`` takes them, density a scalar or (L) -> a dict of device tensors:
    sums (L,14), volume, area, closure, mass (L), com (L,3), inertia (L,6) = ixx ixy ixz iyy iyz izz about com, principal (L,3)
    ascending and axes (L,3,3).  One set of launches for all L; nothing is read back, so only shapes and dtypes raise (the
    kernel clamps tri_start into 0 .. F)."""
    L = _lib.load()
    tri, tri_start = _need(tri, torch.float64, "tri"), _need(tri_start, torch.int64, "tri_start")
    if tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3) or tri_start.dim() != 1 or tri_start.shape[0] < 2:
        raise ValueError(f"mesh_inertia: tri (F,3,3) / tri_start (L+1) with L >= 1 expected, got {tuple(tri.shape)}, "
                         f"{tuple(tri_start.shape)}")
    F, n_links, dev = tri.shape[0], tri_start.shape[0] - 1, tri.device
    if isinstance(density, torch.Tensor):
        density = _need(density, torch.float64, "density")
        if density.dim() == 0:
            density = density.expand(n_links).contiguous()
    else:
        density = torch.as_tensor(np.full(n_links, float(density)) if np.ndim(density) == 0
                                  else np.ascontiguousarray(density, np.float64), device=dev)
    if tuple(density.shape) != (n_links,):
        raise ValueError(f"mesh_inertia: density must be a scalar or ({n_links}), got {tuple(density.shape)}")
    shapes = dict(sums=(14,), volume=(), area=(), closure=(), mass=(), com=(3,), inertia=(6,), principal=(3,), axes=(3, 3))
    out = {k: torch.empty((n_links,) + shapes[k], dtype=torch.float64, device=dev) for k in MESH_INERTIA_KEYS}
    ws_bytes = L.creg_mesh_inertia_workspace_bytes(F, n_links)
    ws = _workspace(dev, ws_bytes)
    _lib.check(L.creg_mesh_inertia_f64(_p(tri) if F else None, _p(tri_start), F, n_links, _p(density), *[_p(out[k]) for k in MESH_INERTIA_KEYS],
                                       _p(ws), ws_bytes, _stream()), "creg_mesh_inertia_f64")
    return out
