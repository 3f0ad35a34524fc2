"""N4 simulator: mesh surface sampling, camera-ring visibility, depth rasters, back-projection and RANSAC planes."""
import numpy as np

import torch

from .. import _lib
from ._common import _need, _p, _stream, _workspace


def _mesh_shapes(who, tri, tri_link, link_T, cum_area=None, cams=None, rows=None, rows_name="", width=1, height=1):
    """The kernels index these arrays by the sizes of OTHER arrays (tri_link[f] for f < F, cams + 12 c, rows + 3 i): a shape that
    disagrees is read out of bounds, so it is refused here, before any launch."""
    F = tri.shape[0]
    if tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3) or F < 1:
        raise ValueError(f"{who}: tri (F,3,3) with F >= 1 expected, got {tuple(tri.shape)}")
    if tuple(tri_link.shape) != (F,):
        raise ValueError(f"{who}: tri_link ({F}) expected, got {tuple(tri_link.shape)}")
    if cum_area is not None and tuple(cum_area.shape) != (F,):
        raise ValueError(f"{who}: cum_area ({F}) expected, got {tuple(cum_area.shape)}")
    if link_T.dim() != 3 or tuple(link_T.shape[1:]) != (4, 4) or link_T.shape[0] < 1:
        raise ValueError(f"{who}: link_T (L,4,4) with L >= 1 expected, got {tuple(link_T.shape)}")
    if cams is not None and (cams.dim() != 2 or cams.shape[1] != 12 or cams.shape[0] < 1):
        raise ValueError(f"{who}: cams (C,12) with C >= 1 expected, got {tuple(cams.shape)}")
    if rows is not None and (rows.dim() != 2 or rows.shape[1] != 3 or rows.shape[0] < 1):
        raise ValueError(f"{who}: {rows_name} (n,3) with n >= 1 expected, got {tuple(rows.shape)}")
    if int(width) < 1 or int(height) < 1:
        raise ValueError(f"{who}: width and height >= 1 expected, got {width} x {height}")


def sample_mesh(tri, cum_area, tri_link, link_T, u, with_links: bool = False):
    """Area-weighted points on an articulated triangle mesh (creg_sample_mesh_f64): tri (F,3,3) f64 in link
    frames, cum_area (F) f64, tri_link (F) i32, link_T (L,4,4) f64, u (n,3) f64 uniforms -> (n,3) f64 world points
    (and the link index of every point when with_links)."""
    L = _lib.load()
    tri, cum_area, link_T, u = (_need(t, torch.float64, nm) for t, nm in ((tri, "tri"), (cum_area, "cum_area"), (link_T, "link_T"), (u, "u")))
    tri_link = _need(tri_link, torch.int32, "tri_link")
    _mesh_shapes("sample_mesh", tri, tri_link, link_T, cum_area=cum_area, rows=u, rows_name="u")
    n, F = u.shape[0], tri.shape[0]
    out = torch.empty(n, 3, dtype=torch.float64, device=u.device)
    links = torch.empty(n, dtype=torch.int32, device=u.device) if with_links else None
    _lib.check(L.creg_sample_mesh_f64(_p(tri), _p(cum_area), _p(tri_link), F, _p(link_T), link_T.shape[0], _p(u), n, _p(out),
                                      _p(links) if with_links else None, _stream()), "creg_sample_mesh_f64")
    return (out, links) if with_links else out


def visibility(tri, tri_link, link_T, cams, pts, fov_deg=60.0, aspect=1.0, near=0.1, far=4.0, width=800, height=800,
               eps=0.004, return_depth=False):
    """Camera-ring visibility (creg_visibility_f64): tri (F,3,3) f64 link-frame triangles, tri_link (F) i32, link_T (L,4,4)
    f64, cams (C,12) f64 = eye | forward | right | up, pts (n,3) f64 world points -> (n) bool tensor (and the (C,H,W) f64
    depth buffers when return_depth)."""
    L = _lib.load()
    tri, link_T, cams, pts = (_need(t, torch.float64, nm) for t, nm in ((tri, "tri"), (link_T, "link_T"), (cams, "cams"), (pts, "pts")))
    tri_link = _need(tri_link, torch.int32, "tri_link")
    _mesh_shapes("visibility", tri, tri_link, link_T, cams=cams, rows=pts, rows_name="pts", width=width, height=height)
    C, n = cams.shape[0], pts.shape[0]
    ws_bytes = L.creg_visibility_workspace_bytes(C, int(width), int(height))
    ws = _workspace(pts.device, ws_bytes)                          # 8 C H W bytes: the depth buffers, returned below as f64
    vis = torch.empty(n, dtype=torch.uint8, device=pts.device)
    _lib.check(L.creg_visibility_f64(_p(tri), _p(tri_link), tri.shape[0], _p(link_T), link_T.shape[0], _p(cams), C, float(fov_deg),
                                     float(aspect), float(near), float(far), int(width), int(height), _p(pts), n, float(eps), _p(vis),
                                     _p(ws), ws_bytes, _stream()), "creg_visibility_f64")
    return (vis.bool(), ws.view(torch.float64).reshape(C, height, width)) if return_depth else vis.bool()


def raster_depth(tri, tri_link, link_T, cams, fov_deg=60.0, aspect=1.0, near=0.1, far=4.0, width=800, height=800):
    """The depth buffers of ``visibility`` alone (creg_raster_depth_f64, the same kernels): (C,H,W) f64, +inf where nothing was drawn."""
    L = _lib.load()
    tri, link_T, cams = (_need(t, torch.float64, nm) for t, nm in ((tri, "tri"), (link_T, "link_T"), (cams, "cams")))
    tri_link = _need(tri_link, torch.int32, "tri_link")
    _mesh_shapes("raster_depth", tri, tri_link, link_T, cams=cams, width=width, height=height)
    C = cams.shape[0]
    depth = torch.empty(C, int(height), int(width), dtype=torch.float64, device=tri.device)
    _lib.check(L.creg_raster_depth_f64(_p(tri), _p(tri_link), tri.shape[0], _p(link_T), link_T.shape[0], _p(cams), C, float(fov_deg),
                                       float(aspect), float(near), float(far), int(width), int(height), _p(depth), _stream()),
               "creg_raster_depth_f64")
    return depth


def depth_points(depth, cams, fov_deg=60.0, aspect=1.0):
    """Back-project every finite pixel of depth (C,H,W) f64 through cams (C,12) f64 (creg_depth_points_*): points (M,3) f64 in
    camera-major, then row-major pixel order and offsets (C+1) int64 on the device -- camera c owns rows offsets[c]:offsets[c+1].
    M is read back from the device between the two launches (the one synchronisation)."""
    L = _lib.load()
    depth, cams = _need(depth, torch.float64, "depth"), _need(cams, torch.float64, "cams")
    if depth.dim() != 3 or cams.dim() != 2 or cams.shape[1] != 12 or cams.shape[0] != depth.shape[0] or depth.numel() == 0:
        raise ValueError(f"depth_points: depth (C,H,W) and cams (C,12) expected, got {tuple(depth.shape)} and {tuple(cams.shape)}")
    C, H, W = depth.shape
    ws_bytes = L.creg_depth_points_workspace_bytes(C, W, H)
    ws = _workspace(depth.device, ws_bytes)
    offsets = torch.empty(C + 1, dtype=torch.int64, device=depth.device)
    _lib.check(L.creg_depth_points_count_f64(_p(depth), C, W, H, _p(offsets), _p(ws), ws_bytes, _stream()), "creg_depth_points_count_f64")
    M = int(offsets[C].item())
    points = torch.empty(M, 3, dtype=torch.float64, device=depth.device)
    _lib.check(L.creg_depth_points_f64(_p(depth), _p(cams), C, float(fov_deg), float(aspect), W, H, _p(ws), ws_bytes,
                                       _p(points) if M else None, M, _stream()), "creg_depth_points_f64")
    return points, offsets


def segment_plane(points, offsets=None, distance_threshold=0.001, ransac_n=6, num_iterations=1000, rng=None, samples=None,
                  want_hypotheses=False):
    """Open3D's ``segment_plane(distance_threshold, ransac_n, num_iterations)`` for every segment of a packed cloud at once
    (creg_segment_plane_f64): points (N,3) f64, offsets (S+1) int64 (``None``: one segment).  ``samples`` (S,H,n) int64 are the
    hypotheses' point indices relative to their segment's start; ``None`` draws ``rng.integers(0, n_seg, (H, n))`` per segment from
    the numpy Generator ``rng`` (with replacement; a segment of fewer than n points draws nothing and has no plane), which reads the
    offsets back once.  Returns (plane (S,4) f64, mask (N) bool, count (S) int64, best (S) int32) and, with ``want_hypotheses``,
    (hyp_planes (S,H,4) f64, hyp_counts (S,H) int32) behind them.  All H hypotheses are evaluated; the mask is the best
    hypothesis's, the plane its inliers' refit; a segment without a valid hypothesis has best -1 and a plane of zeros."""
    L = _lib.load()
    points = _need(points, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"segment_plane: points must be (N,3), got {tuple(points.shape)}")
    dev, N = points.device, points.shape[0]
    if offsets is None:
        offsets = torch.tensor([0, N], dtype=torch.int64, device=dev)
    offsets = _need(torch.as_tensor(offsets, device=dev), torch.int64, "offsets")
    if offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("segment_plane: offsets must be (S+1) with S >= 1")
    S, n = offsets.shape[0] - 1, int(ransac_n)
    if not 3 <= n <= 16:
        raise ValueError(f"segment_plane: 3 <= ransac_n <= 16, got {n}")
    if samples is None:
        H = int(num_iterations)
        if H < 1:
            raise ValueError("segment_plane: num_iterations >= 1")
        rng = np.random.default_rng() if rng is None else rng
        lens = np.diff(offsets.cpu().numpy())
        host = np.zeros((S, H, n), np.int64)
        for s, m in enumerate(lens):
            if m >= n:
                host[s] = rng.integers(0, int(m), (H, n))
        samples = torch.as_tensor(host, device=dev)
    samples = _need(torch.as_tensor(samples, device=dev), torch.int64, "samples")
    if samples.dim() != 3 or samples.shape[0] != S or samples.shape[2] != n or samples.shape[1] < 1:
        raise ValueError(f"segment_plane: samples must be ({S},H,{n}) with H >= 1, got {tuple(samples.shape)}")
    H = samples.shape[1]
    if not float(distance_threshold) > 0:
        raise ValueError("segment_plane: distance_threshold must be positive")
    plane = torch.zeros(S, 4, dtype=torch.float64, device=dev)
    mask = torch.zeros(N, dtype=torch.uint8, device=dev)
    count = torch.zeros(S, dtype=torch.int64, device=dev)
    best = torch.full((S,), -1, dtype=torch.int32, device=dev)
    hp = torch.empty(S, H, 4, dtype=torch.float64, device=dev) if want_hypotheses else None
    hc = torch.empty(S, H, dtype=torch.int32, device=dev) if want_hypotheses else None
    if N == 0:                                                     # nothing to launch on: every segment is empty
        if want_hypotheses:
            hp.fill_(float("nan"))
            hc.zero_()
    else:
        ws_bytes = L.creg_segment_plane_workspace_bytes(N, S, H)
        ws = _workspace(dev, ws_bytes)
        _lib.check(L.creg_segment_plane_f64(_p(points), N, _p(offsets), S, _p(samples), H, n, float(distance_threshold), _p(plane),
                                            _p(mask), _p(count), _p(best), _p(hp), _p(hc), _p(ws), ws_bytes, _stream()),
                   "creg_segment_plane_f64")
    out = (plane, mask.bool(), count, best)
    return out + (hp, hc) if want_hypotheses else out
