"""K4 / N3: AABB-masked and plain point-to-point ICP, one problem or a batch, the closed-form rigid fit, the box mask."""
import ctypes

import torch

from .. import _lib
from ._common import _need, _p, _stream, _workspace
from .chamfer import cluster_transform

ICP_BATCH_MAX = 16


def _icp_problem(names, local, world, offsets, frame, M, woff, toff, expect, msg):
    """One ICP problem, checked and packed for the C entries.  `names`: what the wrapper calls (local, offsets, frame, M);
    `world` / `woff` (its segment offsets) / `toff` (point-to-point mode: target segment offsets) may be None; `expect`: the
    (n, nf | m, k) the problems of a batch share, None for the first; `msg`: the wrapper's ValueError texts.
    Returns (IcpProblem, (n, nf | m, k), the checked tensors it points into, (pose (k,4,4) f64, moved (n,3) f64, iterations (k) i32))."""
    local, frame, M = (_need(t, torch.float64, nm) for t, nm in zip((local, frame, M), (names[0], names[2], names[3])))
    offsets = _need(offsets, torch.int32, names[1])
    world = None if world is None else _need(world, torch.float32, "world")
    woff = None if woff is None else _need(woff, torch.int32, "world_offsets")
    toff = None if toff is None else _need(toff, torch.int32, "tgt_offsets")
    n, nf, k = shape = (local.shape[0], frame.shape[0], offsets.shape[0] - 1)
    if woff is not None:
        if world is None or woff.shape[0] != k + 1:
            raise ValueError(msg["woff"])
    elif world is not None and world.shape[0] != n:
        raise ValueError(msg["world"])
    if shape != (expect or shape) or M.shape[0] != k or (toff is not None and toff.shape[0] != k + 1):
        raise ValueError(msg["sizes"])
    outs = (torch.empty(k, 4, 4, dtype=torch.float64, device=local.device), torch.empty(n, 3, dtype=torch.float64, device=local.device),
            torch.empty(k, dtype=torch.int32, device=local.device))
    prob = _lib.IcpProblem(_p(local), _p(world), _p(offsets), _p(frame), _p(M), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(toff), _p(woff))
    return prob, shape, (local, world, offsets, frame, M, woff, toff), outs


def _icp_call(L, entry, shape, batch, dev, call):
    """The tail of the four ICP wrappers: the workspace of `batch` problems of `shape` (None: one problem, sized by the
    single-problem entry), then call(workspace, bytes, stream), checked under the C entry's name."""
    ws_bytes = L.creg_icp_workspace_bytes(*shape) if batch is None else L.creg_icp_batch_workspace_bytes(*shape, batch)
    ws = _workspace(dev, ws_bytes)
    _lib.check(call(_p(ws), ws_bytes, _stream()), entry)


def _icp_batch(who, problems, unpack, msg, scale, th, max_iteration, ori):
    """`problems` through creg_masked_icp_batch_f64; `unpack` maps one of them to _icp_problem's leading arguments."""
    L = _lib.load()
    B = len(problems)
    if not 1 <= B <= ICP_BATCH_MAX:
        raise ValueError(f"{who}: 1..{ICP_BATCH_MAX} problems per launch, got {B}")
    arr = (_lib.IcpProblem * B)()
    shape, keep, outs = None, [], []
    for b, prob in enumerate(problems):
        arr[b], shape, held, out = _icp_problem(*unpack(prob), shape, msg)
        keep.append(held)
        outs.append(out)
    n, nf, k = shape
    _icp_call(L, "creg_masked_icp_batch_f64", shape, B, keep[0][0].device, lambda ws, ws_bytes, stream: L.creg_masked_icp_batch_f64(
        arr, B, n, k, nf, float(scale), float(th), int(max_iteration), int(bool(ori)), ws, ws_bytes, stream))
    return outs


def icp_p2p_batch(problems, th: float = 1.0, max_iteration: int = 100000):
    """N3: plain point-to-point ICP (open3d registration_icp semantics) of packed cloud pairs.
    problems: list (<= 16) of (src (n,3) f64, src_offsets (k+1) i32, tgt (m,3) f64, tgt_offsets (k+1) i32,
    init (k,4,4) f64) with identical n, m, k -- e.g. the time steps of link.refine_links_clusters
    (link.py:85-127), each holding k links.  One launch (grid links x problems).
    Returns a list of (T (k,4,4) f64, moved source (n,3) f64, iterations (k) i32)."""
    msg = {"sizes": "icp_p2p_batch: all problems must share n_src, n_tgt and k"}
    return _icp_batch("icp_p2p_batch", problems, lambda p: (("src", "src_offsets", "tgt", "init"), p[0], None, p[1], p[2], p[4], None, p[3]),
                      msg, 1.0, th, max_iteration, False)


def kabsch(src, dst, offsets, weights=None):
    """Closed-form (weighted) rigid fit of paired points per segment (creg_kabsch_f64): src, dst (n,3) f64, offsets (k+1)
    i32, weights (n) f64 or None -> T (k,4,4) f64 with T src ~ dst in the least-squares sense (open3d point-to-point
    estimation / Umeyama without scaling); identity for a segment without pairs."""
    L = _lib.load()
    src, dst = _need(src, torch.float64, "src"), _need(dst, torch.float64, "dst")
    offsets = _need(offsets, torch.int32, "offsets")
    if src.shape != dst.shape or src.dim() != 2 or src.shape[1] != 3:
        raise ValueError("kabsch: src and dst must both be (n,3)")
    if weights is not None:
        weights = _need(weights, torch.float64, "weights")
        if weights.shape[0] != src.shape[0]:
            raise ValueError("kabsch: one weight per pair")
    k = offsets.shape[0] - 1
    T = torch.empty(k, 4, 4, dtype=torch.float64, device=src.device)
    _lib.check(L.creg_kabsch_f64(_p(src), _p(dst), _p(weights) if weights is not None else None, src.shape[0], _p(offsets), k, _p(T),
                                 _stream()), "creg_kabsch_f64")
    return T


def icp_p2p(src, src_offsets, tgt, tgt_offsets, init, th: float = 1.0, max_iteration: int = 100000):
    """`icp_p2p_batch` for one problem, through creg_icp_p2p_f64."""
    L = _lib.load()
    msg = {"sizes": "icp_p2p: offsets / init disagree on the number of pairs"}
    _, (n, m, k), (src, _, soff, tgt, init, _, toff), (T, moved, n_it) = _icp_problem(
        ("src", "src_offsets", "tgt", "init"), src, None, src_offsets, tgt, init, None, tgt_offsets, None, msg)
    _icp_call(L, "creg_icp_p2p_f64", (n, m, k), None, src.device, lambda ws, ws_bytes, stream: L.creg_icp_p2p_f64(
        _p(src), n, _p(soff), _p(tgt), m, _p(toff), k, _p(init), float(th), int(max_iteration), _p(T), _p(moved), _p(n_it), ws, ws_bytes, stream))
    return T, moved, n_it


def masked_icp(local: torch.Tensor, world: torch.Tensor, offsets: torch.Tensor, frame: torch.Tensor, M: torch.Tensor,
               scale: float = 1.2, th: float = 1.0, max_iteration: int = 10000, ori: bool = False,
               world_offsets: torch.Tensor = None):
    """K4, device resident: AABB-masked point-to-point ICP of every cluster against `frame`, one launch
    (reference cluster_icp.py:118-191 + open3d registration_icp).  local (n,3) f64 cluster-frame
    points (the ICP sources), offsets (k+1) int32; world f32 predicted clusters back to back (the mask boxes) with
    segment offsets `world_offsets` (None: the same segmentation as `local`; match()'s --mlp_icp branch passes the
    frame-0 clusters as `local` and the trained clouds of the current segmentation as `world`, mlp_reg.py:325),
    frame (nf,3) f64, M (k,4,4) f64 initial poses.  Returns (M_out (k,4,4) f64, world_out (n,3) f64,
    iterations (k) int32).  Stream-ordered with no host sync in the one-launch regime (clusters of at most 1024 points on
    average and frames of at most 65536 points: `masked_icp_regime(n, nf, k) == "one_launch"`); in the many-workgroup regime
    (configs[4]-sized clusters) the host enqueues the iterations in batches of 16 and follows the device one batch behind
    through pinned memory, with no stream synchronisation (creg.h) -- it still waits on events, so the call blocks the host
    until the convergence it has read back says so and cannot be captured in a graph."""
    L = _lib.load()
    msg = {"woff": "world_offsets must hold k+1 entries", "world": "world must have local's size unless world_offsets is given",
           "sizes": "local/world/offsets/M disagree on sizes"}
    _, (n, nf, k), (local, world, offsets, frame, M, world_offsets, _), (M_out, w_out, n_it) = _icp_problem(
        ("local", "offsets", "frame", "M"), local, _need(world, torch.float32, "world"), offsets, frame, M, world_offsets, None, None, msg)
    _icp_call(L, "creg_masked_icp_f64", (n, nf, k), None, local.device, lambda ws, ws_bytes, stream: L.creg_masked_icp_f64(
        _p(local), _p(world), _p(world_offsets), n, _p(offsets), k, _p(frame), nf, _p(M), float(scale), float(th), int(max_iteration),
        int(bool(ori)), _p(M_out), _p(w_out), _p(n_it), ws, ws_bytes, stream))
    return M_out, w_out, n_it


def aabb_mask(world: torch.Tensor, world_offsets: torch.Tensor, frame: torch.Tensor, scale: float = 1.2):
    """Step 1 of masked_icp (cluster_icp.py:133-146): per cluster the scaled float32 box of its world points and the
    frame points strictly inside it.  Returns (mask_idx (k, nf) int32 -- row c holds count[c] ascending indices --,
    count (k) int32, boxes (k,6) fp32)."""
    L = _lib.load()
    world, frame = _need(world, torch.float32, "world"), _need(frame, torch.float64, "frame")
    world_offsets = _need(world_offsets, torch.int32, "world_offsets")
    k, nf = world_offsets.shape[0] - 1, frame.shape[0]
    idx = torch.empty(k, nf, dtype=torch.int32, device=frame.device)
    cnt = torch.empty(k, dtype=torch.int32, device=frame.device)
    boxes = torch.empty(k, 6, dtype=torch.float32, device=frame.device)
    _lib.check(L.creg_aabb_mask_f64(_p(world), _p(world_offsets), k, _p(frame), nf, float(scale), _p(idx), _p(cnt), _p(boxes),
                                    _stream()), "creg_aabb_mask_f64")
    return idx, cnt, boxes


def masked_icp_regime(n: int, nf: int, k: int) -> str:
    """Which form creg_masked_icp_f64 runs for n source points in k clusters against a frame of nf points: "one_launch"
    (everything in one launch, no host sync) or "many_workgroups" (one launch per ICP iteration, the host one batch of 16 behind).
    Mirrors icp_large_regime in csrc/icp.hip (ICP_SRC_LDS = 1024 source points per cluster on average, 65536 frame points)."""
    return "many_workgroups" if n // max(k, 1) > 1024 or nf > 65536 else "one_launch"


def masked_icp_batch(problems, scale: float = 1.2, th: float = 1.0, max_iteration: int = 10000, ori: bool = False):
    """`masked_icp` for a list of (local, world, offsets, frame, M[, world_offsets]) of identical sizes in ONE launch
    (grid clusters x problems); returns a list of (M_out, world_out, iterations), bit-identical to
    separate calls.  `world` None = the clusters in their current pose (`cluster_transform` of the float32 casts),
    evaluated inside the kernel; `world_offsets` as in `masked_icp`."""
    msg = {"woff": "masked_icp_batch: world_offsets needs world and k+1 entries",
           "world": "masked_icp_batch: world must have local's size unless world_offsets is given",
           "sizes": "masked_icp_batch: all problems must share n, nf and k"}
    # (world None: boxes of float32(M) . float32(local))
    return _icp_batch("masked_icp_batch", problems, lambda p: (("local", "offsets", "frame", "M"), p[0], p[1], p[2], p[3], p[4],
                                                                p[5] if len(p) > 5 else None, None), msg, scale, th, max_iteration, ori)


def masked_icp_each(problems):
    """`masked_icp_batch` where its (local, world, offsets, frame, M[, world_offsets]) problems fit one launch, `masked_icp` per
    problem, in order, otherwise (`world` None: the clusters in their current pose, evaluated here by `cluster_transform`)."""
    if 1 <= len(problems) <= ICP_BATCH_MAX and len({(p[0].shape, p[2].shape, p[3].shape) for p in problems}) == 1:
        return masked_icp_batch(problems)
    outs = []
    for local, world, offsets, frame, M, *woff in problems:
        if world is None:
            world = cluster_transform(local.to(torch.float32), offsets, M.to(torch.float32))
        outs.append(masked_icp(local, world, offsets, frame, M, world_offsets=woff[0] if woff else None))
    return outs


def icp_nn_counters(reset: bool = False, timing=None) -> dict:
    """Work counters / launch timing of the many-workgroup ICP search (creg_icp_nn_counters; a measurement hook, synchronises)."""
    out = (ctypes.c_double * 8)()
    L = _lib.load()
    _lib.check(L.creg_icp_nn_counters(out, 1 if reset else 0, -1 if timing is None else int(bool(timing))), "creg_icp_nn_counters")
    keys = ("waves", "f32_trips", "f64_trips", "source_iterations", "tie_rescans", "nn_launch_us_total", "nn_launches_timed")
    return dict(zip(keys, [float(v) for v in out]))
