"""torch-facing wrappers over the C ABI: tensors in, tensors out, current CUDA(HIP) stream.

Only plumbing lives here (pointer extraction, output allocation, autograd glue); all arithmetic is
in libcreg.so.  Every function requires CUDA tensors and raises otherwise -- no CPU path exists.
"""
import ctypes

import numpy as np

import torch

from . import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor on the MI355X (autourdf_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------ K1 nearest neighbour
def nn_l1_bidir(x: torch.Tensor, y: torch.Tensor):
    """x (nx,3), y (ny,3) fp32 -> (dx, ix, dy, iy): L1 nearest neighbour both ways, first min wins."""
    L = _lib.load()
    x, y = _need(x, torch.float32, "x"), _need(y, torch.float32, "y")
    nx, ny = x.shape[0], y.shape[0]
    if nx == 0 or ny == 0:
        raise ValueError("nn_l1_bidir: empty point cloud")      # pytorch3d rejects it as well
    dx = torch.empty(nx, dtype=torch.float32, device=x.device)
    dy = torch.empty(ny, dtype=torch.float32, device=x.device)
    ix = torch.empty(nx, dtype=torch.int64, device=x.device)
    iy = torch.empty(ny, dtype=torch.int64, device=x.device)
    _lib.check(L.creg_nn_l1_bidir_f32(_p(x), nx, _p(y), ny, _p(dx), _p(ix), _p(dy), _p(iy), _stream()),
               "creg_nn_l1_bidir_f32")
    return dx, ix, dy, iy


class _ChamferL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        L = _lib.load()
        dx, ix, dy, iy = nn_l1_bidir(x, y)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        _lib.check(L.creg_chamfer_l1_reduce_f32(_p(dx), dx.numel(), _p(dy), dy.numel(), _p(loss), _stream()),
                   "creg_chamfer_l1_reduce_f32")
        ctx.save_for_backward(x.detach().contiguous(), y.detach().contiguous(), ix, iy)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        x, y, ix, iy = ctx.saved_tensors
        nx, ny = x.shape[0], y.shape[0]
        grad = torch.empty_like(x)
        scratch = torch.empty(L.creg_nn_l1_bwd_scratch_bytes(nx), dtype=torch.uint8, device=x.device)
        one = torch.tensor(1.0, dtype=torch.float32)
        gx, gy = float(one / nx), float(one / ny)
        _lib.check(L.creg_nn_l1_bwd_f32(_p(x), nx, _p(y), ny, _p(ix), _p(iy), gx, gy, _p(grad), _p(scratch),
                                        _stream()), "creg_nn_l1_bwd_f32")
        return grad * g, None


def chamfer_distance(x: torch.Tensor, y: torch.Tensor, norm: int = 1):
    """pytorch3d.loss.chamfer_distance(x, y, norm=1) for the reference's call (mlp_reg.py:96):
    x (1,P1,3) with grad, y (1,P2,3); returns (loss, None)."""
    if norm != 1:
        raise NotImplementedError("only norm=1 is on the registration path")
    if x.dim() != 3 or x.shape[0] != 1 or y.shape[0] != 1:
        raise NotImplementedError("batch of 1 only (as the reference calls it)")
    return _ChamferL1.apply(_need(x[0], torch.float32, "x"), _need(y[0], torch.float32, "y")), None


# ------------------------------------------------------------------------------ K3 cluster transform
class _ClusterTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, offsets, M):
        L = _lib.load()
        out = torch.empty_like(pts)
        k = M.shape[0]
        _lib.check(L.creg_cluster_transform_f32(_p(pts), pts.shape[0], _p(offsets), k, _p(M), _p(out), _stream()),
                   "creg_cluster_transform_f32")
        ctx.save_for_backward(pts, offsets)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        pts, offsets = ctx.saved_tensors
        gM = torch.empty(ctx.k, 4, 4, dtype=torch.float32, device=pts.device)
        _lib.check(L.creg_cluster_transform_bwd_f32(_p(pts), _p(offsets), ctx.k, _p(g.contiguous()), _p(gM), _stream()),
                   "creg_cluster_transform_bwd_f32")
        return None, None, gM


def cluster_transform(pts: torch.Tensor, offsets: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """pts (n,3) fp32 clusters back to back, offsets (k+1) int32, M (k,4,4) fp32 -> world points."""
    return _ClusterTransform.apply(_need(pts, torch.float32, "pts"), _need(offsets, torch.int32, "offsets"),
                                   _need(M, torch.float32, "M"))


def pack_clusters(clusters, device, dtype=torch.float32):
    """list of (M_k,3) tensors/arrays -> (flat (n,3) tensor, offsets (k+1) int32 tensor), on `device`."""
    ts = [torch.as_tensor(c, dtype=dtype).reshape(-1, 3) for c in clusters]
    sizes = [t.shape[0] for t in ts]
    off = torch.zeros(len(ts) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0).to(torch.int32)
    flat = torch.cat([t.to(device) for t in ts], 0) if ts else torch.zeros(0, 3, dtype=dtype, device=device)
    return flat.contiguous(), off.to(device)


# ------------------------------------------------------------------------------ K2 k-means
def _need_n_ge_k(n: int, k: int) -> None:
    """sklearn's refusal, in its words, before the library loads: with fewer points than clusters the empty-cluster relocation of
    the Lloyd kernels runs out of points to take (the C entry points refuse it too)."""
    if n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")


def kmeans_lloyd(X: torch.Tensor, init: torch.Tensor, max_iter: int = 300, tol: float = 1e-4,
                 use_mfma: bool = False):
    """sklearn.cluster.k_means(X, init=init, n_init=1): returns (centers (k,3) f64, labels (n) int32,
    inertia (1) f64, n_iter (1) int32), all on the device."""
    _need_n_ge_k(X.shape[0], init.shape[0])
    L = _lib.load()
    X, init = _need(X, torch.float64, "X"), _need(init, torch.float64, "init")
    n, k = X.shape[0], init.shape[0]
    ws_bytes = L.creg_kmeans_workspace_bytes(n, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device)
    centers = torch.empty(k, 3, dtype=torch.float64, device=X.device)
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    inertia = torch.empty(1, dtype=torch.float64, device=X.device)
    n_iter = torch.empty(1, dtype=torch.int32, device=X.device)
    _lib.check(L.creg_kmeans_lloyd_f64(_p(X), n, _p(init), k, max_iter, tol, int(use_mfma), _p(centers), _p(labels),
                                       _p(inertia), _p(n_iter), _p(ws), ws_bytes, _stream()), "creg_kmeans_lloyd_f64")
    return centers, labels, inertia, n_iter


def kmeans_lloyd_nd(X: torch.Tensor, init: torch.Tensor, max_iter: int = 300, tol: float = 1e-4):
    """sklearn.cluster.k_means(X, init=init, n_init=1) over (n,6) or (n,3) features -- the `--normal` branch clusters
    [xyz | 0.5 normal] (mlp_reg.py:196-203) -- in one workgroup (k <= n < 2^24, k <= 128; the labels stay in LDS up to 16384 points
    and live in the workspace above): (centers (k,d) f64, labels (n) int32, inertia (1) f64, n_iter (1) int32), all on the device."""
    _need_n_ge_k(X.shape[0], init.shape[0])
    L = _lib.load()
    X, init = _need(X, torch.float64, "X"), _need(init, torch.float64, "init")
    n, d, k = X.shape[0], X.shape[1], init.shape[0]
    if init.shape[1] != d:
        raise ValueError("kmeans_lloyd_nd: X and init disagree on the feature count")
    if n > KMEANS_ND_MAX_N or k > KMEANS_ND_MAX_K:
        raise ValueError(f"the --normal re-segmentation (k-means over [xyz | 0.5 normal]) runs in one workgroup: frames of at most "
                         f"{KMEANS_ND_MAX_N} points and {KMEANS_ND_MAX_K} clusters, got {n} points / {k} clusters (the reference's sklearn "
                         "k_means has no such limit: down-sample the frames -- Segments(sample_size=...) -- or run without --normal)")
    ws_bytes = L.creg_kmeans_nd_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device)
    centers = torch.empty(k, d, dtype=torch.float64, device=X.device)
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    inertia = torch.empty(1, dtype=torch.float64, device=X.device)
    n_iter = torch.empty(1, dtype=torch.int32, device=X.device)
    _lib.check(L.creg_kmeans_lloyd_nd_f64(_p(X), n, d, _p(init), k, max_iter, tol, _p(centers), _p(labels), _p(inertia), _p(n_iter),
                                          _p(ws), ws_bytes, _stream()), "creg_kmeans_lloyd_nd_f64")
    return centers, labels, inertia, n_iter


def knn_normals(X: torch.Tensor, radius: float, max_nn: int, want_normals: bool = True, want_idx: bool = False):
    """creg_knn_normals_f64: the (up to) max_nn nearest points of every point of X (n,3) f64 (itself included; radius > 0:
    only squared distances < radius^2, open3d's SearchHybrid; radius <= 0: plain SearchKNN) and, from them, open3d's
    estimate_normals (unoriented).  Returns (normals (n,3) f64 or None, idx (n,max_nn) int32 or None, counts (n) int32)."""
    L = _lib.load()
    X = _need(X, torch.float64, "X")
    n = X.shape[0]
    normals = torch.empty(n, 3, dtype=torch.float64, device=X.device) if want_normals else None
    idx = torch.empty(n, max_nn, dtype=torch.int32, device=X.device) if want_idx else None
    cnt = torch.empty(n, dtype=torch.int32, device=X.device)
    _lib.check(L.creg_knn_normals_f64(_p(X), n, float(radius), int(max_nn), _p(idx) if want_idx else None, _p(cnt),
                                      _p(normals) if want_normals else None, _stream()), "creg_knn_normals_f64")
    return normals, idx, cnt


KMEANS_ND_MAX_N, KMEANS_ND_MAX_K = (1 << 24) - 1, 128      # creg_kmeans_lloyd_nd_f64: one workgroup, centres in LDS (labels too up to 16384 points, in the workspace above)
KMEANS_BATCH_MAX_N = 16384         # labels + centres in one CU's LDS; the frame too up to 5120 points, from L2 above
KMEANS_BATCH_MAX, KMEANS_BATCH_MAX_K = 16, 128             # frames per launch (KMS_MAXB in kmeans.hip), centres in LDS


def _batchable(limit, *lists):
    """The `_each` helpers' rule: 1..limit problems, and every problem has the shapes of the first."""
    B = len(lists[0])
    return 1 <= B <= limit and all(len(l) == B and all(t.shape == l[0].shape for t in l) for l in lists)


def kmeans_lloyd_batch(Xs, inits, max_iter: int = 300, tol: float = 1e-4):
    """k_means() for a list of same-sized frames in ONE asynchronous launch (one workgroup per frame,
    n <= 16384).  Returns a list of (centers, labels, inertia, n_iter) like `kmeans_lloyd`."""
    for x, c in zip(Xs, inits):
        _need_n_ge_k(x.shape[0], c.shape[0])
    L = _lib.load()
    Xs = [_need(x, torch.float64, "X") for x in Xs]
    inits = [_need(c, torch.float64, "init") for c in inits]
    B, n, k = len(Xs), Xs[0].shape[0], inits[0].shape[0]
    if any(x.shape[0] != n for x in Xs) or any(c.shape[0] != k for c in inits) or len(inits) != B:
        raise ValueError("kmeans_lloyd_batch: all problems must have the same n and k")
    dev = Xs[0].device
    ws_bytes = L.creg_kmeans_batch_workspace_bytes(n, k, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    outs = [(torch.empty(k, 3, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
             torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)) for _ in range(B)]
    arr = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    _lib.check(L.creg_kmeans_lloyd_batch_f64(arr(Xs), n, arr(inits), k, B, max_iter, tol, arr([o[0] for o in outs]),
                                             arr([o[1] for o in outs]), arr([o[2] for o in outs]), arr([o[3] for o in outs]),
                                             _p(ws), ws_bytes, _stream()), "creg_kmeans_lloyd_batch_f64")
    return outs


def kmeans_lloyd_each(Xs, inits):
    """`kmeans_lloyd_batch` where the frames fit one launch, `kmeans_lloyd` per frame, in order, otherwise."""
    if _batchable(KMEANS_BATCH_MAX, Xs, inits) and Xs[0].shape[0] <= KMEANS_BATCH_MAX_N and inits[0].shape[0] <= KMEANS_BATCH_MAX_K:
        return kmeans_lloyd_batch(Xs, inits)
    return [kmeans_lloyd(X, c) for X, c in zip(Xs, inits)]


def kmeans_assign(X: torch.Tensor, C: torch.Tensor, use_mfma: bool = False) -> torch.Tensor:
    L = _lib.load()
    X, C = _need(X, torch.float64, "X"), _need(C, torch.float64, "C")
    labels = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    _lib.check(L.creg_kmeans_assign_f64(_p(X), X.shape[0], _p(C), C.shape[0], int(use_mfma), _p(labels), _stream()),
               "creg_kmeans_assign_f64")
    return labels


def group_to_local(X: torch.Tensor, labels: torch.Tensor, M: torch.Tensor, m_is_inverse: bool = False):
    """Stable grouping by label and inv(M_k) change of frame: returns (local (n,3) f64, offsets (k+1) int32).
    m_is_inverse: M already holds the inverted poses (the drop-in inverts them on the host like mlp_reg.py:211)."""
    L = _lib.load()
    X, labels, M = _need(X, torch.float64, "X"), _need(labels, torch.int32, "labels"), _need(M, torch.float64, "M")
    k = M.shape[0]
    out = torch.empty_like(X)
    off = torch.empty(k + 1, dtype=torch.int32, device=X.device)
    _lib.check(L.creg_group_to_local_f64(_p(X), X.shape[0], _p(labels), k, _p(M), int(bool(m_is_inverse)), _p(out), _p(off), _stream()),
               "creg_group_to_local_f64")
    return out, off


GROUP_BATCH_MAX = 16


def group_to_local_batch(Xs, labels, Ms, m_is_inverse: bool = False):
    """`group_to_local` for a list (<= 16) of frames of identical n and k in one pair of launches.
    Returns a list of (local (n,3) f64, offsets (k+1) int32)."""
    L = _lib.load()
    B = len(Xs)
    if not 1 <= B <= GROUP_BATCH_MAX or len(labels) != B or len(Ms) != B:
        raise ValueError(f"group_to_local_batch: 1..{GROUP_BATCH_MAX} problems, one label / pose tensor each")
    Xs = [_need(x, torch.float64, "X") for x in Xs]
    labels = [_need(l, torch.int32, "labels") for l in labels]
    Ms = [_need(m, torch.float64, "M") for m in Ms]
    n, k = Xs[0].shape[0], Ms[0].shape[0]
    if any(x.shape[0] != n for x in Xs) or any(m.shape[0] != k for m in Ms) or any(l.shape[0] != n for l in labels):
        raise ValueError("group_to_local_batch: all problems must share n and k")
    outs = [(torch.empty_like(x), torch.empty(k + 1, dtype=torch.int32, device=x.device)) for x in Xs]
    arr = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    _lib.check(L.creg_group_to_local_batch_f64(arr(Xs), n, arr(labels), k, arr(Ms), int(bool(m_is_inverse)), B, arr([o[0] for o in outs]),
                                               arr([o[1] for o in outs]), _stream()), "creg_group_to_local_batch_f64")
    return outs


def group_to_local_each(Xs, labels, Ms, m_is_inverse: bool = False):
    """`group_to_local_batch` where the frames fit one pair of launches, `group_to_local` per frame, in order, otherwise."""
    if _batchable(GROUP_BATCH_MAX, Xs, labels, Ms):
        return group_to_local_batch(Xs, labels, Ms, m_is_inverse=m_is_inverse)
    return [group_to_local(X, l, M, m_is_inverse=m_is_inverse) for X, l, M in zip(Xs, labels, Ms)]


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
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
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


# ------------------------------------------------------------------------------ N4 mesh surface sampling
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
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=pts.device)
    vis = torch.empty(n, dtype=torch.uint8, device=pts.device)
    _lib.check(L.creg_visibility_f64(_p(tri), _p(tri_link), tri.shape[0], _p(link_T), link_T.shape[0], _p(cams), C, float(fov_deg),
                                     float(aspect), float(near), float(far), int(width), int(height), _p(pts), n, float(eps), _p(vis),
                                     _p(ws), ws_bytes, _stream()), "creg_visibility_f64")
    return (vis.bool(), ws.reshape(C, height, width)) if return_depth else vis.bool()


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
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=depth.device)
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
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
        _lib.check(L.creg_segment_plane_f64(_p(points), N, _p(offsets), S, _p(samples), H, n, float(distance_threshold), _p(plane),
                                            _p(mask), _p(count), _p(best), _p(hp), _p(hc), _p(ws), ws_bytes, _stream()),
                   "creg_segment_plane_f64")
    out = (plane, mask.bool(), count, best)
    return out + (hp, hc) if want_hypotheses else out


def urdf_fk(table, q, base, want_lines: bool = False):
    """Batched forward kinematics (creg_urdf_fk_f64): ``table`` from ``UrdfRobot.fk_table()``, q (P,J) joint values in the
    table's order and base (4,4), host arrays or f64 device tensors -> link_T (P,L,4,4) f64 on the device, and
    joint_lines (P,J,6) = world position of the joint frame | unit world axis when ``want_lines``.  One launch for all P."""
    L = _lib.load()
    dev = _lib.device(q, base)
    tdev = table.get("_dev")
    if tdev is None or tdev[0].device != dev:                     # the table goes up once per robot and device
        tdev = tuple(torch.as_tensor(np.ascontiguousarray(table[k]), device=dev) for k in ("parent", "child", "type", "origin", "axis"))
        table["_dev"] = tdev
    parent, child, kind, origin, axis = tdev
    q = _need(torch.as_tensor(q, dtype=torch.float64, device=dev), torch.float64, "q")
    base = _need(torch.as_tensor(base, dtype=torch.float64, device=dev), torch.float64, "base")
    J, n_links = parent.shape[0], int(table["n_links"])
    if q.dim() != 2 or q.shape[1] != J or tuple(base.shape) != (4, 4):
        raise ValueError(f"urdf_fk: q must be (P,{J}) and base (4,4), got {tuple(q.shape)} and {tuple(base.shape)}")
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


def _shapes_expected(who, arrays):
    """The ValueError that names every array with the expected and the received shape."""
    return ValueError(f"{who}: {' / '.join(f'{name} {want}' for name, want, _ in arrays)} expected, got "
                      f"{', '.join(str(tuple(t.shape)) for _, _, t in arrays)}")


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
    ok = (tri_start[0] == 0) & (tri_start[-1] == F) & (tri_start[1:] >= tri_start[:-1]).all()
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
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
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


MESH_CONTAIN_MAX_POINTS = 16


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
    per_link = pt_start[1:] - pt_start[:-1]
    lo, hi, first_row, last_row = (int(v) for v in torch.stack([per_link.min(), per_link.max(), pt_start[0], pt_start[-1]]).cpu())
    if first_row != 0 or last_row != N or lo < 0 or hi > MESH_CONTAIN_MAX_POINTS:
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
    ok = (tri_start[0] == 0) & (tri_start[-1] == F) & (tri_start[1:] >= tri_start[:-1]).all() \
        & (pt_start[0] == 0) & (pt_start[-1] == N) & (pt_start[1:] >= pt_start[:-1]).all()
    if not bool(ok):
        raise ValueError(f"point_mesh_distance: tri_start must run from 0 to {F} and pt_start from 0 to {N} without decreasing")
    order = _morton_order(pts, pt_start, P) if sort and N else None
    dist2 = torch.empty(N, dtype=torch.float64, device=dev)
    tri_idx = torch.empty(N, dtype=torch.int32, device=dev)
    boxes = torch.empty(P, n_links, 6, dtype=torch.float64, device=dev) if want_boxes else None
    ws_bytes = L.creg_point_mesh_workspace_bytes(F, n_links, P, N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
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


POSE_FIT_MAX_D = 64


def joint_chains(table):
    """chain (L) uint64 of a joint table (``UrdfRobot.fk_table()``): bit j of chain[l] is set iff joint j lies on the path from the
    root to link l.  The table is in topological order, so a child's mask is its parent's plus its own bit; a joint with an index
    outside [0, L) sets no bit, as the forward kinematics skips it.  At most 64 joints."""
    n_links, parent, child = int(table["n_links"]), np.asarray(table["parent"]), np.asarray(table["child"])
    if len(parent) > 64:
        raise ValueError(f"joint_chains: at most 64 joints fit a mask, got {len(parent)}")
    chain = [0] * n_links
    for j, (pa, ch) in enumerate(zip(parent, child)):
        if 0 <= pa < n_links and 0 <= ch < n_links:
            chain[ch] = chain[pa] | (1 << j)
    return np.array(chain, np.uint64)


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
    tdev = table.get("_dev_fit")
    if tdev is None or tdev[0].device != dev:                     # the table and its chain masks go up once per robot and device
        tdev = tuple(torch.as_tensor(np.ascontiguousarray(table[k]), device=dev) for k in ("parent", "child", "type", "origin", "axis")) \
            + (torch.as_tensor(joint_chains(table).view(np.int64), device=dev),)
        table["_dev_fit"] = tdev
    parent, child, kind, origin, axis, chain = tdev
    D = 6 + J
    H = torch.empty(P, D, D, dtype=torch.float64, device=dev)
    g = torch.empty(P, D, dtype=torch.float64, device=dev)
    cost = torch.empty(P, dtype=torch.float64, device=dev)
    n = torch.empty(P, dtype=torch.int64, device=dev)
    ws_bytes = L.creg_pose_fit_workspace_bytes(P, N, J)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    tab = lambda t: _p(t) if J else None
    _lib.check(L.creg_pose_fit_system_f64(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(pts) if N else None,
                                          _p(pt_start), N, d_max, _p(tri_idx) if N else None, tab(parent), tab(child), tab(kind),
                                          tab(origin), tab(axis), J, _p(chain), _p(center), _p(H), _p(g), _p(cost), _p(n), _p(ws),
                                          ws_bytes, _stream()), "creg_pose_fit_system_f64")
    return H, g, cost, n


def link_moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max=float("inf")):
    """The 16 moment sums per (pose, link) of the correspondences (creg_link_moments_f64; the contract is in include/creg.h): tri,
    tri_start, link_T, pts, pt_start, tri_idx and ``d_max`` as ``pose_fit_system`` takes them, ref (P,L,3) f64 the point the
    moments of every (pose, link) are taken about -> (mom (P,L,16) f64, cnt (P,L) int64) on the device: per (pose, link) the sums
    of d d^T (6: xx xy xz yy yz zz), d (3), d x r (3), r (3) and r.r over its contributing points, d = c - ref, and their number.
    One call for all poses; no joint table and no limit on a parameter count (``compute_joints.twist_system`` turns the moments
    into a normal system).  tri_start and pt_start are not read back; the kernel clamps them.  ValueError before any launch: a bad
    shape or dtype, a negative or NaN ``d_max``."""
    L = _lib.load()
    d_max, tri, tri_start, link_T, pts, pt_start, tri_idx, ref, F, P, n_links, N, dev = _point_query_args(
        "link_moments", tri, tri_start, link_T, pts, pt_start, d_max,
        (("tri_idx", tri_idx, torch.int32, "(N)"), ("ref", ref, torch.float64, "(P,L,3)")))
    mom = torch.empty(P, n_links, 16, dtype=torch.float64, device=dev)
    cnt = torch.empty(P, n_links, dtype=torch.int64, device=dev)
    ws_bytes = L.creg_link_moments_workspace_bytes(P, N, n_links)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    _lib.check(L.creg_link_moments_f64(_p(tri) if F else None, _p(tri_start), F, _p(link_T), n_links, P, _p(pts) if N else None,
                                       _p(pt_start), N, d_max, _p(tri_idx) if N else None, _p(ref), _p(mom), _p(cnt), _p(ws), ws_bytes,
                                       _stream()), "creg_link_moments_f64")
    return mom, cnt


MESH_INERTIA_KEYS = ("sums", "volume", "area", "closure", "mass", "com", "inertia", "principal", "axes")


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
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    _lib.check(L.creg_mesh_inertia_f64(_p(tri) if F else None, _p(tri_start), F, n_links, _p(density), *[_p(out[k]) for k in MESH_INERTIA_KEYS],
                                       _p(ws), ws_bytes, _stream()), "creg_mesh_inertia_f64")
    return out


# ------------------------------------------------------------------------------ N2 pose distance maps
def coord_dist_map(M: torch.Tensor, bounding_box: float, diff: bool = True):
    """CoordMap.coord_dist_map (coord_map.py:230-307) for poses M (T,K,4,4) f64 on the device:
    returns (coord_dist_map (K,K,T') f64, sum_map (K,K) f64), T' = T-1 if diff else T."""
    L = _lib.load()
    M = _need(M, torch.float64, "M")
    if M.dim() != 4 or M.shape[2:] != (4, 4):
        raise ValueError("coord_dist_map: M must be (T,K,4,4)")
    T, K = M.shape[:2]
    Tn = T - 1 if diff else T
    d_map = torch.empty(K, K, Tn, dtype=torch.float64, device=M.device)
    s_map = torch.empty(K, K, dtype=torch.float64, device=M.device)
    ws_bytes = L.creg_coord_dist_map_workspace_bytes(T, K)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=M.device)
    _lib.check(L.creg_coord_dist_map_f64(_p(M), T, K, float(bounding_box), int(bool(diff)), _p(d_map), _p(s_map), _p(ws),
                                         ws.numel(), _stream()), "creg_coord_dist_map_f64")
    return d_map, s_map


def pose_coords(M: torch.Tensor) -> torch.Tensor:
    """(...,4,4) f64 poses -> (...,7) [xyz, pytorch3d quaternion wxyz] (load_matrix, coord_map.py:204-219)."""
    L = _lib.load()
    M = _need(M, torch.float64, "M")
    n = M.numel() // 16
    out = torch.empty(M.shape[:-2] + (7,), dtype=torch.float64, device=M.device)
    _lib.check(L.creg_pose_coords_f64(_p(M), n, _p(out), _stream()), "creg_pose_coords_f64")
    return out


# ------------------------------------------------------------------------------ N4 URDF stage: link discovery, MST
LINK_SWEEP_MAX_K = 256


def link_sweep(d_map: torch.Tensor, nl_lo: int, nl_hi: int):
    """coord_clustering for every nl in [nl_lo, nl_hi) plus silhouette_score_method's choice, one launch.
    d_map (K,K) f64 on the device.  Returns (labels (n,K) int32, n_comp (n) int32, thresholds (n) f64,
    scores (n) f64, best (1) int32); best = -1 when a label count fell outside [2, K-1]."""
    L = _lib.load()
    d_map = _need(d_map, torch.float64, "d_map")
    if d_map.dim() != 2 or d_map.shape[0] != d_map.shape[1]:
        raise ValueError("link_sweep: d_map must be (K,K)")
    K, n = d_map.shape[0], nl_hi - nl_lo
    dev = d_map.device
    labels = torch.empty(max(n, 1), K, dtype=torch.int32, device=dev)
    n_comp = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    thr = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    scores = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.creg_link_sweep_f64(_p(d_map), K, int(nl_lo), int(nl_hi), _p(labels), _p(n_comp), _p(thr), _p(scores),
                                     _p(best), _stream()), "creg_link_sweep_f64")
    return labels, n_comp, thr, scores, best


def coord_mst(coords: torch.Tensor):
    """CoordMap.coord_mst's tree over the T-summed xyz of coords (T,K,7) f64: (edges (K-1,2) int32, weights (K-1) f64)
    in Prim's attachment order."""
    L = _lib.load()
    coords = _need(coords, torch.float64, "coords")
    if coords.dim() != 3 or coords.shape[2] != 7:
        raise ValueError("coord_mst: coords must be (T,K,7)")
    T, K = coords.shape[:2]
    edges = torch.empty(max(K - 1, 1), 2, dtype=torch.int32, device=coords.device)
    w = torch.empty(max(K - 1, 1), dtype=torch.float64, device=coords.device)
    _lib.check(L.creg_coord_mst_f64(_p(coords), T, K, _p(edges), _p(w), _stream()), "creg_coord_mst_f64")
    return edges[:K - 1], w[:K - 1]


# ------------------------------------------------------------------------------ N4 URDF stage: joint axes, link clouds
# csrc/joints_dev.h holds the same limits as JOINT_MAX_K (LINK_SWEEP_MAX_K here), JOINT_MAX_SAMPLES and JOINT_THETA_MIN
JOINT_MAX_SAMPLES = 4096
JOINT_THETA_MIN = 2e-4             # rad: a sample below it is not usable (creg.h)


def _max_clusters(who, K):
    if K > LINK_SWEEP_MAX_K:
        raise ValueError(f"{who} supports at most {LINK_SWEEP_MAX_K} clusters, got {K}")


def _link_tables(who, link_clusters, K, dev):
    """The links' clusters as one flat host list with its offsets, and both as int32 device tables (keep them alive across
    the launch): (flat, off, cl, lo).  ValueError under ``who``'s name for an empty link or a cluster outside [0, K).
    ``dev`` None: the host lists alone, for a caller that allocates its outputs before it copies a table -- a host-to-device
    copy waits for the stream's earlier work, whatever the host does after it no longer overlaps that work."""
    flat, off = [], [0]
    for l, c in enumerate(link_clusters):
        c = [int(x) for x in c]
        if not c:
            raise ValueError(f"{who}: link {l} has no cluster")
        bad = [x for x in c if not 0 <= x < K]
        if bad:
            raise ValueError(f"{who}: link {l} names clusters {bad} outside [0, {K})")
        flat.extend(c)
        off.append(len(flat))
    return (flat, off, None, None) if dev is None else (flat, off, *_i32_tables(dev, flat, off))


def _i32_tables(dev, *lists):
    return tuple(torch.tensor(x, dtype=torch.int32, device=dev) for x in lists)


def _joint_pairs(who, joints, L):
    jt = [(int(p), int(c)) for p, c in joints]
    for p, c in jt:
        if not (0 <= p < L and 0 <= c < L):
            raise ValueError(f"{who}: joint ({p}, {c}) names a link outside [0, {L})")
    return jt


def _joint_sample_args(who, coords, link_clusters, joints, start_step, num_steps, interval, outputs):
    """What joint_axes and joint_types check and build alike, under ``who``'s name: coords, the K cap, the steps (ValueError,
    then IndexError in numpy's words), the link table, the joint pairs and the sample count; then the caller's
    ``outputs(J, NS, dev)`` are allocated, and only then the device tables copied (see _link_tables).  Returns (library,
    head, L, tail, keep, J, NS, out): the entry's leading C arguments up to n_link_clusters, the link count, its arguments
    from joints to interval, the tensors that must outlive every launch, and what ``outputs`` returned."""
    lib = _lib.load()
    coords = _need(coords, torch.float64, "coords")
    if coords.dim() != 4 or coords.shape[3] != 7:
        raise ValueError(f"{who}: coords must be (S,T,K,7)")
    S, T, K = coords.shape[:3]
    _max_clusters(who, K)
    start_step, num_steps, interval = int(start_step), int(num_steps), int(interval)
    if start_step < 0 or num_steps < 1 or interval < 1:
        raise ValueError(f"{who}: need start_step >= 0, num_steps >= 1, interval >= 1 "
                         f"(got {start_step}, {num_steps}, {interval})")
    if start_step + num_steps > T:
        raise IndexError(f"index {start_step + num_steps - 1} is out of bounds for axis 0 with size {T}")
    flat, off, _, _ = _link_tables(who, link_clusters, K, None)
    L = len(off) - 1
    jt = _joint_pairs(who, joints, L)
    NS = joint_samples(S, num_steps, interval)
    if NS > JOINT_MAX_SAMPLES:
        raise ValueError(f"{who}: {NS} samples per joint, at most {JOINT_MAX_SAMPLES} are supported")
    J, dev = len(jt), coords.device
    out = outputs(J, NS, dev)
    cl, lo, jn = _i32_tables(dev, flat, off, jt or [(0, 0)])
    return (lib, (_p(coords), S, T, K, _p(cl), _p(lo), len(flat)), L, (_p(jn), J, start_step, num_steps, interval),
            (coords, cl, lo, jn), J, NS, out)


def joint_samples(S: int, num_steps: int, interval: int) -> int:
    """Samples per joint: S sequences x sum over phases a < interval of (len(range(a, num_steps, interval)) - 1)^+."""
    return int(_lib.load(check_device=False).creg_joint_axes_samples(int(S), int(num_steps), int(interval)))


def joint_axes(coords: torch.Tensor, link_clusters, joints, start_step: int = 0, num_steps: int = 500, interval: int = 1):
    """estimate_joint_axes_from_tree's arithmetic for every joint in one launch of creg_joint_axes_f64
    (joint_axes_prepare, then its launch).
    coords (S,T,K,7) f64 [xyz, wxyz]; link_clusters: one cluster list per link (set order); joints: (parent, child)
    indices into link_clusters.  Returns a dict of device tensors: sample_axis (J,NS,3), sample_angle (J,NS),
    sample_point (J,NS,3), sample_usable (J,NS) bool, local_axis (J,3), local_pos (J,4), global_pos (J,3),
    global_axis (J,3), count (J), first_pose (J,2,7).  Raises IndexError for a step past T (as numpy indexing would) and
    ValueError for K > 256, an empty link or more than JOINT_MAX_SAMPLES samples per joint, before any launch."""
    launch, out = joint_axes_prepare(coords, link_clusters, joints, start_step, num_steps, interval)
    launch()
    out["sample_usable"] = out["sample_usable"] != 0
    return out


def joint_axes_prepare(coords: torch.Tensor, link_clusters, joints, start_step: int = 0, num_steps: int = 500,
                       interval: int = 1):
    """Checks and device tables of joint_axes, done once: returns (launch, outputs), where launch() only enqueues
    creg_joint_axes_f64 on the current stream (sample_usable stays int32 here)."""
    def outputs(J, NS, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        return {"sample_axis": torch.empty(J, NS, 3, **f64), "sample_angle": torch.empty(J, NS, **f64),
                "sample_point": torch.empty(J, NS, 3, **f64), "sample_usable": torch.empty(J, NS, **i32),
                "local_axis": torch.empty(J, 3, **f64), "local_pos": torch.empty(J, 4, **f64),
                "global_pos": torch.empty(J, 3, **f64), "global_axis": torch.empty(J, 3, **f64),
                "count": torch.zeros(J, **i32), "first_pose": torch.empty(J, 2, 7, **f64)}
    L, head, _, tail, keep, J, NS, out = _joint_sample_args("joint_axes", coords, link_clusters, joints, start_step, num_steps,
                                                            interval, outputs)
    smp = (_p(out["sample_axis"]), _p(out["sample_angle"]), _p(out["sample_point"]),
           _p(out["sample_usable"])) if NS else (None, None, None, None)
    args = (*head, *tail, *smp, _p(out["local_axis"]), _p(out["local_pos"]), _p(out["global_pos"]), _p(out["global_axis"]),
            _p(out["count"]), _p(out["first_pose"]))

    def launch():                                                  # returns the tables, which must outlive every launch
        if J:
            _lib.check(L.creg_joint_axes_f64(*args, _stream()), "creg_joint_axes_f64")
        return keep
    return launch, out


def joint_types(coords: torch.Tensor, link_clusters, joints, start_step: int = 0, num_steps: int = 1, interval: int = 1,
                turn_min: float = JOINT_THETA_MIN, slide_min=None):
    """Which kind of joint every edge is, over joint_axes' samples, in one launch of creg_joint_types_f64.  coords,
    link_clusters, joints and the steps as ``joint_axes``; a sample turns when its angle reaches turn_min (rad), slides when
    it does not and its translation reaches slide_min, and stands still otherwise.  slide_min is a length in the clouds'
    unit and has no default: None is a ValueError.  Returns a dict of device tensors: sample_angle (J,NS) f64 (the bits of
    joint_axes'), sample_slide (J,NS,3) f64, sample_kind (J,NS) int32 (-1 bad, 0 still, 1 turn, 2 slide), counts (J,4) int32
    (still, turn, slide, bad), type (J) int32 in urdf_fk's numbering (0 fixed, 1 revolute, 2 prismatic, -1 no finite sample),
    slide_axis, global_axis, global_pos (J,3) f64.  The checks and errors are joint_axes', plus ValueError for a threshold
    that is negative or not finite, all before any launch."""
    if slide_min is None:
        raise ValueError("joint_types: slide_min is a length in the clouds' unit and has no default, give one")
    turn_min, slide_min = float(turn_min), float(slide_min)
    if not (np.isfinite(turn_min) and turn_min >= 0.0 and np.isfinite(slide_min) and slide_min >= 0.0):
        raise ValueError(f"joint_types: turn_min and slide_min must be finite and >= 0 (got {turn_min}, {slide_min})")
    def outputs(J, NS, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        return {"sample_angle": torch.empty(J, NS, **f64), "sample_slide": torch.empty(J, NS, 3, **f64),
                "sample_kind": torch.empty(J, NS, **i32), "counts": torch.empty(J, 4, **i32), "type": torch.empty(J, **i32),
                "slide_axis": torch.empty(J, 3, **f64), "global_axis": torch.empty(J, 3, **f64),
                "global_pos": torch.empty(J, 3, **f64)}
    L_, head, L, tail, keep, J, NS, out = _joint_sample_args("joint_types", coords, link_clusters, joints, start_step, num_steps,
                                                             interval, outputs)    # keep: the tables live until the call is enqueued
    if J:
        smp = (_p(out["sample_angle"]), _p(out["sample_slide"]), _p(out["sample_kind"])) if NS else (None, None, None)
        _lib.check(L_.creg_joint_types_f64(*head, L, *tail, turn_min, slide_min, *smp, _p(out["counts"]), _p(out["type"]),
                                           _p(out["slide_axis"]), _p(out["global_axis"]), _p(out["global_pos"]), _stream()),
                   "creg_joint_types_f64")
    return out


def link_clouds_bytes(n_points: int, n_out: int, T: int, K: int, L: int) -> int:
    """HBM traffic of one creg_link_clouds_f64 launch: points read, both clouds written, poses and offsets."""
    return 24 * n_points + 48 * n_out + T * K * (7 + 16) * 8 + (T * K + T * L + 2) * 8 + T * L * 2 * 64


def link_clouds(coords: torch.Tensor, matrices: torch.Tensor, link_clusters, points: torch.Tensor, point_offsets,
                mean_matrices: bool = False):
    """CoordMap.cluster_to_link's arithmetic for every frame and link in one launch of creg_link_clouds_f64
    (link_clouds_prepare, then its launch).
    coords (T,K,7) f64, matrices (T,K,4,4) f64, points (N,3) f64 every frame's local cluster points packed frame-major
    with point_offsets (T*K+1) (host ints: cluster k of frame t is rows [off[t*K+k], off[t*K+k+1])).
    Returns (link_matrices (T,L,4,4) f32, mean_matrices (T,L,4,4) f32 or None, clouds_wf (M,3) f64, clouds_lf (M,3) f64,
    out_offsets (T*L+1) numpy int64: link l of frame t is rows [o[t*L+l], o[t*L+l+1]))."""
    launch, out = link_clouds_prepare(coords, matrices, link_clusters, points, point_offsets, mean_matrices)
    launch()
    return out


def link_clouds_prepare(coords: torch.Tensor, matrices: torch.Tensor, link_clusters, points: torch.Tensor, point_offsets,
                        mean_matrices: bool = False):
    """Checks, output sizing and device tables of link_clouds, done once: returns (launch, outputs), where launch() only
    enqueues creg_link_clouds_f64 on the current stream."""
    L_ = _lib.load()
    coords = _need(coords, torch.float64, "coords")
    matrices = _need(matrices, torch.float64, "matrices")
    points = _need(points, torch.float64, "points")
    if coords.dim() != 3 or coords.shape[2] != 7 or tuple(matrices.shape) != tuple(coords.shape[:2]) + (4, 4):
        raise ValueError("link_clouds: coords must be (T,K,7) and matrices (T,K,4,4)")
    T, K = coords.shape[:2]
    _max_clusters("link_clouds", K)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("link_clouds: points must be (N,3)")
    flat, off, _, _ = _link_tables("link_clouds", link_clusters, K, None)
    L = len(off) - 1
    po = np.asarray(point_offsets, np.int64)
    if po.shape != (T * K + 1,) or po[0] != 0 or np.any(np.diff(po) < 0) or po[-1] != points.shape[0]:
        raise ValueError("link_clouds: point_offsets must be (T*K+1) non-decreasing from 0 to len(points)")
    member = np.zeros((K, L), np.int64)                            # member[k, l]: times cluster k appears in link l
    np.add.at(member, (np.asarray(flat), np.repeat(np.arange(L), np.diff(off))), 1)
    per = np.diff(po).reshape(T, K) @ member                       # (T, L) rows of every (frame, link)
    oo = np.concatenate([[0], np.cumsum(per.reshape(-1))]).astype(np.int64)
    dev = coords.device
    n_out = int(oo[-1])
    lm = torch.empty(T, L, 4, 4, dtype=torch.float32, device=dev)
    mm = torch.empty(T, L, 4, 4, dtype=torch.float32, device=dev) if mean_matrices else None
    wf = torch.empty(max(n_out, 1), 3, dtype=torch.float64, device=dev)
    lf = torch.empty(max(n_out, 1), 3, dtype=torch.float64, device=dev)
    cl, lo = _i32_tables(dev, flat, off)                           # named: they must outlive the launch call
    po_d, oo_d = torch.from_numpy(po).to(dev), torch.from_numpy(oo).to(dev)
    args = (_p(coords), _p(matrices), T, K, _p(cl), _p(lo), len(flat), L, _p(points) if points.shape[0] else None,
            _p(po_d), int(po[-1]), _p(oo_d), n_out, int(per.max()), _p(lm), _p(mm), _p(wf), _p(lf))
    keep = (coords, matrices, points, cl, lo, po_d, oo_d)          # the tables must outlive every launch

    def launch():
        _lib.check(L_.creg_link_clouds_f64(*args, _stream()), "creg_link_clouds_f64")
        return keep
    return launch, (lm, mm, wf[:n_out], lf[:n_out], oo)


# ------------------------------------------------------------------------------ joint motion: positions, limits, replay
def link_poses(coords: torch.Tensor, link_clusters):
    """Every link's mean pose at every step in one launch of creg_link_poses_f64: coords (S,T,K,7) f64 [xyz, wxyz],
    link_clusters one cluster list per link (set order) -> link_T (S,T,L,4,4) f64, the pose creg_joint_axes_f64 works with
    (mean xyz, eigen-averaged quaternion), unrounded.  ValueError for K > 256, an empty link or a cluster outside [0, K)."""
    L_ = _lib.load()
    coords = _need(coords, torch.float64, "coords")
    if coords.dim() != 4 or coords.shape[3] != 7 or 0 in coords.shape[:3]:
        raise ValueError(f"link_poses: coords must be (S,T,K,7) with S, T, K >= 1, got {tuple(coords.shape)}")
    S, T, K = coords.shape[:3]
    _max_clusters("link_poses", K)
    dev = coords.device
    flat, off, cl, lo = _link_tables("link_poses", link_clusters, K, dev)
    L = len(off) - 1
    if L < 1 or S * T * L >= 2 ** 31:
        raise ValueError(f"link_poses: need 1 <= S*T*L < 2^31 (S={S}, T={T}, L={L})")
    link_T = torch.empty(S, T, L, 4, 4, dtype=torch.float64, device=dev)
    _lib.check(L_.creg_link_poses_f64(_p(coords), S, T, K, _p(cl), _p(lo), len(flat), L, _p(link_T), _stream()), "creg_link_poses_f64")
    return link_T


def joint_positions(link_T: torch.Tensor, joints, local_axis, local_pos, ref_seq: int = 0, ref_step: int = 0,
                    start_step: int = 0, num_steps=None):
    """Every joint's position at every step, its residuals against "one revolute axis through one point" and their
    per-joint summary (creg_joint_positions_f64).  link_T (S,T,L,4,4) f64 from ``link_poses``; joints (parent link, child
    link) pairs; local_axis (J,3) and local_pos (J,3 or 4) as ``joint_axes`` returns them (host arrays or f64 device
    tensors); the steps used are start_step .. start_step + num_steps - 1 (to the end when num_steps is None) and the
    position is zero at (ref_seq, ref_step).  Returns a dict of device tensors: q, tilt, slip (J,S,num_steps) f64; lower,
    upper, tilt_rms, tilt_max, slip_rms, slip_max (J) f64; n_used (J) int32; lower_at, upper_at (J,2) int32 = (sequence,
    step - start_step), -1 where n_used is 0.  IndexError for steps or a reference pose outside link_T, ValueError for
    shapes and link indices, all before any launch."""
    def axis_and_pos(J, ax, dev):
        lp = torch.as_tensor(local_pos, dtype=torch.float64, device=dev)
        if lp.numel() == 0:
            lp = lp.reshape(0, 4)
        if ax.shape[0] != J or lp.dim() != 2 or lp.shape[0] != J or (J and lp.shape[1] not in (3, 4)):
            raise ValueError(f"joint_positions: local_axis must be ({J},3) and local_pos ({J},3) or ({J},4), got "
                             f"{tuple(ax.shape)} and {tuple(lp.shape)}")
        if J and lp.shape[1] == 3:
            lp = torch.cat([lp, torch.ones(J, 1, dtype=torch.float64, device=dev)], dim=1)
        return (lp.contiguous(),)
    return _joint_series("joint_positions", "creg_joint_positions_f64", link_T, joints, local_axis, axis_and_pos, ref_seq, ref_step,
                         start_step, num_steps)


def _joint_series(who, entry, link_T, joints, local_axis, extra_args, ref_seq, ref_step, start_step, num_steps):
    """joint_positions and joint_slides but for their entry: the checks under ``who``'s name, the allocation, the call of
    ``entry`` and the output dict.  ``extra_args(J, ax, dev)`` checks the rows of local_axis, with whatever else the entry
    takes after it, and returns those further tensors."""
    L_ = _lib.load()
    link_T = _need(link_T, torch.float64, "link_T")
    if link_T.dim() != 5 or tuple(link_T.shape[3:]) != (4, 4) or 0 in link_T.shape[:3]:
        raise ValueError(f"{who}: link_T must be (S,T,L,4,4) with S, T, L >= 1, got {tuple(link_T.shape)}")
    S, T, L = link_T.shape[:3]
    dev = link_T.device
    jt = _joint_pairs(who, joints, L)
    J = len(jt)
    ax = _need(torch.as_tensor(local_axis, dtype=torch.float64, device=dev).reshape(-1, 3), torch.float64, "local_axis")
    extra = extra_args(J, ax, dev)
    start_step, ref_seq, ref_step = int(start_step), int(ref_seq), int(ref_step)
    num_steps = T - start_step if num_steps is None else int(num_steps)
    if start_step < 0 or num_steps < 1:
        raise ValueError(f"{who}: need start_step >= 0 and num_steps >= 1 (got {start_step}, {num_steps})")
    if start_step + num_steps > T:
        raise IndexError(f"index {start_step + num_steps - 1} is out of bounds for axis 1 with size {T}")
    if not 0 <= ref_seq < S:
        raise IndexError(f"index {ref_seq} is out of bounds for axis 0 with size {S}")
    if not 0 <= ref_step < T:
        raise IndexError(f"index {ref_step} is out of bounds for axis 1 with size {T}")
    if S > 65535 or S * num_steps >= 2 ** 31:
        raise ValueError(f"{who}: at most 65535 sequences and 2^31 samples per joint (S={S}, num_steps={num_steps})")
    f64 = dict(dtype=torch.float64, device=dev)
    q, tilt, slip = (torch.empty(J, S, num_steps, **f64) for _ in range(3))
    summary = torch.empty(J, 6, **f64)
    where = torch.empty(J, 5, dtype=torch.int32, device=dev)
    if J:
        jn = torch.tensor(jt, dtype=torch.int32, device=dev).reshape(-1, 2)
        _lib.check(getattr(L_, entry)(_p(link_T), S, T, L, _p(jn), J, _p(ax), *map(_p, extra), ref_seq, ref_step, start_step,
                                      num_steps, _p(q), _p(tilt), _p(slip), _p(summary), _p(where), _stream()), entry)
    out = {"q": q, "tilt": tilt, "slip": slip}
    for i, k in enumerate(("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")):
        out[k] = summary[:, i]
    out.update(n_used=where[:, 0], lower_at=where[:, 1:3], upper_at=where[:, 3:5])
    return out


def joint_slides(link_T: torch.Tensor, joints, local_axis, ref_seq: int = 0, ref_step: int = 0, start_step: int = 0,
                 num_steps=None):
    """``joint_positions`` for prismatic and fixed joints (creg_joint_slides_f64): q is the slide along local_axis (J,3), a
    unit vector in the child's frame, or zero for a fixed joint; tilt is the whole rotation of the child against the
    reference pose and slip the motion off the axis.  There is no local_pos and nothing is unwrapped.  Returns the dict
    ``joint_positions`` returns and raises what it raises."""
    def axis_alone(J, ax, dev):
        if ax.shape[0] != J:
            raise ValueError(f"joint_slides: local_axis must be ({J},3), got {tuple(ax.shape)}")
        return ()
    return _joint_series("joint_slides", "creg_joint_slides_f64", link_T, joints, local_axis, axis_alone, ref_seq, ref_step,
                         start_step, num_steps)


def motion_error(A, A0, B, B0, point):
    """How differently every link moved from its reference pose under two descriptions (creg_motion_error_f64): A, B (P,L,4,4),
    A0, B0 (L,4,4), point (L,3), f64 device tensors -> (rot_err (P,L) rad, pos_err (P,L)): the angle between A A0^-1 and
    B B0^-1 and the distance between the images of point[l] under the two.  ValueError for shapes before any launch."""
    L_ = _lib.load()
    A, A0, B, B0, point = (_need(t, torch.float64, n) for t, n in ((A, "A"), (A0, "A0"), (B, "B"), (B0, "B0"), (point, "point")))
    if A.dim() != 4 or tuple(A.shape[2:]) != (4, 4) or A.shape != B.shape or 0 in A.shape[:2] \
            or tuple(A0.shape) != tuple(A.shape[1:]) or A0.shape != B0.shape or tuple(point.shape) != (A.shape[1], 3):
        raise ValueError(f"motion_error: A, B (P,L,4,4), A0, B0 (L,4,4) and point (L,3) with P, L >= 1 expected, got "
                         f"{tuple(A.shape)}, {tuple(A0.shape)}, {tuple(B.shape)}, {tuple(B0.shape)}, {tuple(point.shape)}")
    P, L = A.shape[:2]
    if P * L >= 2 ** 31:
        raise ValueError(f"motion_error: P*L must stay below 2^31 (P={P}, L={L})")
    rot = torch.empty(P, L, dtype=torch.float64, device=A.device)
    pos = torch.empty(P, L, dtype=torch.float64, device=A.device)
    _lib.check(L_.creg_motion_error_f64(_p(A), _p(A0), _p(B), _p(B0), _p(point), P, L, _p(rot), _p(pos), _stream()),
               "creg_motion_error_f64")
    return rot, pos


# ------------------------------------------------------------------------------ N4 link meshing
MESH_MAX_NEIGHBORS = 32


def _mesh_inputs(points, offsets, what):
    points = _need(points, torch.float64, "points")
    offsets = _need(offsets, torch.int64, "offsets")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (n,3)")
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError(f"{what}: offsets must be (L+1) with L >= 1")
    off = offsets.cpu().numpy()
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != points.shape[0]:
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
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
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
    fws = torch.empty(max(fb, 1), dtype=torch.uint8, device=dev)
    _check_mesh(L_.creg_mesh_finish_f64(_p(verts_h) if V else None, V, _p(tris) if F else None, F, _p(voff), _p(toff), L, _p(origin),
                                        voxel_size, 1 if smooth else 0, _p(vertices) if V else None, _p(rec) if F else None,
                                        _p(fws), fb, st), "creg_mesh_finish_f64")
    origin_h = origin.cpu().numpy()
    return [dict(vertices=vertices[voff_h[l]:voff_h[l + 1]], verts_h=verts_h[voff_h[l]:voff_h[l + 1]],
                 triangles=tris[toff_h[l]:toff_h[l + 1]], stl_records=rec[toff_h[l]:toff_h[l + 1]],
                 origin=origin_h[l], dims=dims_h[l]) for l in range(L)]


HULL_MAX_COORD = 16383
HULL_STATUS = {0: "ok", 1: "fewer than 4 points", 2: "all points identical", 3: "all points collinear", 4: "all points coplanar",
               5: f"a coordinate beyond {HULL_MAX_COORD}", 6: "offsets are no range of the points", 7: "face slots exhausted",
               8: "round bound exhausted", 9: "a horizon that is no closed cycle"}


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
    if L < 1 or off_h[0] != 0 or np.any(np.diff(off_h) < 0) or off_h[-1] != n:
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
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
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


# ------------------------------------------------------------------------------ K5 row conversions
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


ICP_BATCH_MAX = 16


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


def _rows(fn_name, a, out_shape, b=None, out2_shape=None):
    L = _lib.load()
    a = _need(a, torch.float32, "input")
    k = a.shape[0]
    out = torch.empty((k,) + out_shape, dtype=torch.float32, device=a.device)
    fn = getattr(L, fn_name)
    if k == 0:                                   # an empty tensor's data pointer is null, which the C ABI rejects
        return (out, torch.empty((0,) + out2_shape, dtype=torch.float32, device=a.device)) if out2_shape is not None else out
    if out2_shape is not None:
        out2 = torch.empty((k,) + out2_shape, dtype=torch.float32, device=a.device)
        _lib.check(fn(_p(a), k, _p(out), _p(out2), _stream()), fn_name)
        return out, out2
    if b is not None:
        b = _need(b, torch.float32, "input")
        _lib.check(fn(_p(a), _p(b), k, _p(out), _stream()), fn_name)
    else:
        _lib.check(fn(_p(a), k, _p(out), _stream()), fn_name)
    return out


def se3_to_dq(M): return _rows("creg_se3_to_dq_f32", M, (8,))
def dq_to_se3(dq): return _rows("creg_dq_to_se3_f32", dq, (4, 4))
def dq_to_se3_bwd(dq, gM): return _rows("creg_dq_to_se3_bwd_f32", dq, (8,), b=gM)
def dq_multiply(a, b): return _rows("creg_dq_multiply_f32", a, (8,), b=b)
def dq_invert(dq): return _rows("creg_dq_invert_f32", dq, (8,))
def dq_to_quat_trans(dq): return _rows("creg_dq_to_quat_trans_f32", dq, (4,), out2_shape=(3,))
def quat_trans_to_dq(q, t): return _rows("creg_quat_trans_to_dq_f32", q, (8,), b=t)
def matrix_to_quat(R): return _rows("creg_matrix_to_quat_f32", R, (4,))
def quat_to_matrix(q): return _rows("creg_quat_to_matrix_f32", q, (3, 3))


# ------------------------------------------------------------------------------ A1 train plan
Q_PARAM_ORDER = ["encoder.0.weight", "encoder.0.bias", "decoder_1.0.weight", "decoder_1.0.bias",
                 "decoder_1.2.weight", "decoder_1.2.bias", "decoder_2.0.weight", "decoder_2.0.bias",
                 "decoder_2.2.weight", "decoder_2.2.bias"]
DQ_PARAM_ORDER = ["encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias",
                  "decoder.2.weight", "decoder.2.bias"]
#: creg_train_shape.rot: the reference's four --r choices (mlp_reg.py:64-90).  RRegMLP ('6d') and RegMLP ('rpy') name their
#: tensors like QRegMLP (model_utils.py:170-281): Q_PARAM_ORDER serves the three.
TRAIN_ROT = {"q": 0, "dq": 1, "6d": 2, "rpy": 3}
#: per rot: (input features of the encoder = 8 x the pose row's width, outputs of decoder_2)
_TWO_DECODER = {0: (56, 4), 2: (72, 6), 3: (48, 3)}


TRAIN_HIDDEN_TILES = (64, 128, 256, 512)      # widths the train kernels are instantiated for


def icp_nn_counters(reset: bool = False, timing=None) -> dict:
    """Work counters / launch timing of the many-workgroup ICP search (creg_icp_nn_counters; a measurement hook, synchronises)."""
    out = (ctypes.c_double * 8)()
    L = _lib.load()
    _lib.check(L.creg_icp_nn_counters(out, 1 if reset else 0, -1 if timing is None else int(bool(timing))), "creg_icp_nn_counters")
    keys = ("waves", "f32_trips", "f64_trips", "source_iterations", "tie_rescans", "nn_launch_us_total", "nn_launches_timed")
    return dict(zip(keys, [float(v) for v in out]))


class TrainPlan:
    """Device-resident `train` loop (mlp_reg.py:17-152) for one (rot, K, hidden, N) shape.

    `hidden` may be any width up to 512, like the reference's models (model_utils.py:65-168): a width the kernels are not
    instantiated for runs on the next one that is, with the extra units' weights and biases zero.  Such a unit's activation is
    exactly 0 (LeakyReLU / ReLU of 0), it adds exactly 0 to every sum it enters, and every gradient of its parameters is a
    product with that 0 or with the zero column that leads out of it -- so Adam leaves them at 0 and the trained model, losses
    and poses are those of the unpadded model; the caller's tensors keep their own shapes.

    `rot`: 'q' / 'dq' / '6d' / 'rpy' -- the reference's four --r choices (mlp_reg.py:64-90); `params` in Q_PARAM_ORDER (DQ_PARAM_ORDER
    for 'dq').  `graph_branches`: creg_train_shape.graph_branches (include/creg.h) -- 0 = chain streams, the library's count."""

    def __init__(self, rot: str, k: int, hidden: int, n_pred: int, n_tgt: int, epochs: int = 300,
                 use_graph: bool = True, device=None, batch: int = 1, graph_branches: int = 0,
                 nn_search: int = 0):
        self.L = _lib.load()
        self.rot = TRAIN_ROT[rot]
        self.device = _lib.device(torch.device(device) if device is not None else None)
        self.batch = int(batch)
        self.hidden_model = int(hidden)                                     # the caller's width
        if hidden < 2 or hidden > TRAIN_HIDDEN_TILES[-1]:
            raise ValueError(f"unsupported train shape: hidden {hidden} (2 .. {TRAIN_HIDDEN_TILES[-1]})")
        hidden = next(t for t in TRAIN_HIDDEN_TILES if t >= hidden)         # the width the kernels run at
        self.shape = _lib.TrainShape(self.rot, k, hidden, epochs, n_pred, n_tgt, int(use_graph), self.batch,
                                     int(graph_branches), int(nn_search))
        need = self.L.creg_train_workspace_bytes(ctypes.byref(self.shape))
        if need == 0:
            raise ValueError(f"unsupported train shape (rot {rot!r}, k = {k}, hidden {hidden}): the plan takes 1 <= k <= 256 clusters (fewer for --r 6d at hidden 512: the backward's LDS tiles) "
                             "and hidden widths up to 512 (include/creg.h, creg_train_shape)")
        self.ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = (self.ws.data_ptr() + 255) // 256 * 256
        self.plan = ctypes.c_void_p()
        _lib.check(self.L.creg_train_plan_create(ctypes.byref(self.shape), ctypes.c_void_p(base), need,
                                                 ctypes.byref(self.plan)), "creg_train_plan_create")
        self.k, self.n_pred, self.n_tgt, self.epochs, self.hidden = k, n_pred, n_tgt, epochs, hidden
        info = (ctypes.c_int32 * 9)()
        _lib.check(self.L.creg_train_plan_info(self.plan, info), "creg_train_plan_info")
        #: what the plan chose from its shape (never a result): searches, graph branches, problems per launch, epochs per graph
        self.info = {"pruned_target_search": bool(info[0]), "pruned_predicted_search": bool(info[1]), "graph_branches": int(info[2]),
                     "batch": int(info[3]), "epochs_per_graph": int(info[4]), "nn_points_per_lane": int(info[5]),
                     "nn_boxes_per_lane": (int(info[6]), int(info[7])), "nn_queries_per_wave": 16 if int(info[0]) == 2 else 4}
        if nn_search == 0 and not (self.info["pruned_target_search"] and self.info["pruned_predicted_search"]):
            import warnings
            which = [d for d, on in (("predicted -> target", self.info["pruned_target_search"]),
                                     ("target -> predicted", self.info["pruned_predicted_search"])) if not on]
            warnings.warn(f"creg train plan (k={k}, n_pred={n_pred}, n_tgt={n_tgt}): exhaustive nearest-neighbour search in the "
                          f"{' and '.join(which)} direction(s) -- the shape is beyond the block-pruned search's limits "
                          "(n_tgt <= 65536: four chunks of k-d leaves built in LDS; n_pred < 65535 and at most 512 blocks of the padded "
                          "predicted cloud); same results, several times the launch time", RuntimeWarning, stacklevel=2)

    def chain_probe_us(self) -> int:
        """creg_train_plan_info_t.chain_probe_us AFTER a run: < 250 = the chain streams ran concurrently with the caller's (own hardware queues),
        -1 = a chain shares a queue, 0 = not probed (one chain / no run yet)."""
        info = (ctypes.c_int32 * 9)()
        _lib.check(self.L.creg_train_plan_info(self.plan, info), "creg_train_plan_info")
        return int(info[8])

    def __del__(self):
        plan = getattr(self, "plan", None)
        if plan is not None and plan.value and ctypes is not None:      # (module globals may be gone at interpreter exit)
            self.L.creg_train_plan_destroy(plan)
            self.plan = None

    def _args(self, m, y, pts, offsets, params, lr, factor, patience, stop, outs):
        n = 6 if self.rot == 1 else 10
        if len(params) != n:
            raise ValueError(f"expected {n} parameter tensors, got {len(params)}")
        keep = [_need(m, torch.float32, "m"), _need(y, torch.float32, "y"), _need(pts, torch.float32, "pts"),
                _need(offsets, torch.int32, "offsets")]
        # the kernels index with the PLAN's sizes: a tensor of another shape would be read out of bounds, not rejected
        if tuple(keep[0].shape) != (self.k, 4, 4):
            raise ValueError(f"m must be ({self.k},4,4) for this plan, got {tuple(keep[0].shape)}")
        if tuple(keep[1].shape) != (self.n_tgt, 3):
            raise ValueError(f"y must be ({self.n_tgt},3) for this plan, got {tuple(keep[1].shape)}")
        if tuple(keep[2].shape) != (self.n_pred, 3):
            raise ValueError(f"pts must be ({self.n_pred},3) for this plan, got {tuple(keep[2].shape)}")
        if keep[3].numel() != self.k + 1:
            raise ValueError(f"offsets must hold {self.k + 1} entries, got {keep[3].numel()}")
        shapes_model = self._param_shapes(self.hidden_model)
        for p, want in zip(params, shapes_model):
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise TypeError("model parameters must be contiguous fp32 CUDA tensors")
            if p.numel() != int(np.prod(want)):
                raise ValueError(f"parameter tensor of {p.numel()} elements where the plan's model has {int(np.prod(want))}")
        self._padded = None
        if self.hidden_model != self.hidden:                                # zero-padded copies at the kernels' width (class docstring)
            padded = []
            for p, sm, sp in zip(params, shapes_model, self._param_shapes(self.hidden)):
                q = torch.zeros(sp, dtype=torch.float32, device=p.device)
                q[tuple(slice(0, d) for d in sm)] = p.view(sm)
                padded.append(q)
            self._padded = (padded, list(params), shapes_model)
            params = padded
        arr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in params])
        self._keep = getattr(self, "_keep", [])[-64:] + [keep, arr, params]      # alive until the enqueued work has read them
        a = _lib.TrainArgs()
        a.m, a.y, a.local_pts, a.seg_offsets = [t.data_ptr() for t in keep]
        a.params = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        a.lr, a.sched_factor, a.sched_patience, a.stop = lr, factor, patience, stop
        a.best_m, a.best_pred, a.loss_hist, a.lr_hist, a.result = [o.data_ptr() if o is not None else None for o in outs]
        return a

    def _param_shapes(self, H):
        """Shapes of the model's tensors in Q_PARAM_ORDER / DQ_PARAM_ORDER at width H (model_utils.py:65-168)."""
        if self.rot != 1:      # QRegMLP: enc 56->H, dec1 H->H/2->3, dec2 H->H->4; RRegMLP: 72 features, 6 outputs; RegMLP: 48, 3 (+ Tanh)
            nin, nout = _TWO_DECODER[self.rot]
            return [(H, nin), (H,), (H // 2, H), (H // 2,), (3, H // 2), (3,), (H, H), (H,), (nout, H), (nout,)]
        return [(H, 64), (H,), (H, H), (H,), (8, H), (8,)]        # DQRegMLP: enc 64->H, H->H, H->8

    def _param_numels(self):
        """Element counts of the model's tensors at the kernels' width."""
        return [int(np.prod(s)) for s in self._param_shapes(self.hidden)]

    def _unpad(self, padded):
        """Trained parameters back into the caller's tensors (stream-ordered copies of the leading blocks)."""
        if padded is not None:
            for q, p, sm in zip(*padded):
                p.view(sm).copy_(q[tuple(slice(0, d) for d in sm)])

    def _outs(self):
        dev = self.device
        return (torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev),
                torch.empty(self.n_pred, 3, dtype=torch.float32, device=dev),
                torch.empty(self.epochs, dtype=torch.float32, device=dev),
                torch.empty(self.epochs, dtype=torch.float32, device=dev),
                torch.empty(4, dtype=torch.float32, device=dev))

    def run(self, m, y, pts, offsets, params, lr=2e-4, factor=0.7, patience=5, stop=200, same_target=False):
        """Returns (best_m (k,4,4), best_pred (n_pred,3), result (4) = [min_loss, epochs_run, lr,
        best_epoch], loss_hist (epochs), lr_hist (epochs)); all device tensors, stream-ordered."""
        return self.run_batch([(m, y, pts, offsets, params)], lr, factor, patience, stop, same_target)[0]

    def run_batch(self, problems, lr=2e-4, factor=0.7, patience=5, stop=200, same_target=False):
        """problems: list of `batch` tuples (m, y, pts, offsets, params) of identical shape, advanced
        together (one launch carries all of them).  Returns one result tuple per problem, as `run`.
        same_target: the caller vouches that every problem's `y` holds the values of this plan's previous run of that slot
        ("Anchor" after "Step" on the same frame, mlp_reg.py:338-356): the frame's k-d leaf blocks are kept instead of rebuilt."""
        if len(problems) != self.batch:
            raise ValueError(f"this plan advances {self.batch} problems per launch, got {len(problems)}")
        arr = (_lib.TrainArgs * self.batch)()
        outs, padded = [], []
        for b, (m, y, pts, offsets, params) in enumerate(problems):
            best_m, best_pred, lh, lrh, result = o = self._outs()
            arr[b] = self._args(m, y, pts, offsets, params, lr, factor, patience, stop, o)
            arr[b].y_unchanged = 1 if same_target else 0
            padded.append(self._padded)
            outs.append((best_m, best_pred, result, lh, lrh))
        _lib.check(self.L.creg_train_plan_run_batch(self.plan, arr, self.batch, _stream()), "creg_train_plan_run_batch")
        for pd in padded:
            self._unpad(pd)
        return outs

    #: scalar fields of a train's control state (creg_train_state; `state_out` of creg_train_plan_resume holds them in this order + last_loss)
    STATE_FIELDS = ("step", "epochs_run", "lr", "sched_best", "sched_bad", "count", "min_loss", "best_epoch", "stopped")

    def resume(self, m, y, pts, offsets, params, state, n_epochs=1, factor=0.7, patience=5, stop=200, best=None):
        """`n_epochs` further epochs of one train from a caller-supplied optimizer / control state (creg_train_plan_resume): checkpoint /
        resume, and the teacher-forced parity hook.  `state`: dict with `exp_avg`, `exp_avg_sq` (lists of fp32 CUDA tensors shaped like
        `params`: torch.optim.Adam's moments) and the scalars of STATE_FIELDS (missing ones default to a fresh train's).  `best`:
        (best_m (k,4,4), best_pred (n_pred,3)) so far, required when state['best_epoch'] >= 0.  `params` are updated in place.
        Returns (best_m, best_pred, result, loss_hist, lr_hist, state_after) -- state_after like `state`, its scalars read back
        (synchronises the stream for them)."""
        if self.hidden_model != self.hidden:
            raise ValueError("resume needs the model at one of the kernels' widths (64, 128, 256, 512): no zero-padding of the moments")
        n = 6 if self.rot == 1 else 10
        ea, es = list(state["exp_avg"]), list(state["exp_avg_sq"])
        if len(ea) != n or len(es) != n:
            raise ValueError(f"expected {n} moment tensors of each kind")
        for q, p in zip(ea + es, list(params) * 2):
            if not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.numel() == p.numel()):
                raise TypeError("Adam moments must be contiguous fp32 CUDA tensors shaped like the parameters")
        o = self._outs()
        best_epoch = int(state.get("best_epoch", -1))
        if best_epoch >= 0:
            if best is None:
                raise ValueError("state['best_epoch'] >= 0 needs best=(best_m, best_pred)")
            o[0].copy_(best[0]); o[1].copy_(best[1])
        a = self._args(m, y, pts, offsets, params, float(state.get("lr", 2e-4)), factor, patience, stop, o)
        st = _lib.TrainState()
        arr_a = (ctypes.c_void_p * n)(*[q.data_ptr() for q in ea])
        arr_s = (ctypes.c_void_p * n)(*[q.data_ptr() for q in es])
        st.exp_avg, st.exp_avg_sq = ctypes.cast(arr_a, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(arr_s, ctypes.POINTER(ctypes.c_void_p))
        st.lr, st.sched_best = float(state.get("lr", 2e-4)), float(state.get("sched_best", float("inf")))
        st.step, st.epochs_run = int(state.get("step", 0)), int(state.get("epochs_run", state.get("step", 0)))
        st.sched_bad, st.count, st.best_epoch, st.stopped = int(state.get("sched_bad", 0)), int(state.get("count", 0)), best_epoch, int(state.get("stopped", 0))
        st.min_loss = float(state.get("min_loss", 1000.0))
        ea2, es2 = [torch.empty_like(q) for q in ea], [torch.empty_like(q) for q in es]
        out_a = (ctypes.c_void_p * n)(*[q.data_ptr() for q in ea2])
        out_s = (ctypes.c_void_p * n)(*[q.data_ptr() for q in es2])
        sc = torch.empty(12, dtype=torch.float64, device=self.device)
        _lib.check(self.L.creg_train_plan_resume(self.plan, ctypes.byref(a), ctypes.byref(st), int(n_epochs),
                                                 ctypes.cast(out_a, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(out_s, ctypes.POINTER(ctypes.c_void_p)),
                                                 _p(sc), _stream()), "creg_train_plan_resume")
        h = sc.cpu().tolist()
        after = {"exp_avg": ea2, "exp_avg_sq": es2, "last_loss": h[9]}
        for i, k in enumerate(self.STATE_FIELDS):
            after[k] = h[i] if k in ("lr", "sched_best", "min_loss") else int(h[i])
        return o[0], o[1], o[4], o[2], o[3], after

    def probe(self, m, y, pts, offsets, params):
        """One forward + pose-gradient evaluation (test hook): (m2, pred, loss, grad_m2)."""
        dev = self.device
        m2 = torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev)
        pred = torch.empty(self.n_pred, 3, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gm = torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev)
        a = self._args(m, y, pts, offsets, params, 2e-4, 0.7, 5, 200, (None, None, None, None, None))
        _lib.check(self.L.creg_train_plan_probe(self.plan, ctypes.byref(a), _p(m2), _p(pred), _p(loss), _p(gm),
                                                _stream()), "creg_train_plan_probe")
        return m2, pred, loss, gm

    KERNELS = ("_", "head", "nn_l1", "gradc", "bd", "l2")

    def profile(self, m, y, pts, offsets, params, n_epochs=50):
        """Average event-bracketed microseconds of each of the 5 epoch kernels, and the back-to-back launch time of each
        (synchronises; the plan's copy of the parameters moves on, the caller's tensors are not written)."""
        out = (ctypes.c_float * 16)()
        a = self._args(m, y, pts, offsets, params, 2e-4, 0.7, 5, 200, (None, None, None, None, None))
        _lib.check(self.L.creg_train_plan_profile(self.plan, ctypes.byref(a), n_epochs, out, _stream()),
                   "creg_train_plan_profile")
        d = dict(zip(self.KERNELS, [float(v) for v in out]))
        d.pop("_")
        d["nn_l1_back_to_back"] = float(out[6])
        d["nn_l1_problems_per_launch"] = int(out[7])
        d["bd_back_to_back"] = float(out[8])
        d["l2_back_to_back"] = float(out[9])
        d["head_back_to_back"] = float(out[10])
        d["gradc_back_to_back"] = float(out[11])
        return d
