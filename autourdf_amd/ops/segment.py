"""K2: k-means (Lloyd, one frame or a batch), assignment, grouping into cluster frames, and the normals of `--normal`."""
import torch

from .. import _lib
from ._common import _need, _p, _ptr_array, _stream, _workspace

KMEANS_ND_MAX_N, KMEANS_ND_MAX_K = (1 << 24) - 1, 128      # creg_kmeans_lloyd_nd_f64: one workgroup, centres in LDS (labels too up to 16384 points, in the workspace above)
KMEANS_BATCH_MAX_N = 16384         # labels + centres in one CU's LDS; the frame too up to 5120 points, from L2 above
KMEANS_BATCH_MAX, KMEANS_BATCH_MAX_K = 16, 128             # frames per launch (KMS_MAXB in kmeans.hip), centres in LDS
GROUP_BATCH_MAX = 16


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
    ws = _workspace(X.device, ws_bytes)
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
    ws = _workspace(X.device, ws_bytes)
    centers = torch.empty(k, d, dtype=torch.float64, device=X.device)
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    inertia = torch.empty(1, dtype=torch.float64, device=X.device)
    n_iter = torch.empty(1, dtype=torch.int32, device=X.device)
    _lib.check(L.creg_kmeans_lloyd_nd_f64(_p(X), n, d, _p(init), k, max_iter, tol, _p(centers), _p(labels), _p(inertia), _p(n_iter),
                                          _p(ws), ws_bytes, _stream()), "creg_kmeans_lloyd_nd_f64")
    return centers, labels, inertia, n_iter


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
    ws = _workspace(dev, ws_bytes)
    outs = [(torch.empty(k, 3, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
             torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)) for _ in range(B)]
    _lib.check(L.creg_kmeans_lloyd_batch_f64(_ptr_array(Xs), n, _ptr_array(inits), k, B, max_iter, tol, *map(_ptr_array, zip(*outs)),
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
    _lib.check(L.creg_group_to_local_batch_f64(_ptr_array(Xs), n, _ptr_array(labels), k, _ptr_array(Ms), int(bool(m_is_inverse)), B,
                                               *map(_ptr_array, zip(*outs)), _stream()), "creg_group_to_local_batch_f64")
    return outs


def group_to_local_each(Xs, labels, Ms, m_is_inverse: bool = False):
    """`group_to_local_batch` where the frames fit one pair of launches, `group_to_local` per frame, in order, otherwise."""
    if _batchable(GROUP_BATCH_MAX, Xs, labels, Ms):
        return group_to_local_batch(Xs, labels, Ms, m_is_inverse=m_is_inverse)
    return [group_to_local(X, l, M, m_is_inverse=m_is_inverse) for X, l, M in zip(Xs, labels, Ms)]


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
