"""N2 / N4 URDF stage: pose distance maps, link discovery, the tree, joint axes / types / motion and link clouds."""
import numpy as np

import torch

from .. import _lib
from ._common import _host_offsets_ok, _need, _p, _stream, _workspace

LINK_SWEEP_MAX_K = 256
# csrc/joints_dev.h holds the same limits as JOINT_MAX_K (LINK_SWEEP_MAX_K here), JOINT_MAX_SAMPLES and JOINT_THETA_MIN
JOINT_MAX_SAMPLES = 4096
JOINT_THETA_MIN = 2e-4             # rad: a sample below it is not usable (creg.h)


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
    ws = _workspace(M.device, max(ws_bytes, 256))                  # never below 256 bytes, and the entry is told the buffer's own size
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
    if po.shape != (T * K + 1,) or not _host_offsets_ok(po, points.shape[0]):
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
