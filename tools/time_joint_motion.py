"""Time the three joint-motion entry points (creg_link_poses_f64, creg_joint_positions_f64, creg_motion_error_f64) on the GPU.
Event-timed back-to-back calls on device inputs built once, per shape (K clusters in 6 links, 5 joints in a chain, S sequences
of T steps; random poses, which cost what real ones cost):

* each entry through the C ABI with its arguments built beforehand, and through its ops wrapper (checks, tables, allocations);
* the yardstick, timed the same way on the same device input: a torch restatement of the same arithmetic -- batched eigh for
  the mean quaternion, whole-array rotation algebra, the unwrap as a cumulative sum of wrapped differences, min / max / sum
  reductions -- and the largest difference of its outputs from the kernels'.

Warm-up: every callable runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the (min, max) beside it.  All three launches are latency-bound: no throughput is derived.

    python tools/time_joint_motion.py [--repeats 5] [--min_ms 200]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autourdf_amd import _lib, ops  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
SHAPES = ((20, 5, 10), (45, 5, 10), (20, 5, 500))       # (K, S, T)
N_LINKS = 6


def event_ms(fn, repeats, min_ms):
    """Median and (min, max) milliseconds per call of fn over `repeats` windows of at least min_ms each."""
    fn()
    torch.cuda.synchronize()
    reps, out = 1, []
    while len(out) < repeats:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms < min_ms and reps < (1 << 20):
            reps = max(reps * 2, int(reps * min_ms / max(ms, 1e-3)) + 1)
            continue
        out.append(ms / reps)
    return [round(float(np.median(out)), 5), round(float(min(out)), 5), round(float(max(out)), 5)]


# ---- the torch restatement ---------------------------------------------------------------------------------------
def quat_to_matrix(q):
    w, x, y, z = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    return torch.stack([1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
                        s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w),
                        s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def torch_link_poses(coords, clusters):
    out = torch.zeros(coords.shape[:2] + (len(clusters), 4, 4), dtype=torch.float64, device=coords.device)
    for l, idx in enumerate(clusters):
        c = coords[:, :, idx]
        q = c[..., 3:]
        A = torch.einsum("stka,stkb->stab", q, q) / len(idx)
        out[:, :, l, :3, :3] = quat_to_matrix(torch.linalg.eigh(A)[1][..., -1])
        out[:, :, l, :3, 3] = c[..., :3].mean(2)
    out[..., 3, 3] = 1.0
    return out


def rigid_inv(M):
    out = torch.zeros_like(M)
    Rt = M[..., :3, :3].transpose(-1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ M[..., :3, 3:]).squeeze(-1)
    out[..., 3, 3] = 1.0
    return out


def skew_and_cos(R):
    v = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return v, (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0) * 0.5


def rotation(a, x):
    """Rot(a, x) for a (J,3) and x (J,S,n)."""
    K = torch.zeros(a.shape[0], 3, 3, dtype=a.dtype, device=a.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    K, KK = K[:, None, None], (K @ K)[:, None, None]
    eye = torch.eye(3, dtype=a.dtype, device=a.device)
    return eye + torch.sin(x)[..., None, None] * K + (1 - torch.cos(x))[..., None, None] * KK


def torch_joint_positions(link_T, joints, axis, pos):
    par, chi = joints[:, 0].long(), joints[:, 1].long()
    X = (rigid_inv(link_T[:, :, par]) @ link_T[:, :, chi]).permute(2, 0, 1, 3, 4)          # (J,S,T,4,4)
    D = rigid_inv(X[:, :1, :1]) @ X
    R = D[..., :3, :3]
    v, c = skew_and_cos(R)
    w = torch.atan2((v * axis[:, None, None]).sum(-1), c)
    d = w[..., 1:] - w[..., :-1]
    q = torch.cat([w[..., :1], w[..., :1] + torch.cumsum(d - 2 * math.pi * torch.round(d / (2 * math.pi)), -1)], -1)
    ve, ce = skew_and_cos(rotation(axis, -w) @ R)
    tilt = torch.atan2(ve.norm(dim=-1), ce)
    pt = pos[:, None, None, :3, None]
    slip = ((R @ pt).squeeze(-1) + D[..., :3, 3] - pt.squeeze(-1)).norm(dim=-1)
    flat = lambda t: t.reshape(t.shape[0], -1)
    summary = torch.stack([flat(q).min(1)[0], flat(q).max(1)[0], (flat(tilt) ** 2).mean(1).sqrt(), flat(tilt).max(1)[0],
                           (flat(slip) ** 2).mean(1).sqrt(), flat(slip).max(1)[0]], 1)
    return q, tilt, slip, summary


def torch_motion_error(A, A0, B, B0, point):
    Ma, Mb = A @ rigid_inv(A0), B @ rigid_inv(B0)
    v, c = skew_and_cos(Ma[..., :3, :3].transpose(-1, -2) @ Mb[..., :3, :3])
    x = torch.cat([point, torch.ones_like(point[:, :1])], 1)[..., None]
    return torch.atan2(v.norm(dim=-1), c), ((Ma @ x) - (Mb @ x)).squeeze(-1)[..., :3].norm(dim=-1)


# ---- one shape ---------------------------------------------------------------------------------------------------
def time_shape(K, S, T, args):
    L, dev = _lib.load(), _lib.device()
    g = torch.Generator(device="cpu").manual_seed(K * 1000 + T)
    coords = torch.randn(S, T, K, 7, generator=g, dtype=torch.float64)
    coords[..., 3:] /= coords[..., 3:].norm(dim=-1, keepdim=True)
    coords = coords.to(dev)
    bounds = np.linspace(0, K, N_LINKS + 1).astype(int)
    clusters = [list(range(bounds[l], bounds[l + 1])) for l in range(N_LINKS)]
    pairs = [(l, l + 1) for l in range(N_LINKS - 1)]
    J = len(pairs)
    axis = torch.randn(J, 3, generator=g, dtype=torch.float64)
    axis = (axis / axis.norm(dim=1, keepdim=True)).to(dev)
    pos = torch.cat([torch.randn(J, 3, generator=g, dtype=torch.float64) * 0.1, torch.ones(J, 1, dtype=torch.float64)], 1).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    cl = torch.tensor([k for c in clusters for k in c], **i32)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in clusters])]), **i32)
    jn = torch.tensor(pairs, **i32)
    link_T = torch.empty(S, T, N_LINKS, 4, 4, **f64)
    q, tilt, slip = (torch.empty(J, S, T, **f64) for _ in range(3))
    summary, where = torch.empty(J, 6, **f64), torch.empty(J, 5, **i32)
    poses = lambda: _lib.check(L.creg_link_poses_f64(p(coords), S, T, K, p(cl), p(off), K, N_LINKS, p(link_T), stream), "link_poses")
    positions = lambda: _lib.check(L.creg_joint_positions_f64(p(link_T), S, T, N_LINKS, p(jn), J, p(axis), p(pos), 0, 0, 0, T, p(q), p(tilt),
                                                              p(slip), p(summary), p(where), stream), "joint_positions")
    res = {"K": K, "S": S, "T": T, "links": N_LINKS, "joints": J}
    res["creg_link_poses_ms"] = event_ms(poses, args.repeats, args.min_ms)
    res["creg_joint_positions_ms"] = event_ms(positions, args.repeats, args.min_ms)
    A = link_T.reshape(S * T, N_LINKS, 4, 4)
    B = A.roll(1, 0).contiguous()
    A0, B0, point = A[0].contiguous(), B[0].contiguous(), A[0, :, :3, 3].contiguous()
    rot, err = torch.empty(S * T, N_LINKS, **f64), torch.empty(S * T, N_LINKS, **f64)
    motion = lambda: _lib.check(L.creg_motion_error_f64(p(A), p(A0), p(B), p(B0), p(point), S * T, N_LINKS, p(rot), p(err), stream),
                                "motion_error")
    res["creg_motion_error_ms"] = event_ms(motion, args.repeats, args.min_ms)
    res["ops_link_poses_ms"] = event_ms(lambda: ops.link_poses(coords, clusters), args.repeats, args.min_ms)
    res["ops_joint_positions_ms"] = event_ms(lambda: ops.joint_positions(link_T, pairs, axis, pos), args.repeats, args.min_ms)
    res["ops_motion_error_ms"] = event_ms(lambda: ops.motion_error(A, A0, B, B0, point), args.repeats, args.min_ms)
    res["torch_link_poses_ms"] = event_ms(lambda: torch_link_poses(coords, clusters), args.repeats, args.min_ms)
    res["torch_joint_positions_ms"] = event_ms(lambda: torch_joint_positions(link_T, jn, axis, pos), args.repeats, args.min_ms)
    res["torch_motion_error_ms"] = event_ms(lambda: torch_motion_error(A, A0, B, B0, point), args.repeats, args.min_ms)
    for k in ("link_poses", "joint_positions", "motion_error"):
        res[f"torch_over_creg_{k}"] = round(res[f"torch_{k}_ms"][0] / res[f"creg_{k}_ms"][0], 2)
    # eigh fixes the mean quaternion up to a sign, the rotation does not care
    tq, tt, ts, tsum = torch_joint_positions(link_T, jn, axis, pos)
    trot, terr = torch_motion_error(A, A0, B, B0, point)
    res["max_difference"] = {"link_poses": float((torch_link_poses(coords, clusters) - link_T).abs().max()),
                             "q": float((tq - q).abs().max()), "tilt": float((tt - tilt).abs().max()),
                             "slip": float((ts - slip).abs().max()), "summary": float((tsum - summary).abs().max()),
                             "rot_err": float((trot - rot).abs().max()), "pos_err": float((terr - err).abs().max())}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/time_joint_motion.py measures on an MI355X: no GPU is visible")
    for K, S, T in SHAPES:
        time_shape(K, S, T, args)


if __name__ == "__main__":
    main()
