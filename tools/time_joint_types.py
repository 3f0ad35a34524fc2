"""Time the two joint-type entry points (creg_joint_types_f64, creg_joint_slides_f64) on the GPU, in the manner of
tools/time_joint_motion.py and at its three shapes (K clusters in 6 links, 5 joints in a chain, S sequences of T steps;
random poses, which cost what real ones cost; interval 4, as main() passes):

* each entry through the C ABI with its arguments built beforehand, and through its ops wrapper (checks, tables, allocations);
* the yardstick, timed the same way on the same device input: a torch restatement of the same arithmetic -- batched eigh for
  the mean quaternions, whole-array rigid algebra, one 3x3 eigh per joint, min / max / sum reductions -- and the largest
  difference of its outputs from the kernels'.

creg_joint_types_f64 runs with turn_min above pi and slide_min 0, so every sample is a slide and the whole path runs: the
six sums, the eigenvector and its sign.  Warm-up, windows and medians as in tools/time_joint_motion.py.  Both entries are
latency-bound launches: no throughput is derived.

    python tools/time_joint_types.py [--repeats 5] [--min_ms 200]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from autourdf_amd import _lib, ops  # noqa: E402
from time_joint_motion import N_LINKS, SHAPES, event_ms, p, rigid_inv, skew_and_cos, torch_link_poses  # noqa: E402

INTERVAL, TURN_MIN, SLIDE_MIN = 4, 4.0, 0.0


def sample_index(T, interval, dev):
    """(step_prev, step) of one sequence's samples in the kernel's order: phase, then step."""
    i1 = [a + k * interval for a in range(interval) for k in range(1, len(range(a, T, interval)))]
    i1 = torch.tensor(i1, dtype=torch.long, device=dev)
    return i1 - interval, i1


def torch_joint_types(coords, clusters, joints, i0, i1, turn_min, slide_min):
    link_T = torch_link_poses(coords, clusters)
    par, chi = joints[:, 0].long(), joints[:, 1].long()
    X = (rigid_inv(link_T[:, :, par]) @ link_T[:, :, chi]).permute(2, 0, 1, 3, 4)          # (J,S,T,4,4)
    D = (rigid_inv(X[:, :, i0]) @ X[:, :, i1]).reshape(X.shape[0], -1, 4, 4)               # (J,NS,4,4), sequence-major
    v, c = skew_and_cos(D[..., :3, :3])
    theta, t = torch.atan2(v.norm(dim=-1), c), D[..., :3, 3]
    turn = theta >= turn_min
    slide = ~turn & (t.norm(dim=-1) >= slide_min)
    kind = torch.where(turn, 1, torch.where(slide, 2, 0)).int()
    counts = torch.stack([(kind == 0).sum(1), turn.sum(1), slide.sum(1), torch.zeros_like(turn.sum(1))], 1).int()
    ts = t * slide[..., None]
    a = torch.linalg.eigh(torch.einsum("jna,jnb->jab", ts, ts))[1][..., -1]
    first = t[torch.arange(t.shape[0]), slide.int().argmax(1)]
    a = a * torch.where((a * first).sum(-1) < 0, -1.0, 1.0)[:, None]
    return theta, t, kind, counts, a, (link_T[0, 0, chi, :3, :3] @ a[..., None]).squeeze(-1)


def torch_joint_slides(link_T, joints, axis):
    par, chi = joints[:, 0].long(), joints[:, 1].long()
    X = (rigid_inv(link_T[:, :, par]) @ link_T[:, :, chi]).permute(2, 0, 1, 3, 4)
    D = rigid_inv(X[:, :1, :1]) @ X
    v, c = skew_and_cos(D[..., :3, :3])
    d = D[..., :3, 3]
    q = (d * axis[:, None, None]).sum(-1)
    tilt = torch.atan2(v.norm(dim=-1), c)
    slip = (d - q[..., None] * axis[:, None, None]).norm(dim=-1)
    flat = lambda x: x.reshape(x.shape[0], -1)
    summary = torch.stack([flat(q).min(1)[0], flat(q).max(1)[0], (flat(tilt) ** 2).mean(1).sqrt(), flat(tilt).max(1)[0],
                           (flat(slip) ** 2).mean(1).sqrt(), flat(slip).max(1)[0]], 1)
    return q, tilt, slip, summary


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
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    cl = torch.tensor([k for c in clusters for k in c], **i32)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in clusters])]), **i32)
    jn = torch.tensor(pairs, **i32)
    NS = ops.joint_samples(S, T, INTERVAL)
    angle, slide, kind = torch.empty(J, NS, **f64), torch.empty(J, NS, 3, **f64), torch.empty(J, NS, **i32)
    counts, kinds = torch.empty(J, 4, **i32), torch.empty(J, **i32)
    s_axis, g_axis, g_pos = (torch.empty(J, 3, **f64) for _ in range(3))
    link_T = ops.link_poses(coords, clusters)
    q, tilt, slip = (torch.empty(J, S, T, **f64) for _ in range(3))
    summary, where = torch.empty(J, 6, **f64), torch.empty(J, 5, **i32)
    types_ = lambda: _lib.check(L.creg_joint_types_f64(p(coords), S, T, K, p(cl), p(off), K, N_LINKS, p(jn), J, 0, T, INTERVAL, TURN_MIN,
                                                       SLIDE_MIN, p(angle), p(slide), p(kind), p(counts), p(kinds), p(s_axis), p(g_axis),
                                                       p(g_pos), stream), "joint_types")
    slides = lambda: _lib.check(L.creg_joint_slides_f64(p(link_T), S, T, N_LINKS, p(jn), J, p(axis), 0, 0, 0, T, p(q), p(tilt), p(slip),
                                                        p(summary), p(where), stream), "joint_slides")
    i0, i1 = sample_index(T, INTERVAL, dev)
    t_types = lambda: torch_joint_types(coords, clusters, jn, i0, i1, TURN_MIN, SLIDE_MIN)
    res = {"K": K, "S": S, "T": T, "links": N_LINKS, "joints": J, "samples_per_joint": NS}
    res["creg_joint_types_ms"] = event_ms(types_, args.repeats, args.min_ms)
    res["creg_joint_slides_ms"] = event_ms(slides, args.repeats, args.min_ms)
    res["ops_joint_types_ms"] = event_ms(lambda: ops.joint_types(coords, clusters, pairs, 0, T, INTERVAL, TURN_MIN, SLIDE_MIN),
                                         args.repeats, args.min_ms)
    res["ops_joint_slides_ms"] = event_ms(lambda: ops.joint_slides(link_T, pairs, axis), args.repeats, args.min_ms)
    res["torch_joint_types_ms"] = event_ms(t_types, args.repeats, args.min_ms)
    res["torch_joint_slides_ms"] = event_ms(lambda: torch_joint_slides(link_T, jn, axis), args.repeats, args.min_ms)
    for k in ("joint_types", "joint_slides"):
        res[f"torch_over_creg_{k}"] = round(res[f"torch_{k}_ms"][0] / res[f"creg_{k}_ms"][0], 2)
    th, t, kd, cn, ax, gax = t_types()
    tq, tt, ts, tsum = torch_joint_slides(link_T, jn, axis)
    res["kinds_equal"] = bool((kd == kind).all() and (cn == counts).all())
    res["max_difference"] = {"sample_angle": float((th - angle).abs().max()), "sample_slide": float((t - slide).abs().max()),
                             "slide_axis": float((ax - s_axis).abs().max()), "global_axis": float((gax - g_axis).abs().max()),
                             "q": float((tq - q).abs().max()), "tilt": float((tt - tilt).abs().max()),
                             "slip": float((ts - slip).abs().max()), "summary": float((tsum - summary).abs().max())}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/time_joint_types.py measures on an MI355X: no GPU is visible")
    for K, S, T in SHAPES:
        time_shape(K, S, T, args)


if __name__ == "__main__":
    main()
