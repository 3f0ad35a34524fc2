"""Time the containment entry (creg_mesh_contain_f64) on the GPU.  Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests at P = 10 poses, its non-adjacent link pairs and ``UrdfRobot.containment_points``, and the
  synthetic robot of tools/time_collide.py (12 links x 20 000 triangles, UV spheres strung along a random walk, all 66 pairs,
  P = 10) with one point per link, the first vertex of its first triangle;
* the whole entry (pose pass + pair pass + finishing pass), the pose pass alone (the entry with n_pairs = 0), the points that
  pass the box gate and the winding terms they cost per second;
* the yardsticks, timed the same way on the same input in the same run: creg_mesh_collide_f64 (the check this one completes),
  and a chunked torch restatement of the gated sum -- link boxes, the gate, the solid-angle terms of the gated points in chunks
  of --chunk triangles, torch.sum -- with the largest |w| difference against the kernel.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_contain.py [--toy_only] [--repeats 5] [--min_ms 200]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from autourdf_amd import _lib, ops, sim_data  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402
from time_collide import event_ms, synthetic_robot  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def t_dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def t_pose(v, T):
    return torch.stack([((T[i, 0] * v[..., 0] + T[i, 1] * v[..., 1]) + T[i, 2] * v[..., 2]) + T[i, 3] for i in range(3)], -1)


def t_omega(tri, x):
    a, b, c = tri[:, 0] - x, tri[:, 1] - x, tri[:, 2] - x
    la, lb, lc = t_dot(a, a).sqrt(), t_dot(b, b).sqrt(), t_dot(c, c).sqrt()
    det = t_dot(a, torch.linalg.cross(b, c))
    den = (((la * lb) * lc + t_dot(a, b) * lc) + t_dot(b, c) * la) + t_dot(c, a) * lb
    return 2.0 * torch.atan2(det, den)


def torch_contain(tri, start, pts, pt_start, link_T, pairs, Q, chunk):
    """(winding (P,M,2,Q), gated points) by the contract, in torch."""
    P, L = link_T.shape[:2]
    wind = torch.zeros(P, len(pairs), 2, Q, dtype=torch.float64, device=tri.device)
    gated = 0
    for q in range(P):
        posed = [t_pose(tri[start[l]:start[l + 1]], link_T[q, l]) for l in range(L)]
        points = [t_pose(pts[pt_start[l]:pt_start[l + 1]], link_T[q, l]) for l in range(L)]
        box = [(t.reshape(-1, 3).amin(0), t.reshape(-1, 3).amax(0)) if len(t) else None for t in posed]
        for m, (la, lb) in enumerate(pairs):
            for d, (inner, outer) in enumerate(((la, lb), (lb, la))):
                if box[outer] is None or not len(points[inner]):
                    continue
                ok = ((box[outer][0] <= points[inner]) & (points[inner] <= box[outer][1])).all(-1).cpu()
                for j in ok.nonzero()[:, 0].tolist():
                    gated += 1
                    total = sum(t_omega(posed[outer][k:k + chunk], points[inner][j]).sum() for k in range(0, len(posed[outer]), chunk))
                    wind[q, m, d, j] = total / (4.0 * math.pi)
    return wind, gated


def time_entry(name, tri, start, pts, pt_start, link_T, pairs, args):
    L, dev = _lib.load(), _lib.device()
    d_tri, d_start, d_pts, d_ps, d_T, d_pairs = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (tri, start, pts, pt_start, link_T, pairs))
    F, N, (P, n_links), M = len(tri), len(pts), link_T.shape[:2], len(pairs)
    Q = max(1, int(np.diff(pt_start).max()))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_c = torch.empty(L.creg_mesh_collide_workspace_bytes(F, n_links, P, M) // 8, dtype=torch.float64, device=dev)
    count = torch.empty(P, M, dtype=torch.int32, device=dev)
    first_c = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    collide = event_ms(lambda: _lib.check(L.creg_mesh_collide_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(d_pairs), M, p(count), p(first_c),
                                                                  None, p(ws_c), ws_c.numel() * 8, stream), "creg_mesh_collide_f64"),
                       args.repeats, args.min_ms)
    ws_bytes = L.creg_mesh_contain_workspace_bytes(F, n_links, P, M, Q)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    inside = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    first = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    wind = torch.empty(P, M, 2, Q, dtype=torch.float64, device=dev)
    call = lambda m: _lib.check(L.creg_mesh_contain_f64(p(d_tri), p(d_start), F, p(d_pts), p(d_ps), N, p(d_T), n_links, P, p(d_pairs), m, Q,
                                                        p(inside), p(first), p(wind), None, p(ws), ws_bytes, stream), "creg_mesh_contain_f64")
    pose = event_ms(lambda: call(0), args.repeats, args.min_ms)
    whole = event_ms(lambda: call(M), args.repeats, args.min_ms)
    torch.cuda.synchronize()
    host_pairs, host_start, host_ps = [tuple(int(x) for x in pr) for pr in pairs], [int(s) for s in start], [int(s) for s in pt_start]
    run = lambda: torch_contain(d_tri, host_start, d_pts, host_ps, d_T, host_pairs, Q, args.chunk)
    want, gated = run()
    t = event_ms(run, max(1, args.repeats // 2), 0.0)
    sizes = np.diff(start)
    terms = float(((want != 0).sum((0, 3)).cpu().numpy() * np.array([[sizes[b], sizes[a]] for a, b in pairs])).sum())
    print(json.dumps({"robot": name, "triangles": F, "links": int(n_links), "pairs": M, "poses": int(P), "points": N, "q_stride": Q,
                      "workspace_MB": round(ws_bytes / 2 ** 20, 1), "pose_pass_ms": round(pose[0], 4), "whole_entry_ms": round(whole[0], 4),
                      "whole_entry_ms_min_max": [round(whole[1], 4), round(whole[2], 4)], "pair_and_finish_ms": round(whole[0] - pose[0], 4),
                      "gated_points": gated, "inside_points": int(inside.sum()), "winding_terms": terms,
                      "winding_terms_per_s": terms / (whole[0] * 1e-3), "mesh_collide_ms": round(collide[0], 4),
                      "mesh_collide_ms_min_max": [round(collide[1], 4), round(collide[2], 4)], "vs_mesh_collide": round(whole[0] / collide[0], 2),
                      "torch_chunked_contain_ms": round(t[0], 3), "torch_chunked_contain_ms_min_max": [round(t[1], 3), round(t[2], 3)],
                      "torch_max_abs_w_difference": float((want - wind).abs().max()), "speedup_vs_torch_contain": round(t[0] / whole[0], 2)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--chunk", type=int, default=1 << 16, help="triangles per chunk of the torch yardstick")
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic robot")
    ap.add_argument("--synthetic_only", action="store_true", help="skip the toy robot")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        if not args.synthetic_only:
            toy, _, _ = write_toy_robot(d)
            env = SimEnv(toy, dof=3, radius=1.2, num_cameras=3)
            r = env.robot
            rows = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
            link_T = ops.urdf_fk(r.fk_table(), r.q_rows([env.set_joint_positions(c) for c in rows]), env.base).cpu().numpy()
            time_entry("toy", r.tri, r.tri_start, *r.containment_points(), link_T, r.collision_pairs(), args)
        if not args.toy_only:
            tri, start, link_T, pairs = synthetic_robot()
            pts = np.array([tri[s, 0] for s in start[:-1]])
            time_entry("12 spheres x 20000", tri, start, pts, np.arange(len(start), dtype=np.int64), link_T, pairs, args)


if __name__ == "__main__":
    main()
